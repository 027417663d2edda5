"""DPMSolverMultistepScheduler without a GPU: its schedules and steps against the reference's recorded traces (tests/golden/dpmsolver.npz,
tools/make_golden_dpmsolver.py), its device plan against its own step() (the numpy row interpreter of test_sched_plan_cpu.py, where
hip.axpby_n and the kernel's ops are ONE fp32 routine, so the two must agree exactly), its refusals and its place in the pipeline loader.

The bound against the reference: per case, 4 x the reference's OWN fp32 deviation, max |ref32 - ref64| / (1 + |ref64|) over all steps
(dpmsolver_envelope.json "fp32"; 2.4e-7 .. 2.5e-6 over the cases).  Our sums associate differently — D1 / D2 folded into the coefficients,
fmaf chaining — a second independent rounding of the same size, not another algorithm.  Ratios reached here (printed by the test; also
in profiles/dpmsolver_bench.txt): 0.6 .. 2.9."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from reflecting_reality_amd import hip, schedulers
from reflecting_reality_amd.schedulers import DPMSolverMultistepScheduler as DPM, PNDMScheduler, UniPCMultistepScheduler, device_plan
from test_sched_plan_cpu import _axpby, _check_rows, _rows, _run_row, _same, numpy_hip  # noqa: F401  (numpy_hip: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SD = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SHAPE = (2, 4, 8, 8)
STEPS = (5, 20)
ENVELOPE_K = 4.0


def _pndm_config():
    return PNDMScheduler(**SD, steps_offset=1, skip_prk_steps=True, set_alpha_to_one=False).config


CASES = {
    "from_pndm": lambda: DPM.from_config(_pndm_config()),
    "2m_karras": lambda: DPM(**SD, use_karras_sigmas=True),
    "2m_heun_v": lambda: DPM(**SD, solver_type="heun", prediction_type="v_prediction", timestep_spacing="trailing"),
    "o1": lambda: DPM(**SD, solver_order=1),
    "o3": lambda: DPM(**SD, solver_order=3),
    "euler_final": lambda: DPM(**SD, euler_at_final=True, timestep_spacing="leading", steps_offset=1),
    "sigma_min": lambda: DPM(**SD, final_sigmas_type="sigma_min"),
    "sde": lambda: DPM(**SD, algorithm_type="sde-dpmsolver++"),
    "sde_karras_o1": lambda: DPM(**SD, algorithm_type="sde-dpmsolver++", use_karras_sigmas=True, solver_order=1),
}
_cache = {}


def trace_inputs():
    """The inputs tools/make_golden_dpmsolver.py fed the reference: ONE np.random.default_rng(7), cases in table order, 5 then 20 steps;
    per entry the start sample, the model outputs, then (SDE) the noises."""
    if "inputs" not in _cache:
        rng = np.random.default_rng(7)
        out = {}
        for name in CASES:
            for n in STEPS:
                x0 = rng.standard_normal(SHAPE, dtype=np.float32)
                mos = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(n)]
                noises = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(n)] if name.startswith("sde") else None
                out[(name, n)] = (x0, mos, noises)
        _cache["inputs"] = out
    return _cache["inputs"]


def golden():
    if "gold" not in _cache:
        _cache["gold"] = np.load(os.path.join(GOLD, "dpmsolver.npz"))
        with open(os.path.join(GOLD, "dpmsolver_envelope.json")) as f:
            _cache["env"] = json.load(f)
    return _cache["gold"], _cache["env"]


def _host_steps(s, x0, mos, noises):
    x, out = torch.from_numpy(x0.copy()), []
    for k, t in enumerate(s.timesteps):
        kw = dict(variance_noise=torch.from_numpy(noises[k].copy())) if noises is not None else {}
        x = s.step(torch.from_numpy(mos[k].copy()), t, x, return_dict=False, **kw)[0]
        out.append(x)
    return out


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("case", list(CASES))
def test_schedule_equals_the_reference(case, steps):
    G, _ = golden()
    s = CASES[case]()
    s.set_timesteps(steps)
    ts, sig = G[f"trace/{case}/{steps}/timesteps"], G[f"trace/{case}/{steps}/sigmas"]
    assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), ts)
    assert s.sigmas.dtype == torch.float32 and s.sigmas.shape == sig.shape
    ulp = np.abs(s.sigmas.numpy().view(np.int32).astype(np.int64) - sig.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, f"sigmas differ by {ulp.max()} ulp"
    assert s.num_inference_steps == steps and s.step_index is None and s.order == 1 and s.init_noise_sigma == 1.0


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("case", list(CASES))
def test_host_step_stays_inside_the_reference_fp32_envelope(numpy_hip, case, steps):
    G, env = golden()
    x0, mos, noises = trace_inputs()[(case, steps)]
    s = CASES[case]()
    s.set_timesteps(steps)
    got = torch.stack(_host_steps(s, x0, mos, noises)).numpy().astype(np.float64)
    ref = G[f"trace/{case}/{steps}/ref64"]
    assert ref.dtype == np.float64 and got.shape == ref.shape
    err = (np.abs(got - ref) / (1 + np.abs(ref))).max()
    dev = env["fp32"][f"{case}/{steps}"]
    print(f"{case}/{steps}: err {err:.3e}, the reference's fp32 deviation {dev:.3e}, ratio {err / dev:.2f}")
    assert err <= ENVELOPE_K * dev, f"{case}/{steps}: {err:.3e} > {ENVELOPE_K} x {dev:.3e}"
    assert s.step_index == steps


def test_the_recorded_fp32_deviation_is_that_of_the_recorded_traces():
    G, env = golden()
    R32 = np.load(os.path.join(GOLD, "dpmsolver_ref32.npz"))
    for case in CASES:
        for n in STEPS:
            r64, r32 = G[f"trace/{case}/{n}/ref64"], R32[f"trace/{case}/{n}/ref32"]
            assert r32.dtype == np.float32
            dev = (np.abs(r32.astype(np.float64) - r64) / (1 + np.abs(r64))).max()
            assert dev == pytest.approx(env["fp32"][f"{case}/{n}"], rel=1e-12) and 1e-7 < dev < 1e-5


def _plan_vs_host(make, steps, x0, mos, noises, g=7.5):
    """test_sched_plan_cpu._compare with a noise register and the recorded inputs: the guided e of step k is the trace's model output."""
    host, dev = make(), make()
    host.set_timesteps(steps)
    dev.set_timesteps(steps)
    plan = device_plan(dev)
    assert dev.step_index is None and dev.lower_order_nums == 0 and all(m is None for m in dev.model_outputs)
    rows = _rows(plan)
    assert len(rows) == steps
    lat_h, lat_d = torch.from_numpy(x0.copy()), x0.copy()
    state = np.full((max(plan.nslots, 1),) + SHAPE, np.nan, dtype=np.float32)
    written = set()
    for k in range(steps):
        e = mos[k]
        kw = dict(variance_noise=torch.from_numpy(noises[k].copy())) if noises is not None else {}
        lat_h = host.step(torch.from_numpy(e.copy()), host.timesteps[k], lat_h, return_dict=False, **kw)[0]
        lat_d = _run_noise_row(rows[k], e, lat_d, state, written, plan.noise_reg, None if noises is None else noises[k])
        assert np.array_equal(lat_h.numpy().view(np.int32), lat_d.view(np.int32)), f"step {k}: the plan's latents differ"
    plan.finish(dev, torch.from_numpy(state))
    assert set(vars(dev)) == set(vars(host))
    for key in vars(host):
        _same(getattr(dev, key), getattr(host, key), f"{type(host).__name__}.{key} after {steps} steps")
    return plan, rows


def _run_noise_row(row, e, lat, state, written, noise_reg, noise):
    """One mf_sched_step_noise_dev launch in numpy: test_sched_plan_cpu._run_row, with register noise_reg (a temporary, neither loaded
    nor stored) holding the step's noise before the ops run."""
    if noise is None:
        return _run_row(row, e, lat, state, written)
    S = row.nslots
    assert noise_reg >= 2 + S, "the noise register is a temporary"
    assert not (row.load >> noise_reg) & 1 and not (row.store >> noise_reg) & 1
    R = {0: e, noise_reg: noise.copy()}
    for r in range(1, hip.SCHED_MAX_REGS):
        if (row.load >> r) & 1 and (r == 1 or r - 2 < S):
            if r >= 2:
                assert r - 2 in written, f"the row loads slot {r - 2}, which no earlier step wrote"
            R[r] = lat.copy() if r == 1 else state[r - 2].copy()
    for j in range(row.nops):
        op = row.ops[j]
        srcs = [op.src[k] for k in range(max(op.nterms, 1))]
        for s in srcs:
            assert s in R, f"op {j} reads register {s}, which holds nothing yet"
        R[op.dst] = R[srcs[0]].copy() if op.nterms == 0 else _axpby([R[s] for s in srcs], [op.coef[k] for k in range(op.nterms)])
    out = lat
    for r in range(1, hip.SCHED_MAX_REGS):
        if (row.store >> r) & 1:
            assert r in R and (r == 1 or r - 2 < S)
            if r == 1:
                out = R[1]
            else:
                state[r - 2] = R[r]
                written.add(r - 2)
    return out


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("case", list(CASES))
def test_plan_equals_the_host_steps(numpy_hip, case, steps):
    x0, mos, noises = trace_inputs()[(case, steps)]
    plan, rows = _plan_vs_host(CASES[case], steps, x0, mos, noises)
    _check_rows(plan, rows)
    if case.startswith("sde"):
        assert plan.noise_reg == 2 + plan.nslots and plan.noise_reg < hip.SCHED_MAX_REGS
        assert any(plan.noise_reg in [r.ops[j].src[k] for j in range(r.nops) for k in range(r.ops[j].nterms)] for r in rows)
    else:
        assert plan.noise_reg == -1


def test_plans_without_noise_report_no_register_and_the_row_layout_stays():
    for s in (UniPCMultistepScheduler(**SD), PNDMScheduler(**SD, skip_prk_steps=True)):
        s.set_timesteps(8)
        assert device_plan(s).noise_reg == -1
    assert C.sizeof(hip.SchedRow) == hip.load().mf_sizeof_sched_row() == 16 + hip.SCHED_MAX_OPS * (8 + 8 * hip.SCHED_MAX_TERMS)
    assert (hip.SCHED_MAX_OPS, hip.SCHED_MAX_TERMS, hip.SCHED_MAX_REGS) == (8, 6, 16)


def test_a_partial_sde_plan_ends_in_the_state_of_as_many_host_steps(numpy_hip):
    x0, mos, noises = trace_inputs()[("sde", 20)]
    host, dev = CASES["sde"](), CASES["sde"]()
    host.set_timesteps(20)
    dev.set_timesteps(20)
    plan = device_plan(dev, steps=7)
    assert plan.rows.shape[0] == 7 and plan.noise_reg >= 2
    _host_steps_n = 7
    x = torch.from_numpy(x0.copy())
    for k in range(_host_steps_n):
        x = host.step(torch.from_numpy(mos[k]), host.timesteps[k], x, variance_noise=torch.from_numpy(noises[k]), return_dict=False)[0]
    plan.finish(dev, torch.zeros((plan.nslots,) + SHAPE))
    assert dev.step_index == host.step_index == 7 and dev.lower_order_nums == host.lower_order_nums == 2


@pytest.mark.parametrize("kw, word", [
    (dict(thresholding=True), "thresholding"), (dict(use_lu_lambdas=True), "use_lu_lambdas"),
    (dict(algorithm_type="dpmsolver"), "dpmsolver"), (dict(algorithm_type="sde-dpmsolver"), "sde-dpmsolver"),
    (dict(variance_type="learned_range"), "variance_type"), (dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr"),
    (dict(algorithm_type="sde-dpmsolver++", solver_order=3), "solver_order")])
def test_refused_options_raise_by_name(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        DPM(**SD, **kw)


def test_add_noise_is_refused_and_step_needs_set_timesteps():
    s = DPM(**SD)
    with pytest.raises(NotImplementedError, match="add_noise"):
        s.add_noise(torch.zeros(SHAPE), torch.zeros(SHAPE), torch.tensor([1]))
    with pytest.raises(ValueError, match="set_timesteps"):
        s.step(torch.zeros(SHAPE), 1, torch.zeros(SHAPE))
    with pytest.raises(ValueError):
        DPM(**SD, prediction_type="nonsense")


def test_prediction_type_sample_and_lambda_min_clipped(numpy_hip):
    """prediction_type 'sample': the model output IS the data prediction, so the last step (final sigma 0) returns it unchanged;
    lambda_min_clipped cuts the schedule's first timestep (squaredcos-style stability switch) exactly where lambda_t crosses it."""
    s = DPM(**SD, prediction_type="sample")
    s.set_timesteps(3)
    x = torch.from_numpy(np.random.default_rng(1).standard_normal(SHAPE, dtype=np.float32))
    for t in s.timesteps:
        m = torch.from_numpy(np.random.default_rng(int(t)).standard_normal(SHAPE, dtype=np.float32))
        x = s.step(m, t, x, return_dict=False)[0]
    assert torch.equal(x, m)
    c = DPM(**SD, lambda_min_clipped=-2.0)
    c.set_timesteps(10)
    last = 1000 - int(torch.searchsorted(torch.flip(c.lambda_t, [0]), -2.0))
    assert last < 1000 and int(c.timesteps[0]) == last - 1 and float(c.lambda_t[last - 1]) >= -2.0 > float(c.lambda_t[last])


def test_config_round_trips_and_crosses_classes(tmp_path):
    s = DPM(**SD, use_karras_sigmas=True, solver_order=3, euler_at_final=True)
    s.save_config(str(tmp_path))
    with open(tmp_path / "scheduler_config.json") as f:
        saved = json.load(f)
    assert saved["_class_name"] == "DPMSolverMultistepScheduler" and saved["use_karras_sigmas"] is True and saved["solver_order"] == 3
    back = DPM.from_pretrained(str(tmp_path))
    assert {k: v for k, v in dict(back.config).items() if not k.startswith("_")} == \
        {k: v for k, v in dict(s.config).items() if not k.startswith("_")}
    # from a PNDM / DDIM config: foreign keys dropped, the source's defaults replaced by THIS class's (timestep_spacing: linspace)
    d = DPM.from_config(_pndm_config())
    assert d.config["steps_offset"] == 1 and d.config["beta_schedule"] == "scaled_linear" and d.config["timestep_spacing"] == "linspace"
    assert "skip_prk_steps" not in d.config and "set_alpha_to_one" not in d.config
    from reflecting_reality_amd.schedulers import DDIMScheduler
    d2 = DPM.from_config(DDIMScheduler(**SD, clip_sample=False, timestep_spacing="trailing").config)
    assert d2.config["timestep_spacing"] == "trailing" and "clip_sample" not in d2.config
    u = UniPCMultistepScheduler.from_config(d.config)          # and onward, as the reference's scripts chain them
    assert u.config["steps_offset"] == 1 and u.config["solver_order"] == 2


def test_the_pipeline_saves_and_loads_the_class(tmp_path):
    """save_pretrained writes the scheduler's class and config, from_pretrained of that folder loads it (NotImplementedError before the
    class existed).  The three networks are stand-ins: only the scheduler's round trip is under test."""
    from reflecting_reality_amd.pipeline import StableDiffusionBrushNetPipeline as Pipe
    import reflecting_reality_amd as pkg
    from reflecting_reality_amd.compat import diffusers as compat
    assert "DPMSolverMultistepScheduler" in Pipe._scheduler_classes
    assert pkg.DPMSolverMultistepScheduler is DPM and compat.DPMSolverMultistepScheduler is DPM
    sched = DPM(**SD, algorithm_type="sde-dpmsolver++", use_karras_sigmas=True, solver_type="heun")
    pipe = Pipe(vae=_Stub(), text_encoder=None, tokenizer=None, unet=_Stub(), brushnet=_Stub(), scheduler=sched, safety_checker=None,
                feature_extractor=None, requires_safety_checker=False, depth_conditioning_mode="concat")
    pipe.save_pretrained(str(tmp_path))
    with open(tmp_path / "model_index.json") as f:
        assert json.load(f)["scheduler"] == ["diffusers", "DPMSolverMultistepScheduler"]
    with open(tmp_path / "scheduler" / "scheduler_config.json") as f:
        assert json.load(f)["_class_name"] == "DPMSolverMultistepScheduler"
    sentinel = _Stub()
    back = Pipe.from_pretrained(str(tmp_path), vae=_Stub(), unet=_Stub(), brushnet=sentinel, device="cpu")
    assert type(back.scheduler) is DPM and back.brushnet is sentinel
    assert {k: v for k, v in dict(back.scheduler.config).items() if not k.startswith("_")} == \
        {k: v for k, v in dict(sched.config).items() if not k.startswith("_")}
    back.scheduler.set_timesteps(7)
    sched.set_timesteps(7)
    assert torch.equal(back.scheduler.sigmas, sched.sigmas) and torch.equal(back.scheduler.timesteps, sched.timesteps)


class _Stub:
    """What the pipeline's constructor and save_pretrained read of a model they are handed."""
    class _Config(dict):
        block_out_channels = (8, 8)
    config = _Config(block_out_channels=(8, 8))
    _class_name = "Stub"

    def save_pretrained(self, path):
        os.makedirs(path, exist_ok=True)


def test_the_noise_thunks_have_a_table_of_their_own():
    """csrc/program.hip's kNoiseFns restates program.SIGNATURES_NOISE (the header's prototypes without the stream), apart from the two
    tables whose contents test_program_cpu.py / test_program_call_cpu.py pin; each thunk reads exactly its signature's arguments."""
    import re
    import abi_header
    from reflecting_reality_amd import program
    src = open(os.path.join(ROOT, "reflecting-reality_amd", "csrc", "program.hip")).read()
    table = dict(re.findall(r'\{H_\w+,\s*"(mf_\w+)",\s*"(\w+)"\}', src))
    assert table == program.SIGNATURES_NOISE and set(table) == {"mf_sched_step_noise_dev", "mf_philox_advance"}
    assert not set(table) & (set(program.SIGNATURES) | set(program.SIGNATURES_CALL)), "an entry belongs to one of the three tables"
    protos = abi_header.prototypes()
    for name, sig in table.items():
        assert "".join(protos[name][1][:-1]) == sig, name
    kinds = {"P": "p", "FP": "p", "I": "i", "L": "l", "F": "f"}
    for hid, name in re.findall(r'\{(H_\w+),\s*"(mf_\w+)"', src):
        body = re.search(r"case %s:(.*?)(?=\n    case |\n    default:)" % hid, src, flags=re.S).group(1)
        used = {int(i): kinds[k] for k, i in re.findall(r"\b(FP|P|I|L|F)\((\d+)\)", body)}
        assert used == dict(enumerate(table[name])), f"{name}: the thunk reads {used}, the signature is {table[name]!r}"


def test_the_new_entry_is_declared_exported_and_bound():
    import abi_header
    protos = abi_header.prototypes()
    name = "mf_sched_step_noise_dev"
    assert name in protos and name in hip.SIGNATURES and name in hip.EXPORTS and hasattr(hip.load(), name)
    ret, params = protos[name]
    assert ret + ":" + "".join(params) == hip.SIGNATURES[name] == "i:ppfppplilllllpp"
    # mf_sched_step_dev's arguments, then noise_reg, per_sample, first_sample, global_batch, seed, offset, state (and the stream)
    assert hip.SIGNATURES[name].startswith(hip.SIGNATURES["mf_sched_step_dev"][:-1])
    assert hip.SIGNATURES[name][-5:] == hip.SIGNATURES["mf_philox_normal"][-5:]
    assert callable(hip.sched_step_noise_dev)
