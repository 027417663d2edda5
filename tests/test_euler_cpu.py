"""EulerDiscreteScheduler / EulerAncestralDiscreteScheduler without a GPU: schedules and steps against the reference's recorded traces
(tests/golden/euler*.npz, tools/make_golden_euler.py), the device plan against the schedulers' own step() and scale_model_input (the numpy
row interpreter of test_sched_plan_cpu.py, where hip.axpby_n and the kernel's ops are ONE fp32 routine, so the two agree exactly), the
refusals, and the pipeline loader.

The bound against the reference: per case, ENVELOPE_K = 4 x the reference's OWN fp32 deviation, max |ref32 - ref64| / (1 + |ref64|)
over all steps (euler_envelope.json "fp32": 2.6e-7 .. 2.1e-6 for the samples, 2.1e-7 .. 1.6e-6 for the model inputs), as
tests/test_dpmsolver_cpu.py: ours is a second independent fp32 rounding of the same size (folded coefficients, fmaf chaining, a multiply
by the reciprocal where the reference divides), not another algorithm.  Ratios reached (printed by the test, written into
profiles/euler_bench.txt): samples 0.24 .. 1.19, model inputs 0.41 .. 1.31."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from reflecting_reality_amd import hip, schedulers
from reflecting_reality_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler as EulerA,
                                               EulerDiscreteScheduler as Euler, PNDMScheduler, UniPCMultistepScheduler, device_plan)
from test_dpmsolver_cpu import ENVELOPE_K, _Stub, _run_noise_row
from test_sched_plan_cpu import _check_rows, _rows, _same, numpy_hip  # noqa: F401  (numpy_hip: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SD = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SHAPE = (2, 4, 8, 8)
STEPS = (5, 20)
assert ENVELOPE_K == 4.0


def _pndm_config():
    """The checkpoint's scheduler as its scheduler_config.json states it: the spacing is an explicit key there, so it crosses classes."""
    return PNDMScheduler(**SD, steps_offset=1, skip_prk_steps=True, set_alpha_to_one=False, timestep_spacing="leading").config


# (a_linspace_karras: the reference's ancestral class has no Karras option; from_config drops the key there and here, which leaves the
# ancestral sampler on the fractional `linspace` timesteps — tools/make_golden_euler.py)
CASES = {
    "from_pndm": lambda: Euler.from_config(_pndm_config()),
    "linspace": lambda: Euler(**SD),
    "trailing_karras": lambda: Euler(**SD, timestep_spacing="trailing", use_karras_sigmas=True),
    "v_pred": lambda: Euler(**SD, prediction_type="v_prediction"),
    "sample": lambda: Euler(**SD, prediction_type="sample"),
    "a_from_pndm": lambda: EulerA.from_config(_pndm_config()),
    "a_linspace_karras": lambda: EulerA.from_config(Euler(**SD, use_karras_sigmas=True).config),
    "a_v_trailing": lambda: EulerA(**SD, prediction_type="v_prediction", timestep_spacing="trailing"),
}
_cache = {}


def trace_inputs():
    """The inputs tools/make_golden_euler.py fed the reference: ONE np.random.default_rng(7), cases in table order, 5 then 20 steps; per
    entry the unit-normal start (times init_noise_sigma: the sample), the model outputs, then (ancestral) the noises."""
    if "inputs" not in _cache:
        rng = np.random.default_rng(7)
        out = {}
        for name in CASES:
            for n in STEPS:
                x0 = rng.standard_normal(SHAPE, dtype=np.float32)
                mos = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(n)]
                noises = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(n)] if name.startswith("a_") else None
                out[(name, n)] = (x0, mos, noises)
        _cache["inputs"] = out
    return _cache["inputs"]


def golden():
    if "gold" not in _cache:
        _cache["gold"] = {}
        for name in ("euler.npz", "euler_scaled64.npz", "euler_ref32.npz"):
            with np.load(os.path.join(GOLD, name)) as z:
                _cache["gold"].update({k: z[k] for k in z.files if k.startswith("trace/")})
        with open(os.path.join(GOLD, "euler_envelope.json")) as f:
            _cache["env"] = json.load(f)
    return _cache["gold"], _cache["env"]


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def assert_timesteps(got, want, karras):
    """The schedule's timesteps against the recorded ones: float32 and exactly equal.  One exception, Karras sigmas on a machine whose numpy
    rounds the float32 log of the training sigmas differently from the machine that ran the reference (numpy dispatches that loop by CPU
    features; the recorded table is `machine/log_sigmas`).  There neither the reference nor this class reproduces the recorded bits:
    _sigma_to_t gives t = low_idx + (low - log sigma) / (low - high) with low, high entries of that table, so an error eps in each moves
    t by at most 3 eps / |low - high|.  eps: 4 ulp of a float32 below 4 in magnitude (numpy's stated bound for that loop), 4 * 2^-22;
    |low - high|: at least the table's smallest difference.  That is below 1e-3 of a training timestep."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    with np.load(os.path.join(GOLD, "euler.npz")) as z:
        table = z["machine/log_sigmas"]
    s = Euler(**SD)
    here = np.log(s._sigma_table())
    assert table.dtype == here.dtype == np.float32 and np.abs(here - table).max() <= 4 * 2.0 ** -22
    if not karras or np.array_equal(here, table):
        assert np.array_equal(got, want), f"timesteps differ: {got} != {want}"
        return
    tol = 3 * 4 * 2.0 ** -22 / np.abs(np.diff(table.astype(np.float64))).min()
    assert tol < 1e-3
    print(f"this machine's float32 log differs from the recorded one in {int((here != table).sum())} of {table.size} entries: "
          f"Karras timesteps within {tol:.2e}, max difference {np.abs(got.astype(np.float64) - want).max():.2e}")
    assert np.abs(got.astype(np.float64) - want).max() <= tol, f"timesteps differ by more than {tol:.2e}: {got} != {want}"


def _host_trace(s, x0, mos, noises):
    """(samples after every step, model inputs before every step), starting from x0 * init_noise_sigma as prepare_latents does."""
    x = hip.axpby_n([torch.from_numpy(x0.copy())], [float(s.init_noise_sigma)])
    samples, inputs = [], []
    for k, t in enumerate(s.timesteps):
        inputs.append(s.scale_model_input(x, t))
        kw = dict(variance_noise=torch.from_numpy(noises[k].copy())) if noises is not None else {}
        x = s.step(torch.from_numpy(mos[k].copy()), t, x, return_dict=False, **kw)[0]
        samples.append(x)
    return samples, inputs


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("case", list(CASES))
def test_schedule_equals_the_reference(case, steps):
    G, _ = golden()
    s = CASES[case]()
    s.set_timesteps(steps)
    key = f"trace/{case}/{steps}"
    ts, sig = G[f"{key}/timesteps"], G[f"{key}/sigmas"]
    assert s.timesteps.dtype == torch.float32
    assert_timesteps(s.timesteps.numpy(), ts, karras=bool(s.config.get("use_karras_sigmas")))
    if case in ("linspace", "trailing_karras", "a_linspace_karras"):
        assert np.any(ts != np.round(ts)), "these schedules have fractional timesteps"
    assert s.sigmas.dtype == torch.float32 and s.sigmas.shape == sig.shape and float(s.sigmas[-1]) == 0.0
    assert _ulps(s.sigmas.numpy(), sig) <= 1
    assert _ulps(s.init_noise_sigma, G[f"{key}/init_noise_sigma"]) <= 1
    assert s.num_inference_steps == steps and s.step_index is None and s.order == 1
    leading = s.config["timestep_spacing"] == "leading"
    assert (case in ("from_pndm", "a_from_pndm")) == leading
    want = float(torch.sqrt(s.sigmas.max() ** 2 + 1)) if leading else float(s.sigmas.max())
    assert s.init_noise_sigma == want and s.init_noise_sigma > 1.0


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("case", list(CASES))
def test_host_step_and_model_input_stay_inside_the_reference_fp32_envelope(numpy_hip, case, steps):
    G, env = golden()
    x0, mos, noises = trace_inputs()[(case, steps)]
    s = CASES[case]()
    s.set_timesteps(steps)
    samples, inputs = _host_trace(s, x0, mos, noises)
    lines = []
    for what, got, ref, dev in (("samples", samples, G[f"trace/{case}/{steps}/ref64"], env["fp32"][f"{case}/{steps}"]),
                                ("model inputs", inputs, G[f"trace/{case}/{steps}/scaled64"], env["fp32"][f"{case}/{steps}/scaled"])):
        got = torch.stack(got).numpy().astype(np.float64)
        assert ref.dtype == np.float64 and got.shape == ref.shape
        err = (np.abs(got - ref) / (1 + np.abs(ref))).max()
        lines.append((what, err, dev))
        print(f"{case}/{steps} {what}: err {err:.3e}, the reference's fp32 deviation {dev:.3e}, ratio {err / dev:.2f}")
    for what, err, dev in lines:
        assert err <= ENVELOPE_K * dev, f"{case}/{steps} {what}: {err:.3e} > {ENVELOPE_K} x {dev:.3e}"
    assert s.step_index == steps
    if case == "sample":                           # the last step (sigma -> 0) returns the data prediction itself
        assert np.array_equal(samples[-1].numpy(), mos[-1])


def test_the_recorded_fp32_deviation_is_that_of_the_recorded_traces():
    G, env = golden()
    for case in CASES:
        for n in STEPS:
            for k64, k32, name in (("ref64", "ref32", f"{case}/{n}"), ("scaled64", "scaled32", f"{case}/{n}/scaled")):
                r64, r32 = G[f"trace/{case}/{n}/{k64}"], G[f"trace/{case}/{n}/{k32}"]
                assert r32.dtype == np.float32 and r64.dtype == np.float64
                dev = (np.abs(r32.astype(np.float64) - r64) / (1 + np.abs(r64))).max()
                assert dev == pytest.approx(env["fp32"][name], rel=1e-12) and 1e-7 < dev < 1e-5


def _plan_vs_host(make, steps, x0, mos, noises, plan_steps=None):
    """Every row through the numpy interpreter against the host's step() + scale_model_input: the slot's sample and register 1's model
    input after every step, bit for bit; then finish()."""
    host, dev = make(), make()
    host.set_timesteps(steps)
    dev.set_timesteps(steps)
    plan = device_plan(dev, steps=plan_steps)
    n = steps if plan_steps is None else plan_steps
    assert dev.step_index is None and plan.x_slot == 0 and plan.nslots == 1 and plan.steps == n
    rows = _rows(plan)
    assert len(rows) == n
    x_h = hip.axpby_n([torch.from_numpy(x0.copy())], [float(host.init_noise_sigma)])
    # the documented start: x0 into the slot, x0 * first_scale into the latents
    state = np.full((plan.nslots,) + SHAPE, np.nan, dtype=np.float32)
    state[plan.x_slot] = x_h.numpy()
    written = {plan.x_slot}
    lat_d = (np.float32(plan.first_scale) * x_h.numpy()).astype(np.float32)
    assert np.array_equal(lat_d, host.scale_model_input(x_h, host.timesteps[0]).numpy())
    for k in range(n):
        kw = dict(variance_noise=torch.from_numpy(noises[k].copy())) if noises is not None else {}
        x_h = host.step(torch.from_numpy(mos[k].copy()), host.timesteps[k], x_h, return_dict=False, **kw)[0]
        lat_h = hip.axpby_n([x_h], [host._input_scale(host.step_index)])
        lat_d = _run_noise_row(rows[k], mos[k], lat_d, state, written, plan.noise_reg, None if noises is None else noises[k])
        assert np.array_equal(x_h.numpy().view(np.int32), state[plan.x_slot].view(np.int32)), f"step {k}: the slot's sample differs"
        assert np.array_equal(lat_h.numpy().view(np.int32), lat_d.view(np.int32)), f"step {k}: the model input differs"
        if k + 1 < steps:
            assert np.array_equal(lat_d, host.scale_model_input(x_h, host.timesteps[k + 1]).numpy())
    if n == steps:                                 # sigma 0: the factor is exactly 1 and the latents are the result
        assert np.array_equal(lat_d.view(np.int32), state[plan.x_slot].view(np.int32))
    plan.finish(dev, torch.from_numpy(state))
    assert set(vars(dev)) == set(vars(host))
    for key in vars(host):
        _same(getattr(dev, key), getattr(host, key), f"{type(host).__name__}.{key} after {n} steps")
    return plan, rows


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("case", list(CASES))
def test_plan_equals_the_host_steps(numpy_hip, case, steps):
    x0, mos, noises = trace_inputs()[(case, steps)]
    plan, rows = _plan_vs_host(CASES[case], steps, x0, mos, noises)
    _check_rows(plan, rows)
    if case.startswith("a_"):
        assert plan.noise_reg >= 2 + plan.nslots and plan.noise_reg < hip.SCHED_MAX_REGS
        assert all(plan.noise_reg in [r.ops[j].src[k] for j in range(r.nops) for k in range(r.ops[j].nterms)] for r in rows)
    else:
        assert plan.noise_reg == -1
    for r in rows:                                 # the update, then the model input: two ops, the sample's slot loaded and stored
        assert r.nops == 2 and r.load == 1 << 2 and r.store == (1 << 1) | (1 << 2)
        assert r.ops[1].dst == 1 and r.ops[1].nterms == 1 and r.ops[1].src[0] == 2
    assert rows[-1].ops[1].coef[0] == 1.0


def test_a_partial_ancestral_plan_ends_in_the_state_of_as_many_host_steps(numpy_hip):
    x0, mos, noises = trace_inputs()[("a_from_pndm", 20)]
    plan, rows = _plan_vs_host(CASES["a_from_pndm"], 20, x0, mos, noises, plan_steps=7)
    assert plan.rows.shape[0] == 7 and 0 < rows[-1].ops[1].coef[0] < 1.0


def host_math_fingerprint():
    """What the existing schedulers' coefficient arithmetic gives on THIS machine for a grid of fp32 values: their tables and 0-dim
    tensor formulas go through torch's float32 pow (`** 0.5`), log, exp and expm1, whose last bits depend on the CPU's vector path."""
    x = torch.linspace(0.01, 5.0, 256, dtype=torch.float32)
    return np.stack([(x ** 0.5).numpy(), np.array([float(v ** 0.5) for v in x], dtype=np.float32), torch.log(x).numpy(),
                     torch.exp(-x).numpy(), torch.expm1(-x).numpy()])


def plan_row_bytes():
    """The rows of fixed PNDM / UniPC / DPM-Solver++ plans as bytes.  tests/golden/sched_plan_rows.npz holds what this function returned
    on the commit before the Euler classes (recorded by running it there), and that machine's host_math_fingerprint()."""
    sd = dict(SD, steps_offset=1)
    makes = {
        "pndm_prk_10": (lambda: PNDMScheduler(**sd, set_alpha_to_one=False), 10),
        "pndm_skip_v_12": (lambda: PNDMScheduler(**sd, set_alpha_to_one=False, skip_prk_steps=True, prediction_type="v_prediction"), 12),
        "unipc_o3_10": (lambda: UniPCMultistepScheduler(**sd, solver_order=3), 10),
        "unipc_bh1_v_8": (lambda: UniPCMultistepScheduler(**sd, solver_type="bh1", prediction_type="v_prediction"), 8),
        "dpm_2m_karras_10": (lambda: DPMSolverMultistepScheduler(**SD, use_karras_sigmas=True), 10),
        "dpm_o3_12": (lambda: DPMSolverMultistepScheduler(**SD, solver_order=3), 12),
        "dpm_sde_heun_10": (lambda: DPMSolverMultistepScheduler(**SD, algorithm_type="sde-dpmsolver++", solver_type="heun"), 10),
    }
    out = {}
    for name, (make, n) in makes.items():
        s = make()
        s.set_timesteps(n)
        plan = device_plan(s)
        out[name] = np.frombuffer(plan.rows.numpy().tobytes(), dtype=np.uint8).copy()
        out[name + "/meta"] = np.array([plan.nslots, plan.noise_reg, plan.rows.shape[0]], dtype=np.int64)
    return out


def test_row_layout_and_the_existing_plans_rows_are_unchanged():
    assert C.sizeof(hip.SchedRow) == hip.load().mf_sizeof_sched_row() == 16 + hip.SCHED_MAX_OPS * (8 + 8 * hip.SCHED_MAX_TERMS)
    assert (hip.SCHED_MAX_OPS, hip.SCHED_MAX_TERMS, hip.SCHED_MAX_REGS) == (8, 6, 16)
    now = plan_row_bytes()
    with np.load(os.path.join(GOLD, "sched_plan_rows.npz")) as z:
        then = {k: z[k] for k in z.files}
    same_math = np.array_equal(then.pop("machine/fingerprint"), host_math_fingerprint())
    assert set(then) == set(now)
    for k in then:
        if same_math or k.endswith("/meta"):
            assert np.array_equal(then[k], now[k]), f"{k}: the plan's rows differ from the recorded ones"
            continue
        # Another CPU's pow / log / exp: the coefficients the schedulers' own step() computes differ in their last bits (these formulas
        # take differences of neighbouring table entries, condition up to ~1e3 on 2^-23: below 1e-3 relative), so the bytes cannot be
        # the recorded ones.  What device_plan decides must still be: every integer of every row, bit for bit, and each coefficient in
        # its place within 1e-3 of max(1, |c|) (a coefficient carried into the wrong term is off by its own size).
        a = [hip.SchedRow.from_buffer_copy(r.tobytes()) for r in then[k].reshape(-1, C.sizeof(hip.SchedRow))]
        b = [hip.SchedRow.from_buffer_copy(r.tobytes()) for r in now[k].reshape(-1, C.sizeof(hip.SchedRow))]
        assert len(a) == len(b)
        for i, (ra, rb) in enumerate(zip(a, b)):
            assert (ra.nops, ra.nslots, ra.load, ra.store) == (rb.nops, rb.nslots, rb.load, rb.store), f"{k}, row {i}"
            for j in range(hip.SCHED_MAX_OPS):
                oa, ob = ra.ops[j], rb.ops[j]
                assert (oa.dst, oa.nterms, list(oa.src)) == (ob.dst, ob.nterms, list(ob.src)), f"{k}, row {i}, op {j}"
                for ca, cb in zip(oa.coef, ob.coef):
                    assert abs(ca - cb) <= 1e-3 * max(1.0, abs(ca)), f"{k}, row {i}, op {j}: coefficient {cb} was {ca}"
    print(f"plan rows: {'byte-identical' if same_math else 'integers identical, coefficients within 1e-3 (another host math path)'}")
    for s in (UniPCMultistepScheduler(**SD), PNDMScheduler(**SD, skip_prk_steps=True), DPMSolverMultistepScheduler(**SD)):
        s.set_timesteps(8)
        plan = device_plan(s)
        assert plan.x_slot == -1 and plan.first_scale == 1.0 and plan.noise_reg == -1


@pytest.mark.parametrize("cls, kw, word", [
    (Euler, dict(interpolation_type="log_linear"), "log_linear"), (Euler, dict(timestep_type="continuous"), "continuous"),
    (Euler, dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr"), (EulerA, dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr"),
    (Euler, dict(sigma_min=0.1), "sigma_min"), (Euler, dict(sigma_max=10.0), "sigma_max"), (EulerA, dict(prediction_type="sample"), "sample")])
def test_refused_options_raise_by_name(cls, kw, word):
    with pytest.raises(NotImplementedError, match=word):
        cls(**SD, **kw)


def test_churn_and_add_noise_are_refused_and_step_needs_set_timesteps(numpy_hip):
    z = torch.zeros(SHAPE)
    for cls in (Euler, EulerA):
        s = cls(**SD)
        with pytest.raises(NotImplementedError, match="add_noise"):
            s.add_noise(z, z, torch.tensor([1.0]))
        with pytest.raises(ValueError, match="set_timesteps"):
            s.step(z, 1.0, z)
        with pytest.raises(ValueError, match="set_timesteps"):
            s.scale_model_input(z, 1.0)
        with pytest.raises(ValueError):
            cls(**SD, prediction_type="nonsense")
        s.set_timesteps(4)
        with pytest.raises(ValueError, match="integer"):
            s.step(z, 3, z)
    s = Euler(**SD)
    s.set_timesteps(4)
    with pytest.raises(NotImplementedError, match="s_churn"):
        s.step(z, s.timesteps[0], z, s_churn=0.5)
    assert s.step_index is None


def test_step_index_begin_index_and_the_prescaled_switch(numpy_hip):
    s = Euler(**SD)
    s.set_timesteps(6)
    x = torch.ones(SHAPE)
    assert s.begin_index is None
    scaled = s.scale_model_input(x, s.timesteps[0])          # sets the index from the timestep, like the reference
    assert s.step_index == 0 and float(scaled[0, 0, 0, 0]) == s._input_scale(0) < 0.1
    s.step(x, s.timesteps[0], x)
    assert s.step_index == 1
    s.model_input_prescaled = True                           # the captured step's latents already hold the model input
    assert s.scale_model_input(x, None) is x
    s.set_timesteps(6)
    assert s.model_input_prescaled is False and s.step_index is None
    s.set_begin_index(3)
    s.step(x, s.timesteps[3], x)
    assert s.step_index == 4
    a = EulerA(**SD)
    a.set_timesteps(3)
    g = torch.Generator().manual_seed(1)
    for t in a.timesteps:                                    # one draw per step, the last included
        before = g.get_state().clone()
        a.step(x, t, x, generator=g)
        assert not torch.equal(g.get_state(), before)
    e = Euler(**SD)
    e.set_timesteps(3)
    before = g.get_state().clone()
    e.step(x, e.timesteps[0], x, generator=g)                # the deterministic class draws nothing (the reference does, unused)
    assert torch.equal(g.get_state(), before)


def test_config_round_trips_and_crosses_classes(tmp_path):
    s = Euler(**SD, use_karras_sigmas=True, timestep_spacing="trailing", prediction_type="v_prediction")
    s.save_config(str(tmp_path / "e"))
    with open(tmp_path / "e" / "scheduler_config.json") as f:
        saved = json.load(f)
    assert saved["_class_name"] == "EulerDiscreteScheduler" and saved["use_karras_sigmas"] is True and saved["timestep_spacing"] == "trailing"
    assert set(saved) - {"_class_name", "_diffusers_version"} == set(Euler._defaults)
    back = Euler.from_pretrained(str(tmp_path / "e"))
    pub = lambda c: {k: v for k, v in dict(c).items() if not k.startswith("_")}
    assert pub(back.config) == pub(s.config)
    a = EulerA(**SD, steps_offset=1, timestep_spacing="leading")
    a.save_config(str(tmp_path / "a"))
    with open(tmp_path / "a" / "scheduler_config.json") as f:
        saved = json.load(f)
    assert saved["_class_name"] == "EulerAncestralDiscreteScheduler" and set(saved) - {"_class_name", "_diffusers_version"} == set(EulerA._defaults)
    assert pub(EulerA.from_pretrained(str(tmp_path / "a")).config) == pub(a.config)
    # from the checkpoint's PNDM config: foreign keys dropped, what PNDM set explicitly kept (leading, steps_offset 1)
    for cls in (Euler, EulerA):
        d = cls.from_config(PNDMScheduler(**SD, steps_offset=1, skip_prk_steps=True).config)      # (its spacing left at PNDM's default)
        assert d.config["steps_offset"] == 1 and d.config["beta_schedule"] == "scaled_linear" and d.config["timestep_spacing"] == "linspace"
        assert "skip_prk_steps" not in d.config and "set_alpha_to_one" not in d.config
        p = cls.from_config(_pndm_config())
        assert p.config["timestep_spacing"] == "leading" and p.config["steps_offset"] == 1
        p.set_timesteps(10)
        assert p.init_noise_sigma == float(torch.sqrt(p.sigmas.max() ** 2 + 1)) and p.timesteps.tolist() == [float(t) for t in range(901, 0, -100)]
    d2 = Euler.from_config(DDIMScheduler(**SD, clip_sample=False, timestep_spacing="trailing").config)
    assert d2.config["timestep_spacing"] == "trailing" and "clip_sample" not in d2.config
    assert "use_karras_sigmas" not in EulerA.from_config(s.config).config and EulerA.from_config(s.config).config["prediction_type"] == "v_prediction"
    back2 = Euler.from_config(EulerA.from_config(s.config).config)
    assert back2.config["use_karras_sigmas"] is False and back2.config["timestep_spacing"] == "trailing"
    u = UniPCMultistepScheduler.from_config(Euler.from_config(_pndm_config()).config)       # and onward
    assert u.config["steps_offset"] == 1 and u.config["solver_order"] == 2


def _stub_pipe(cls, sched):
    from reflecting_reality_amd.pipeline import StableDiffusionBrushNetPipeline as Pipe, StableDiffusionXLBrushNetPipeline as PipeXL
    if cls == "xl":
        return PipeXL, PipeXL(vae=_Stub(), text_encoder=None, text_encoder_2=None, tokenizer=None, tokenizer_2=None, unet=_Stub(),
                              brushnet=_Stub(), scheduler=sched)
    return Pipe, Pipe(vae=_Stub(), text_encoder=None, tokenizer=None, unet=_Stub(), brushnet=_Stub(), scheduler=sched, safety_checker=None,
                      feature_extractor=None, requires_safety_checker=False, depth_conditioning_mode="concat")


@pytest.mark.parametrize("which", ["sd15", "xl"])
@pytest.mark.parametrize("cls", [Euler, EulerA], ids=lambda c: c.__name__)
def test_the_pipelines_load_a_directory_that_names_the_class(cls, which, tmp_path):
    """A pipeline directory whose scheduler/scheduler_config.json names an Euler class (SDXL base checkpoints do) loads through
    from_pretrained: NotImplementedError("scheduler ... is outside the MirrorFusion path") before the classes existed.  The three
    networks are stand-ins: only the scheduler's round trip is under test."""
    import reflecting_reality_amd as pkg
    from reflecting_reality_amd.compat import diffusers as compat
    name = cls.__name__
    assert getattr(pkg, name) is cls and getattr(compat, name) is cls
    sched = cls(**SD, steps_offset=1, timestep_spacing="leading") if cls is EulerA else cls(**SD, steps_offset=1, timestep_spacing="leading",
                                                                                             use_karras_sigmas=True)
    Pipe, pipe = _stub_pipe(which, sched)
    assert name in Pipe._scheduler_classes
    pipe.save_pretrained(str(tmp_path))
    with open(tmp_path / "model_index.json") as f:
        assert json.load(f)["scheduler"] == ["diffusers", name]
    with open(tmp_path / "scheduler" / "scheduler_config.json") as f:
        assert json.load(f)["_class_name"] == name
    sentinel = _Stub()
    back = Pipe.from_pretrained(str(tmp_path), vae=_Stub(), unet=_Stub(), brushnet=sentinel, device="cpu")
    assert type(back) is Pipe and type(back.scheduler) is cls and back.brushnet is sentinel
    assert {k: v for k, v in dict(back.scheduler.config).items() if not k.startswith("_")} == \
        {k: v for k, v in dict(sched.config).items() if not k.startswith("_")}
    back.scheduler.set_timesteps(7)
    sched.set_timesteps(7)
    assert torch.equal(back.scheduler.sigmas, sched.sigmas) and torch.equal(back.scheduler.timesteps, sched.timesteps)
    assert back.scheduler.init_noise_sigma == sched.init_noise_sigma > 1.0


def test_export_call_refuses_the_class_before_writing(tmp_path):
    _, pipe = _stub_pipe("sd15", Euler(**SD))
    with pytest.raises(NotImplementedError, match="EulerDiscreteScheduler"):
        pipe.export_call(str(tmp_path / "call"))
    assert not os.path.exists(tmp_path / "call")
