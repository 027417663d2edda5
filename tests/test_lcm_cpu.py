"""LCMScheduler, the guidance-scale embedding and the pipeline's LCM plumbing without a GPU: the integer schedules and the steps against
the reference's recordings (tests/golden/lcm.npz, tools/make_golden_lcm.py), the device plan against the scheduler's own step() through
the numpy row interpreter of test_dpmsolver_cpu.py / test_sched_plan_cpu.py (hip.axpby_n and the kernel's ops are ONE fp32 routine
there, so the two agree bit for bit), the refusals, the config round trips and the kernels' compile-time resources.

The bound against the reference: per prediction type and PER STEP, ENVELOPE_K = 4 x the reference's OWN fp32 deviation,
max |ref32 - ref64| / (1 + |ref64|) (lcm_envelope.json "fp32", whose "_about" gives the reason, that of tests/test_dpmsolver_cpu.py and
tests/test_euler_cpu.py), for `prev_sample` and for `denoised`.  Ratios reached (printed by the test, written into
profiles/lcm_bench.txt): v_prediction and sample 0.99 .. 1.00 (the reference's own two operations); epsilon prev_sample 1.63 .. 2.83,
denoised 1.63 .. 3.82: there the folded coefficients of sample and model output are +-1 / sqrt(alpha_t), up to 15 at t = 999, and cancel,
where the reference subtracts first and divides after."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from reflecting_reality_amd import hip, schedulers
from reflecting_reality_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, LCMScheduler, PNDMScheduler,
                                               UniPCMultistepScheduler, device_plan)
from test_dpmsolver_cpu import ENVELOPE_K, _Stub, _run_noise_row
from test_sched_plan_cpu import _cfg, _check_rows, _rows, _run_row, _same, numpy_hip  # noqa: F401  (numpy_hip: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SD = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SHAPE = (2, 4, 8, 8)
STEPS = 4
PREDICTIONS = ("epsilon", "v_prediction", "sample")
SCHEDULES = [(n, o, s) for n in (1, 2, 4, 8) for o in (50, 25) for s in (1.0, 0.5)]
CUSTOM = [999, 759, 499, 259]
W = (0.0, 0.5, 6.5)
# (tools/make_golden_lcm.py RAISES: the inputs for which the reference raises)
RAISES = {
    "neither": dict(),
    "both": dict(num_inference_steps=4, timesteps=CUSTOM),
    "original_above_train": dict(num_inference_steps=4, original_inference_steps=2000),
    "steps_above_train": dict(num_inference_steps=1001),
    "steps_above_original": dict(num_inference_steps=60),
    "steps_above_original_x_strength": dict(num_inference_steps=30, strength=0.5),
    "custom_ascending": dict(timesteps=[999, 499, 759, 259]),
    "custom_repeated": dict(timesteps=[999, 499, 499]),
    "custom_past_train": dict(timesteps=[1000, 499]),
}
assert ENVELOPE_K == 4.0
_cache = {}


def trace_inputs():
    """The inputs tools/make_golden_lcm.py fed the reference: ONE np.random.default_rng(7), prediction types in table order; per type
    the start sample, 4 model outputs, 4 noises (the last step reads none)."""
    if "inputs" not in _cache:
        rng = np.random.default_rng(7)
        out = {}
        for p in PREDICTIONS:
            x0 = rng.standard_normal(SHAPE, dtype=np.float32)
            mos = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(STEPS)]
            noises = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(STEPS)]
            out[p] = (x0, mos, noises)
        _cache["inputs"] = out
    return _cache["inputs"]


def golden():
    if "gold" not in _cache:
        with np.load(os.path.join(GOLD, "lcm.npz")) as z:
            _cache["gold"] = {k: z[k] for k in z.files}
        with open(os.path.join(GOLD, "lcm_envelope.json")) as f:
            _cache["env"] = json.load(f)
    return _cache["gold"], _cache["env"]


# ---- timesteps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, orig, strength", SCHEDULES)
def test_the_schedule_equals_the_reference(n, orig, strength):
    G, _ = golden()
    s = LCMScheduler(**SD)
    s.set_timesteps(n, original_inference_steps=orig, strength=strength)
    want = G[f"ts/{n}_{orig}_{strength}"]
    assert s.timesteps.dtype == torch.int64 and want.dtype == np.int64 and np.array_equal(s.timesteps.numpy(), want)
    assert s.num_inference_steps == n and s.step_index is None and s.begin_index is None and s.order == 1 and s.init_noise_sigma == 1.0
    assert not s.custom_timesteps
    if orig == 50:                                     # the config's own original_inference_steps is the default
        d = LCMScheduler(**SD)
        d.set_timesteps(n, strength=strength)
        assert torch.equal(d.timesteps, s.timesteps)


def test_custom_timesteps_equal_the_reference():
    G, _ = golden()
    s = LCMScheduler(**SD)
    s.set_timesteps(timesteps=list(CUSTOM))
    assert np.array_equal(s.timesteps.numpy(), G["ts/custom"]) and s.timesteps.tolist() == CUSTOM and s.timesteps.dtype == torch.int64
    assert s.num_inference_steps == 4 and s.custom_timesteps
    s.set_timesteps(timesteps=list(CUSTOM), strength=0.5)
    assert np.array_equal(s.timesteps.numpy(), G["ts/custom_half"]) and len(s.timesteps) == 2


@pytest.mark.parametrize("name", list(RAISES))
def test_set_timesteps_raises_where_the_reference_does(name):
    G, _ = golden()
    assert str(G[f"raises/{name}"]) == "ValueError"
    with pytest.raises(ValueError):
        LCMScheduler(**SD).set_timesteps(**RAISES[name])


# ---- steps -----------------------------------------------------------------------------------------------------------------------------
def _host_steps(s, x0, mos, noises):
    x, prevs, dens = torch.from_numpy(x0.copy()), [], []
    for k, t in enumerate(s.timesteps):
        x, den = s.step(torch.from_numpy(mos[k].copy()), t, x, variance_noise=torch.from_numpy(noises[k].copy()), return_dict=False)
        prevs.append(x)
        dens.append(den)
    return prevs, dens


@pytest.mark.parametrize("p", PREDICTIONS)
def test_host_step_stays_inside_the_reference_fp32_envelope(numpy_hip, p):
    G, env = golden()
    x0, mos, noises = trace_inputs()[p]
    s = LCMScheduler(**SD, prediction_type=p)
    s.set_timesteps(STEPS)
    assert np.array_equal(s.timesteps.numpy(), G[f"trace/{p}/timesteps"])
    prevs, dens = _host_steps(s, x0, mos, noises)
    failures = []
    for what, got, ref, devs in (("prev_sample", prevs, G[f"trace/{p}/ref64"], env["fp32"][p]),
                                 ("denoised", dens, G[f"trace/{p}/den64"], env["fp32"][f"{p}/denoised"])):
        got = torch.stack(got).numpy().astype(np.float64)
        assert ref.dtype == np.float64 and got.shape == ref.shape and len(devs) == STEPS
        for k in range(STEPS):
            err = (np.abs(got[k] - ref[k]) / (1 + np.abs(ref[k]))).max()
            print(f"{p} step {k} {what}: err {err:.3e}, the reference's fp32 deviation {devs[k]:.3e}, ratio {err / devs[k]:.2f}")
            if not err <= ENVELOPE_K * devs[k]:
                failures.append(f"{p} step {k} {what}: {err:.3e} > {ENVELOPE_K} x {devs[k]:.3e}")
    assert not failures, failures
    assert s.step_index == STEPS
    assert prevs[-1] is dens[-1], "the last step returns `denoised` as `prev_sample`"
    out = LCMScheduler(**SD, prediction_type=p)
    out.set_timesteps(STEPS)
    o = out.step(torch.from_numpy(mos[0].copy()), out.timesteps[0], torch.from_numpy(x0.copy()), variance_noise=torch.from_numpy(noises[0].copy()))
    assert isinstance(o, schedulers.LCMSchedulerOutput) and torch.equal(o.prev_sample, prevs[0]) and torch.equal(o.denoised, dens[0])


def test_the_recorded_fp32_deviation_is_that_of_the_recorded_traces():
    G, env = golden()
    for p in PREDICTIONS:
        for k64, k32, name in (("ref64", "ref32", p), ("den64", "den32", f"{p}/denoised")):
            r64, r32 = G[f"trace/{p}/{k64}"], G[f"trace/{p}/{k32}"]
            assert r32.dtype == np.float32 and r64.dtype == np.float64
            for k in range(STEPS):
                dev = (np.abs(r32[k].astype(np.float64) - r64[k]) / (1 + np.abs(r64[k]))).max()
                assert dev == pytest.approx(env["fp32"][name][k], rel=1e-12) and 1e-9 < dev < 1e-5
    assert "ENVELOPE_K = 4" in env["_about"]


def test_the_last_step_draws_nothing_and_the_others_draw_once(numpy_hip):
    s = LCMScheduler(**SD)
    s.set_timesteps(3)
    x, g = torch.ones(SHAPE), torch.Generator().manual_seed(1)
    for k, t in enumerate(s.timesteps):
        before = g.get_state().clone()
        prev, den = s.step(x, t, x, generator=g, return_dict=False)
        assert torch.equal(g.get_state(), before) == (k == 2)
    assert prev is den
    one = LCMScheduler(**SD)
    one.set_timesteps(1)                               # one-step sampling: no noise at all (:580)
    before = g.get_state().clone()
    prev, den = one.step(x, one.timesteps[0], x, generator=g, return_dict=False)
    assert prev is den and torch.equal(g.get_state(), before)


def test_step_index_begin_index_scale_model_input_and_the_refusals(numpy_hip):
    z = torch.zeros(SHAPE)
    s = LCMScheduler(**SD)
    with pytest.raises(ValueError, match="set_timesteps"):
        s.step(z, 999, z)
    with pytest.raises(NotImplementedError, match="add_noise"):
        s.add_noise(z, z, torch.tensor([1]))
    s.set_timesteps(4)
    assert s.scale_model_input(z, s.timesteps[0]) is z and s.step_index is None
    s.step(z, s.timesteps[0], z, variance_noise=z)
    assert s.step_index == 1
    s.set_timesteps(4)
    assert s.step_index is None
    s.set_begin_index(2)
    assert s.begin_index == 2
    s.step(z, s.timesteps[2], z, variance_noise=z)
    assert s.step_index == 3
    c_skip, c_out = s.get_scalings_for_boundary_condition_discrete(0)
    assert c_skip == 1.0 and c_out == 0.0              # the boundary condition: f(x, 0) = x


@pytest.mark.parametrize("kw, word", [(dict(thresholding=True), "thresholding"), (dict(clip_sample=True), "clip_sample"),
                                      (dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr")])
def test_refused_options_raise_by_name(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        LCMScheduler(**SD, **kw)
    with pytest.raises(ValueError):
        LCMScheduler(**SD, prediction_type="nonsense")


# ---- the device plan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [True, False], ids=["eps_c given", "no guidance"])
@pytest.mark.parametrize("p", PREDICTIONS)
def test_plan_equals_the_host_steps(numpy_hip, p, guided):
    """Every row through the numpy interpreter against the host's step(), the latents bit for bit after every step, then finish().
    Register 0 is the guided combination of (eps_u, eps_c) as the kernel forms it, or eps_u as loaded (g < 0)."""
    x0, mos, noises = trace_inputs()[p]
    mk = lambda: LCMScheduler(**SD, prediction_type=p)
    host, dev = mk(), mk()
    host.set_timesteps(STEPS)
    dev.set_timesteps(STEPS)
    plan = device_plan(dev)
    assert dev.step_index is None and plan.steps == STEPS and plan.x_slot == -1 and plan.first_scale == 1.0
    assert plan.nslots == 0 and plan.noise_reg == 2 and plan.draws == [True, True, True, False]
    rows = _rows(plan)
    _check_rows(plan, rows)
    lat_h, lat_d = torch.from_numpy(x0.copy()), x0.copy()
    state = np.full((1,) + SHAPE, np.nan, dtype=np.float32)
    written = set()
    rng = np.random.default_rng(11)
    for k in range(STEPS):
        if guided:
            eu, ec = mos[k], rng.standard_normal(SHAPE, dtype=np.float32)
            e = _cfg(eu, ec, 1.5)
        else:
            e = mos[k]
        lat_h = host.step(torch.from_numpy(e.copy()), host.timesteps[k], lat_h, variance_noise=torch.from_numpy(noises[k].copy()),
                          return_dict=False)[0]
        reads = [rows[k].ops[j].src[i] for j in range(rows[k].nops) for i in range(max(rows[k].ops[j].nterms, 1))]
        if k < STEPS - 1:
            assert plan.noise_reg in reads
            lat_d = _run_noise_row(rows[k], e, lat_d, state, written, plan.noise_reg, noises[k])
        else:                                          # the last row must not read the noise register: run it with that register EMPTY
            assert plan.noise_reg not in reads
            lat_d = _run_row(rows[k], e, lat_d, state, written)
        assert np.array_equal(lat_h.numpy().view(np.int32), lat_d.view(np.int32)), f"step {k}: the plan's latents differ"
        assert rows[k].load == 1 << 1 and rows[k].store == 1 << 1 and not written
    assert rows[-1].nops == 1 and all(r.nops == 2 for r in rows[:-1])
    plan.finish(dev, torch.from_numpy(state))
    assert set(vars(dev)) == set(vars(host))
    for key in vars(host):
        _same(getattr(dev, key), getattr(host, key), f"LCMScheduler.{key} after {STEPS} steps")


def test_a_partial_plan_and_the_other_plans_draw_columns(numpy_hip):
    s = LCMScheduler(**SD)
    s.set_timesteps(8)
    plan = device_plan(s, steps=3)
    assert plan.rows.shape[0] == 3 and plan.draws == [True] * 3
    d = DPMSolverMultistepScheduler(**SD, algorithm_type="sde-dpmsolver++")
    d.set_timesteps(5)
    assert device_plan(d).draws == [True] * 5          # (the SDE type reads its noise at every step, with a zero coefficient at the last)
    u = UniPCMultistepScheduler(**SD)
    u.set_timesteps(5)
    assert device_plan(u).draws == [False] * 5 and device_plan(u).noise_reg == -1


# ---- the embedding ---------------------------------------------------------------------------------------------------------------------
def _stub_pipe(sched, unet_cfg=None):
    from reflecting_reality_amd.pipeline import StableDiffusionBrushNetPipeline as Pipe
    unet = _Stub()
    if unet_cfg is not None:
        unet = type("U", (_Stub,), dict(config=_Stub._Config(block_out_channels=(8, 8), **unet_cfg)))()
    return Pipe, Pipe(vae=_Stub(), text_encoder=None, tokenizer=None, unet=unet, brushnet=_Stub(), scheduler=sched, safety_checker=None,
                      feature_extractor=None, requires_safety_checker=False, depth_conditioning_mode="concat")


@pytest.mark.parametrize("dim", [32, 33, 256])
def test_the_guidance_scale_embedding_equals_the_reference(dim):
    G, _ = golden()
    _, pipe = _stub_pipe(LCMScheduler(**SD))
    emb = pipe.get_guidance_scale_embedding(torch.tensor(W), embedding_dim=dim)
    want = G[f"emb/{dim}"]
    assert emb.dtype == torch.float32 and tuple(emb.shape) == want.shape == (3, dim)
    # torch's float32 exp differs in its last bits between CPU vector paths (the recording machine's and this one's may be different
    # ones): 2 ulp of a frequency <= 1 times the largest argument, 1000 * max(W), moves the angle, and so sin / cos, by at most this
    tol = 2 * 2.0 ** -23 * 1000 * max(W) + 2 * 2.0 ** -23
    assert tol < 1.6e-3 and np.abs(emb.numpy().astype(np.float64) - want).max() <= tol
    if dim % 2:
        assert torch.all(emb[:, -1] == 0) and np.all(want[:, -1] == 0)
    assert torch.all(emb[0, :dim // 2] == 0) and torch.all(emb[0, dim // 2:2 * (dim // 2)] == 1)     # w = 0: sin 0, cos 0


# ---- config, registration, the pipeline's rules ----------------------------------------------------------------------------------------
def test_config_round_trips_and_crosses_classes(tmp_path):
    pub = lambda c: {k: v for k, v in dict(c).items() if not k.startswith("_")}
    d = LCMScheduler()
    assert pub(d.config) == dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None,
                                 original_inference_steps=50, clip_sample=False, clip_sample_range=1.0, set_alpha_to_one=True, steps_offset=0,
                                 prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                                 timestep_spacing="leading", timestep_scaling=10.0, rescale_betas_zero_snr=False)
    s = LCMScheduler(**SD, original_inference_steps=25, prediction_type="v_prediction", timestep_scaling=5.0)
    s.save_config(str(tmp_path / "l"))
    with open(tmp_path / "l" / "scheduler_config.json") as f:
        saved = json.load(f)
    assert saved["_class_name"] == "LCMScheduler" and saved["original_inference_steps"] == 25 and saved["timestep_scaling"] == 5.0
    assert set(saved) - {"_class_name", "_diffusers_version"} == set(LCMScheduler._defaults)
    back = LCMScheduler.from_pretrained(str(tmp_path / "l"))
    assert pub(back.config) == pub(s.config)
    back.set_timesteps(4)
    s.set_timesteps(4)
    assert torch.equal(back.timesteps, s.timesteps) and s.timesteps.tolist() == [999, 759, 519, 279]     # (k = 40: indices 0, 6, 12, 18 from 999 down)
    # the swap of INTEGRATION.md: from the pipeline's DDIM / PNDM config, foreign keys dropped, explicit ones kept
    ddim = DDIMScheduler(**SD, clip_sample=False, set_alpha_to_one=False, steps_offset=1)
    lcm = LCMScheduler.from_config(ddim.config)
    assert lcm.config["clip_sample"] is False and lcm.config["steps_offset"] == 1 and lcm.config["set_alpha_to_one"] is False
    assert lcm.config["original_inference_steps"] == 50 and lcm.config["timestep_scaling"] == 10.0 and lcm.config["beta_schedule"] == "scaled_linear"
    with pytest.raises(NotImplementedError, match="clip_sample"):
        LCMScheduler.from_config(DDIMScheduler(**SD, clip_sample=True).config)       # (set explicitly there: it crosses, and is refused)
    p = LCMScheduler.from_config(PNDMScheduler(**SD, steps_offset=1, skip_prk_steps=True).config)
    assert "skip_prk_steps" not in p.config and p.config["steps_offset"] == 1
    assert UniPCMultistepScheduler.from_config(lcm.config).config["steps_offset"] == 1


def test_the_pipeline_loads_a_directory_that_names_the_class(tmp_path):
    import reflecting_reality_amd as pkg
    from reflecting_reality_amd.compat import diffusers as compat
    assert pkg.LCMScheduler is LCMScheduler and compat.LCMScheduler is LCMScheduler
    sched = LCMScheduler(**SD, original_inference_steps=25)
    Pipe, pipe = _stub_pipe(sched)
    assert "LCMScheduler" in Pipe._scheduler_classes
    pipe.save_pretrained(str(tmp_path))
    with open(tmp_path / "scheduler" / "scheduler_config.json") as f:
        assert json.load(f)["_class_name"] == "LCMScheduler"
    back = Pipe.from_pretrained(str(tmp_path), vae=_Stub(), unet=_Stub(), brushnet=_Stub(), device="cpu")
    assert type(back.scheduler) is LCMScheduler and back.scheduler.config["original_inference_steps"] == 25


def test_classifier_free_guidance_is_off_for_a_guidance_distilled_unet():
    _, plain = _stub_pipe(LCMScheduler(**SD))
    _, distilled = _stub_pipe(LCMScheduler(**SD), dict(time_cond_proj_dim=256))
    _, none = _stub_pipe(LCMScheduler(**SD), dict(time_cond_proj_dim=None))
    for g, want in ((7.5, True), (1.5, True), (1.0, False), (0.0, False)):
        plain._guidance_scale = distilled._guidance_scale = none._guidance_scale = g
        assert plain.do_classifier_free_guidance is want and none.do_classifier_free_guidance is want
        assert distilled.do_classifier_free_guidance is False


def test_custom_timesteps_under_ddim_raise_todays_error():
    _, pipe = _stub_pipe(DDIMScheduler(**SD, clip_sample=False))
    img = torch.rand(1, 3, 16, 16)
    with pytest.raises(ValueError) as e:
        pipe(prompt_embeds=torch.zeros(1, 77, 32), negative_prompt_embeds=torch.zeros(1, 77, 32), image=img, mask=img[:, :1],
             depth=img[:, :1], timesteps=[900, 500, 100], output_type="latent", height=16, width=16)
    assert str(e.value) == (f"The current scheduler class {DDIMScheduler}'s `set_timesteps` does not support custom"
                            f" timestep schedules. Please check whether you are using the correct scheduler.")


def test_the_exports_refuse_an_unguided_call_before_writing(tmp_path):
    from reflecting_reality_amd.models import UNet2DConditionModel
    from reflecting_reality_amd import configs
    _, pipe = _stub_pipe(LCMScheduler(**SD))
    with pytest.raises(NotImplementedError, match="classifier-free guidance"):
        pipe.export_call(str(tmp_path / "call"), guidance_scale=1.0)
    _, distilled = _stub_pipe(LCMScheduler(**SD), dict(time_cond_proj_dim=32))
    with pytest.raises(NotImplementedError, match="time_cond_proj_dim"):
        distilled.export_call(str(tmp_path / "call"), guidance_scale=7.5)
    assert not os.path.exists(tmp_path / "call")
    u = UNet2DConditionModel(dict(configs.TINY_UNET, time_cond_proj_dim=32), device="cpu")
    shapes = u.param_shapes()
    assert shapes["time_embedding.cond_proj.weight"] == (configs.TINY_UNET["block_out_channels"][0], 32)
    assert "time_embedding.cond_proj.bias" not in shapes
    assert "time_embedding.cond_proj.weight" not in UNet2DConditionModel(dict(configs.TINY_UNET), device="cpu").param_shapes()


# ---- the kernels' resources ------------------------------------------------------------------------------------------------------------
def test_the_unguided_kernels_build_without_scratch_and_the_guided_ones_keep_their_registers(tmp_path):
    """The four instantiations compile for gfx950 with 0 bytes of scratch; the guided ones report the VGPRs they had before the
    compile-time form existed (75 and 106, profiles/lcm_bench.txt); the unguided ones need no more."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    from reflecting_reality_amd import _build
    res = subprocess.run([hipcc, *_build.HIPCC_FLAGS, "--cuda-device-only", "-c", os.path.join(_build.CSRC, "elementwise.hip"),
                          "-o", str(tmp_path / "e.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    info = {}
    for block in res.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        m = re.match(r"_ZN12_GLOBAL__N_1\d+(sched_step(?:_noise)?_kernel)ILb([01])E", name)
        if m:
            info[(m.group(1), m.group(2) == "1")] = {k: int(v) for k, v in re.findall(r"remark:\s+(\w+)(?: \[bytes/lane\])?: (\d+) \[", block)}
    print(info)
    assert set(info) == {("sched_step_kernel", True), ("sched_step_kernel", False), ("sched_step_noise_kernel", True),
                         ("sched_step_noise_kernel", False)}
    assert all(v["ScratchSize"] == 0 for v in info.values())
    assert info[("sched_step_kernel", True)]["VGPRs"] == 75 and info[("sched_step_noise_kernel", True)]["VGPRs"] == 106
    assert info[("sched_step_kernel", False)]["VGPRs"] <= 75 and info[("sched_step_noise_kernel", False)]["VGPRs"] <= 106
