"""Euler / Euler-ancestral on the device: the plan's rows through mf_sched_step_dev / mf_sched_step_noise_dev against the host schedulers'
own step() and scale_model_input, the pipeline's captured step (device update and host step) against its eager loop, the pipeline against
the reference's recorded results (tests/golden/euler.npz, tools/make_golden_euler.py), the step programs of both classes, and the XL
pipeline.  Bit-exactness everywhere but against the reference, where the project's latent bound (PREC_TOL) and the reference's own bf16 /
fp16 envelopes hold.

The invariant under test: under a captured graph the static latents buffer holds the MODEL INPUT, sample / sqrt(sigma_i^2 + 1) of the step
about to run; the sample is the update object's (a slot of the plan's state, or a tensor of the host step), and no step-dependent factor is
a constant of the capture."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import util  # noqa: E402
from reflecting_reality_amd import (DDIMScheduler, EulerAncestralDiscreteScheduler as EulerA, EulerDiscreteScheduler as Euler,  # noqa: E402
                                    PNDMScheduler, StableDiffusionXLBrushNetPipeline, hip, program, synth)
from reflecting_reality_amd.pipeline import StableDiffusionBrushNetPipeline  # noqa: E402
from reflecting_reality_amd.rng import PhiloxGenerator  # noqa: E402
from reflecting_reality_amd.schedulers import device_plan  # noqa: E402
from test_euler_cpu import assert_timesteps  # noqa: E402
from test_models_gpu import build  # noqa: E402
from test_pipeline_gpu import PREC_TOL, SD_SCHED, _run, _tiny_pipe  # noqa: E402
from test_program_gpu import _call_args  # noqa: E402
from test_sched_device_gpu import _grab_steps  # noqa: E402
from test_xl_gpu import build_xl  # noqa: E402
from util import check, golden  # noqa: E402

DEV = "cuda"
SD = {k: v for k, v in SD_SCHED.items() if k not in ("steps_offset", "set_alpha_to_one")}


def _pndm_config():
    """The checkpoint's scheduler as its scheduler_config.json states it (the spacing an explicit key, so it crosses classes)."""
    return PNDMScheduler(**SD_SCHED, skip_prk_steps=True, timestep_spacing="leading").config


KERNEL_CASES = {
    "from_pndm": lambda: Euler.from_config(_pndm_config()),
    "linspace_karras": lambda: Euler(**SD, use_karras_sigmas=True),
    "a_from_pndm": lambda: EulerA.from_config(_pndm_config()),
    "a_linspace_karras": lambda: EulerA.from_config(Euler(**SD, use_karras_sigmas=True).config),
}


def _same_counters(got, want, what):
    assert got.step_index == want.step_index and got.begin_index == want.begin_index, f"{what}: step_index {got.step_index} != {want.step_index}"
    assert got.model_input_prescaled is False and want.model_input_prescaled is False, what
    assert torch.equal(got.sigmas, want.sigmas) and torch.equal(got.timesteps, want.timesteps) and got.init_noise_sigma == want.init_noise_sigma


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_walks_every_row_like_the_host_scheduler(name):
    """10 steps at 4 x 4 x 16 x 16: after every row the latents (the next step's model input) and the slot (the sample) are bitwise
    hip.cfg_combine + the scheduler's own mf_axpby_n launches (and, ancestral, its PhiloxGenerator draw); state and offsets after."""
    mk = KERNEL_CASES[name]
    host, full = mk(), mk()
    host.set_timesteps(10)
    full.set_timesteps(10)
    ts = host.timesteps
    plan = device_plan(full)
    anc = name.startswith("a_")
    assert (plan.noise_reg >= 2 + plan.nslots) == anc and plan.x_slot == 0 and plan.nslots == 1
    rows = plan.rows.to(DEV)
    gen = torch.Generator().manual_seed(11)
    shape = (4, 4, 16, 16)
    x_h = hip.axpby_n([torch.randn(shape, generator=gen).to(DEV)], [host.init_noise_sigma])
    state = torch.full((plan.nslots,) + shape, float("nan"), device=DEV)
    state[plan.x_slot].copy_(x_h)                                     # the documented start of a run
    lat_d = hip.axpby_n([state[plan.x_slot]], [plan.first_scale])
    assert torch.equal(lat_d, host.scale_model_input(x_h, ts[0]))
    g_host, g_dev = PhiloxGenerator(5, DEV), PhiloxGenerator(5, DEV)
    rng_state = g_dev.device_state()
    blocks = hip.philox_normal_blocks(shape[0], x_h[0].numel())
    g = 7.5
    for k in range(len(ts)):
        eu, ec = torch.randn(shape, generator=gen).to(DEV), torch.randn(shape, generator=gen).to(DEV)
        x_h = host.step(hip.cfg_combine(eu, ec, g), ts[k], x_h, generator=g_host, return_dict=False)[0]
        lat_h = hip.axpby_n([x_h], [host._input_scale(host.step_index)])
        if anc:
            hip.sched_step_noise_dev(eu, ec, g, lat_d, state, rows[k].contiguous(), plan.noise_reg, rng_state=rng_state)
            hip.philox_advance(rng_state, blocks)
            g_dev.note_advanced(blocks, on_device=True)
        else:
            hip.sched_step_dev(eu, ec, g, lat_d, state, rows[k].contiguous())
        torch.cuda.synchronize()
        assert torch.isfinite(lat_d).all()
        assert torch.equal(state[plan.x_slot], x_h), f"{name}, step {k}: the sample differs by {(state[plan.x_slot] - x_h).abs().max()}"
        assert torch.equal(lat_d, lat_h), f"{name}, step {k}: the model input differs by {(lat_d - lat_h).abs().max()}"
    assert torch.equal(lat_d, x_h), "sigma 0 after the last step: the latents are the result"
    plan.finish(full, state)
    _same_counters(full, host, name)
    assert full.step_index == 10
    assert g_dev.offset == g_host.offset == (10 * blocks if anc else 0)
    assert rng_state.cpu().tolist() == [5, g_host.offset]


class _Log:
    """The library calls of the update, in order, with a mark where prepare_latents returned."""
    NAMES = ("mf_sched_step_dev", "mf_sched_step_noise_dev", "mf_philox_advance", "mf_axpby_n", "mf_cfg_combine", "mf_philox_normal")

    def __init__(self, monkeypatch, pipe):
        self.calls = []
        lib = hip.load()
        for name in self.NAMES:
            def wrap(*a, _fn=getattr(lib, name), _name=name):
                self.calls.append(_name)
                return _fn(*a)
            monkeypatch.setattr(lib, name, wrap)
        real = pipe.prepare_latents

        def prepared(*a, **k):
            out = real(*a, **k)
            self.calls.append("prepared")
            return out
        monkeypatch.setattr(pipe, "prepare_latents", prepared)

    def count(self, name, calls=None):
        return sum(1 for c in (self.calls if calls is None else calls) if c == name)


PIPE_CASES = {
    "euler": lambda: Euler.from_config(_pndm_config()),
    "euler_karras": lambda: Euler.from_config(_pndm_config(), use_karras_sigmas=True),
    "euler_a": lambda: EulerA.from_config(_pndm_config()),
}


def _pipe_inputs():
    return synth.pipeline_inputs(2, 16, 16, seed=17, cross_dim=32, vae_scale=2), torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(4))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(PIPE_CASES))
def test_tiny_pipeline_graph_with_the_device_update_equals_the_eager_loop(name, prec, monkeypatch):
    """use_hip_graph True / False: bitwise-equal latents, the scheduler in the host's end state, the same generator offset.  The graph
    path launches the update entry twice (its eager first step and the capture) and nothing else of the update's between the first and
    the last step; the one-off scaling of the first model input, between prepare_latents and the first step, is one mf_axpby_n."""
    pipe = _tiny_pipe(prec)
    inp, noise = _pipe_inputs()
    anc = name == "euler_a"
    gen = lambda: dict(generator=PhiloxGenerator(3, DEV)) if anc else {}
    pipe.scheduler = PIPE_CASES[name]()
    pipe.use_hip_graph, pipe._graph_state = False, None
    kw_h = gen()
    want = _run(pipe, inp, 6, 16, 16, noise, **kw_h)
    host = pipe.scheduler
    pipe.scheduler = PIPE_CASES[name]()
    pipe.use_hip_graph, pipe._graph_state = True, None
    log = _Log(monkeypatch, pipe)
    kw_d = gen()
    got = _run(pipe, inp, 6, 16, 16, noise, **kw_d)
    monkeypatch.undo()
    assert pipe._graph_state is not None and pipe._graph_state["graph"] is not None and "state" in pipe._graph_state
    new, old = ("mf_sched_step_noise_dev", "mf_sched_step_dev") if anc else ("mf_sched_step_dev", "mf_sched_step_noise_dev")
    assert log.count(new) == 2 and log.count(old) == 0 and log.count("mf_philox_advance") == (2 if anc else 0), log.calls
    at = log.calls.index("prepared")
    first = log.calls.index(new)
    assert at < first
    before, loop = log.calls[at + 1:first], log.calls[first:]
    assert before == ["mf_axpby_n"], f"the one-off model-input scaling is one launch: {before}"
    for entry in ("mf_axpby_n", "mf_cfg_combine", "mf_philox_normal"):
        assert log.count(entry, loop) == 0, log.calls
    assert torch.isfinite(got).all() and torch.equal(got, want), f"{name} [{prec}]: differs by {(got - want).abs().max()}"
    _same_counters(pipe.scheduler, host, f"{name} [{prec}]")
    assert pipe.scheduler.step_index == 6
    if anc:
        blocks = hip.philox_normal_blocks(2, 4 * 8 * 8)
        assert kw_d["generator"].offset == kw_h["generator"].offset == 6 * blocks
        assert kw_d["generator"].device_state().cpu().tolist() == [3, 6 * blocks]
    # a second call replays the kept graph from its first step (ancestral: the same generator object, seeded again): the same result
    pipe.scheduler = PIPE_CASES[name]()
    again = dict(generator=kw_d["generator"].manual_seed(3)) if anc else {}
    assert torch.equal(_run(pipe, inp, 6, 16, 16, noise, **again), want)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(PIPE_CASES))
def test_tiny_pipeline_graph_with_the_host_step_equals_the_eager_loop(name, prec):
    """A callback_on_step_end takes the host step under the graph.  Output and every tensor the callback saw are bitwise the eager loop's,
    and those tensors are the UNSCALED samples: six steps of `leading` spacing have six different sigmas, so a factor baked into the
    capture (that of step 1 replayed for steps 2..5) would show in every later step."""
    pipe = _tiny_pipe(prec)
    inp, noise = _pipe_inputs()
    runs = {}
    for graph in (False, True):
        pipe.scheduler = PIPE_CASES[name]()
        pipe.use_hip_graph, pipe._graph_state = graph, None
        seen = []
        kw = dict(generator=torch.Generator(DEV).manual_seed(9)) if name == "euler_a" else {}
        out = _run(pipe, inp, 6, 16, 16, noise, callback_on_step_end=lambda p, i, t, k: seen.append(k["latents"].float().cpu().clone()) or {}, **kw)
        runs[graph] = (out, seen, pipe.scheduler)
        if graph:
            assert "eps" in pipe._graph_state and "state" not in pipe._graph_state and pipe._graph_state["graph"] is not None
    (want, seen_h, host), (got, seen_g, sched) = runs[False], runs[True]
    assert len(seen_h) == len(seen_g) == 6
    for i, (a, b) in enumerate(zip(seen_g, seen_h)):
        assert torch.equal(a, b), f"{name} [{prec}], step {i}: the callback's latents differ by {(a - b).abs().max()}"
    assert torch.isfinite(got).all() and torch.equal(got, want) and torch.equal(got, seen_g[-1])
    _same_counters(sched, host, f"{name} [{prec}]")
    # (unscaled: the eager loop hands its callback what step() returned, and the graph's callback saw the same bits)
    assert len(set(host.sigmas.tolist())) == 7


def _euler_envelope(prec):
    """util.report_env reads `<prec>_envelope.json` through util's cache: the Euler cases' entries (euler_envelope.json, the reference's own
    bf16 / fp16 deviation on these very cases) join it under their own keys; util's multipliers stay as they are."""
    util.envelope("tiny_pipeline/ddim/image", prec)
    with open(os.path.join(util.GOLD, "euler_envelope.json")) as f:
        util._ENV[prec].update(json.load(f)[prec])


REF_CASES = {
    "euler": lambda: Euler.from_config(_pndm_config()),
    "euler_linspace_karras": lambda: Euler.from_config(_pndm_config(), timestep_spacing="linspace", use_karras_sigmas=True),
}


@pytest.mark.parametrize("prec,tol", PREC_TOL)
@pytest.mark.parametrize("name", list(REF_CASES))
def test_tiny_pipeline_per_step_against_the_reference(prec, tol, name):
    """test_dpmsolver_gpu.test_tiny_pipeline_per_step_against_the_reference for the two Euler cases of euler.npz (the second with fractional
    timesteps)."""
    if prec in ("bf16", "fp16"):
        _euler_envelope(prec)
    unet, bn, vae = build("tiny", prec)
    G = golden("euler.npz")
    pipe = StableDiffusionBrushNetPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, brushnet=bn, scheduler=REF_CASES[name](),
                                           safety_checker=None, feature_extractor=None, requires_safety_checker=False,
                                           depth_conditioning_mode="concat")
    pipe.set_progress_bar_config(disable=True)
    inp = synth.pipeline_inputs(1, 16, 16, seed=1234, cross_dim=32, vae_scale=2)
    noise = torch.from_numpy(G[f"{name}_vae_noise"])
    cond = pipe.build_conditioning(inp["image"], inp["mask"], inp["depth"], 16, 16, 1, 1, True, noise)
    check(f"conditioning[{prec}]", cond, G[f"{name}_cond"], prec, dict(atol=2e-4), f"euler/{name}/cond")
    trace = []
    res = pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"],
               mask=inp["mask"], depth=inp["depth"], num_inference_steps=4, guidance_scale=7.5, latents=inp["latents"].clone(),
               output_type="pt", brushnet_conditioning_scale=1.0,
               callback_on_step_end=lambda p, i, t, kw: trace.append(kw["latents"].clone()) or {}, height=16, width=16,
               conditioning_noise=noise)
    ts = G[f"{name}_timesteps"]
    assert_timesteps(pipe.scheduler.timesteps.numpy(), ts, karras=name.endswith("karras"))
    assert (name == "euler_linspace_karras") == bool(np.any(ts != np.round(ts)))
    assert len(trace) == 4
    for i in range(4):
        check(f"{name} latents step {i}[{prec}]", trace[i], torch.from_numpy(G[f"{name}_latents_{i}"]), prec, dict(atol=tol),
              f"euler/{name}/latents_{i}")
    check(f"{name} image[{prec}]", res.images, G[f"{name}_image"], prec, dict(atol=tol), f"euler/{name}/image")


@pytest.mark.parametrize("name", ["euler", "euler_a"])
def test_device_scheduler_program_replays_the_loop_bit_exactly(name, tmp_path):
    """export_denoise_step(..., scheduler="device") at 2 x 16 x 32, 4 steps.  Replayed from Python with the documented start (x0 into slot
    meta["sample_slot"] of sched_state, x0 * meta["first_input_scale"] into latents) it gives the pipeline's samples after every step,
    read from the slot, and its final latents; euler_a gives them again from a reset philox_state."""
    anc = name == "euler_a"
    pipe = _tiny_pipe("bf16")
    mk = PIPE_CASES[name]
    gen = lambda: dict(generator=PhiloxGenerator(3, DEV)) if anc else {}
    inp = synth.pipeline_inputs(2, 16, 32, seed=7, cross_dim=32, vae_scale=2)
    noise = torch.randn(4, 4, 8, 16, generator=torch.Generator().manual_seed(3))
    steps = 4
    pipe.scheduler = mk()
    per_step, ref = _grab_steps(pipe, _call_args(inp, steps, noise, **gen()))       # (a callback: the host's scheduler steps)
    sigma0 = pipe.scheduler.init_noise_sigma
    pipe.scheduler = mk()
    pipe._graph_state = None
    path = str(tmp_path / "step.mfprog")
    info = pipe.export_denoise_step(path, scheduler="device", **_call_args(inp, steps, noise, **gen()))
    assert torch.equal(info["result"].images.float().cpu(), ref), "the exporting run itself must give the host loop's latents"
    assert "mf_cfg_combine" not in info["entries"] and "mf_axpby_n" not in info["entries"] and "mf_philox_normal" not in info["entries"]
    assert type(pipe.scheduler).__name__ in info["meta"]["result"]
    n = len(per_step)
    prog = program.Program(path, DEV)
    meta = json.loads(prog.meta)
    slot, scale = meta["sample_slot"], meta["first_input_scale"]
    assert slot == 0 and scale == pipe.scheduler._input_scale(0) and 0 < scale < 1
    shape = per_step[0].shape
    tables = {nm[6:]: prog.buffer(nm) for nm in prog.names if nm.startswith("table.")}
    assert set(tables) == {"sched_row", "temb_unet", "temb_brushnet"}
    if anc:
        assert "mf_sched_step_noise_dev" in info["entries"] and "mf_philox_advance" in info["entries"] and "mf_sched_step_dev" not in info["entries"]
        blocks = hip.philox_normal_blocks(shape[0], shape[1] * shape[2] * shape[3])
        assert meta["philox"]["blocks_per_step"] == blocks and "philox_state" in prog.names
    else:
        assert "mf_sched_step_dev" in info["entries"] and "philox_state" not in prog.names
    lib = hip.load()
    x0 = hip.axpby_n([inp["latents"].float().contiguous().to(DEV)], [sigma0])
    numel = x0.numel()
    for replay in range(2 if anc else 1):
        state = prog.buffer("sched_state", torch.float32)
        state[slot * numel:(slot + 1) * numel].copy_(x0.reshape(-1))
        prog.buffer("latents", torch.float32).copy_(hip.axpby_n([x0], [scale]).reshape(-1))
        if anc:                                                # the generator's pair as the call found it: seed 3, nothing drawn
            prog.buffer("philox_state", torch.int64).copy_(torch.tensor([3, 0]))
        for i in range(n):
            for dst, tab in tables.items():
                prog.buffer(dst).copy_(tab.view(n, -1)[i])
            hip._check(lib.mf_denoise_step_fused(prog._h, None, None, None, None, hip._stream()), "mf_denoise_step_fused")
            torch.cuda.synchronize()
            got = prog.buffer("sched_state", torch.float32)[slot * numel:(slot + 1) * numel].view(shape).cpu()
            assert torch.equal(got, per_step[i]), f"{name}, replay {replay}, step {i}: differs by {(got - per_step[i]).abs().max()}"
        assert torch.equal(prog.buffer("latents", torch.float32).view(shape).cpu(), ref)
        if anc:
            assert prog.buffer("philox_state", torch.int64).cpu().tolist() == [3, n * blocks]
    prog.close()
    before = set(os.listdir(tmp_path))
    with pytest.raises(NotImplementedError, match=type(pipe.scheduler).__name__):
        pipe.export_call(str(tmp_path / "call"), **_call_args(inp, steps, noise))
    assert set(os.listdir(tmp_path)) == before, "export_call wrote something before refusing"
    if anc:                                                    # the kernel draws the library's stream only
        pipe.scheduler = mk()
        with pytest.raises(NotImplementedError, match="PhiloxGenerator"):
            pipe.export_denoise_step(path, scheduler="device", generator=torch.Generator(DEV).manual_seed(3), **_call_args(inp, steps, noise))


def test_xl_pipeline_under_euler_graph_equals_eager_and_denoising_end_counts_steps():
    """The SDXL pipeline under EulerDiscreteScheduler.from_config(its DDIM config), 3 steps: graph = eager bitwise, finite.  With
    denoising_end = 0.67 the loop runs exactly the timesteps at or above the cutoff, num_train * (1 - 0.67), and returns the sample."""
    unet, bn, vae = build_xl("fp32")
    ddim = DDIMScheduler(**SD_SCHED, clip_sample=False)
    pipe = StableDiffusionXLBrushNetPipeline(vae=vae, text_encoder=None, text_encoder_2=None, tokenizer=None, tokenizer_2=None,
                                             unet=unet, brushnet=bn, scheduler=Euler.from_config(ddim.config))
    pipe.set_progress_bar_config(disable=True)
    assert pipe.scheduler.config["steps_offset"] == 1 and pipe.scheduler.config["beta_schedule"] == "scaled_linear"
    inp = synth.pipeline_inputs(1, 16, 16, seed=99, cross_dim=48, vae_scale=2)
    gp = torch.Generator().manual_seed(100)
    pooled, npooled = torch.randn(1, 24, generator=gp), torch.randn(1, 24, generator=gp)
    kw = dict(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], pooled_prompt_embeds=pooled,
              negative_pooled_prompt_embeds=npooled, image=inp["image"], mask=inp["mask"], guidance_scale=5.0, output_type="latent",
              height=16, width=16, conditioning_noise=inp["vae_noise"])
    outs = []
    for graph in (True, False):
        pipe.use_hip_graph, pipe._graph_state = graph, None
        outs.append(pipe(latents=inp["latents"].clone(), num_inference_steps=3, **kw).images.float().cpu())
        assert pipe.scheduler.step_index == 3
    assert pipe.scheduler.timesteps.dtype == torch.float32
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    full = Euler.from_config(ddim.config)
    full.set_timesteps(10)
    cutoff = int(round(1000 - 0.67 * 1000))
    expect = [float(t) for t in full.timesteps if float(t) >= cutoff]
    assert 0 < len(expect) < 10
    cut = {}
    for graph in (True, False):
        pipe.use_hip_graph, pipe._graph_state = graph, None
        seen = []
        cut[graph] = pipe(latents=inp["latents"].clone(), num_inference_steps=10, denoising_end=0.67,
                          callback_on_step_end=lambda p, i, t, k: seen.append(float(t)) or {}, **kw).images.float().cpu()
        assert seen == expect and pipe.scheduler.step_index == len(expect)
    assert torch.isfinite(cut[True]).all() and torch.equal(cut[True], cut[False])
    pipe.use_hip_graph, pipe._graph_state = True, None        # (and on the device plan, cut short: the sample, not the model input)
    assert torch.equal(pipe(latents=inp["latents"].clone(), num_inference_steps=10, denoising_end=0.67, **kw).images.float().cpu(), cut[False])
