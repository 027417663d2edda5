"""DPM-Solver++ on the device: mf_sched_step_noise_dev's noise against the library's stream, the plan's rows through the kernels against
the host scheduler's own step(), the pipeline's captured step against its host loop, the pipeline against the reference's recorded
results (tests/golden/dpmsolver.npz, tools/make_golden_dpmsolver.py), and the step programs of both types (from Python; the deterministic one from the C host too).  Bit-exactness
everywhere but against the reference, where the project's latent bound (1e-3) and the reference's own bf16 / fp16 envelopes hold."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import util  # noqa: E402
from reflecting_reality_amd import DPMSolverMultistepScheduler as DPM, PNDMScheduler, hip, program, synth  # noqa: E402
from reflecting_reality_amd.pipeline import StableDiffusionBrushNetPipeline  # noqa: E402
from reflecting_reality_amd.rng import PhiloxGenerator  # noqa: E402
from reflecting_reality_amd.schedulers import device_plan  # noqa: E402
from test_models_gpu import build  # noqa: E402
from test_pipeline_gpu import PREC_TOL, SD_SCHED, _run, _tiny_pipe  # noqa: E402
from test_program_gpu import _call_args  # noqa: E402
from test_sched_device_gpu import _assert_same_state, _c_host, _grab_steps  # noqa: E402
from util import check, golden  # noqa: E402

DEV = "cuda"
MF_EINVAL = -1                     # include/mfhip.h
SD = {k: v for k, v in SD_SCHED.items() if k not in ("steps_offset", "set_alpha_to_one")}


def _one_op_row(noise_reg, nslots=0):
    """latents = register noise_reg (a move), nothing loaded."""
    row = hip.SchedRow(nops=1, nslots=nslots, load=0, store=2)
    row.ops[0].dst, row.ops[0].nterms = 1, 0
    row.ops[0].src[0] = noise_reg
    return torch.frombuffer(bytearray(bytes(row)), dtype=torch.int32).clone().to(DEV)


@pytest.mark.parametrize("shape, first, total", [((3, 4, 8, 8), 1, 5), ((2, 4, 64, 64), 0, 2)])
def test_the_kernel_noise_is_the_library_stream(shape, first, total):
    """Sample boundaries and a shard in the middle of a draw (3 of 5 rows); more than one block and, with the grid capped at a few
    blocks per CU, whatever stride the loop takes at 2 x 4 x 64 x 64."""
    seed, offset, reg = 0x1234_5678_9ABC_DEF0, 77, 9
    row = _one_op_row(reg)
    zeros = torch.zeros(shape, device=DEV)
    per = zeros[0].numel()
    want = hip.philox_normal(shape, seed, offset, DEV, first_sample=first, global_batch=total)
    lat = torch.full(shape, float("nan"), device=DEV)
    hip.sched_step_noise_dev(zeros, zeros, 7.5, lat, None, row, reg, seed=seed, offset=offset, first_sample=first, global_batch=total)
    assert torch.equal(lat, want)
    # through a device state, two launches in a row with the advance between them: the second is the host draw at the advanced offset
    gen = PhiloxGenerator(seed, DEV).set_state((seed, offset))
    state = gen.device_state()
    blocks = hip.philox_normal_blocks(total, per)
    assert blocks == total * per // 4
    a, b = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
    for out in (a, b):
        hip.sched_step_noise_dev(zeros, zeros, 7.5, out, None, row, reg, seed=1, offset=2, first_sample=first, global_batch=total,
                                 rng_state=state)
        hip.philox_advance(state, blocks)
        gen.note_advanced(blocks, on_device=True)
    assert torch.equal(a, want)
    assert torch.equal(b, hip.philox_normal(shape, seed, offset + blocks, DEV, first_sample=first, global_batch=total))
    assert state.cpu().tolist() == [hip._s64(seed), offset + 2 * blocks] and gen.offset == offset + 2 * blocks


def test_the_entry_refuses_what_it_cannot_draw():
    z = torch.zeros(2, 3, 2, device=DEV)                      # per_sample = 6: n % 4 == 0 but a sample is no whole number of blocks
    assert z.numel() % 4 == 0
    with pytest.raises(hip.MfhipError, match="per_sample"):
        hip.sched_step_noise_dev(z, z, 1.0, z.clone(), None, _one_op_row(5), 5)
    ok = torch.zeros(2, 8, device=DEV)
    for reg in (1, hip.SCHED_MAX_REGS):
        with pytest.raises(hip.MfhipError, match="noise_reg"):
            hip.sched_step_noise_dev(ok, ok, 1.0, ok.clone(), None, _one_op_row(5), reg)
    with pytest.raises(hip.MfhipError, match="global_batch"):
        hip.sched_step_noise_dev(ok, ok, 1.0, ok.clone(), None, _one_op_row(5), 5, first_sample=1, global_batch=2)
    lib = hip.load()
    rc = lib.mf_sched_step_noise_dev(z.data_ptr(), z.data_ptr(), 1.0, z.clone().data_ptr(), None, _one_op_row(5).data_ptr(), 12, 5, 6, 0, 2,
                                     0, 0, None, hip._stream())
    assert rc == MF_EINVAL and b"per_sample" in lib.mf_last_error()


KERNEL_CASES = {
    "from_pndm": lambda: DPM.from_config(PNDMScheduler(**SD_SCHED, skip_prk_steps=True).config),
    "2m_karras": lambda: DPM(**SD, use_karras_sigmas=True),
    "o3": lambda: DPM(**SD, solver_order=3),
    "sde": lambda: DPM(**SD, algorithm_type="sde-dpmsolver++"),
    "sde_karras_o1": lambda: DPM(**SD, algorithm_type="sde-dpmsolver++", use_karras_sigmas=True, solver_order=1),
}


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_walks_every_row_like_the_host_scheduler(name):
    """10 steps at 4 x 4 x 16 x 16: every row of the plan through mf_sched_step_dev / mf_sched_step_noise_dev equals hip.cfg_combine + the
    scheduler's own mf_axpby_n sequence (and, SDE, its PhiloxGenerator draw): latents after every step, history after finish, offsets."""
    mk = KERNEL_CASES[name]
    host, full = mk(), mk()
    host.set_timesteps(10)
    full.set_timesteps(10)
    ts = host.timesteps
    plan = device_plan(full)
    sde = name.startswith("sde")
    assert (plan.noise_reg >= 2) == sde
    rows = plan.rows.to(DEV)
    gen = torch.Generator().manual_seed(11)
    shape = (4, 4, 16, 16)
    lat0 = torch.randn(shape, generator=gen).to(DEV)
    lat_h, lat_d = lat0.clone(), lat0.clone()
    state = torch.full((max(plan.nslots, 1),) + shape, float("nan"), device=DEV)
    g_host, g_dev = PhiloxGenerator(5, DEV), PhiloxGenerator(5, DEV)
    rng_state = g_dev.device_state()
    blocks = hip.philox_normal_blocks(shape[0], lat0[0].numel())
    g = 7.5
    for k in range(len(ts)):
        eu, ec = torch.randn(shape, generator=gen).to(DEV), torch.randn(shape, generator=gen).to(DEV)
        lat_h = host.step(hip.cfg_combine(eu, ec, g), ts[k], lat_h, generator=g_host, return_dict=False)[0]
        if sde:
            hip.sched_step_noise_dev(eu, ec, g, lat_d, state, rows[k].contiguous(), plan.noise_reg, rng_state=rng_state)
            hip.philox_advance(rng_state, blocks)
            g_dev.note_advanced(blocks, on_device=True)
        else:
            hip.sched_step_dev(eu, ec, g, lat_d, state, rows[k].contiguous())
        torch.cuda.synchronize()
        assert torch.isfinite(lat_d).all()
        assert torch.equal(lat_d, lat_h), f"{name}, step {k}: latents differ by {(lat_d - lat_h).abs().max()}"
    plan.finish(full, state)
    _assert_same_state(full, host, name)
    assert g_dev.offset == g_host.offset == (10 * blocks if sde else 0)
    assert rng_state.cpu().tolist() == [5, g_host.offset]


def _counting(monkeypatch):
    lib = hip.load()
    counts = {n: 0 for n in ("mf_sched_step_dev", "mf_sched_step_noise_dev", "mf_philox_advance", "mf_axpby_n", "mf_cfg_combine",
                             "mf_philox_normal")}
    for name in counts:
        fn = getattr(lib, name)

        def wrap(*a, _fn=fn, _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    return counts


PIPE_CASES = {
    "dpmpp_2m": lambda base: DPM.from_config(base),
    "dpmpp_2m_karras": lambda base: DPM.from_config(base, use_karras_sigmas=True),
    "sde": lambda base: DPM.from_config(base, algorithm_type="sde-dpmsolver++"),
}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(PIPE_CASES))
def test_tiny_pipeline_graph_with_the_device_update_equals_the_host_loop(name, prec, monkeypatch):
    """use_hip_graph True / False: bitwise-equal latents, the scheduler in the host's end state and the same final generator offset; the
    graph path makes no mf_axpby_n / mf_cfg_combine / mf_philox_normal call for the update (its eager first step and its capture call
    the update entry once each), and the SDE case calls the new entry."""
    pipe = _tiny_pipe(prec)
    base = pipe.scheduler.config
    inp = synth.pipeline_inputs(2, 16, 16, seed=17, cross_dim=32, vae_scale=2)
    noise = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    sde = name == "sde"
    gen = lambda: dict(generator=PhiloxGenerator(3, DEV)) if sde else {}
    pipe.scheduler = PIPE_CASES[name](base)
    pipe.use_hip_graph, pipe._graph_state = False, None
    kw_h = gen()
    want = _run(pipe, inp, 6, 16, 16, noise, **kw_h)
    host = pipe.scheduler
    pipe.scheduler = PIPE_CASES[name](base)
    pipe.use_hip_graph, pipe._graph_state = True, None
    counts = _counting(monkeypatch)
    kw_d = gen()
    got = _run(pipe, inp, 6, 16, 16, noise, **kw_d)
    monkeypatch.undo()
    assert pipe._graph_state is not None and pipe._graph_state["graph"] is not None and "state" in pipe._graph_state
    new, old = ("mf_sched_step_noise_dev", "mf_sched_step_dev") if sde else ("mf_sched_step_dev", "mf_sched_step_noise_dev")
    assert counts[new] == 2 and counts[old] == 0 and counts["mf_philox_advance"] == (2 if sde else 0), counts
    assert counts["mf_axpby_n"] == 0 and counts["mf_cfg_combine"] == 0 and counts["mf_philox_normal"] == 0, counts
    assert torch.isfinite(got).all() and torch.equal(got, want), f"{name} [{prec}]: differs by {(got - want).abs().max()}"
    _assert_same_state(pipe.scheduler, host, f"{name} [{prec}]")
    if sde:
        blocks = hip.philox_normal_blocks(2, 4 * 8 * 8)
        assert kw_d["generator"].offset == kw_h["generator"].offset == 6 * blocks
        assert kw_d["generator"].device_state().cpu().tolist() == [3, 6 * blocks]
    # a second call replays the kept graph from its first step (SDE: the same generator object, seeded again): the same result
    pipe.scheduler = PIPE_CASES[name](base)
    again = dict(generator=kw_d["generator"].manual_seed(3)) if sde else {}
    assert torch.equal(_run(pipe, inp, 6, 16, 16, noise, **again), want)


def test_sde_with_a_torch_generator_steps_on_the_host_and_is_reproducible():
    pipe = _tiny_pipe("fp32")
    base = pipe.scheduler.config
    inp = synth.pipeline_inputs(2, 16, 16, seed=17, cross_dim=32, vae_scale=2)
    noise = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    outs = []
    for seed in (9, 9, 10):
        pipe.scheduler = PIPE_CASES["sde"](base)
        outs.append(_run(pipe, inp, 6, 16, 16, noise, generator=torch.Generator(DEV).manual_seed(seed)))
        assert "eps" in pipe._graph_state and "state" not in pipe._graph_state, "a torch.Generator takes the host step"
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    pipe.scheduler = PIPE_CASES["sde"](base)                   # a list of Philox generators: the host step too
    gens = [PhiloxGenerator(1, DEV), PhiloxGenerator(2, DEV)]
    _run(pipe, inp, 6, 16, 16, noise, generator=gens)
    assert "eps" in pipe._graph_state and gens[0].offset == gens[1].offset == 6 * hip.philox_normal_blocks(1, 4 * 8 * 8)


def _dpm_envelope(prec):
    """util.report_env reads `<prec>_envelope.json` through util's cache: the DPM-Solver cases' entries (dpmsolver_envelope.json, the
    reference's own bf16 / fp16 deviation on these very cases) join it under their own keys; util's multipliers stay as they are."""
    util.envelope("tiny_pipeline/ddim/image", prec)
    with open(os.path.join(util.GOLD, "dpmsolver_envelope.json")) as f:
        util._ENV[prec].update(json.load(f)[prec])


@pytest.mark.parametrize("prec,tol", PREC_TOL)
@pytest.mark.parametrize("name", ["dpmpp_2m", "dpmpp_2m_karras"])
def test_tiny_pipeline_per_step_against_the_reference(prec, tol, name):
    """test_pipeline_gpu.test_tiny_pipeline_per_step for the two DPM-Solver++ cases of dpmsolver.npz."""
    if prec in ("bf16", "fp16"):
        _dpm_envelope(prec)
    unet, bn, vae = build("tiny", prec)
    G = golden("dpmsolver.npz")
    base = PNDMScheduler(**SD_SCHED, skip_prk_steps=True).config
    sched = DPM.from_config(base, **(dict(use_karras_sigmas=True) if name.endswith("karras") else {}))
    pipe = StableDiffusionBrushNetPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, brushnet=bn, scheduler=sched,
                                           safety_checker=None, feature_extractor=None, requires_safety_checker=False,
                                           depth_conditioning_mode="concat")
    pipe.set_progress_bar_config(disable=True)
    inp = synth.pipeline_inputs(1, 16, 16, seed=1234, cross_dim=32, vae_scale=2)
    noise = torch.from_numpy(G[f"{name}_vae_noise"])
    cond = pipe.build_conditioning(inp["image"], inp["mask"], inp["depth"], 16, 16, 1, 1, True, noise)
    check(f"conditioning[{prec}]", cond, G[f"{name}_cond"], prec, dict(atol=2e-4), f"dpmsolver/{name}/cond")
    trace = []
    res = pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"],
               mask=inp["mask"], depth=inp["depth"], num_inference_steps=4, guidance_scale=7.5, latents=inp["latents"].clone(),
               output_type="pt", brushnet_conditioning_scale=1.0,
               callback_on_step_end=lambda p, i, t, kw: trace.append(kw["latents"].clone()) or {}, height=16, width=16,
               conditioning_noise=noise)
    assert pipe.scheduler.timesteps.tolist() == G[f"{name}_timesteps"].tolist()
    assert len(trace) == 4
    for i in range(4):
        check(f"{name} latents step {i}[{prec}]", trace[i], torch.from_numpy(G[f"{name}_latents_{i}"]), prec, dict(atol=tol),
              f"dpmsolver/{name}/latents_{i}")
    check(f"{name} image[{prec}]", res.images, G[f"{name}_image"], prec, dict(atol=tol), f"dpmsolver/{name}/image")


PROGRAM_CASES = {
    "dpmpp_2m": lambda: DPM.from_config(PNDMScheduler(**SD_SCHED, skip_prk_steps=True).config),
    "sde": lambda: DPM.from_config(PNDMScheduler(**SD_SCHED, skip_prk_steps=True).config, algorithm_type="sde-dpmsolver++"),
}


@pytest.mark.parametrize("name", list(PROGRAM_CASES))
def test_device_scheduler_program_replays_the_loop_bit_exactly(name, tmp_path):
    """export_denoise_step(..., scheduler="device"): the program carries the update — mf_sched_step_dev for dpmpp_2m (no new thunk),
    mf_sched_step_noise_dev + mf_philox_advance on the io buffer "philox_state" for the SDE type.  Replayed from Python over 4 steps it
    gives the pipeline's latents after every step; the SDE program gives them again when replayed from a reset state."""
    sde = name == "sde"
    pipe = _tiny_pipe("bf16")
    mk = PROGRAM_CASES[name]
    gen = lambda: dict(generator=PhiloxGenerator(3, DEV)) if sde else {}
    inp = synth.pipeline_inputs(2, 16, 32, seed=7, cross_dim=32, vae_scale=2)
    noise = torch.randn(4, 4, 8, 16, generator=torch.Generator().manual_seed(3))
    steps = 4
    pipe.scheduler = mk()
    per_step, ref = _grab_steps(pipe, _call_args(inp, steps, noise, **gen()))       # (a callback: the host's scheduler steps)
    pipe.scheduler = mk()
    pipe._graph_state = None
    path = str(tmp_path / "step.mfprog")
    info = pipe.export_denoise_step(path, scheduler="device", **_call_args(inp, steps, noise, **gen()))
    assert torch.equal(info["result"].images.float().cpu(), ref), "the exporting run itself must give the host loop's latents"
    assert "mf_cfg_combine" not in info["entries"] and "mf_axpby_n" not in info["entries"] and "mf_philox_normal" not in info["entries"]
    assert "DPMSolverMultistepScheduler" in info["meta"]["result"]
    n = len(per_step)
    prog = program.Program(path, DEV)
    shape = per_step[0].shape
    tables = {nm[6:]: prog.buffer(nm) for nm in prog.names if nm.startswith("table.")}
    assert set(tables) == {"sched_row", "temb_unet", "temb_brushnet"}
    if sde:
        assert "mf_sched_step_noise_dev" in info["entries"] and "mf_philox_advance" in info["entries"] and "mf_sched_step_dev" not in info["entries"]
        per = shape[1] * shape[2] * shape[3]
        blocks = hip.philox_normal_blocks(shape[0], per)
        meta = json.loads(prog.meta)["philox"]
        assert meta["per_sample"] == per and meta["global_batch"] == shape[0] and meta["blocks_per_step"] == blocks
        assert "philox_state" in prog.names
        # as recorded (step 1): the state after one step's draw
        assert prog.buffer("philox_state", torch.int64).cpu().tolist() == [3, blocks]
    else:
        assert "mf_sched_step_dev" in info["entries"] and "philox_state" not in prog.names
    lib = hip.load()
    for replay in range(2 if sde else 1):
        prog.buffer("latents", torch.float32).copy_(inp["latents"].float().reshape(-1).to(DEV))
        if sde:                                                # the generator's pair as the call found it: seed 3, nothing drawn
            prog.buffer("philox_state", torch.int64).copy_(torch.tensor([3, 0]))
        for i in range(n):
            for dst, tab in tables.items():
                prog.buffer(dst).copy_(tab.view(n, -1)[i])
            hip._check(lib.mf_denoise_step_fused(prog._h, None, None, None, None, hip._stream()), "mf_denoise_step_fused")
            torch.cuda.synchronize()
            got = prog.buffer("latents", torch.float32).view(shape).cpu()
            assert torch.equal(got, per_step[i]), f"{name}, replay {replay}, step {i}: differs by {(got - per_step[i]).abs().max()}"
        if sde:
            assert prog.buffer("philox_state", torch.int64).cpu().tolist() == [3, n * blocks]
    prog.close()
    if sde:                                                    # the kernel draws the library's stream only
        pipe.scheduler = mk()
        with pytest.raises(NotImplementedError, match="PhiloxGenerator"):
            pipe.export_denoise_step(path, scheduler="device", generator=torch.Generator(DEV).manual_seed(3), **_call_args(inp, steps, noise))


def test_c_host_runs_a_dpmpp_2m_loop(tmp_path):
    """examples/c_host/denoise_host.c, eager and --graph: a 6-step DPM-Solver++ 2M run from latents_in.bin writes the pipeline's latents
    bit for bit (test_sched_device_gpu.test_c_host_runs_a_unipc_loop for the new class; the host program is unchanged)."""
    exe, env = _c_host(tmp_path)
    pipe = _tiny_pipe("bf16")
    pipe.scheduler = PROGRAM_CASES["dpmpp_2m"]()
    inp = synth.pipeline_inputs(2, 16, 32, seed=7, cross_dim=32, vae_scale=2)
    noise = torch.randn(4, 4, 8, 16, generator=torch.Generator().manual_seed(3))
    path = str(tmp_path / "step.mfprog")
    info = pipe.export_denoise_step(path, scheduler="device", **_call_args(inp, 6, noise))
    ref = info["result"].images.float().cpu()
    lat_in = str(tmp_path / "in.bin")
    inp["latents"].float().contiguous().numpy().tofile(lat_in)
    for extra in ([], ["--graph"]):
        lat_out = str(tmp_path / f"out{len(extra)}.bin")
        out = subprocess.run([exe, path, lat_in, lat_out] + extra, capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        got = torch.from_numpy(np.fromfile(lat_out, dtype=np.float32)).view(ref.shape)
        assert torch.isfinite(got).all() and torch.equal(got, ref), f"C host {extra}: differs from the pipeline by {(got - ref).abs().max()}"
