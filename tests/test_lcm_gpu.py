"""LCM sampling on the device: the plan's rows through mf_sched_step_noise_dev / mf_sched_step_dev in both guidance forms (eps_c given,
and g < 0 with eps_c NULL) against the host scheduler fed the same Philox noise, the UNet's timestep_cond against the reference's
recorded output (tests/golden/lcm_tiny.npz, tools/make_golden_lcm.py), and the tiny pipeline with a fused tiny LoRA: the captured step
with and without classifier-free guidance against the eager host loop, bit for bit (every kernel is deterministic and the update's
arithmetic is one routine in both), the launch census, the generator's offset, custom timesteps, and the step programs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lora_ref  # noqa: E402
from oracle import mirrorfusion_ref as R  # noqa: E402
from reflecting_reality_amd import LCMScheduler, hip, models as M, program, synth  # noqa: E402
from reflecting_reality_amd.rng import PhiloxGenerator  # noqa: E402
from reflecting_reality_amd.schedulers import device_plan  # noqa: E402
from test_euler_gpu import _Log  # noqa: E402
from test_lora_gpu import fresh_unet, tiny_pipe  # noqa: E402
from test_models_gpu import TOL, build, tiny_inputs  # noqa: E402
from test_pipeline_gpu import SD_SCHED, _run  # noqa: E402
from util import check, golden, keys, report  # noqa: E402

DEV = "cuda"
SD = {k: v for k, v in SD_SCHED.items() if k not in ("steps_offset", "set_alpha_to_one")}
# 864 elements: 216 float4 lanes, less than one block of 256, a ragged tail; 4608 elements: 4.5 blocks
KERNEL_SHAPES = [(3, 4, 8, 9), (2, 4, 16, 36)]
CUSTOM = [999, 759, 499, 259]


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [True, False], ids=["eps_c given", "ec=None"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("p", ["epsilon", "v_prediction", "sample"])
def test_kernels_walk_every_row_like_the_host_scheduler(p, shape, guided):
    """4 steps: the three drawing rows through mf_sched_step_noise_dev (+ mf_philox_advance), the noiseless last row through
    mf_sched_step_dev; after every row the latents are bitwise the host step()'s on hip.cfg_combine(eu, ec, g), or on eu itself."""
    host, full = LCMScheduler(**SD, prediction_type=p), LCMScheduler(**SD, prediction_type=p)
    host.set_timesteps(4)
    full.set_timesteps(4)
    ts = host.timesteps
    plan = device_plan(full)
    assert plan.noise_reg == 2 and plan.nslots == 0 and plan.draws == [True, True, True, False]
    rows = plan.rows.to(DEV)
    gen = torch.Generator().manual_seed(11)
    lat0 = torch.randn(shape, generator=gen).to(DEV)
    lat_h, lat_d = lat0.clone(), lat0.clone()
    assert lat_d.numel() // 4 in (216, 1152)                        # float4 lanes: under one block of 256, and 4.5 blocks
    g_host, g_dev = PhiloxGenerator(5, DEV), PhiloxGenerator(5, DEV)
    rng_state = g_dev.device_state()
    blocks = hip.philox_normal_blocks(shape[0], lat0[0].numel())
    g = 1.5
    for k in range(4):
        eu, ec = torch.randn(shape, generator=gen).to(DEV), torch.randn(shape, generator=gen).to(DEV)
        e = hip.cfg_combine(eu, ec, g) if guided else eu
        lat_h = host.step(e, ts[k], lat_h, generator=g_host, return_dict=False)[0]
        args = (eu, ec, g) if guided else (eu, None, -1.0)
        if plan.draws[k]:
            hip.sched_step_noise_dev(*args, lat_d, None, rows[k].contiguous(), plan.noise_reg, rng_state=rng_state)
            hip.philox_advance(rng_state, blocks)
            g_dev.note_advanced(blocks, on_device=True)
        else:
            hip.sched_step_dev(*args, lat_d, None, rows[k].contiguous())
        torch.cuda.synchronize()
        assert torch.isfinite(lat_d).all()
        assert torch.equal(lat_d, lat_h), f"{p} {shape}, step {k}: latents differ by {(lat_d - lat_h).abs().max()}"
    assert g_dev.offset == g_host.offset == 3 * blocks and rng_state.cpu().tolist() == [5, 3 * blocks]
    plan.finish(full, torch.empty((1,) + shape, device=DEV))
    assert full.step_index == host.step_index == 4


def _copy_noise_row(reg=2):
    """A row whose only op moves the noise register into the latents (coefficient 1: exact)."""
    row = hip.SchedRow(nops=1, nslots=0)
    row.ops[0].dst, row.ops[0].nterms = 1, 1
    row.ops[0].src[0], row.ops[0].coef[0] = reg, 1.0
    row.load, row.store = 0, 1 << 1
    return torch.frombuffer(bytearray(bytes(row)), dtype=torch.int32).clone().to(DEV)


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_unguided_kernel_draws_the_library_stream_bit_for_bit(shape):
    """The noise the g < 0 instantiation puts into its register equals mf_philox_normal at the same (seed, offset), from the host pair and
    from a device state, for a whole draw and for the second sample of a larger one."""
    row = _copy_noise_row()
    eu = torch.zeros(shape, device=DEV)
    seed, offset = 0x1234_5678_9ABC, 77
    want = hip.philox_normal(shape, seed, offset, DEV)
    lat = torch.full(shape, float("nan"), device=DEV)
    hip.sched_step_noise_dev(eu, None, -1.0, lat, None, row, 2, seed=seed, offset=offset)
    assert torch.equal(lat, want)
    gen = PhiloxGenerator(seed, DEV).set_state((seed, offset))
    lat.fill_(float("nan"))
    hip.sched_step_noise_dev(eu, None, -1.0, lat, None, row, 2, rng_state=gen.device_state())
    assert torch.equal(lat, want)
    part = torch.full((1,) + shape[1:], float("nan"), device=DEV)
    hip.sched_step_noise_dev(eu[:1].contiguous(), None, -1.0, part, None, row, 2, seed=seed, offset=offset, first_sample=1, global_batch=shape[0])
    assert torch.equal(part[0], want[1])
    guided = torch.full(shape, float("nan"), device=DEV)             # (and the guided instantiation still does)
    hip.sched_step_noise_dev(eu, eu, 1.5, guided, None, row, 2, seed=seed, offset=offset)
    assert torch.equal(guided, want)


def test_guidance_without_eps_c_is_the_argument_error_not_a_launch():
    shape = KERNEL_SHAPES[0]
    eu = torch.zeros(shape, device=DEV)
    lat = torch.full(shape, 3.0, device=DEV)
    row = _copy_noise_row()
    for g in (0.0, 1.5):
        with pytest.raises(hip.MfhipError, match="eps_c is NULL"):
            hip.sched_step_noise_dev(eu, None, g, lat, None, row, 2, seed=1, offset=0)
        with pytest.raises(hip.MfhipError, match="eps_c is NULL"):
            hip.sched_step_dev(eu, None, g, lat, None, row)
    torch.cuda.synchronize()
    assert bool((lat == 3.0).all()), "nothing ran"
    lib = hip.load()
    rc = lib.mf_sched_step_dev(C.c_void_p(eu.data_ptr()), None, C.c_float(7.5), C.c_void_p(lat.data_ptr()), None, C.c_void_p(row.data_ptr()),
                               C.c_int64(lat.numel()), None)
    assert rc == -1                                                  # MF_EINVAL (include/mfhip.h)


# ---- the UNet's timestep_cond ----------------------------------------------------------------------------------------------------------
def _distilled_unet(prec):
    G = golden("lcm_tiny.npz")
    unet = M.UNet2DConditionModel(dict(R.TINY_UNET, time_cond_proj_dim=32), precision=prec, device=DEV)
    sd = synth.state_dict_for(keys("tiny")["unet"], 0)               # the tiny fixture's weights, plus the one the key adds
    sd["time_embedding.cond_proj.weight"] = torch.from_numpy(G["cond_proj_weight"])
    unet.load_state_dict(sd)
    return unet, G


@pytest.mark.parametrize("prec", ["fp32", "f16x3", "bf16"])
def test_tiny_unet_with_timestep_cond_against_the_reference(prec):
    """fp32 / f16x3: the tiny-model tests' bound (test_models_gpu.TOL; fp32_envelope.json holds the full-size latents only, no tiny entry).
    bf16: the reference's own bf16 deviation on this net and these inputs without the embedding (bf16_envelope.json tiny/unet_eps_plain;
    the time embedding is fp32 in every precision)."""
    unet, G = _distilled_unet(prec)
    x, _, ehs = tiny_inputs()
    cond = torch.from_numpy(G["timestep_cond"]).to(DEV)
    t = int(G["timestep"])
    eps = unet(x.to(DEV), t, ehs.to(DEV), timestep_cond=cond, return_dict=False)[0]
    check(f"unet_eps_timestep_cond[{prec}]", eps, G["eps"], prec, TOL.get(prec), "tiny/unet_eps_plain")
    plain = unet(x.to(DEV), t, ehs.to(DEV), return_dict=False)[0]
    assert float((plain.float() - eps.float()).abs().max()) > 0.05, "the embedding moves the output"
    # the table's row is what forward computes, and forward(_temb=row) is forward(timestep_cond=)
    table = unet.time_embedding_table(torch.tensor([float(t), 100.0]), 2, None, cond)
    assert tuple(table.shape[:2]) == (2, 2)
    assert torch.equal(table[0], unet._time_embedding(t, 2, None, cond))
    assert torch.equal(unet(x.to(DEV), t, ehs.to(DEV), return_dict=False, _temb=table[0])[0], eps)
    assert not torch.equal(table[0][0], table[0][1]), "one row per image: the two guidance scales differ"
    assert "time_embedding.cond_proj.weight" in unet.state_dict()
    with pytest.raises(ValueError, match="time_cond_proj_dim"):
        build("tiny", prec)[0](x.to(DEV), t, ehs.to(DEV), timestep_cond=cond)


def test_a_distilled_unet_has_no_training_layout():
    unet, _ = _distilled_unet("fp32")
    with pytest.raises(NotImplementedError, match="time_cond_proj_dim"):
        unet.train()


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
_pipes = {}


def _lcm_pipe():
    """The tiny pipeline with the tiny LoRA of lora_tiny.npz loaded and fused, under LCMScheduler.from_config(its DDIM config)."""
    if "pipe" not in _pipes:
        G = golden("lora_tiny.npz")
        pipe = tiny_pipe(fresh_unet("tiny", "fp32"), "fp32")
        asd, alphas = lora_ref.adapter_of(G, "tiny", pipe.unet.param_shapes(), prefix="unet.")
        pipe.load_lora_weights({**asd, **{k: torch.tensor(v) for k, v in alphas.items()}}, adapter_name="lcm")
        pipe.fuse_lora(lora_scale=1.0)
        _pipes["pipe"], _pipes["base"] = pipe, pipe.scheduler.config
    pipe = _pipes["pipe"]
    pipe.scheduler = LCMScheduler.from_config(_pipes["base"])
    return pipe


def _inputs():
    return synth.pipeline_inputs(2, 16, 16, seed=17, cross_dim=32, vae_scale=2), torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(4))


def _spy(monkeypatch, pipe):
    """What _predict_noise was told and returned: (do_cfg, rows of eps_u, ec is None) per call."""
    seen, real = [], pipe._predict_noise

    def wrapped(*a, **k):
        eu, ec = real(*a, **k)
        seen.append((a[7], eu.shape[0], ec is None))
        return eu, ec
    monkeypatch.setattr(pipe, "_predict_noise", wrapped)
    return seen


@pytest.mark.parametrize("guidance", [1.0, 1.5])
def test_the_captured_step_equals_the_eager_loop_and_launches_one_update(guidance, monkeypatch):
    pipe = _lcm_pipe()
    inp, noise = _inputs()
    nb, cfg = 2, guidance > 1
    noise = noise if cfg else noise[:nb]                             # (the conditioning's VAE noise: one draw per row of the UNet's batch)
    blocks = hip.philox_normal_blocks(nb, 4 * 8 * 8)
    pipe.use_hip_graph, pipe._graph_state = False, None
    g_h = PhiloxGenerator(3, DEV)
    want = _run(pipe, inp, 4, 16, 16, noise, guidance_scale=guidance, generator=g_h)
    host = pipe.scheduler
    assert host.timesteps.tolist() == [999, 759, 499, 259] and host.step_index == 4 and g_h.offset == 3 * blocks
    pipe = _lcm_pipe()
    pipe.use_hip_graph, pipe._graph_state = True, None
    log, seen = _Log(monkeypatch, pipe), _spy(monkeypatch, pipe)
    g_d = PhiloxGenerator(3, DEV)
    got = _run(pipe, inp, 4, 16, 16, noise, guidance_scale=guidance, generator=g_d)
    monkeypatch.undo()
    st = pipe._graph_state
    assert st is not None and st["graph"] is not None and "state" in st and "eps" not in st, "the device plan, inside the captured step"
    # the update of a step is ONE mf_sched_step_noise_dev and ONE mf_philox_advance (the eager first step and the capture: two each)
    loop = log.calls[log.calls.index("prepared") + 1:]
    assert log.count("mf_sched_step_noise_dev", loop) == 2 and log.count("mf_philox_advance", loop) == 2, loop
    for entry in ("mf_sched_step_dev", "mf_cfg_combine", "mf_axpby_n", "mf_philox_normal"):
        assert log.count(entry, loop) == 0, loop
    # the UNet's batch: nb without guidance, 2 nb with
    assert seen == [(cfg, nb, not cfg)] * 2, seen
    assert st["pe"].shape[0] == (2 * nb if cfg else nb) and st["lat"].shape[0] == nb
    assert torch.isfinite(got).all() and torch.equal(got, want), f"guidance {guidance}: differs by {(got - want).abs().max()}"
    assert pipe.scheduler.step_index == 4 and torch.equal(pipe.scheduler.timesteps, host.timesteps)
    # 3 draws for 4 steps: the host pair is where the host loop leaves it, and the device state is level with it on its next use
    assert g_d.offset == g_h.offset == 3 * blocks
    assert g_d.device_state().cpu().tolist() == [3, 3 * blocks]
    # another seed, the same generator object: the kept graph serves every step (same key, nothing captured or launched eagerly again)
    graph = st["graph"]
    pipe.scheduler = LCMScheduler.from_config(_pipes["base"])
    log = _Log(monkeypatch, pipe)
    other = _run(pipe, inp, 4, 16, 16, noise, guidance_scale=guidance, generator=g_d.manual_seed(8))
    monkeypatch.undo()
    assert pipe._graph_state is st and st["graph"] is graph and log.count("mf_sched_step_noise_dev") == 0
    assert g_d.get_state() == (8, 3 * blocks) and not torch.equal(other, want)
    pipe = _lcm_pipe()
    pipe.use_hip_graph, pipe._graph_state = False, None
    assert torch.equal(other, _run(pipe, inp, 4, 16, 16, noise, guidance_scale=guidance, generator=PhiloxGenerator(8, DEV)))


def test_a_torch_generator_takes_the_host_step_and_gives_the_eager_loops_latents():
    pipe = _lcm_pipe()
    inp, noise = _inputs()
    noise = noise[:2]
    outs = {}
    for graph in (False, True):
        pipe.scheduler = LCMScheduler.from_config(_pipes["base"])
        pipe.use_hip_graph, pipe._graph_state = graph, None
        outs[graph] = _run(pipe, inp, 4, 16, 16, noise, guidance_scale=1.0, generator=torch.Generator(DEV).manual_seed(9))
        if graph:
            st = pipe._graph_state
            assert st["graph"] is not None and "eps" in st and "state" not in st, "a torch.Generator takes the host step"
    assert torch.isfinite(outs[True]).all() and torch.equal(outs[True], outs[False])


def test_custom_timesteps_are_honoured_and_short_calls_run_eagerly():
    pipe = _lcm_pipe()
    inp, noise = _inputs()
    noise = noise[:2]
    custom = [999, 700, 400, 100]
    outs = {}
    for graph in (False, True):
        pipe.scheduler = LCMScheduler.from_config(_pipes["base"])
        pipe.use_hip_graph, pipe._graph_state = graph, None
        seen = []
        outs[graph] = _run(pipe, inp, 50, 16, 16, noise, guidance_scale=1.0, generator=PhiloxGenerator(3, DEV), timesteps=custom)
        assert pipe.scheduler.timesteps.tolist() == custom and pipe.scheduler.step_index == 4 and pipe.num_timesteps == 4
        assert (pipe._graph_state is not None) == graph
    assert torch.equal(outs[True], outs[False])
    default = _run(pipe, inp, 4, 16, 16, noise, guidance_scale=1.0, generator=PhiloxGenerator(3, DEV))
    assert not torch.equal(default, outs[True])
    pipe.scheduler = LCMScheduler.from_config(_pipes["base"])      # two steps: the eager loop (the graph needs more than two)
    pipe.use_hip_graph, pipe._graph_state = True, None
    g = PhiloxGenerator(3, DEV)
    two = _run(pipe, inp, 2, 16, 16, noise, guidance_scale=1.0, generator=g)
    assert pipe._graph_state is None and torch.isfinite(two).all() and g.offset == hip.philox_normal_blocks(2, 4 * 8 * 8)


def test_a_distilled_unet_runs_unguided_whatever_the_guidance_scale(monkeypatch):
    """time_cond_proj_dim set: guidance_scale 7.5 enters as the embedding of w = 6.5, the batch is not doubled, BrushNet never sees
    timestep_cond, and the captured step (whose time-embedding table carries the embedding) equals the eager loop."""
    unet, _ = _distilled_unet("fp32")
    pipe = tiny_pipe(unet, "fp32")
    pipe.scheduler = LCMScheduler.from_config(pipe.scheduler.config)
    inp, noise = _inputs()
    noise = noise[:2]
    outs = {}
    for graph in (False, True):
        pipe.scheduler = LCMScheduler.from_config(pipe.scheduler.config)
        pipe.use_hip_graph, pipe._graph_state = graph, None
        seen = _spy(monkeypatch, pipe)
        outs[graph] = _run(pipe, inp, 4, 16, 16, noise, guidance_scale=7.5, generator=PhiloxGenerator(3, DEV))
        monkeypatch.undo()
        assert pipe.do_classifier_free_guidance is False and all(s == (False, 2, True) for s in seen) and len(seen) == (2 if graph else 4)
    assert torch.isfinite(outs[True]).all() and torch.equal(outs[True], outs[False])
    pipe.use_hip_graph, pipe._graph_state = False, None
    pipe.scheduler = LCMScheduler.from_config(pipe.scheduler.config)
    assert not torch.equal(_run(pipe, inp, 4, 16, 16, noise, guidance_scale=3.0, generator=PhiloxGenerator(3, DEV)), outs[False])


# ---- step programs ---------------------------------------------------------------------------------------------------------------------
def test_export_with_guidance_carries_the_noisy_update_and_without_it_is_refused(tmp_path):
    pipe = _lcm_pipe()
    inp, noise = _inputs()
    args = dict(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"], mask=inp["mask"],
                depth=inp["depth"], num_inference_steps=4, latents=inp["latents"].clone(), height=16, width=16, conditioning_noise=noise)
    pipe.use_hip_graph, pipe._graph_state = False, None
    want = pipe(**args, guidance_scale=1.5, generator=PhiloxGenerator(3, DEV), output_type="latent").images.float().cpu()
    pipe = _lcm_pipe()
    pipe.use_hip_graph, pipe._graph_state = True, None
    path = str(tmp_path / "step.mfprog")
    info = pipe.export_denoise_step(path, scheduler="device", guidance_scale=1.5, generator=PhiloxGenerator(3, DEV), **args)
    assert torch.equal(info["result"].images.float().cpu(), want), "the exporting run itself gives the host loop's latents"
    assert "mf_sched_step_noise_dev" in info["entries"] and "mf_philox_advance" in info["entries"]
    assert "mf_cfg_combine" not in info["entries"] and "mf_axpby_n" not in info["entries"]
    assert "LCMScheduler" in info["meta"]["result"] and info["meta"]["philox"]["noise_reg"] == 2
    prog = program.Program(path, DEV)
    assert "philox_state" in prog.names and "sched_row" in prog.names
    prog.close()
    before = set(os.listdir(tmp_path))
    pipe = _lcm_pipe()
    with pytest.raises(NotImplementedError, match="classifier-free guidance"):
        pipe.export_denoise_step(str(tmp_path / "unguided.mfprog"), scheduler="device", guidance_scale=1.0, generator=PhiloxGenerator(3, DEV), **args)
    with pytest.raises(NotImplementedError, match="classifier-free guidance"):
        pipe.export_call(str(tmp_path / "call"), guidance_scale=1.0, **args)
    assert set(os.listdir(tmp_path)) == before, "a refused export wrote something"
