"""PNDM / UniPC updates on the device (mf_sched_step_dev, schedulers.device_plan): the kernel, the captured step graph of the
pipeline, and step programs (from Python and from the C host).  The bar everywhere is bit-exactness against the host scheduler's own
step(): hip.cfg_combine followed by its mf_axpby_n calls."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from reflecting_reality_amd import PNDMScheduler, UniPCMultistepScheduler, hip, program, synth  # noqa: E402
from reflecting_reality_amd.schedulers import device_plan  # noqa: E402
from test_pipeline_gpu import SD_SCHED, _config1_pipe, _run, _tiny_pipe  # noqa: E402
from test_program_gpu import _call_args  # noqa: E402
from util import check, golden  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIPC_SD = {k: v for k, v in SD_SCHED.items() if k != "set_alpha_to_one"}
HISTORY = ("model_outputs", "last_sample", "ets", "cur_sample", "cur_model_output")
COUNTERS = ("_step_index", "lower_order_nums", "this_order", "counter")


def _assert_same_state(got, want, what):
    for k in COUNTERS:
        assert getattr(got, k, None) == getattr(want, k, None), f"{what}: {k} {getattr(got, k, None)} != {getattr(want, k, None)}"
    for k in HISTORY:
        a, b = getattr(got, k, None), getattr(want, k, None)
        a, b = (a if isinstance(a, list) else [a]), (b if isinstance(b, list) else [b])
        assert len(a) == len(b), f"{what}: {k} has {len(a)} entries, the host's {len(b)}"
        for j, (x, y) in enumerate(zip(a, b)):
            assert (x is None) == (y is None), f"{what}: {k}[{j}]"
            if x is not None:
                assert torch.equal(x.float().cpu(), y.float().cpu()), f"{what}: {k}[{j}] differs by {(x.float().cpu() - y.float().cpu()).abs().max()}"


KERNEL_CASES = {
    "unipc_bh2_o2": lambda: UniPCMultistepScheduler(**UNIPC_SD, solver_type="bh2", solver_order=2),
    "unipc_bh2_o3": lambda: UniPCMultistepScheduler(**UNIPC_SD, solver_type="bh2", solver_order=3),
    "pndm_prk": lambda: PNDMScheduler(**SD_SCHED, skip_prk_steps=False),
    "pndm_skip_prk": lambda: PNDMScheduler(**SD_SCHED, skip_prk_steps=True),
}


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_walks_every_row_like_the_host_scheduler(name):
    """Random tensors at batch 4 x 64^2: every row of the plan through mf_sched_step_dev equals hip.cfg_combine + the scheduler's
    mf_axpby_n sequence (torch.equal), for the latents and for the history, after every step."""
    mk = KERNEL_CASES[name]
    host = mk()
    host.set_timesteps(10)
    ts = host.timesteps
    n = len(ts)
    full = mk()
    full.set_timesteps(10)
    plan = device_plan(full)
    rows = plan.rows.to(DEV)
    gen = torch.Generator().manual_seed(11)
    shape = (4, 4, 64, 64)
    lat0 = torch.randn(shape, generator=gen).to(DEV)
    lat_h, lat_d = lat0.clone(), lat0.clone()
    state = torch.full((plan.nslots,) + shape, float("nan"), device=DEV)
    g = 7.5
    for k in range(n):
        eu, ec = torch.randn(shape, generator=gen).to(DEV), torch.randn(shape, generator=gen).to(DEV)
        lat_h = host.step(hip.cfg_combine(eu, ec, g), ts[k], lat_h, return_dict=False)[0]
        hip.sched_step_dev(eu, ec, g, lat_d, state, rows[k].contiguous())
        torch.cuda.synchronize()
        assert torch.isfinite(lat_d).all()
        assert torch.equal(lat_d, lat_h), f"{name}, step {k}: latents differ by {(lat_d - lat_h).abs().max()}"
        # the history after k + 1 steps: the plan of the first k + 1 steps (slots are given out step by step, so its values sit in
        # the slots the full plan used) maps it onto the state
        part_s = mk()
        part_s.set_timesteps(10)
        part = device_plan(part_s, steps=k + 1)
        assert part.nslots <= plan.nslots
        part.finish(part_s, state)
        _assert_same_state(part_s, host, f"{name}, after step {k}")


def _counting(monkeypatch):
    """Wrap hip.load()'s library: count the calls of the two update entries (the graph path's eager first step and its capture)."""
    lib = hip.load()
    counts = {"mf_sched_step_dev": 0, "mf_axpby_n": 0, "mf_cfg_combine": 0}
    for name in counts:
        fn = getattr(lib, name)

        def wrap(*a, _fn=fn, _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    return counts


PIPE_CASES = {
    "unipc_from_pndm": lambda base: UniPCMultistepScheduler.from_config(base),
    "unipc_o3_bh1_v": lambda base: UniPCMultistepScheduler.from_config(base, solver_order=3, solver_type="bh1",
                                                                     prediction_type="v_prediction"),
    "pndm_skip_prk": lambda base: PNDMScheduler.from_config(base, skip_prk_steps=True),
    "pndm_prk": lambda base: PNDMScheduler.from_config(base, skip_prk_steps=False),
}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(PIPE_CASES))
def test_tiny_pipeline_graph_with_the_device_update_equals_the_host_loop(name, prec, monkeypatch):
    """The captured step graph ends with mf_sched_step_dev (no mf_axpby_n, no eager scheduler step): the latents equal the eager
    host-scheduler loop bit for bit, and pipe.scheduler ends in the host's state (counters and history tensors)."""
    pipe = _tiny_pipe(prec)
    base = pipe.scheduler.config
    inp = synth.pipeline_inputs(2, 16, 16, seed=17, cross_dim=32, vae_scale=2)
    noise = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    pipe.scheduler = PIPE_CASES[name](base)
    pipe.use_hip_graph, pipe._graph_state = False, None
    want = _run(pipe, inp, 6, 16, 16, noise)
    host = pipe.scheduler
    pipe.scheduler = PIPE_CASES[name](base)
    pipe.use_hip_graph, pipe._graph_state = True, None
    counts = _counting(monkeypatch)
    got = _run(pipe, inp, 6, 16, 16, noise)
    monkeypatch.undo()
    assert pipe._graph_state is not None and pipe._graph_state["graph"] is not None and "state" in pipe._graph_state
    assert counts["mf_sched_step_dev"] == 2 and counts["mf_axpby_n"] == 0 and counts["mf_cfg_combine"] == 0, counts
    assert torch.isfinite(got).all() and torch.equal(got, want), f"{name} [{prec}]: differs by {(got - want).abs().max()}"
    _assert_same_state(pipe.scheduler, host, f"{name} [{prec}]")
    # a second call replays the kept graph from its first step: the same result again
    pipe.scheduler = PIPE_CASES[name](base)
    assert torch.equal(_run(pipe, inp, 6, 16, 16, noise), want)


def test_a_kept_graph_is_never_replayed_under_another_scheduler_update():
    """One pipeline object, _graph_state never reset, the scheduler (and with it the form of the update that ends the captured step)
    switched between calls: DDIM (fused), PNDM (device plan), PNDM with a callback_on_step_end (host step), UniPC (device plan), DDIM.
    The graph-cache key carries the update's own part, so every call equals the eager loop of a fresh scheduler bit for bit, and the
    last one holds no buffer of another form."""
    from reflecting_reality_amd import DDIMScheduler
    pipe = _tiny_pipe("fp32")
    base = pipe.scheduler.config
    inp = synth.pipeline_inputs(2, 16, 16, seed=17, cross_dim=32, vae_scale=2)
    noise = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    ddim = lambda: DDIMScheduler.from_config(base)
    pndm = lambda: PNDMScheduler.from_config(base, skip_prk_steps=True)
    unipc = lambda: UniPCMultistepScheduler.from_config(base)
    cb = dict(callback_on_step_end=lambda p, i, t, k: {})
    sequence = [("ddim", ddim, {}), ("pndm", pndm, {}), ("pndm + callback", pndm, cb), ("unipc", unipc, {}), ("ddim again", ddim, {})]
    want = {}
    pipe.use_hip_graph = False
    for name, mk in (("ddim", ddim), ("pndm", pndm), ("unipc", unipc)):        # the eager loop, once per scheduler
        pipe.scheduler = mk()
        want[name] = _run(pipe, inp, 6, 16, 16, noise)
    pipe.use_hip_graph, pipe._graph_state = True, None
    for name, mk, kw in sequence:
        pipe.scheduler = mk()
        got = _run(pipe, inp, 6, 16, 16, noise, **kw)
        assert pipe._graph_state is not None and pipe._graph_state["graph"] is not None, f"{name}: not on the graph path"
        ref = want[name.split()[0]]
        assert torch.equal(got, ref), f"{name}: differs from the eager loop by {(got - ref).abs().max()}"
    assert "state" not in pipe._graph_state and "eps" not in pipe._graph_state, "the last DDIM call kept another update's graph state"


@pytest.mark.parametrize("name", ["unipc", "pndm"])
def test_config1_device_update_equals_the_host_update(name):
    """configs[1] (batch 4 x 512^2, bf16, 10 steps) under the schedulers the shipped scripts run: the device update gives the host
    update's latents bit for bit, inside the bounds of tests/golden/sd15_config1_sched.npz."""
    from test_models_gpu import build
    unet, bn, vae = build("sd15", "bf16")
    G = golden("sd15_config1_sched.npz")
    mk = lambda: UniPCMultistepScheduler.from_config(PNDMScheduler(skip_prk_steps=True, **SD_SCHED).config) if name == "unipc" \
        else PNDMScheduler(skip_prk_steps=True, **SD_SCHED)
    pipe = _config1_pipe(unet, bn, vae, mk())
    inp = synth.pipeline_inputs(4, 512, 512, seed=77)
    args = dict(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"],
                mask=inp["mask"], depth=inp["depth"], num_inference_steps=10, guidance_scale=7.5, output_type="latent", height=512,
                width=512, conditioning_noise=inp["vae_noise"])
    trace = []
    host = pipe(latents=inp["latents"].clone(), callback_on_step_end=lambda p, i, t, kw: trace.append(1) or {}, **args).images.float().cpu()
    host_sched = pipe.scheduler
    pipe.scheduler = mk()
    dev = pipe(latents=inp["latents"].clone(), **args).images.float().cpu()
    assert "state" in pipe._graph_state, "the call without a callback must take the device update"
    assert torch.isfinite(dev).all() and torch.equal(dev, host), f"config1 {name}: device update differs by {(dev - host).abs().max()}"
    _assert_same_state(pipe.scheduler, host_sched, f"config1 {name}")
    last = len(trace) - 1
    check(f"config1 {name}, device update, image 0, final latents [bf16]", dev[:1], G[f"{name}_latents_{last}"], "bf16", None,
          f"sd15_config1_sched/{name}_latents_{last}")


def _grab_steps(pipe, kw):
    per_step = []

    def grab(p, i, t, k):
        per_step.append(k["latents"].detach().float().cpu().clone())
        return {}
    ref = pipe(**kw, callback_on_step_end=grab, callback_on_step_end_tensor_inputs=["latents"]).images.float().cpu()
    return per_step, ref


@pytest.mark.parametrize("sched", ["unipc", "pndm_prk"])
def test_device_scheduler_program_replays_the_loop_bit_exactly(sched, tmp_path):
    """export_denoise_step(..., scheduler="device"): the program carries the update; replayed from Python by copying the tables' rows
    into their io buffers only, it gives the pipeline's latents after every step."""
    pipe = _tiny_pipe("bf16")
    mk = (lambda: UniPCMultistepScheduler(**UNIPC_SD)) if sched == "unipc" else (lambda: PNDMScheduler(**SD_SCHED, skip_prk_steps=False))
    inp = synth.pipeline_inputs(2, 16, 32, seed=7, cross_dim=32, vae_scale=2)
    noise = torch.randn(4, 4, 8, 16, generator=torch.Generator().manual_seed(3))
    steps = 6
    pipe.scheduler = mk()
    per_step, ref = _grab_steps(pipe, _call_args(inp, steps, noise))
    pipe.scheduler = mk()
    pipe._graph_state = None
    path = str(tmp_path / "step.mfprog")
    info = pipe.export_denoise_step(path, scheduler="device", **_call_args(inp, steps, noise))
    assert torch.equal(info["result"].images.float().cpu(), ref), "the exporting run itself must give the host loop's latents"
    assert "mf_sched_step_dev" in info["entries"] and "mf_cfg_combine" not in info["entries"] and "mf_axpby_n" not in info["entries"]
    assert "mf_sched_step_dev" in info["meta"]["result"] and type(pipe.scheduler).__name__ in info["meta"]["result"]
    n = len(per_step)
    prog = program.Program(path, DEV)
    meta = json.loads(prog.meta)
    assert meta["entry"] == "mf_denoise_step_fused" and meta["steps"] == n
    shape = per_step[0].shape
    tables = {nm[6:]: prog.buffer(nm) for nm in prog.names if nm.startswith("table.")}
    assert set(tables) == {"sched_row", "temb_unet", "temb_brushnet"}

    def load_row(i):
        for dst, tab in tables.items():
            io = prog.buffer(dst)
            io.copy_(tab.view(n, -1)[i])
    # (1) the file as it is reproduces the recorded step (latents and history after step 0 -> latents after step 1)
    assert torch.equal(prog.buffer("latents", torch.float32).view(shape).cpu(), per_step[0])
    prog.run()
    torch.cuda.synchronize()
    assert torch.equal(prog.buffer("latents", torch.float32).view(shape).cpu(), per_step[1])
    # (2) every step from the initial noise: rows copied in, nothing else
    prog.buffer("latents", torch.float32).copy_(inp["latents"].float().reshape(-1).to(DEV))
    lib = hip.load()
    for i in range(n):
        load_row(i)
        hip._check(lib.mf_denoise_step_fused(prog._h, None, None, None, None, hip._stream()), "mf_denoise_step_fused")
        torch.cuda.synchronize()
        got = prog.buffer("latents", torch.float32).view(shape).cpu()
        assert torch.equal(got, per_step[i]), f"{sched}, step {i}: the program differs from the pipeline by {(got - per_step[i]).abs().max()}"
    prog.close()


def _c_host(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc / ROCm headers on this machine")
    exe = str(tmp_path / "denoise_host")
    libdir = os.path.join(ROOT, "reflecting-reality_amd", "lib")
    subprocess.run([gcc, "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "examples", "c_host", "denoise_host.c"), f"-L{libdir}", "-lmfhip", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return exe, env


def test_c_host_runs_a_unipc_loop(tmp_path):
    """examples/c_host/denoise_host.c, eager and --graph: a 6-step UniPC run (from_config of the PNDM config) from latents_in.bin writes
    the pipeline's latents bit for bit; an eps-form program is refused with a message that names scheduler="device"."""
    exe, env = _c_host(tmp_path)
    pipe = _tiny_pipe("bf16")
    base = PNDMScheduler(**SD_SCHED, skip_prk_steps=True).config
    pipe.scheduler = UniPCMultistepScheduler.from_config(base)
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
        print(out.stdout)
        got = torch.from_numpy(np.fromfile(lat_out, dtype=np.float32)).view(ref.shape)
        assert torch.equal(got, ref), f"C host {extra}: differs from the pipeline by {(got - ref).abs().max()}"
    eps_path = str(tmp_path / "eps.mfprog")
    pipe.scheduler = UniPCMultistepScheduler.from_config(base)
    pipe.export_denoise_step(eps_path, **_call_args(inp, 6, noise))
    out = subprocess.run([exe, eps_path, lat_in], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode != 0 and 'scheduler="device"' in out.stderr, out.stderr[-2000:]
