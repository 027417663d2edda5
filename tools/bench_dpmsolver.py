"""Writes profiles/dpmsolver_bench.txt: kernel resources, accuracy ratios, timings of DPM-Solver++.

    python tools/bench_dpmsolver.py --static      sections 1 and 2, no GPU: the resource lines of the two scheduler-step kernels (hipcc's
                                                  kernel-resource-usage remarks) and the host step()'s error against the reference's float64
                                                  traces as a ratio of the reference's own fp32 deviation (the cases of tests/test_dpmsolver_cpu.py)
    python tools/bench_dpmsolver.py [--config1]   section 3, on the GPU; the other sections of the file are kept

Section 3: (a) the scheduler update alone, batch 4 x 4 x 64 x 64 latents, from a captured graph of 200 updates, in three forms:
mf_sched_step_dev (a UniPC row), mf_sched_step_noise_dev + mf_philox_advance (a DPM-Solver++ SDE row, noise drawn in the kernel), and the
host form of the same SDE step (philox_normal + cfg_combine + the scheduler's two axpby_n).  The three graphs are replayed in turn, 7 rounds
after a warm-up round.  (b) The tiny pipeline and, with --config1, the benchmark's pipeline (batch 4 x 512 x 512, bf16, random weights): 20
DPM-Solver++ steps (2M, 2M Karras, SDE with a PhiloxGenerator) against 50 DDIM steps; the denoise loop by device events, per case 5 calls
after 2 warm-up calls, and the first case once more at the end as a drift check.  Median, minimum and maximum everywhere.
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reflecting_reality_amd import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler, hip, synth  # noqa: E402
from reflecting_reality_amd.rng import PhiloxGenerator  # noqa: E402
from reflecting_reality_amd.schedulers import device_plan  # noqa: E402

DEV = torch.device("cuda", 0)       # (only named here: --static touches no device)
SD = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
REPS = 200


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    return g


def updates():
    shape = (4, 4, 64, 64)
    eu, ec, lat = (torch.randn(shape, device=DEV) for _ in range(3))
    unipc = UniPCMultistepScheduler(**SD)
    unipc.set_timesteps(20)
    pu = device_plan(unipc)
    sde = DPMSolverMultistepScheduler(**SD, algorithm_type="sde-dpmsolver++")
    sde.set_timesteps(20)
    ps = device_plan(sde)
    k = 5                                                        # a full-order step of both
    row_u, row_s = pu.rows[k].to(DEV).contiguous(), ps.rows[k].to(DEV).contiguous()
    st_u = torch.zeros((pu.nslots,) + shape, device=DEV)
    st_s = torch.zeros((ps.nslots,) + shape, device=DEV)
    gen = PhiloxGenerator(1, DEV)
    rng = gen.device_state()
    blocks = hip.philox_normal_blocks(4, 4 * 64 * 64)
    m0, noise = torch.zeros(shape, device=DEV), torch.empty(shape, device=DEV)

    def host_form():                                             # what _HostStep launches for one SDE step
        hip.philox_normal(shape, 1, 0, DEV, out=noise)
        e = hip.cfg_combine(eu, ec, 7.5)
        m = hip.axpby_n([lat, e], [1.1, -0.4])
        hip.axpby_n([lat, m, m0, noise], [0.9, 0.2, -0.1, 0.05], out=lat)

    def noise_form():
        hip.sched_step_noise_dev(eu, ec, 7.5, lat, st_s, row_s, ps.noise_reg, rng_state=rng)
        hip.philox_advance(rng, blocks)

    forms = {"mf_sched_step_dev (UniPC row)": graph_of(lambda: hip.sched_step_dev(eu, ec, 7.5, lat, st_u, row_u)),
             "mf_sched_step_noise_dev + mf_philox_advance (SDE row)": graph_of(noise_form),
             "host form: philox_normal + cfg_combine + 2 x axpby_n": graph_of(host_form)}
    times = {n: [] for n in forms}
    for rnd in range(8):
        for name, g in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(a.elapsed_time(b) * 1e3 / (5 * REPS))
    emit(f"scheduler update alone, latents 4 x 4 x 64 x 64 fp32, {REPS} updates per graph x 5 replays, 7 rounds in turn (us per update)")
    for name, t in times.items():
        emit(f"  {name:58s} median {statistics.median(t):7.2f}  min {min(t):7.2f}  max {max(t):7.2f}")


def pipeline(pipe, inp, h, w, label):
    base = pipe.scheduler.config
    cases = (("DDIM, 50 steps", lambda: DDIMScheduler.from_config(base), 50, None),
             ("DPM-Solver++ 2M, 20 steps", lambda: DPMSolverMultistepScheduler.from_config(base), 20, None),
             ("DPM-Solver++ 2M Karras, 20 steps", lambda: DPMSolverMultistepScheduler.from_config(base, use_karras_sigmas=True), 20, None),
             ("DPM-Solver++ SDE, 20 steps, PhiloxGenerator", lambda: DPMSolverMultistepScheduler.from_config(base, algorithm_type="sde-dpmsolver++"),
              20, PhiloxGenerator(3, DEV)))
    cases += (("DDIM, 50 steps (again, last: drift check)",) + cases[0][1:],)
    emit(f"{label}: denoise loop, device events, ms; per case 2 warm-up calls (the second replays the kept graph), then 5 timed calls")
    for name, mk, steps, gen in cases:
        pipe._graph_state, t = None, []
        for rnd in range(7):
            pipe.scheduler = mk()
            timing = {}
            pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"], mask=inp["mask"],
                 depth=inp["depth"], num_inference_steps=steps, guidance_scale=7.5, latents=inp["latents"], output_type="latent", height=h,
                 width=w, conditioning_noise=inp["vae_noise"], generator=gen, _timing=timing)
            torch.cuda.synchronize()
            if rnd >= 2:
                t.append(timing["denoise_start"].elapsed_time(timing["denoise_end"]))
        emit(f"  {name:46s} median {statistics.median(t):8.1f}  min {min(t):8.1f}  max {max(t):8.1f}   ({statistics.median(t) / steps:6.2f} per step)")


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "dpmsolver_bench.txt")
MARK = "3. Timings on one MI355X"
_lines = []


def emit(line=""):
    print(line, flush=True)
    _lines.append(line)


def static_sections():
    """Sections 1 and 2 (no GPU)."""
    import re
    import subprocess
    import numpy as np
    from reflecting_reality_amd import _build
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_dpmsolver_cpu as T
    emit("DPM-Solver++ (schedulers.DPMSolverMultistepScheduler, mf_sched_step_noise_dev): resources, accuracy ratios, timings")
    emit("(written by tools/bench_dpmsolver.py: --static for sections 1 and 2, on the GPU for section 3)")
    emit()
    emit("1. Kernel resources (hipcc, the library's flags, -Rpass-analysis=kernel-resource-usage on csrc/elementwise.hip)")
    emit()
    res = subprocess.run([_build._hipcc(), *_build.HIPCC_FLAGS, "--cuda-device-only", "-c", os.path.join(_build.CSRC, "elementwise.hip"), "-o",
                          os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
    for kernel, entry in (("17sched_step_kernel", "mf_sched_step_dev"), ("23sched_step_noise_kernel", "mf_sched_step_noise_dev")):
        text = res[res.index("Function Name: _ZN12_GLOBAL__N_1" + kernel):]
        text = text[:text.index("Function Name", 20)]
        v = {m.group(1): m.group(2) for m in re.finditer(r"remark:\s+([\w ]+?)(?: \[[\w/]+\])?: (\w+) \[", text)}
        emit(f"   {kernel[2:]:24s} ({entry + ')':25s} VGPRs {v['VGPRs']:>3s}  AGPRs {v['AGPRs']}  SGPRs {v['TotalSGPRs']}  scratch {v['ScratchSize']} bytes/lane  "
             f"occupancy {v['Occupancy']} waves/SIMD")
    emit()
    emit("   Both kernels are instances of one body (NOISE = false / true).  The extra VGPRs of the second hold the Philox block and the accurate")
    emit("   logf / sinpif / cospif; the register file itself (16 x float4) stays in VGPRs through the same literal-index compare chains.")
    emit()
    emit("2. Host step() against the reference on float64 tensors (the cases and inputs of tests/test_dpmsolver_cpu.py; numpy stand-in for mf_axpby_n)")
    emit()
    emit("   err = max |x - ref64| / (1 + |ref64|) over all steps; ref = the reference's own fp32 deviation max |ref32 - ref64| / (1 + |ref64|)")
    emit("   (tests/golden/dpmsolver_envelope.json); the test's bound is ratio <= 4.")
    emit()
    emit("   case / steps        err        ref        ratio")
    hip.axpby_n = lambda xs, coefs, out=None: torch.from_numpy(T._axpby([x.numpy() for x in xs], coefs))
    G, env = T.golden()
    for (case, n), (x0, mos, noises) in T.trace_inputs().items():
        sch = T.CASES[case]()
        sch.set_timesteps(n)
        got = torch.stack(T._host_steps(sch, x0, mos, noises)).numpy().astype(np.float64)
        ref = G[f"trace/{case}/{n}/ref64"]
        err, dev = (np.abs(got - ref) / (1 + np.abs(ref))).max(), env["fp32"][f"{case}/{n}"]
        emit(f"   {case + '/' + str(n):18s} {err:.3e}  {dev:.3e}  {err / dev:.2f}")
    emit()


if __name__ == "__main__":
    old = open(OUT).read() if os.path.exists(OUT) else ""
    if "--static" in sys.argv:
        static_sections()
        text = "\n".join(_lines) + "\n" + (old[old.index(MARK):] if MARK in old else "")
    else:
        emit(f"{MARK} (device events; one process)")
        emit()
        updates()
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_pipeline_gpu import _tiny_pipe
        tiny = synth.pipeline_inputs(2, 16, 16, seed=17, cross_dim=32, vae_scale=2)
        tiny["vae_noise"] = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(4))
        pipeline(_tiny_pipe("bf16"), tiny, 16, 16, "tiny pipeline (batch 2 x 16 x 16, bf16)")
        if "--config1" in sys.argv:
            import bench
            pipe, _ = bench.build_pipeline("bf16", DEV)
            pipeline(pipe, synth.pipeline_inputs(4, 512, 512), 512, 512, "benchmark pipeline (batch 4 x 512 x 512, bf16, random weights)")
        text = (old[:old.index(MARK)] if MARK in old else old) + "\n".join(_lines) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
