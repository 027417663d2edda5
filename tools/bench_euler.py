"""Writes profiles/euler_bench.txt: kernel note, accuracy ratios, timings of the Euler / Euler-ancestral samplers.

    python tools/bench_euler.py --static                   sections 1 and 2, no GPU: the note on kernels and the host step()'s and
                                                           scale_model_input's error against the reference's float64 traces as a ratio of the
                                                           reference's own fp32 deviation (the cases of tests/test_euler_cpu.py)
    python tools/bench_euler.py [--config1]                section 3, on the GPU; the other sections of the file are kept
    python tools/bench_euler.py --dpm-runs BEFORE AFTER    section 4: two outputs of tools/bench_dpmsolver.py --config1 (profiles/dpmsolver_bench.txt
                                                           of the commit before the Euler classes and of this tree, run on one machine), their
                                                           benchmark-pipeline sections side by side and the no-slower check on DDIM-50 / DPM-2M-20

Section 3: the tiny pipeline and, with --config1, the benchmark's pipeline (batch 4 x 512 x 512, bf16, random weights): 30 Euler steps
(plain, Karras sigmas, ancestral with a PhiloxGenerator) against 50 DDIM steps; the denoise loop by device events, per case 5 calls after
2 warm-up calls, and the first case once more at the end as a drift check (tools/bench_dpmsolver.py's loop).  Median, minimum, maximum.
"""
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from reflecting_reality_amd import DDIMScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, hip, synth  # noqa: E402
from reflecting_reality_amd.rng import PhiloxGenerator  # noqa: E402

DEV = torch.device("cuda", 0)       # (only named here: --static and --dpm-runs touch no device)
OUT = os.path.join(ROOT, "profiles", "euler_bench.txt")
MARK3, MARK4 = "3. Timings on one MI355X", "4. The existing samplers before and after"
_lines = []


def emit(line=""):
    print(line, flush=True)
    _lines.append(line)


def pipeline(pipe, inp, h, w, label):
    base = dict(pipe.scheduler.config, timestep_spacing="leading")       # (explicit, as a checkpoint's scheduler_config.json states it)
    base["_use_default_values"] = [k for k in base.get("_use_default_values", []) if k != "timestep_spacing"]
    cases = (("DDIM, 50 steps", lambda: DDIMScheduler.from_config(base), 50, None),
             ("Euler, 30 steps", lambda: EulerDiscreteScheduler.from_config(base), 30, None),
             ("Euler Karras, 30 steps", lambda: EulerDiscreteScheduler.from_config(base, use_karras_sigmas=True), 30, None),
             ("Euler-ancestral, 30 steps, PhiloxGenerator", lambda: EulerAncestralDiscreteScheduler.from_config(base), 30, PhiloxGenerator(3, DEV)))
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


def static_sections():
    """Sections 1 and 2 (no GPU)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_euler_cpu as T
    from test_sched_plan_cpu import _axpby
    emit("Euler / Euler-ancestral (schedulers.EulerDiscreteScheduler, EulerAncestralDiscreteScheduler): kernels, accuracy ratios, timings")
    emit("(written by tools/bench_euler.py: --static for sections 1 and 2, on the GPU for section 3, --dpm-runs for section 4)")
    emit()
    emit("1. Kernels")
    emit()
    emit("   No kernel was added and none changed.  A step is a row of two ops for mf_sched_step_dev (Euler) or mf_sched_step_noise_dev")
    emit("   (Euler-ancestral): the update into the sample's state slot, then the next step's model input, sample / sqrt(sigma^2 + 1), into the")
    emit("   latents.  Their resource lines are those of profiles/dpmsolver_bench.txt section 1; MF_ABI_VERSION and mf_sched_row are unchanged.")
    emit()
    emit("2. Host step() and scale_model_input against the reference on float64 tensors (the cases and inputs of tests/test_euler_cpu.py; numpy")
    emit("   stand-in for mf_axpby_n)")
    emit()
    emit("   err = max |x - ref64| / (1 + |ref64|) over all steps; ref = the reference's own fp32 deviation max |ref32 - ref64| / (1 + |ref64|)")
    emit("   (tests/golden/euler_envelope.json); the test's bound is ratio <= 4.  `samples`: what step() returns; `inputs`: what")
    emit("   scale_model_input returns before it.")
    emit()
    emit("   case / steps            samples: err  ref        ratio   inputs: err   ref        ratio")
    hip.axpby_n = lambda xs, coefs, out=None: torch.from_numpy(_axpby([x.numpy() for x in xs], coefs))
    G, env = T.golden()
    for (case, n), (x0, mos, noises) in T.trace_inputs().items():
        sch = T.CASES[case]()
        sch.set_timesteps(n)
        cols = []
        for got, ref, dev in zip(T._host_trace(sch, x0, mos, noises), (G[f"trace/{case}/{n}/ref64"], G[f"trace/{case}/{n}/scaled64"]),
                                 (env["fp32"][f"{case}/{n}"], env["fp32"][f"{case}/{n}/scaled"])):
            got = torch.stack(got).numpy().astype(np.float64)
            err = (np.abs(got - ref) / (1 + np.abs(ref))).max()
            cols.append(f"{err:.3e}  {dev:.3e}  {err / dev:.2f}")
        emit(f"   {case + '/' + str(n):22s}  {cols[0]}    {cols[1]}")
    emit()


def _bench_section(text):
    """{case label: (median, min, max)} of the benchmark-pipeline section of a tools/bench_dpmsolver.py output."""
    sec = text[text.index("benchmark pipeline"):]
    rows = re.findall(r"^  (.+?)\s+median\s+([\d.]+)\s+min\s+([\d.]+)\s+max\s+([\d.]+)", sec, flags=re.M)
    return {name.strip(): tuple(float(v) for v in vals) for name, *vals in rows}, sec.rstrip().splitlines()


def dpm_runs(before_path, after_path):
    emit(f"{MARK4} (tools/bench_dpmsolver.py --config1 of the commit before the Euler classes, then of this tree, one after the other on")
    emit("   one machine; benchmark pipeline, batch 4 x 512 x 512, bf16; ms)")
    emit()
    runs = {}
    for label, path in (("before", before_path), ("after", after_path)):
        runs[label], lines = _bench_section(open(path).read())
        emit(f"   {label}:")
        for line in lines:
            emit("   " + line)
        emit()
    b, a = runs["before"], runs["after"]
    first, last = b["DDIM, 50 steps"], b["DDIM, 50 steps (again, last: drift check)"]
    emit("   Check: this tree's median lies no further from the earlier commit's than that run's own spread, its first-to-last DDIM drift plus")
    emit("   the min-max of its five calls.")
    ok = True
    for case in ("DDIM, 50 steps", "DPM-Solver++ 2M, 20 steps"):
        spread = abs(first[0] - last[0]) + (b[case][2] - b[case][1])
        diff = a[case][0] - b[case][0]
        good = abs(diff) <= spread
        ok = ok and good
        emit(f"   {case:28s} before {b[case][0]:8.1f}  after {a[case][0]:8.1f}  difference {diff:+7.1f}  spread {spread:6.1f}  {'inside' if good else 'OUTSIDE'}")
    emit()
    return ok


if __name__ == "__main__":
    old = open(OUT).read() if os.path.exists(OUT) else ""
    cut = lambda s, mark: s[:s.index(mark)] if mark in s else s
    if "--static" in sys.argv:
        static_sections()
        text = "\n".join(_lines) + "\n" + (old[old.index(MARK3):] if MARK3 in old else "")
    elif "--dpm-runs" in sys.argv:
        i = sys.argv.index("--dpm-runs")
        dpm_runs(sys.argv[i + 1], sys.argv[i + 2])
        text = cut(old, MARK4) + "\n".join(_lines) + "\n"
    else:
        emit(f"{MARK3} (device events; one process)")
        emit()
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_pipeline_gpu import _tiny_pipe
        tiny = synth.pipeline_inputs(2, 16, 16, seed=17, cross_dim=32, vae_scale=2)
        tiny["vae_noise"] = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(4))
        pipeline(_tiny_pipe("bf16"), tiny, 16, 16, "tiny pipeline (batch 2 x 16 x 16, bf16)")
        if "--config1" in sys.argv:
            import bench
            pipe, _ = bench.build_pipeline("bf16", DEV)
            pipeline(pipe, synth.pipeline_inputs(4, 512, 512), 512, 512, "benchmark pipeline (batch 4 x 512 x 512, bf16, random weights)")
        emit()
        text = cut(cut(old, MARK4), MARK3) + "\n".join(_lines) + "\n" + (old[old.index(MARK4):] if MARK4 in old else "")
    with open(OUT, "w") as f:
        f.write(text)
