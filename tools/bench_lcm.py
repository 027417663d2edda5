"""Writes profiles/lcm_bench.txt: kernel resources, accuracy ratios and timings of LCM sampling (schedulers.LCMScheduler).

    python tools/bench_lcm.py --static [--parent-log FILE]  sections 1 and 2, no GPU: the four instantiations' resource lines (FILE: the
                                                           compiler's -Rpass-analysis=kernel-resource-usage output for csrc/elementwise.hip
                                                           on the commit before the compile-time guidance form), and the host step()'s
                                                           error per step against the reference's float64 traces as a ratio of the
                                                           reference's own fp32 deviation (the cases of tests/test_lcm_cpu.py)
    python tools/bench_lcm.py [--config1]                  section 3, on the GPU; the other sections of the file are kept
    python tools/bench_lcm.py --dpm-runs BEFORE AFTER [BEFORE AFTER ...]
                                                           section 4: outputs of tools/bench_dpmsolver.py --config1 (of the commit before
                                                           this sampler and of this tree, one process each, on one machine) side by side and
                                                           the inside-each-other's-range check on DDIM-50 / DPM-2M-20; further pairs are
                                                           repeats (other sessions, other order of the processes): their check lines only

Section 3: the tiny pipeline and, with --config1, the benchmark's pipeline (batch 4 x 512 x 512, bf16, random weights): 4 LCM steps at
guidance_scale 1.0 through the captured step, the same call with use_hip_graph off, 4 LCM steps at 1.5 (classifier-free guidance on);
the denoise loop by device events, per case 5 calls after 2 warm-up calls, and the first case once more at the end as a drift check.
"""
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from reflecting_reality_amd import LCMScheduler, hip, synth  # noqa: E402
from reflecting_reality_amd.rng import PhiloxGenerator  # noqa: E402

DEV = torch.device("cuda", 0)       # (only named here: --static and --dpm-runs touch no device)
OUT = os.path.join(ROOT, "profiles", "lcm_bench.txt")
MARK3, MARK4 = "3. Timings on one MI355X", "4. The existing samplers before and after"
_lines = []


def emit(line=""):
    print(line, flush=True)
    _lines.append(line)


def pipeline(pipe, inp, h, w, label):
    base = pipe.scheduler.config
    nb = inp["latents"].shape[0]
    cases = (("LCM, 4 steps, guidance 1.0, captured step", 1.0, True), ("LCM, 4 steps, guidance 1.0, use_hip_graph off", 1.0, False),
             ("LCM, 4 steps, guidance 1.5 (CFG), captured step", 1.5, True))
    cases += (("LCM, 4 steps, guidance 1.0, captured step (again: drift)",) + cases[0][1:],)
    emit(f"{label}: denoise loop, device events, ms; per case 2 warm-up calls (the second replays the kept graph), then 5 timed calls")
    gen = PhiloxGenerator(3, DEV)
    was = pipe.use_hip_graph
    for name, g, graph in cases:
        pipe._graph_state, pipe.use_hip_graph, t = None, graph, []
        noise = inp["vae_noise"] if g > 1 else inp["vae_noise"][:nb]
        pe = dict(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"])
        for rnd in range(7):
            pipe.scheduler = LCMScheduler.from_config(base)
            timing = {}
            pipe(**pe, image=inp["image"], mask=inp["mask"], depth=inp["depth"], num_inference_steps=4, guidance_scale=g, latents=inp["latents"],
                 output_type="latent", height=h, width=w, conditioning_noise=noise, generator=gen, _timing=timing)
            torch.cuda.synchronize()
            if rnd >= 2:
                t.append(timing["denoise_start"].elapsed_time(timing["denoise_end"]))
        emit(f"  {name:56s} median {statistics.median(t):8.2f}  min {min(t):8.2f}  max {max(t):8.2f}   ({statistics.median(t) / 4:6.2f} per step)")
    pipe.use_hip_graph = was


def _resources(text):
    out = {}
    for block in text.split("Function Name: ")[1:]:
        m = re.match(r"_ZN12_GLOBAL__N_1\d+(sched_step(?:_noise)?_kernel)(?:ILb([01])E)?", block.split()[0])
        if m:
            v = dict(re.findall(r"remark:\s+([\w ]+?)(?: \[[\w/]+\])?: (\d+) \[", block))
            out[m.group(1) + ("" if m.group(2) is None else "<guided>" if m.group(2) == "1" else "<unguided>")] = v
    return out


def static_sections(parent_log):
    """Sections 1 and 2 (no GPU)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_lcm_cpu as T
    from reflecting_reality_amd import _build
    from test_sched_plan_cpu import _axpby
    emit("LCM sampling (schedulers.LCMScheduler; the no-guidance form of mf_sched_step_dev / mf_sched_step_noise_dev): resources, accuracy, timings")
    emit("(written by tools/bench_lcm.py: --static for sections 1 and 2, on the GPU for section 3, --dpm-runs for section 4)")
    emit()
    emit("1. Kernels (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    emit()
    emit("   sched_step_kernel / sched_step_noise_kernel gained a compile-time parameter: <guided> is the code there was, <unguided> (g < 0 at the")
    emit("   entry) takes register 0 from eps_u as loaded and has no load of eps_c.  MF_ABI_VERSION, the signatures and mf_sched_row are unchanged.")
    emit()
    res = subprocess.run([_build._hipcc(), *_build.HIPCC_FLAGS, "--cuda-device-only", "-c", os.path.join(_build.CSRC, "elementwise.hip"), "-o",
                          os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    tables = [("this tree", _resources(res.stderr))]
    if parent_log:
        tables.insert(0, ("the commit before", _resources(open(parent_log).read())))
    for label, tab in tables:
        emit(f"   {label}:")
        for name in sorted(tab):
            v = tab[name]
            emit(f"     {name:36s} VGPRs {v['VGPRs']:>3s}  SGPRs {v['TotalSGPRs']:>3s}  scratch {v['ScratchSize']} B/lane  occupancy {v['Occupancy']} waves/SIMD")
    emit()
    emit("2. Host step() against the reference on float64 tensors (the cases and inputs of tests/test_lcm_cpu.py; numpy stand-in for mf_axpby_n)")
    emit()
    emit("   per step: err = max |x - ref64| / (1 + |ref64|); ref = the reference's own fp32 deviation max |ref32 - ref64| / (1 + |ref64|)")
    emit("   (tests/golden/lcm_envelope.json); the test's bound is ratio <= 4 at every step.")
    emit()
    emit("   prediction type / step   prev_sample: err  ref        ratio   denoised: err   ref        ratio")
    hip.axpby_n = lambda xs, coefs, out=None: torch.from_numpy(_axpby([x.numpy() for x in xs], coefs))
    G, env = T.golden()
    for p, (x0, mos, noises) in T.trace_inputs().items():
        sch = LCMScheduler(**T.SD, prediction_type=p)
        sch.set_timesteps(T.STEPS)
        prevs, dens = T._host_steps(sch, x0, mos, noises)
        for k in range(T.STEPS):
            cols = []
            for got, ref, dev in ((prevs, G[f"trace/{p}/ref64"], env["fp32"][p]), (dens, G[f"trace/{p}/den64"], env["fp32"][f"{p}/denoised"])):
                err = (np.abs(got[k].numpy().astype(np.float64) - ref[k]) / (1 + np.abs(ref[k]))).max()
                cols.append(f"{err:.3e}  {dev[k]:.3e}  {err / dev[k]:.2f}")
            emit(f"   {p + ' / ' + str(k):24s} {cols[0]}    {cols[1]}")
    emit()
    emit("   epsilon: the folded coefficients of sample and model output are +-c_out / sqrt(alpha_t) (15 at t = 999) and their products cancel,")
    emit("   where the reference subtracts first and divides after; v_prediction and sample are the reference's own two operations.")
    emit()


def _bench_section(text):
    """{case label: (median, min, max)} of the benchmark-pipeline section of a tools/bench_dpmsolver.py output."""
    sec = text[text.index("benchmark pipeline"):]
    rows = re.findall(r"^  (.+?)\s+median\s+([\d.]+)\s+min\s+([\d.]+)\s+max\s+([\d.]+)", sec, flags=re.M)
    return {name.strip(): tuple(float(v) for v in vals) for name, *vals in rows}, sec.rstrip().splitlines()


def dpm_runs(paths, notes=()):
    emit(f"{MARK4} (tools/bench_dpmsolver.py --config1 of the commit before this sampler, then of this tree, one after the other in one")
    emit("   session on one machine; benchmark pipeline, batch 4 x 512 x 512, bf16; ms)")
    emit()
    ok = True
    for n in range(0, len(paths), 2):
        ok = _dpm_pair(paths[n], paths[n + 1], n // 2) and ok
    for line in notes:
        emit("   " + line)
    if notes:
        emit()
    return ok


def _dpm_pair(before_path, after_path, index):
    runs = {}
    for label, path in (("before", before_path), ("after", after_path)):
        runs[label], lines = _bench_section(open(path).read())
        if index == 0:
            emit(f"   {label}:")
            for line in lines:
                emit("   " + line)
            emit()
    b, a = runs["before"], runs["after"]
    if index == 0:
        emit("   Check: each run's median lies inside the other's repeat range, the min-max of its five calls widened by that run's own")
        emit("   first-to-last DDIM drift.")
    else:
        emit(f"   Repeat {index}:")
    ok = True
    for case in ("DDIM, 50 steps", "DPM-Solver++ 2M, 20 steps"):
        verdicts = []
        for x, y in ((a, b), (b, a)):
            drift = abs(y["DDIM, 50 steps"][0] - y["DDIM, 50 steps (again, last: drift check)"][0])
            verdicts.append(y[case][1] - drift <= x[case][0] <= y[case][2] + drift)
        ok = ok and all(verdicts)
        emit(f"   {case:28s} before {b[case][0]:8.1f} [{b[case][1]:.1f}, {b[case][2]:.1f}]  after {a[case][0]:8.1f} [{a[case][1]:.1f}, {a[case][2]:.1f}]  "
             f"{'inside' if all(verdicts) else 'OUTSIDE'}")
    emit()
    return ok


if __name__ == "__main__":
    old = open(OUT).read() if os.path.exists(OUT) else ""
    cut = lambda s, mark: s[:s.index(mark)] if mark in s else s
    if "--static" in sys.argv:
        static_sections(sys.argv[sys.argv.index("--parent-log") + 1] if "--parent-log" in sys.argv else None)
        text = "\n".join(_lines) + "\n" + (old[old.index(MARK3):] if MARK3 in old else "")
    elif "--dpm-runs" in sys.argv:
        i = sys.argv.index("--dpm-runs")
        j = sys.argv.index("--note") if "--note" in sys.argv else len(sys.argv)
        dpm_runs(sys.argv[i + 1:j], sys.argv[j + 1:])
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
