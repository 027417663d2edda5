#!/usr/bin/env python
"""bench.py — images/sec of the MirrorFusion hot path (SD1.5 + BrushNet depth-conditioned inpainting) on MI355X.

Contract (one JSON line on rank 0): a "step" is one pass of the whole accelerated path over one batch of synthetic
inputs: conditioning build (incl. VAE-encode of the masked image) + `--denoise-steps` DDIM steps of BrushNet+UNet
with classifier-free guidance 7.5 + VAE decode.  Default workload = BASELINE.json configs[1]:
batch 4 x 512x512, 50-step DDIM, bf16, one MI355X.  With --gpus N each rank runs the same per-GPU batch on its own
images (weak scaling, no data-path collective); value = images all ranks produced / max-over-ranks time.

    python bench.py --gpus 1 --steps 3 --warmup 1
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29511 \
        bench.py --gpus 8 --steps 3 --warmup 1

A plain run sets up, warms up, times `--steps` passes and prints the line.  Everything else the line can carry (the
roofline / FLOP census pass, host-input, shared-sample and f16x3 parity passes, the fp16 / training / SDXL legs, the CPU
baseline, the training all-reduce time) runs only with --full.  --dump-outputs DIR writes what the last timed pass
returned as DIR/<name>.npy (float32; rank 0), from inputs that are the same on every run with the same arguments.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

GFLOP_PER_IMAGE_STEP = {512: 2489.2, 256: 581.0}      # BASELINE.md §2 (CFG on): BrushNet 882.6 + UNet 1606.5 @512
PEAK_BF16_TFLOPS = 2500.0                             # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3
PEAK_FP8_TFLOPS = 5000.0                              # dense e4m3 (block-scaled MFMA forms): 2 x the bf16 rate


def log(*a):
    print(*a, file=sys.stderr, flush=True)


DUMP_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every tensor as out_dir/<name>.npy in float32.  A tensor larger than its share of DUMP_BYTES is
    replaced by a fixed sample of its flattened elements (seeded indices, ascending), the same on every run."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    cap = DUMP_BYTES // 4 // max(1, len(arrays))
    for name, t in arrays.items():
        t = t.detach()
        sampled = t.numel() > cap
        if sampled:
            idx = torch.randint(0, t.numel(), (cap,), generator=torch.Generator().manual_seed(0)).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        arr = t.float().cpu().numpy()
        np.save(os.path.join(out_dir, f"{name}.npy"), arr)
        log(f"[bench] wrote {name}.npy {list(arr.shape)}{' (sampled)' if sampled else ''} to {out_dir}")


def build_pipeline(precision, device, keep_cpu_sd=False, model="sd15"):
    from reflecting_reality_amd import (AutoencoderKL, BrushNetModel, DDIMScheduler, StableDiffusionBrushNetPipeline,
                                        StableDiffusionXLBrushNetPipeline, UNet2DConditionModel, synth)
    from reflecting_reality_amd.configs import SD15_SCHED, SD15_UNET, SD15_VAE, SDXL_UNET, SDXL_VAE, brushnet_config
    t0 = time.time()
    sds = {}
    if model == "sdxl":          # SURVEY.md §8 f-3 (config 5): secondary workload, same engine
        SD15_UNET, SD15_VAE, cond_ch = SDXL_UNET, SDXL_VAE, 5
    else:
        cond_ch = 6
    unet = UNet2DConditionModel(dict(SD15_UNET), precision=precision, device=device)
    sd = synth.state_dict_for(unet.param_shapes(), 0)
    unet.load_state_dict(sd)
    sds["unet"] = sd
    bn = BrushNetModel(dict(brushnet_config(SD15_UNET, cond_ch)), precision=precision, device=device)
    sd = synth.state_dict_for(bn.param_shapes(), 1)
    bn.load_state_dict(sd)
    sds["brushnet"] = sd
    vae = AutoencoderKL(dict(SD15_VAE), precision=precision, device=device)
    sd = synth.state_dict_for(vae.param_shapes(), 2)
    vae.load_state_dict(sd)
    sds["vae"] = sd
    for m in (unet, bn, vae):
        m._src = None
    sched = DDIMScheduler(**{k: v for k, v in SD15_SCHED.items() if k != "skip_prk_steps"})
    if model == "sdxl":
        pipe = StableDiffusionXLBrushNetPipeline(vae=vae, text_encoder=None, text_encoder_2=None, tokenizer=None,
                                                 tokenizer_2=None, unet=unet, brushnet=bn, scheduler=sched)
    else:
        pipe = StableDiffusionBrushNetPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, brushnet=bn,
                                               scheduler=sched, safety_checker=None, feature_extractor=None,
                                               requires_safety_checker=False, depth_conditioning_mode="concat")
    pipe.set_progress_bar_config(disable=True)
    log(f"[bench] models built in {time.time() - t0:.1f}s (seeded random weights, {model} shapes)")
    return pipe, (sds if keep_cpu_sd else None)


def cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or "unknown"


def cpu_baseline(sds, size, threads, denoise_steps):
    """The CPU oracle (a port of the reference's arithmetic, pinned bit-exact to it) on the host cores at the workload's
    OWN shapes: one image at `size` x `size`, TWO denoise steps (BrushNet + UNet on the CFG batch of 2) + VAE encode +
    decode, timed with torch.utils.benchmark.Timer (the reference's idiom, benchmarks/utils.py:52-58) after one untimed
    step.  Only the step count is extrapolated (the per-step cost does not depend on the step index).  Beside it:
    BASELINE.json configs[0] (1 x 256 x 256, 4 DDIM steps + VAE) measured whole, nothing extrapolated."""
    from torch.utils import benchmark
    from oracle import mirrorfusion_ref as R
    torch.set_num_threads(threads)
    g = torch.Generator().manual_seed(7)
    bcfg = R.brushnet_config(R.SD15_UNET, 6)

    def make(sz):
        hl = sz // 8
        return dict(lat=torch.randn(1, 4, hl, hl, generator=g), cond=torch.randn(2, 6, hl, hl, generator=g),
                    ehs=torch.randn(2, 77, 768, generator=g), img=torch.randn(1, 3, sz, sz, generator=g))

    def steps(d, n):
        lat = d["lat"]
        for _ in range(n):
            x2 = torch.cat([lat] * 2)
            dn, m, u = R.brushnet_forward(sds["brushnet"], bcfg, x2, 981, d["cond"], 1.0)
            eps = R.unet_forward(sds["unet"], R.SD15_UNET, x2, 981, d["ehs"], dn, m, u)
            lat = lat - 1e-3 * (eps[:1] + 7.5 * (eps[1:] - eps[:1]))        # keep the steps data-dependent
        return lat

    def vae(d):
        R.vae_decode(sds["vae"], R.SD15_VAE, d["lat"])
        R.vae_encode_moments(sds["vae"], R.SD15_VAE, d["img"])

    with torch.no_grad():
        d1 = make(size)
        steps(d1, 1)                                                        # warm-up: thread pool, first-touch pages
        t_steps = benchmark.Timer(stmt="f(d, 2)", globals=dict(f=steps, d=d1), num_threads=threads).timeit(1).mean
        t_vae = benchmark.Timer(stmt="f(d)", globals=dict(f=vae, d=d1), num_threads=threads).timeit(1).mean
        d0 = make(256)
        t_cfg0 = benchmark.Timer(stmt="f(d, 4); v(d)", globals=dict(f=steps, v=vae, d=d0), num_threads=threads).timeit(1).mean
    return t_steps / 2.0, t_vae, t_cfg0


def self_launch(argv, n):
    """`python bench.py --gpus N` without a torchrun environment: start the N ranks as CHILD processes (this parent has
    not touched the GPU and only waits: a process that has initialised the GPU must never exec another program) and relay
    their output; rank 0 prints the JSON line."""
    import subprocess
    from reflecting_reality_amd.distributed import torchrun_argv      # imports torch only: nothing touches the GPU
    cmd = torchrun_argv(n) + [os.path.abspath(__file__)] + argv      # the rendezvous store binds its own free port
    log(f"[bench] --gpus {n} without WORLD_SIZE: launching {n} ranks: {' '.join(cmd)}")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def stub_main(a, D):
    """--stub: the multi-rank skeleton of main() with a sleeping pass (rank r sleeps 20 ms * (r + 1) per pass)."""
    rank, world, _ = D.init_process_group("gloo")
    if world != a.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus {a.gpus}")
    if a.dump_outputs:
        raise SystemExit("bench.py: --stub computes nothing to dump")
    for _ in range(a.warmup):
        time.sleep(0.001)
    D.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        time.sleep(0.02 * (rank + 1))
    D.barrier()
    elapsed = D.max_over_ranks(time.perf_counter() - t0)
    if rank == 0:
        print(json.dumps({"metric": "stub", "value": round(a.batch * a.steps * world / elapsed, 4), "unit": "images/sec",
                          "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 2),
                          "higher_is_better": True, "scaling": "weak", "data": "stub"}), flush=True)
    D.barrier()


def train_main(a, D):
    """--mode train: BASELINE.json configs[3] — the MirrorFusion fine-tune step (train_brushnet_mirror.py:1407-1466) on
    synthetic latents: BrushNet trains, the UNet is frozen (the script's default), per-GPU batch `--batch` (8), 512 x 512
    (64 x 64 latents), fp32 master weights, split-precision (f16x3) or fp32-MFMA contractions, clip 1.0, AdamW; with
    --gpus N every rank trains its own batch and the gradient arena is all-reduced in buckets over RCCL under the
    backward pass.  Secondary workload: reported with its own metric, never as the inference number."""
    from reflecting_reality_amd import (BrushNetModel, DDPMScheduler, UNet2DConditionModel, hip, synth)
    from reflecting_reality_amd.configs import SD15_SCHED, SD15_UNET, brushnet_config
    from reflecting_reality_amd.training import AdamW, GraphedTrainStep, MirrorFusionModel, train_step
    backend = os.environ.get("MF_BENCH_BACKEND") or None
    rank, world, local = D.init_process_group(backend)
    if world != a.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus {a.gpus}")
    if backend == "gloo":
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    hip.load()
    # --precision bf16 (the default) = the arithmetic of the reference's --mixed_precision=bf16: bf16 products on pre-rounded operands,
    # fp32 master weights / residual stream / summed gradients ("bf16x1", pinned to the reference's own bf16 deviation); f16x3 is the
    # mode that meets the fp32-class bounds (2e-4 of every gradient) and fp32 the plain one
    prec = {"bf16": "bf16x1"}.get(a.precision, a.precision)
    prec = prec if prec in ("fp32", "f16x3", "bf16x1") else "f16x3"
    t0 = time.time()
    unet = UNet2DConditionModel(dict(SD15_UNET), precision=prec, device=device)
    unet.load_state_dict(synth.state_dict_for(unet.param_shapes(), 0))
    bn = BrushNetModel(dict(brushnet_config(SD15_UNET, 6)), precision=prec, device=device)
    bn.load_state_dict(synth.state_dict_for(bn.param_shapes(), 1))
    model = MirrorFusionModel(unet, bn).prepare_training(train_base_unet=a.train_base_unet)
    opt = AdamW(model.get_trainable_modules(), lr=1e-5)
    sync = D.GradBuckets(model.get_trainable_modules()) if (world > 1 or os.environ.get("MF_FORCE_GRAD_SYNC") == "1") else None
    ns = DDPMScheduler(**{k: v for k, v in SD15_SCHED.items() if k in ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule")})
    log(f"[bench] training models built in {time.time() - t0:.1f}s: BrushNet {bn.num_arena_floats() / 1e6:.1f} M trainable floats")
    hl = a.size // 8
    g = torch.Generator().manual_seed(99 + rank)
    b = a.batch
    lat, noi = torch.randn(b, 4, hl, hl, generator=g).to(device) * 0.8, torch.randn(b, 4, hl, hl, generator=g).to(device)
    cond, ehs = torch.randn(b, 6, hl, hl, generator=g).to(device), torch.randn(b, 77, 768, generator=g).to(device)

    # one process, no gradient sync: zero_grad + forward + backward + clip replayed from one hipGraph (training.GraphedTrainStep;
    # its first two calls are the eager step — run them inside the warm-up).  MF_TRAIN_GRAPH=0: the eager step throughout.
    graphed = GraphedTrainStep(model, ns, opt, max_grad_norm=1.0, grad_sync=sync) if os.environ.get("MF_TRAIN_GRAPH", "1") != "0" else None

    def one_step(i):
        ts = torch.randint(0, 1000, (b,), generator=g)
        if graphed is not None:
            return graphed(lat, noi, ts, ehs, cond)
        return train_step(model, ns, opt, lat, noi, ts, ehs, cond, max_grad_norm=1.0, grad_sync=sync)

    def warm():
        if graphed is not None and a.warmup < 3:
            for i in range(3 - a.warmup):        # untimed: the graph is captured on the third call
                one_step(i)
        for i in range(a.warmup):
            one_step(i)

    if sync is None:
        D.tuned_once(warm)                       # (with a gradient sync every rank must take part in every step's exchange)
    else:
        warm()
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        loss, norm = one_step(i)
    D.barrier()
    torch.cuda.synchronize()
    reduce_device = "cpu" if backend == "gloo" else device
    elapsed = D.max_over_ranks(time.perf_counter() - t0, device=reduce_device)
    assert torch.isfinite(loss).all() and torch.isfinite(norm).all()
    if a.dump_outputs and rank == 0:
        # what train_step hands back, and a fixed sample of each trainable network's fp32 master weights after the step
        dump_outputs(a.dump_outputs, {"loss": loss, "grad_norm": norm,
                                      **{f"{type(m).__name__.lower()}_weights": m.flat_w[:m.num_arena_floats()]
                                         for m in model.get_trainable_modules()}})
    # configs[3] asks for the all-reduce time beside samples/s: one un-overlapped pass over every gradient bucket, after
    # the timed steps (inside a step the buckets are reduced on a side stream under the backward pass)
    ar_ms = sync.time_all_reduce() if sync is not None and a.full else None
    ar_bytes = sum(m.num_arena_floats() for m in model.get_trainable_modules()) * 4
    if rank == 0:
        gflop = 3 * 441.3 + 2 * 803.3            # per sample: BrushNet fwd + dgrad + wgrad, frozen UNet fwd + dgrad (no CFG)
        step_s = elapsed / a.steps
        print(json.dumps({
            "metric": f"samples/sec, MirrorFusion fine-tune step at 512x512 (BrushNet trains, UNet {'trains' if a.train_base_unet else 'frozen'}) — secondary workload",
            "value": round(b * a.steps * world / elapsed, 4), "unit": "samples/sec", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(step_s * 1e3, 2), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": prec, "data": "synthetic",
            "config": {"workload": f"train_brushnet_mirror.py step, per-GPU batch {b} x {a.size}x{a.size}, BrushNet(6 cond ch) trainable / UNet "
                                   f"{'trainable' if a.train_base_unet else 'frozen'}, clip 1.0, AdamW lr 1e-5, random-init weights", "per_gpu_batch": b, "global_batch": b * world,
                       "parallelism": f"data-parallel x{world}" + (" (bucketed gradient all-reduce over RCCL)" if world > 1 else ""),
                       "launch": "hipGraph replay (forward + backward + clip), eager noising / optimizer" if graphed is not None else "eager"},
            "all_reduce": ({"ms": round(ar_ms, 2), "bytes": ar_bytes, "GB/s_per_rank": round(2 * (world - 1) / max(world, 1) * ar_bytes / (ar_ms * 1e-3) / 1e9, 1),
                            "note": "one un-overlapped bucketed all-reduce of the gradient arenas (64 Mi-float buckets), measured after the timed steps; "
                                    "in the step it runs on a side stream under the backward pass"} if ar_ms else None),
            "achieved_tflops": round(b * gflop * 1e9 / step_s / 1e12, 2),
            # the whole step (forward, data and weight gradients, norms, clip, AdamW) against the dense bf16 MFMA peak: the
            # algorithmic contraction FLOPs of the step / its wall time.  fp32 mode: fp32 MFMA peak; f16x3: three MFMAs per product
            "roofline": {"bound": "mfma", "kernel": "whole training step (gemm_conv_kernel forward + dgrad, conv_wgrad, flash backward)",
                         "achieved": round(b * gflop * 1e9 / step_s / 1e12, 2), "peak": PEAK_F32_TFLOPS if prec == "fp32" else PEAK_BF16_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(b * gflop * 1e9 / step_s / 1e12 / (PEAK_F32_TFLOPS if prec == "fp32" else PEAK_BF16_TFLOPS), 4),
                         "traffic": None, "algorithmic_gflop_per_step": round(b * gflop, 1),
                         "note": "per sample 3 x 441.3 (BrushNet forward + dgrad + wgrad) + 2 x 803.3 (frozen UNet forward + dgrad) GFLOP, BASELINE.md"},
            "algorithmic_gflop_per_sample": round(gflop, 1), "last_loss": round(float(loss), 5), "last_grad_norm": round(float(norm), 5)}),
            flush=True)
        hip.tune_save()
        if os.path.isdir("gpurun_out"):
            hip.tune_save(os.path.join("gpurun_out", "tune_cache_new.json"))
    D.barrier()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="infer", choices=["infer", "train"],
                    help="infer = BASELINE.json's north-star workload; train = configs[3], the fine-tune step (secondary)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=None, help="images per GPU per step (default 4; 8 for --mode train)")
    ap.add_argument("--size", type=int, default=None, help="image side (default 512; 1024 for --model sdxl)")
    ap.add_argument("--model", default="sd15", choices=["sd15", "sdxl"],
                    help="sd15 = BASELINE.json's north-star workload; sdxl = the §8 f-3 secondary workload")
    ap.add_argument("--denoise-steps", type=int, default=None, help="default 50; 30 for --model sdxl (BASELINE.json configs[4])")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "f16x3", "bf16x3", "bf16x1", "fp8"])
    ap.add_argument("--no-parity-mode", action="store_true",
                    help="skip the extra passes in the f16x3 parity mode (the mode that meets the 1e-3 latent bound)")
    ap.add_argument("--inputs", default="device", choices=["device", "host"],
                    help="device: inputs resident in HBM when the timed region starts (the contract's `value`); host: the "
                         "caller hands over host tensors, so every pass pays preprocessing on the CPU and the PCIe upload")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--train-base-unet", action="store_true", help="--mode train: the UNet trains too (train_brushnet_mirror.py --train_base_unet)")
    ap.add_argument("--stub", action="store_true",
                    help="test hook: a sleeping stand-in for the pipeline on the CPU (gloo), to exercise the rank logic — "
                         "launch, rendezvous, barrier, max-over-ranks timing, the JSON line — where there is no GPU")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="skip the secondary legs of the default line: fp16 mode, the training step (configs[3]) and SDXL fp8 (configs[4])")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every secondary measurement of the line (roofline, host inputs, shared "
                         "sample, f16x3 parity, fp16 / train / SDXL legs, CPU baseline, training all-reduce); the --no-* options "
                         "switch single ones off again.  Without it only the headline passes run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32, at most 64 MB; rank 0)")
    a = ap.parse_args()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(sys.argv[1:], a.gpus))          # before anything touches the GPU
    xl = a.model == "sdxl"
    if a.batch is None:          # BASELINE.json: configs[1] batch 4, configs[3] per-GPU batch 8, configs[4] (SDXL) batch 2
        a.batch = 8 if a.mode == "train" else 2 if xl else 4
    if a.denoise_steps is None:  # configs[1] 50-step DDIM, configs[4] 30-step
        a.denoise_steps = 30 if xl else 50
    if a.size is None:
        a.size = 1024 if xl else 512

    from reflecting_reality_amd import distributed as D
    if a.stub:
        return stub_main(a, D)
    if a.mode == "train":
        if a.size is None:
            a.size = 512
        return train_main(a, D)
    from reflecting_reality_amd import hip, synth
    # MF_BENCH_BACKEND=gloo: test hook for boxes with fewer GPUs than ranks (ranks then share devices, timings mean
    # nothing); the driver's multi-GPU runs use the default, "nccl" = RCCL, one rank per GPU
    backend = os.environ.get("MF_BENCH_BACKEND") or None
    rank, world, local = D.init_process_group(backend)
    if world != a.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus {a.gpus}: launch with torch.distributed.run "
                         f"--nproc-per-node {a.gpus} (or plain `python bench.py --gpus {a.gpus}`, which starts the ranks itself)")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the hot path has no CPU fallback")
    if backend == "gloo":
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    reduce_device = "cpu" if backend == "gloo" else device
    hip.load()
    # host preprocessing is a few 12 MB elementwise ops and copies: a small OpenMP team avoids the wake-up jitter of a
    # 100+-core host (cpu_baseline sets its own thread count later)
    torch.set_num_threads(max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8)))

    want_cpu = a.full and rank == 0 and world == 1 and not a.no_cpu_baseline and not xl
    pipe, sds = build_pipeline(a.precision, device, keep_cpu_sd=want_cpu, model=a.model)
    # every rank works on its own images: rank-dependent seed, same shapes (weak scaling)
    inp = synth.pipeline_inputs(a.batch, a.size, a.size, seed=1234 + rank, cross_dim=2048 if xl else 768)
    timing = {}
    if xl:
        gp = torch.Generator().manual_seed(4321 + rank)
        pooled, npooled = torch.randn(a.batch, 1280, generator=gp), torch.randn(a.batch, 1280, generator=gp)
    inp_host = inp
    if a.inputs == "device":
        inp = {k: v.to(device) for k, v in inp.items()}
        if xl:
            pooled, npooled = pooled.to(device), npooled.to(device)
        torch.cuda.synchronize()
    inp_timed = inp

    def one_pass():
        if xl:
            return pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"],
                        pooled_prompt_embeds=pooled, negative_pooled_prompt_embeds=npooled, image=inp["image"],
                        mask=inp["mask"], num_inference_steps=a.denoise_steps, guidance_scale=7.5, latents=inp["latents"],
                        output_type="pt", brushnet_conditioning_scale=1.0, height=a.size, width=a.size,
                        conditioning_noise=inp["vae_noise"], _timing=timing).images
        return pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"],
                    image=inp["image"], mask=inp["mask"], depth=inp["depth"], num_inference_steps=a.denoise_steps,
                    guidance_scale=7.5, latents=inp["latents"], output_type="pt", brushnet_conditioning_scale=1.0,
                    height=a.size, width=a.size, conditioning_noise=inp["vae_noise"], _timing=timing).images

    # several ranks and a cold tune cache: rank 0 warms (and tunes) first, the others read its winners (distributed.tuned_once)
    D.tuned_once(lambda: [one_pass() for _ in range(a.warmup)])
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    denoise_ms = 0.0
    for _ in range(a.steps):
        tp0 = time.perf_counter()
        img = one_pass()
        torch.cuda.synchronize()
        tp1 = time.perf_counter()
        dms = timing["denoise_start"].elapsed_time(timing["denoise_end"])
        denoise_ms += dms
        log(f"[bench] pass {(tp1 - tp0) * 1e3:.1f} ms: before the denoise loop {(timing['host_before_denoise'] - tp0) * 1e3:.1f} ms "
            f"(preprocess + upload + VAE encode), denoise {dms:.1f} ms, after it {(tp1 - timing['host_after_denoise']) * 1e3:.1f} ms "
            f"(host view; VAE decode + postprocess)")
    D.barrier()
    torch.cuda.synchronize()
    elapsed = D.max_over_ranks(time.perf_counter() - t0, device=reduce_device)
    assert torch.isfinite(img).all(), "non-finite output image"
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, {"images": img})

    images = a.batch * a.steps * world
    value = images / elapsed
    gflop = GFLOP_PER_IMAGE_STEP.get(a.size, 2489.2 * (a.size / 512.0) ** 2) if not xl else None
    peak = PEAK_F32_TFLOPS if a.precision == "fp32" else PEAK_BF16_TFLOPS
    step_s = denoise_ms * 1e-3 / (a.steps * a.denoise_steps)
    step_tflops = a.batch * gflop * 1e9 / step_s / 1e12 if gflop else None

    roofline = None
    if a.full and rank == 0 and not a.no_profile:
        # live per-launch timing of the dominant kernel family (mf_gemm_conv: every conv / linear, ~90 % of the
        # algorithmic FLOPs) over ONE denoise step, HIP events on the launch stream
        x2 = torch.cat([inp["latents"].to(device)] * 2)
        cond = torch.randn(2 * a.batch, 5 if xl else 6, a.size // 8, a.size // 8, device=device)
        pe = torch.cat([inp["negative_prompt_embeds"], inp["prompt_embeds"]]).to(device)
        added = dict(text_embeds=torch.cat([npooled, pooled]).to(device),
                     time_ids=torch.tensor([[a.size, a.size, 0, 0, a.size, a.size]], dtype=torch.float32,
                                           device=device).repeat(2 * a.batch, 1)) if xl else None
        for rep in range(2):
            if rep == 1:
                hip.profile_begin()
            d, m, u = pipe.brushnet(x2, 981, encoder_hidden_states=pe, brushnet_cond=cond, added_cond_kwargs=added,
                                    return_dict=False)
            pipe.unet(x2, 981, pe, added_cond_kwargs=added, down_block_add_samples=d, mid_block_add_sample=m,
                      up_block_add_samples=u)
        n_launch, secs, flops = hip.profile_end()
        attn_flops = hip.PROFILE_ATTN_FLOPS
        # algorithmic bytes: activations read once, weights once, output written once (bf16 = 2 B)
        alg_bytes = 0.0
        # each launch priced at the dense MFMA peak of ITS operand type (SDXL's fp8 mode: the transformer Linears run on e4m3
        # operands, 5 PF; convs and everything else on bf16, 2.5 PF): ideal_s = sum flops_i / peak_i, frac = ideal_s / measured
        ideal_s, flops_fp8 = 0.0, 0.0
        for _, fl, (m, n, k, kh, stride, ups, nz, _tile, _sk, dt) in hip.LAST_PROFILE:
            a_px = m * stride * stride / (4.0 if ups else 1.0)
            esz = 1.0 if dt == hip.MF_FP8 else 2.0
            alg_bytes += nz * (esz * (a_px * k / (kh * kh) + n * k) + 2.0 * m * n)
            pk = PEAK_FP8_TFLOPS if dt == hip.MF_FP8 else (PEAK_F32_TFLOPS if dt == hip.MF_F32 else PEAK_BF16_TFLOPS)
            ideal_s += fl / (pk * 1e12)
            flops_fp8 += fl if dt == hip.MF_FP8 else 0.0
        if flops_fp8 > 0:
            peak = round(flops / ideal_s / 1e12, 1)          # FLOP-weighted harmonic blend of the two peaks
        traffic, traffic_src = None, None
        pdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
        pmc = next((q for q in (os.path.join(pdir, f"r0{r}_pmc_gemm_family.json") for r in (6, 5, 4, 3)) if os.path.exists(q)), "")
        if os.path.exists(pmc) and a.batch == 4 and a.size == 512 and a.precision == "bf16" and not xl:
            with open(pmc) as f:
                pj = json.load(f)
            traffic = pj["traffic_bytes_per_launch"]          # separate rocprofv3 --pmc passes (tools/pmc_step.sh)
            traffic_src = "profiles/" + os.path.basename(pmc) + ": " + pj["method"]
        roofline = {"bound": "mfma", "kernel": "gemm_conv_kernel (all tile instantiations)",
                    "achieved": round(flops / secs / 1e12, 2), "peak": peak, "unit": "TFLOP/s",
                    "frac": round(flops / secs / 1e12 / peak, 4), "traffic": traffic, "traffic_unit": "HBM-side bytes per launch",
                    "traffic_source": traffic_src, "algorithmic_bytes_per_launch": round(alg_bytes / n_launch),
                    "launches_per_denoise_step": n_launch, "avg_launch_us": round(secs / n_launch * 1e6, 2),
                    "flop_per_denoise_step": flops,
                    "fp8_flop_share": round(flops_fp8 / flops, 4) if flops_fp8 > 0 else None,
                    "peak_note": (f"FLOP-weighted blend of the dense fp8 ({PEAK_FP8_TFLOPS:.0f} TF/s, e4m3 transformer Linears) and bf16 "
                                  f"({PEAK_BF16_TFLOPS:.0f} TF/s, everything else) MFMA peaks: sum flops / sum (flops_i / peak_i)") if flops_fp8 > 0 else None,
                    "denoise_step": ({"ms": round(step_s * 1e3, 3), "achieved": round(step_tflops, 2),
                                      "frac": round(step_tflops / peak, 4), "algorithmic_gflop_per_image_step": gflop}
                                     if gflop else
                                     # no published census for this config: the live one of the instantiated model — every
                                     # mf_gemm_conv launch's 2MNK plus 4 B H Sq Skv d of every flash-attention launch of the step
                                     {"ms": round(step_s * 1e3, 3), "achieved": round((flops + attn_flops) / step_s / 1e12, 2),
                                      "frac": round((ideal_s + attn_flops / (PEAK_BF16_TFLOPS * 1e12)) / step_s, 4),
                                      "algorithmic_gflop_per_image_step": round((flops + attn_flops) / a.batch / 1e9, 1),
                                      "attention_gflop_per_image_step": round(attn_flops / a.batch / 1e9, 1),
                                      "note": "live FLOP census of the instantiated config (conv / GEMM + flash attention, both CFG halves); "
                                              "frac = time at each launch's own dense MFMA peak (fp8 Linears 5 PF, the rest 2.5 PF) / step time"})}

    host_inputs = None
    if a.full and rank == 0 and world == 1 and a.inputs == "device" and not a.no_profile and not xl:
        # the same passes with the inputs handed over as HOST tensors (what a caller of the reference's pipeline does):
        # CPU preprocessing + pinned-staging upload inside the pass.  Reported beside `value`, never as `value`.
        inp = inp_host
        one_pass()
        torch.cuda.synchronize()
        th = time.perf_counter()
        for _ in range(a.steps):
            one_pass()
        torch.cuda.synchronize()
        th = time.perf_counter() - th
        host_inputs = {"value": round(a.batch * a.steps / th, 4), "unit": "images/sec", "ms_per_step": round(th / a.steps * 1e3, 2),
                       "note": "inputs as host tensors: CPU preprocessing and the PCIe upload (pinned staging) inside the pass"}

    shared = None
    if a.full and rank == 0 and world == 1 and not a.no_parity_mode and not a.no_profile and not xl:
        # Secondary line, never `value`: the same workload with ONE VAE-posterior sample of the conditioning latents used
        # for both classifier-free-guidance halves (the reference draws one per half, pipeline_brushnet.py:1188 on the
        # image doubled at :771-772).  BrushNet is attention-free, so with identical conditioning its two halves are the
        # same function of the same inputs and the pipeline evaluates it once per image (mf_gemm_desc.res1_rows).
        inp = dict(inp_timed)
        inp["vae_noise"] = torch.cat([inp_timed["vae_noise"][:a.batch]] * 2)
        one_pass()
        assert pipe._brushnet_once
        torch.cuda.synchronize()
        ts_ = time.perf_counter()
        sd_ms = 0.0
        for _ in range(a.steps):
            one_pass()
            torch.cuda.synchronize()
            sd_ms += timing["denoise_start"].elapsed_time(timing["denoise_end"])
        ts_ = time.perf_counter() - ts_
        shared = {"value": round(a.batch * a.steps / ts_, 4), "unit": "images/sec", "ms_per_step": round(ts_ / a.steps * 1e3, 2),
                  "denoise_step_ms": round(sd_ms / (a.steps * a.denoise_steps), 3),
                  "executed_gflop_per_image_step": round(gflop - 882.6 / 2, 1) if gflop and a.size == 512 else None,
                  "note": "NOT the reference's sampling: both CFG halves share one posterior sample of the conditioning latents "
                          "(each half's distribution is unchanged), so the attention-free BrushNet runs once per image instead "
                          "of twice; opt-in (pipe.cfg_shared_conditioning_sample or conditioning_noise with equal halves)"}
        inp = inp_timed

    parity = None
    if a.full and rank == 0 and world == 1 and not a.no_parity_mode and not a.no_profile and not xl and a.precision == "bf16":
        # The SAME workload in the precision mode that meets BASELINE.json's 1e-3 latent bound against the reference
        # (f16x3: fp32 storage, three fp16 MFMAs per product; asserted in tests/ and smoke()): one warm-up, then timed.
        del pipe
        torch.cuda.empty_cache()
        inp = inp_timed
        ppipe, _ = build_pipeline("f16x3", device, model=a.model)
        pipe = ppipe
        ptiming = timing
        one_pass()
        torch.cuda.synchronize()
        tp = time.perf_counter()
        pd_ms = 0.0
        for _ in range(a.steps):
            one_pass()
            torch.cuda.synchronize()
            pd_ms += ptiming["denoise_start"].elapsed_time(ptiming["denoise_end"])
        tp = time.perf_counter() - tp
        pstep = pd_ms * 1e-3 / (a.steps * a.denoise_steps)
        parity = {"precision": "f16x3", "value": round(a.batch * a.steps / tp, 4), "unit": "images/sec",
                  "ms_per_step": round(tp / a.steps * 1e3, 2), "denoise_step_ms": round(pstep * 1e3, 3),
                  "denoise_step_tflops": round(a.batch * gflop * 1e9 / pstep / 1e12, 2) if gflop else None,
                  "tolerance": "latent L-inf <= 1e-3 vs the reference: on THIS workload over all 50 DDIM steps (image 0 of the batch, "
                               "5.4e-4 at step 50 where |latents| reach 71; the reference's own fp32 arithmetic is 1.8e-4 from the "
                               "float64 value there), on BASELINE configs[0] and the tiny pipelines "
                               "(tests/test_pipeline_gpu.py::test_baseline_config1_all_50_steps_against_reference, __graft_entry__.smoke); "
                               "`value` (bf16) is NOT inside 1e-3: it is asserted inside the reference's own bf16 deviation instead",
                  "note": "same workload and inputs as `value`; fp32 activations, GEMM operands split into two fp16 halves, "
                          "three v_mfma_f32_32x32x16_f16 per product (ceiling 1/3 of the 16-bit MFMA peak)"}
        del ppipe, pipe
        torch.cuda.empty_cache()

    # ---- secondary legs of the driver's line: never `value` ---------------------------------------------
    fp16_mode = train_leg = sdxl_leg = None
    extra = (a.full and rank == 0 and world == 1 and not a.no_extra_legs and not a.no_parity_mode and not a.no_profile and not xl
             and a.precision == "bf16" and a.batch == 4 and a.size == 512)
    if extra:
        # (1) the SAME workload in the reference scripts' default precision, torch_dtype=torch.float16 (test_brushnet.py:122-126):
        # fp16 storage, one f16 MFMA per product — the bf16 kernels' byte layout
        try:
            pipe = None
            torch.cuda.empty_cache()
            inp = inp_timed
            hpipe, _ = build_pipeline("fp16", device, model=a.model)
            pipe = hpipe
            one_pass()
            torch.cuda.synchronize()
            th_ = time.perf_counter()
            hd_ms = 0.0
            for _ in range(a.steps):
                himg = one_pass()
                torch.cuda.synchronize()
                hd_ms += timing["denoise_start"].elapsed_time(timing["denoise_end"])
            th_ = time.perf_counter() - th_
            hstep = hd_ms * 1e-3 / (a.steps * a.denoise_steps)
            assert torch.isfinite(himg).all(), "non-finite fp16 image"
            fp16_mode = {"precision": "fp16", "value": round(a.batch * a.steps / th_, 4), "unit": "images/sec",
                         "ms_per_step": round(th_ / a.steps * 1e3, 2), "denoise_step_ms": round(hstep * 1e3, 3),
                         "denoise_step_tflops": round(a.batch * gflop * 1e9 / hstep / 1e12, 2) if gflop else None,
                         "tolerance": "inside 1.25 x (L-inf) / 1.1 x (mean) of the REFERENCE's own fp16 deviation from its fp32 results on the "
                                      "same cases (tests/golden/fp16_envelope.json: ~1/9 of its bf16 deviation), tests/test_*_gpu.py [fp16]",
                         "note": "the default precision of the reference's inference script; same workload and inputs as `value`"}
            del hpipe, pipe
            torch.cuda.empty_cache()
        except Exception as e:          # a secondary leg must never take the headline line down
            fp16_mode = {"error": f"{type(e).__name__}: {e}"[:300]}
        pipe = None
        torch.cuda.empty_cache()
        # (2), (3) the other two workloads BASELINE.json names, each as its own child process of this one (this process only
        # keeps its HIP context; nothing is exec'ed): configs[3] per-GPU training step, configs[4] SDXL + BrushNet-XL in fp8
        import subprocess

        def child(args, keys, profile=False):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), *args, "--no-cpu-baseline", "--no-parity-mode",
                                    *(["--full"] if profile else ["--no-profile"]), "--no-extra-legs"], capture_output=True, text=True, timeout=900)
                line = next((l for l in reversed(r.stdout.splitlines()) if l.startswith("{") and '"metric"' in l), None)
                if line is None:
                    return {"error": (r.stderr or r.stdout)[-300:]}
                rec = json.loads(line)
                return {k: rec.get(k) for k in keys}
            except Exception as e:
                return {"error": f"{type(e).__name__}: {e}"[:300]}

        train_leg = child(["--mode", "train", "--precision", "bf16", "--steps", "8", "--warmup", "3"],
                          ("metric", "value", "unit", "ms_per_step", "dtype", "roofline", "achieved_tflops", "algorithmic_gflop_per_sample", "config"))
        # (--no-parity-mode also switches off the xl child's secondary passes; its own FLOP census / HIP-event pass stays on)
        sdxl_leg = child(["--model", "sdxl", "--precision", "fp8", "--steps", "2", "--warmup", "1"],
                         ("metric", "value", "unit", "ms_per_step", "dtype", "roofline", "config"), profile=True)

    cpu = None
    if want_cpu:
        # cores this process may actually use (cgroup / affinity aware), capped: PyTorch's CPU conv/GEMM kernels
        # degrade badly when oversubscribed on very wide hosts
        threads = min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 32)
        t_step, t_vae, t_cfg0 = cpu_baseline(sds, a.size, threads, a.denoise_steps)
        per_image = a.denoise_steps * t_step + t_vae
        cpu = {"value": round(1.0 / per_image, 6), "unit": "images/sec", "cores": threads, "kind": "port",
               "cpu_model": cpu_model(),
               "sample": f"CPU oracle (PyTorch fp32, pinned bit-exact to the reference), torch.utils.benchmark.Timer, "
                         f"{threads} threads: 1 image @ {a.size}x{a.size}, 2 denoise steps with CFG ({t_step:.2f} s per step) + "
                         f"VAE encode + decode ({t_vae:.2f} s); only the step count is extrapolated to {a.denoise_steps}",
               "configs0": {"value": round(1.0 / t_cfg0, 6), "unit": "images/sec", "seconds": round(t_cfg0, 2),
                            "sample": "BASELINE.json configs[0] measured whole: 1 x 256 x 256, 4 denoise steps with CFG + "
                                      "VAE encode + decode (the reference pipeline itself ran 0.080 images/s on 8 threads in "
                                      "the build container, BASELINE.md)"}}

    if rank == 0:
        out = {
            "metric": (f"images/sec at {a.size}x{a.size}, {a.denoise_steps}-step DDIM, SD1.5+BrushNet" if not xl else
                       f"images/sec at {a.size}x{a.size}, {a.denoise_steps}-step DDIM, SDXL+BrushNet-XL (secondary workload)"),
            "value": round(value, 4), "unit": "images/sec", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(elapsed / a.steps * 1e3, 2), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": a.precision, "data": "synthetic",
            "config": {"workload": f"{'SDXL + BrushNet-XL(5 cond ch)' if xl else 'SD1.5 + BrushNet(6 cond ch) depth-cond'} inpaint, batch {a.batch}x{a.size}x{a.size} per GPU, "
                                   f"{a.denoise_steps}-step DDIM, CFG 7.5, VAE encode+decode included, random-init weights, inputs resident on the {a.inputs}",
                       "per_gpu_batch": a.batch, "global_batch": a.batch * world, "height": a.size, "width": a.size,
                       "denoise_steps": a.denoise_steps, "parallelism": f"batch-shard x{world} (no collective)"},
            "roofline": roofline, "parity_mode": parity, "shared_conditioning_sample": shared, "cpu_baseline": cpu,
            "host_inputs": host_inputs, "fp16_mode": fp16_mode, "train_step": train_leg, "sdxl": sdxl_leg,
        }
        print(json.dumps(out), flush=True)
        hip.tune_save()                      # per-shape (tile, split-K) winners found during warmup, for later processes
        if os.path.isdir("gpurun_out"):      # ... and a copy the developer can merge into the shipped cache
            hip.tune_save(os.path.join("gpurun_out", "tune_cache_new.json"))
    D.barrier()


if __name__ == "__main__":
    try:
        main()
    finally:
        import torch.distributed as _dist
        if _dist.is_available() and _dist.is_initialized():
            _dist.destroy_process_group()
