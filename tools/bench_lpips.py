"""LPIPS (net_type="squeeze") on the libmfhip path against the same network composed from torch ops on the same device in fp32 — what a
user without torchmetrics' own copy would run today: normalisation and scaling layer on fp32 copies, F.conv2d / F.relu / F.max_pool2d
(ceil_mode) / torch.cat in NCHW, the per-layer normalise / difference / 1 x 1 conv / spatial mean, then the values read on the host.
Batch 4 of 512 x 512 x 3 uint8 device images, seeded weights (tests/lpips_ref.py).  Needs the device.

Method (tools/bench_image_metrics.py's): every variant is warmed, then timed with device events around a run of ITERS scorings, REPEATS
times, the variants alternating inside each repeat (other work shares the box); reported are the median microseconds per scoring of the
batch and the spread (max - min over the repeats).  "rows" queues everything and reads nothing; "+ read" adds the copy of the [B, 7] row a
caller needs to see the number; "torch" ends in the copy of its values.  Also printed: the library entries of one scoring, and
mf_lpips_layer alone on the 255 x 255 x 64 feature of this batch (the largest tensor the metric reads) with its bytes per second, to be
read beside profiles/r03_hbm_bandwidth.md.  The agreement of the two sides is printed as a check, not timed.

    python tools/bench_lpips.py [--out profiles/lpips_bench.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lpips_ref as R  # noqa: E402
from reflecting_reality_amd import hip, metrics  # noqa: E402
from reflecting_reality_amd.lpips import LPIPS  # noqa: E402

BATCH, SIZE = 4, 512
ITERS, REPEATS, WARMUP = 20, 7, 3


def torch_rows(pred, gt, sd):
    """The [B, 7] table with torch ops on the device in fp32 (tests/lpips_ref.py's functions on device tensors)."""
    shift = torch.tensor(R.SHIFT, device=pred.device)[None, :, None, None]
    scale = torch.tensor(R.SCALE, device=pred.device)[None, :, None, None]
    x = torch.cat([pred, gt]).permute(0, 3, 1, 2).float()
    x = ((x / 127.5 - 1) - shift) / scale
    cols = []
    for l, f in enumerate(R.features(x, sd, torch.float32)):
        cols.append(R.layer_distance(f[:BATCH], f[BATCH:], sd[f"lin{l}.model.1.weight"]))
    return torch.stack(cols, dim=1)


def count_entries(fn):
    """Library entries (mf_* calls that launch) of one fn(): hip._launch is the door of every entry but mf_gemm_conv."""
    calls = []
    real, real_gemm = hip._launch, hip.gemm_conv
    hip._launch = lambda entry, *a: (calls.append(entry), real(entry, *a))[1]
    hip.gemm_conv = lambda *a, **k: (calls.append("mf_gemm_conv"), real_gemm(*a, **k))[1]
    try:
        fn()
    finally:
        hip._launch, hip.gemm_conv = real, real_gemm
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips needs the device: a timing taken elsewhere says nothing about it")
    hip.load()
    dev = torch.device("cuda", 0)
    p, g, _ = R.images(R.IMAGE_SEED, BATCH, SIZE, SIZE)
    pred, gt = torch.as_tensor(p).to(dev), torch.as_tensor(g).to(dev)
    sd = R.weights(R.WEIGHT_SEED)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    models = {}
    for name, prec, tune in (("fp32", "fp32", False), ("fp32 tuned", "fp32", True), ("f16x3", "f16x3", False), ("bf16", "bf16", False)):
        models[name] = LPIPS(precision=prec, device=dev, autotune=tune)
        models[name].load_state_dict(sd)

    fns = {}
    for name, m in models.items():
        fns[f"hip {name} rows"] = (lambda m=m: m(pred, gt))
    fns["hip fp32 + read"] = lambda: models["fp32"](pred, gt).cpu()
    fns["torch fp32 + read"] = lambda: torch_rows(pred, gt, sd_dev).cpu()
    with torch.no_grad():
        for fn in fns.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        ours = metrics.lpips_finish(models["fp32"](pred, gt).cpu().numpy(), SIZE, SIZE)
        theirs = torch_rows(pred, gt, sd_dev).double().sum(dim=1).cpu().numpy()
        us = {k: [] for k in fns}
        for _ in range(REPEATS):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(ITERS):
                    fn()
                b.record()
                b.synchronize()
                us[name].append(a.elapsed_time(b) * 1000.0 / ITERS)
        # the hot kernel alone on the first tapped feature of this batch
        h1 = LPIPS.stage_shapes(SIZE, SIZE)[0]
        layer_us = {}
        for dt in (torch.float32, torch.bfloat16):
            feat = torch.rand(2 * BATCH, h1[0], h1[1], 64, device=dev).to(dt)
            w = torch.rand(64, device=dev)
            ws = hip.lpips_ws(BATCH, dev)
            for _ in range(WARMUP):
                hip.lpips_layer(feat, w, 0, ws)
            t = []
            for _ in range(REPEATS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(ITERS):
                    hip.lpips_layer(feat, w, 0, ws)
                b.record()
                b.synchronize()
                t.append(a.elapsed_time(b) * 1000.0 / ITERS)
            layer_us[dt] = (statistics.median(t), max(t) - min(t), feat.numel() * feat.element_size())
    calls = count_entries(lambda: models["fp32"](pred, gt))
    kinds = {k: calls.count(k) for k in sorted(set(calls))}
    med = {k: statistics.median(v) for k, v in us.items()}
    spr = {k: max(v) - min(v) for k, v in us.items()}
    lines = [f"LPIPS (squeeze) of batch {BATCH} x {SIZE} x {SIZE} x 3 uint8 device images, {torch.cuda.get_device_name(0)}",
             f"median us per scoring of the batch over {REPEATS} repeats of {ITERS} (spread = max - min over the repeats)",
             f"{'variant':>20} {'median us':>10} {'spread':>8}"]
    lines += [f"{k:>20} {med[k]:>10.1f} {spr[k]:>8.1f}" for k in fns]
    lines.append(f"(torch fp32 + read) / (hip fp32 + read) = {med['torch fp32 + read'] / med['hip fp32 + read']:.2f}")
    lines.append(f"library entries of one scoring: {len(calls)}  " + ", ".join(f"{k} x {v}" for k, v in kinds.items()))
    for dt, (m_us, s_us, nbytes) in layer_us.items():
        lines.append(f"mf_lpips_layer alone, {2 * BATCH} x {h1[0]} x {h1[1]} x 64 {str(dt).replace('torch.', '')}: {nbytes / 1e6:.1f} MB read, median {m_us:.1f} us "
                     f"(spread {s_us:.1f}), {nbytes / m_us / 1e3:.0f} GB/s")
    lines.append(f"agreement of the two sides (fp32, per pair): hip {np.array2string(ours, precision=6)}, torch {np.array2string(theirs, precision=6)}, "
                 f"max relative difference {np.abs(ours / theirs - 1).max():.2e}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
