"""mf_image_metrics (csrc/metrics.hip: PSNR + SSIM rows in one launch sequence over the uint8 bytes) against the torch-on-device
composition a user would write today — masking, five grouped conv2d with the 11 x 11 Gaussian window on fp32 copies, the elementwise SSIM
formula, per-image reductions, then the values read on the host — on batch 4 x 512 x 512 x 3 with all three regions (frame, "mask",
"mirror"): the scoring of one validation sample.  Needs the device.

Method: every variant is warmed, then timed with device events around a run of ITERS scorings, REPEATS times, the variants alternating
inside each repeat (other work shares the box); reported are the median microseconds per scoring (batch 4, three regions) and the spread
(max - min over the repeats).  "fused" queues the nine launch sequences' rows into one buffer and reads nothing; "fused + read" adds the
one copy of the rows to the host that a caller needs to see the numbers; "torch" ends in the copy of its 24 values (its .item()).  Both
sides give the same numbers to the bound of tests/test_image_metrics_gpu.py (printed as a check, not timed).

    python tools/bench_image_metrics.py [--out profiles/image_metrics_bench.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_metrics_ref as R  # noqa: E402
from reflecting_reality_amd import hip, metrics  # noqa: E402

BATCH, SIZE, CH = 4, 512, 3
ITERS, REPEATS, WARMUP = 50, 7, 5
REGIONS = (None, "mask", "mirror")


def torch_scores(pred, gt, mask, kernel):
    """[3 regions][batch][psnr, ssim] as one device tensor: torchmetrics' arithmetic, each image with its own data range."""
    out = []
    for region in REGIONS:
        p, t = pred, gt
        if region is not None:
            hole = (mask == 255) if region == "mask" else (mask == 0)
            p, t = p.masked_fill(hole[:, :, :, None], 0), t.masked_fill(hole[:, :, :, None], 0)
        p, t = p.permute(0, 3, 1, 2).float(), t.permute(0, 3, 1, 2).float()
        mse = ((p - t) ** 2).mean(dim=(1, 2, 3))
        t_rng = t.amax(dim=(1, 2, 3)) - t.amin(dim=(1, 2, 3))
        psnr = 10.0 * torch.log10(t_rng * t_rng / mse)
        rng = torch.maximum(p.amax(dim=(1, 2, 3)) - p.amin(dim=(1, 2, 3)), t_rng)
        c1, c2 = ((0.01 * rng) ** 2)[:, None, None, None], ((0.03 * rng) ** 2)[:, None, None, None]
        mu_p, mu_t = F.conv2d(p, kernel, groups=CH), F.conv2d(t, kernel, groups=CH)
        e_pp, e_tt, e_pt = F.conv2d(p * p, kernel, groups=CH), F.conv2d(t * t, kernel, groups=CH), F.conv2d(p * t, kernel, groups=CH)
        var_p, var_t, cov = (e_pp - mu_p * mu_p).clamp_min(0), (e_tt - mu_t * mu_t).clamp_min(0), e_pt - mu_p * mu_t
        s = ((2 * mu_p * mu_t + c1) * (2 * cov + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (var_p + var_t + c2))
        out.append(torch.stack([psnr, s.mean(dim=(1, 2, 3))], dim=1))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_metrics needs the device: a timing taken elsewhere says nothing about it")
    hip.load()
    dev = torch.device("cuda", 0)
    pairs = [R.smooth_pair(SIZE, SIZE, seed=40 + i) for i in range(BATCH)]
    pred = torch.as_tensor(np.stack([p for p, _ in pairs])).to(dev)
    gt = torch.as_tensor(np.stack([g for _, g in pairs])).to(dev)
    mask = torch.as_tensor(np.stack([R.rect_mask(SIZE, SIZE, seed=40 + i) for i in range(BATCH)])).to(dev)
    w = torch.as_tensor(R.window(dtype=np.float32)).to(dev)
    kernel = torch.outer(w, w).expand(CH, 1, R.WIN, R.WIN).contiguous()
    rows = torch.empty(len(REGIONS), BATCH, hip.C.sizeof(hip.MetricsRow), dtype=torch.uint8, device=dev)

    def fused():
        for i, region in enumerate(REGIONS):
            hip.image_metrics(pred, gt, mask if region else None, region, out=rows[i])

    def fused_read():
        fused()
        return rows.cpu()

    def torch_read():
        return torch_scores(pred, gt, mask, kernel).cpu()

    fns = dict(fused=fused, fused_read=fused_read, torch=torch_read)
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    # the same numbers from both sides
    n = SIZE * SIZE * CH
    ours = np.array([[[f["psnr"], f["ssim"]] for f in (metrics.finish(r, n) for r in hip.metrics_rows(rows[i]))] for i in range(len(REGIONS))])
    theirs = torch_read().double().numpy()
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
    med = {k: statistics.median(v) for k, v in us.items()}
    spr = {k: max(v) - min(v) for k, v in us.items()}
    lines = [f"mf_image_metrics vs the torch composition (masking + 5 grouped conv2d + elementwise + reductions + read); batch {BATCH} x {SIZE} x {SIZE} x "
             f"{CH} uint8, regions frame / mask / mirror",
             f"median us per scoring of the batch in all three regions over {REPEATS} repeats of {ITERS} (spread = max - min over the repeats)",
             f"{'variant':>14} {'median us':>10} {'spread':>8}"]
    lines += [f"{k:>14} {med[k]:>10.1f} {spr[k]:>8.1f}" for k in fns]
    lines.append(f"torch / (fused + read) = {med['torch'] / med['fused_read']:.2f}")
    lines.append(f"agreement of the two sides: max |PSNR diff| {np.abs(ours[:, :, 0] - theirs[:, :, 0]).max():.2e} dB, "
                 f"max |SSIM diff| {np.abs(ours[:, :, 1] - theirs[:, :, 1]).max():.2e}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
