"""mf_attention_ip_bf16 (decoupled cross-attention in one launch) against the composition it replaces — mf_attention_bf16 on the text keys,
mf_attention_bf16 on the ip keys, mf_axpby_n over the two results — on the four SD1.5 cross-attention shapes (64^2 / 32^2 / 16^2 / 8^2
tokens, head dim 40 / 80 / 160 / 160, 8 heads, batch 8, 74 text keys + 4 ip keys), with the plain 77-key mf_attention_bf16 launch for
scale.  Needs the device.

Method: per shape every variant is warmed, then timed with device events around a run of ITERS launches, REPEATS times, the variants
alternating inside each repeat (other work shares the box); reported are the median microseconds per call and the spread
(max - min over the repeats).  The composition's fp32 combine runs on fp32 copies of the two results, as ops.attention's composition
path does for the fp32 modes; its bf16 form would add two casts, which are NOT counted here (the composition is flattered).

    python tools/bench_ip_attention.py [--out profiles/ip_attention_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reflecting_reality_amd import hip  # noqa: E402

SHAPES = ((64 * 64, 40), (32 * 32, 80), (16 * 16, 160), (8 * 8, 160))       # (query tokens, head dim); 8 heads each
BATCH, HEADS, SKV, SKV_IP, SKV_PLAIN = 8, 8, 74, 4, 77
ITERS, REPEATS, WARMUP = 200, 7, 20


def operands(sq, d, dev):
    c = HEADS * d
    g = torch.Generator(device="cpu").manual_seed(sq + d)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev, torch.bfloat16)
    vt = lambda n: torch.zeros(BATCH, c, (n + 7) // 8 * 8, dtype=torch.bfloat16, device=dev).copy_(
        torch.nn.functional.pad(rn(BATCH, c, n), (0, (n + 7) // 8 * 8 - n)))
    return dict(q=rn(BATCH, sq, c), k=rn(BATCH, SKV, c), vt=vt(SKV), k_ip=rn(BATCH, SKV_IP, c), vt_ip=vt(SKV_IP), k77=rn(BATCH, SKV_PLAIN, c),
                vt77=vt(SKV_PLAIN), o=torch.empty(BATCH, sq, c, dtype=torch.bfloat16, device=dev),
                o2=torch.empty(BATCH, sq, c, dtype=torch.bfloat16, device=dev),
                f0=torch.zeros(BATCH, sq, c, dtype=torch.float32, device=dev), f1=torch.zeros(BATCH, sq, c, dtype=torch.float32, device=dev),
                fo=torch.empty(BATCH, sq, c, dtype=torch.float32, device=dev))


def variants(t, sq, d):
    c = HEADS * d
    kw = dict(ldq=c, ldo=c, batch=BATCH, heads=HEADS, sq=sq, head_dim=d, scale=d ** -0.5)

    def fused():
        hip.attention_ip_bf16(t["q"], t["k"], t["vt"], t["k_ip"], t["vt_ip"], t["o"], ldk=c, ldvt=t["vt"].shape[-1], ldk_ip=c,
                              ldvt_ip=t["vt_ip"].shape[-1], skv=SKV, skv_ip=SKV_IP, ip_scale=1.0, **kw)

    def composed():
        hip.attention_bf16(t["q"], t["k"], t["vt"], t["o"], ldk=c, ldvt=t["vt"].shape[-1], skv=SKV, **kw)
        hip.attention_bf16(t["q"], t["k_ip"], t["vt_ip"], t["o2"], ldk=c, ldvt=t["vt_ip"].shape[-1], skv=SKV_IP, **kw)
        hip.axpby_n([t["f0"], t["f1"]], [1.0, 1.0], out=t["fo"])

    def plain77():
        hip.attention_bf16(t["q"], t["k77"], t["vt77"], t["o"], ldk=c, ldvt=t["vt77"].shape[-1], skv=SKV_PLAIN, **kw)
    return dict(fused=fused, composed=composed, plain77=plain77)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ip_attention needs the device: a timing taken elsewhere says nothing about it")
    hip.load()
    dev = torch.device("cuda", 0)
    lines = [f"mf_attention_ip_bf16 vs mf_attention_bf16 x 2 + mf_axpby_n; batch {BATCH}, {HEADS} heads, {SKV} + {SKV_IP} keys; plain: {SKV_PLAIN} keys",
             f"median us per call over {REPEATS} repeats of {ITERS} launches (spread = max - min over the repeats)",
             f"{'tokens':>7} {'d':>4} {'fused':>9} {'spread':>7} {'composed':>9} {'spread':>7} {'plain77':>9} {'spread':>7}  fused/composed"]
    for sq, d in SHAPES:
        t = operands(sq, d, dev)
        fns = variants(t, sq, d)
        for fn in fns.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
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
        lines.append(f"{sq:>7} {d:>4} " + " ".join(f"{med[k]:>9.2f} {spr[k]:>7.2f}" for k in ("fused", "composed", "plain77"))
                     + f"  {med['fused'] / med['composed']:.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
