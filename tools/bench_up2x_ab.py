"""Same-box A/B of the upsampler convs of one denoise step (batch 8): the 3x3 conv over the nearest-2x upsampled tensor
(ops.conv2d(upsample=True), its tile from the tune cache) against the phase form (ops.conv_up2x -> mf_conv_up2x) on every tile that has
one, each launch with the GroupNorm sums the step asks for.  Every launch is graph-replayed (tools/ab_ops.py `timed`).

  python tools/bench_up2x_ab.py                                 one process, this tree: JSON {case: us}
  python tools/bench_up2x_ab.py --ab TREE_A TREE_B --rounds 3   processes of the two source trees (each with its own built library)
                                                                alternate; prints per case the mean of each, the repeat-to-repeat
                                                                spread of A (max - min over its rounds) and the verdict.  A tree
                                                                without the phase entry reports the 3x3 cases only."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (low-resolution H = W, channels): the UNet / BrushNet upsamplers of SD1.5 at 512 x 512, batch 8 — M x N x K of the 3x3 form:
# 32768 x 640 x 5760, 8192 x 1280 x 11520, 2048 x 1280 x 11520
LEVELS = [(32, 640), (16, 1280), (8, 1280)]
BATCH = 8


def child(root):
    import torch
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from reflecting_reality_amd import hip, ops
    from ab_ops import timed
    dev, prec = torch.device("cuda:0"), ops.Precision.get("bf16")
    torch.manual_seed(0)
    out = {}
    for hw, c in LEVELS:
        x = torch.randn(BATCH, hw, hw, c, device=dev).to(torch.bfloat16)
        wt = torch.randn(c, c, 3, 3) / (9 * c) ** 0.5
        bias = torch.randn(c)
        cw = ops.ConvWeight(wt, bias, prec, dev)
        name = f"{hw}x{hw}x{c}"
        flops3 = 2.0 * BATCH * 4 * hw * hw * c * 9 * c
        t = timed(lambda: ops.conv2d(x, cw, upsample=True, gn_part=32))
        out[f"{name} 3x3"] = (t, flops3 / t / 1e6)
        if not hasattr(ops, "conv_up2x"):
            continue
        pw = ops.PhaseWeight(wt, bias, prec, dev)
        for tile in hip.UP2X_TILES:
            for sk in ((1,) if hw > 8 else (1, 2, 4)):
                t = timed(lambda: ops.conv_up2x(x, pw, tile=tile, splitk=sk, gn_part=32))
                out[f"{name} phases tile {tile}" + (f" split-K {sk}" if sk > 1 else "")] = (t, flops3 * 4 / 9 / t / 1e6)
    print("UP2X_AB " + json.dumps(out), flush=True)


def run_child(root):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(root)], capture_output=True, text=True, timeout=600,
                         cwd=os.path.abspath(root))
    if res.returncode != 0:
        raise SystemExit(f"{root}: exit {res.returncode}\n{res.stderr[-2000:]}")
    return json.loads([l for l in res.stdout.splitlines() if l.startswith("UP2X_AB ")][-1][8:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", nargs=2, metavar=("A", "B"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not a.ab:
        return child(a.child or ROOT)
    runs = {"A": [], "B": []}
    for _ in range(a.rounds):
        runs["A"].append(run_child(a.ab[0]))
        runs["B"].append(run_child(a.ab[1]))
    print(f"A = {a.ab[0]}, B = {a.ab[1]}, {a.rounds} alternating rounds, us per launch (graph replay, best of 5 replays of 40); TF/s of the multiply-adds "
          "each form performs (phases: 4/9 of the 3x3 form's)")
    print(f"{'case':40s} {'A mean':>8s} {'A spread':>8s} {'B mean':>8s} {'B spread':>8s} {'B TF/s':>8s}  B against A's 3x3 (3 x spread of A)")
    for case in runs["B"][0]:
        base = case.split()[0] + " 3x3"
        va, vb = [r[base][0] for r in runs["A"]], [r[case][0] for r in runs["B"]]
        ma, mb, sa, sb = sum(va) / len(va), sum(vb) / len(vb), max(va) - min(va), max(vb) - min(vb)
        verdict = "faster" if mb < ma - 3 * sa else "slower" if mb > ma + 3 * sa else "same"
        print(f"{case:40s} {ma:8.2f} {sa:8.2f} {mb:8.2f} {sb:8.2f} {runs['B'][-1][case][1]:8.0f}  {mb - ma:+8.2f} us {verdict}")


if __name__ == "__main__":
    main()
