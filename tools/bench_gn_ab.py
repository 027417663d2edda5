"""Same-box A/B of mf_groupnorm between two builds of libmfhip.so: the GroupNorm shapes of one denoise step at batch 8, one- and
two-segment, with the statistics from the kernel's own pass and from the producer's sums, plus mf_add on 8 x 4096 x 320 as the yardstick
of what a streaming kernel reaches on the box.  Every launch is graph-replayed (tools/ab_ops.py `timed`).

  python tools/bench_gn_ab.py                                  one process, the library MFHIP_LIB selects: JSON {case: us}
  python tools/bench_gn_ab.py --ab A.so B.so --rounds 3        processes of A and B alternate; prints per case the mean of each, the
                                                               repeat-to-repeat spread of A (max - min over its rounds) and the verdict
  --env K=V ...                                                extra environment of the B processes (developer switches)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT = {640: (320, 320), 960: (640, 320), 1280: (640, 640), 1920: (1280, 640), 2560: (1280, 1280)}
SHAPES = [(4096, c) for c in (320, 640, 960)] + [(1024, c) for c in (320, 640, 960, 1280, 1920)] + [(hw, c) for hw in (256, 64) for c in (1280, 2560)]


def child():
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from reflecting_reality_amd import hip
    from ab_ops import timed
    dev, bf, b, groups, rows = torch.device("cuda:0"), torch.bfloat16, 8, 32, 128
    torch.manual_seed(0)
    out = {}
    a0, a1 = torch.randn(b, 4096, 320, device=dev).to(bf), torch.randn(b, 4096, 320, device=dev).to(bf)
    out["mf_add 8x4096x320"] = timed(lambda: hip.add(a0, a1, bf))
    for hw, c in SHAPES:
        for c0, c1 in [(c, 0)] + ([SPLIT[c]] if c in SPLIT else []):
            x0 = torch.randn(b, hw, c0, device=dev).to(bf)
            x1 = torch.randn(b, hw, c1, device=dev).to(bf) if c1 else None
            g, be = torch.randn(c, device=dev), torch.randn(c, device=dev)
            y = torch.empty(b, hw, c, device=dev, dtype=bf)
            name = f"{hw:4d} x {c0}" + (f"+{c1}" if c1 else "")
            out[f"{name} own"] = timed(lambda: hip.groupnorm(x0, g, be, groups=groups, eps=1e-5, silu=True, out_dtype=bf, x1=x1, out=y))
            if hw <= 256:
                continue
            for x in (x0, x1):                 # the producer's sums, as a GEMM with gn_part leaves them (per-group sums: one segment only)
                if x is not None:
                    v = x.float().view(-1, rows, x.shape[-1])
                    chan = torch.stack([v.sum(1), (v * v).sum(1)], dim=-1)
                    if c1 == 0 and x.shape[-1] % groups == 0:
                        grp = chan.view(-1, groups, x.shape[-1] // groups, 2).sum(2)
                        x._gn_part = (torch.cat([chan.reshape(-1), grp.reshape(-1)]).contiguous(), rows, groups)
                    else:
                        x._gn_part = (chan.contiguous().view(-1), rows)
            out[f"{name} producer"] = timed(lambda: hip.groupnorm(x0, g, be, groups=groups, eps=1e-5, silu=True, out_dtype=bf, x1=x1, out=y))
    print("GN_AB " + json.dumps(out), flush=True)


def run_child(lib, extra_env):
    env = dict(os.environ, MFHIP_LIB=os.path.abspath(lib), **extra_env)
    res = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise SystemExit(f"{lib}: exit {res.returncode}\n{res.stderr[-2000:]}")
    return json.loads([l for l in res.stdout.splitlines() if l.startswith("GN_AB ")][-1][6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", nargs=2, metavar=("A", "B"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--env", nargs="*", default=[])
    a = ap.parse_args()
    if not a.ab:
        return child()
    extra = dict(kv.split("=", 1) for kv in a.env)
    runs = {"A": [], "B": []}
    for _ in range(a.rounds):
        runs["A"].append(run_child(a.ab[0], {}))
        runs["B"].append(run_child(a.ab[1], extra))
    print(f"A = {a.ab[0]}, B = {a.ab[1]} {extra or ''}, {a.rounds} alternating rounds, us per launch (graph replay, best of 5 replays of 40)")
    print(f"{'case':28s} {'A mean':>8s} {'A spread':>8s} {'B mean':>8s} {'B spread':>8s} {'B - A':>8s}  verdict (|B - A| against 3 x spread of A)")
    for case in runs["A"][0]:
        va, vb = [r[case] for r in runs["A"]], [r[case] for r in runs["B"]]
        ma, mb, sa, sb = sum(va) / len(va), sum(vb) / len(vb), max(va) - min(va), max(vb) - min(vb)
        verdict = "faster" if mb < ma - 3 * sa else "slower" if mb > ma + 3 * sa else "same"
        extra_col = f"  {2 * 3 * 8 * 4096 * 320 / mb / 1e6:.2f} TB/s (B)" if case.startswith("mf_add") else (
            f"  {2 * 2 * 8 * int(case.split()[0]) * sum(int(t) for t in case.split()[2].split('+')) / mb / 1e6:.2f} TB/s read+write (B)")
        print(f"{case:28s} {ma:8.2f} {sa:8.2f} {mb:8.2f} {sb:8.2f} {mb - ma:8.2f}  {verdict}{extra_col}")


if __name__ == "__main__":
    main()
