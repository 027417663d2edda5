"""Every GEMM launch of the benchmark step, each on its own, against the float64 model of its descriptor (tests/gemm_ref.py).

One bench.py pass (num_inference_steps = 1: the eager first step, so VAE encode, BrushNet, the UNet and VAE decode all launch) is
traced through a proxy of the library handle that copies every mf_gemm_conv descriptor.  The tile each launch ran is the one the
shipped tune cache, hip.PREFER_PERS or the library heuristic chose for that call at that position; the fused epilogue forms are the
ones the step turned on.  Launches that agree on every non-pointer field and on each pointer's null-ness and address modulo 256 are
one case.  Every case is replayed with fresh seeded data in buffers sized from its descriptor (each pointer keeps its address
modulo 256, so the alignment paths take the same branch), sentinel-filled output, 4 KB guard tails, and checked against float64:
16-bit outputs to 0.5 ulp + 2^-18 S per element and unbiased, correctly-rounded statistics; fp32 outputs to 2^-19 S."""
import ctypes as C
import os
import sys
import time
from collections import Counter, OrderedDict

import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from reflecting_reality_amd import hip, synth  # noqa: E402
from gemm_audit import case_key, replay, trace_gemms  # noqa: E402


def features(d, rec):
    f = []
    if d.kh > 1:
        f.append(f"{d.kh}x{d.kw}")
    if d.c1:
        f.append("2seg")
    if d.stride > 1:
        f.append(f"s{d.stride}")
    if d.upsample:
        f.append("ups")
    if d.nz > 1:
        f.append(f"nz{d.nz}")
    if d.a_dtype != d.dtype:
        f.append("aF32")
    if d.w_split:
        f.append("wsplit")
    if d.bias:
        f.append("biasM" if d.bias_mode else "bias")
    if d.temb:
        f.append("temb")
    if d.alpha != 1.0:
        f.append(f"a{d.alpha:g}")
    if d.res0:
        f.append("res0")
    if d.res1:
        f.append(f"res1/{d.res1_rows}" if d.res1_rows else "res1")
    f += {G.ACT_SILU: ["silu"], G.ACT_GEGLU4: ["geglu"]}.get(d.act, [])
    if d.ln_colsum:
        f.append("ln")
    if d.vt_out:
        f.append("vt")
    if d.gn_part:
        f.append(f"gn{rec.part_rows}" + ("g" if rec.grouped else ""))
    if rec.deferred:
        f.append(f"defer{rec.deferred}")
    if d.sk_tickets:
        f.append("skf")
    return f


def run_precision(prec):
    import bench
    dev = torch.device("cuda", 0)
    pipe, _ = bench.build_pipeline(prec, dev)
    inp = {k: v.to(dev) for k, v in synth.pipeline_inputs(4, 512, 512, seed=1234, cross_dim=768).items()}
    torch.cuda.synchronize()
    with trace_gemms() as tr:
        pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"],
             mask=inp["mask"], depth=inp["depth"], num_inference_steps=1, guidance_scale=7.5, latents=inp["latents"],
             output_type="pt", brushnet_conditioning_scale=1.0, height=512, width=512, conditioning_noise=inp["vae_noise"])
    del pipe, inp
    torch.cuda.empty_cache()
    return tr


def plan_disagreements(x):
    """mf_gemm_conv_plan on a recorded descriptor against what its launch reported through the host ints (the plan never reads them).
    A launch on tile 70 gives every block hip.PERS_MIN_NLOOP output tiles or more — unless tile 70 was not hip.PREFER_PERS' choice but the
    tuner's (the call looked up a tune key, so its tile is the cache's or a fresh measurement's).  Asserted for every tile-70 launch
    alike, 6 of the bf16 step's 131 cases fail it with ONE tile per block: M8192 N640 K320; M8192 N640 K640 plain, with a residual and
    with a folded LayerNorm; M2048 N1280 K1280 with a folded LayerNorm; M512 N10240 K1280 GEGLU.  The shipped tune cache holds tile 70
    for them (measured the winner there), and they launched the same way before the plan existed."""
    p = hip.GemmPlan()
    if hip.load().mf_gemm_conv_plan(C.byref(x.d), C.byref(p)) != 0:
        return [f"the plan refuses a call that launched: {hip.load().mf_last_error().decode()}"]
    out = []
    got, want = (p.gn_part_rows, p.gn_grouped, p.deferred_splits), (x.part_rows, x.grouped, x.deferred)
    if got != want:
        out.append(f"plan (gn_part_rows, gn_grouped, deferred_splits) {got} != launch {want}")
    if x.d.tile == hip.PERS_TILE and p.tiles_per_block < hip.PERS_MIN_NLOOP:
        if x.key is None:
            out.append(f"routed to tile {hip.PERS_TILE} with {p.tiles_per_block} output tiles per block")
    return out


def audit(prec):
    t0 = time.time()
    tr = run_precision(prec)
    launches = [x for x in tr.launches if not x.tuner]
    refused = [x for x in launches if x.rc != 0]
    cases = OrderedDict()
    for x in launches:
        if x.rc == 0:
            cases.setdefault(case_key(x.d), []).append(x)
    tagged = sorted({k for k in tr.keys if "@" in k and k in tr.shipped})
    print(f"\n[{prec}] traced {len(tr.launches)} launches ({len(tr.launches) - len(launches)} tuner trials), {len(cases)} cases, "
          f"{len(refused)} refused, trace {time.time() - t0:.1f}s")
    fails = []
    worst_mean = worst_rms = 0.0
    for i, (key, group) in enumerate(cases.items()):
        rec = group[0]
        d = rec.d
        m, k = G.m_rows(d), G.k_depth(d)
        shape = f"M{m} N{d.n} K{k}"
        fails += [f"case {i} {shape} tile {d.tile} sk {d.splitk} {features(d, rec)}: {msg}" for x in group for msg in plan_disagreements(x)]
        try:
            v, extra, nrows = replay(d, rec, 1000 + i, torch.device("cuda", 0))
        except (AssertionError, G.NotModelled, hip.MfhipError) as e:
            fails.append(f"case {i} {shape} tile {d.tile} sk {d.splitk} {features(d, rec)}: {type(e).__name__}: {e}")
            print(f"  case {i:3d} {shape:24s} tile {d.tile:2d} sk {d.splitk:2d} FAILED {type(e).__name__}: {e}")
            continue
        if d.out_dtype != G.MF_F32 and v.n_stat >= 1000:
            worst_mean = max(worst_mean, abs(v.mean_e))
            worst_rms = max(worst_rms, v.rms_e)
        ok = v.ok and not extra
        print(f"  case {i:3d} {shape:24s} tile {d.tile:2d} sk {d.splitk:2d} out {'f32' if d.out_dtype == G.MF_F32 else 'b16' if d.out_dtype == G.MF_BF16 else 'f16'} "
              f"x{len(group):<3d} rows {nrows:5d} maxulp {v.max_ulp:8.3f} mean(e) {v.mean_e:+.4f} rms(e) {v.rms_e:.4f} "
              f"bound {v.worst:.3f} [{','.join(features(d, rec))}]" + ("" if ok else "  FAIL"))
        if not ok:
            fails.append(f"case {i} {shape} tile {d.tile} sk {d.splitk} {features(d, rec)}: {v.msg} {' | '.join(extra)}")
        torch.cuda.empty_cache()
    tiles = Counter(x.d.tile for x in launches)
    print(f"[{prec}] summary: {len(cases)} cases, {len(launches)} launches, tiles {dict(sorted(tiles.items()))}, "
          f"tune misses {tr.misses}, tagged cache hits {len(tagged)}, worst |mean(e)| {worst_mean:.4f}, worst rms(e) {worst_rms:.4f}, "
          f"{time.time() - t0:.1f}s")
    return tr, launches, refused, cases, tagged, fails


@pytest.mark.parametrize("prec", ["bf16", "fp16", "f16x3"])
def test_every_gemm_launch_of_the_benchmark_step(prec):
    tr, launches, refused, cases, tagged, fails = audit(prec)
    assert launches, "no mf_gemm_conv launch was traced"
    assert not refused, "the library refused cached (tile, split-K) choices: " + "; ".join(
        f"tile {x.d.tile} sk {x.d.splitk} M{G.m_rows(x.d)} N{x.d.n} K{G.k_depth(x.d)}" for x in refused[:8])
    assert not fails, f"{len(fails)} of {len(cases)} cases failed:\n" + "\n".join(fails)
    if prec == "bf16":
        ds = [(x.d, x) for x in launches]
        need = {
            # (the decoder's cat(h, skip) reaches a conv as two segments in the 1x1 shortcut; its 3x3 conv1 reads the GroupNorm output)
            "two-segment conv": any(d.c1 for d, _ in ds),
            "stride 2": any(d.stride == 2 for d, _ in ds),
            "upsample": any(d.upsample for d, _ in ds),
            "tile 70": any(d.tile == hip.PERS_TILE for d, _ in ds),
            "folded LN with vt_out": any(d.ln_colsum and d.vt_out for d, _ in ds),
            "GEGLU": any(d.act == G.ACT_GEGLU4 for d, _ in ds),
            "gn_part": any(d.gn_part for d, _ in ds),
            "deferred split-K": any(r.deferred for _, r in ds),
            "@-tagged cache hit": bool(tagged),
        }
        missing = [k for k, v in need.items() if not v]
        assert not missing, f"the traced bf16 step no longer uses: {missing}"
