"""Float64 model of one mf_gemm_desc (include/mfhip.h) and the comparator that holds a launch's output to it.

`reference(d, ops, rows)` computes, for the chosen output rows of every z, the exact value the descriptor defines (implicit-GEMM
gather, operand values as the kernel multiplies them, the epilogue in the kernel's order: csrc/gemm_conv_kernel.h epilogue_store /
epilogue_store8) together with S, the sum of |a_k w_k| carried through the epilogue by first-order error propagation.  It never
calls a project kernel: plain torch float64, on whatever device the operands live on.

`ops` maps a descriptor pointer field ("a0", "a1", "w", "bias", "temb", "res0", "res1", "ln_colsum") to a flat tensor whose element
0 sits at that pointer, in the pointer's storage dtype.  A descriptor that uses a field the model does not cover raises NotModelled.

fp8 (dtype == a_dtype == MF_FP8): "a0" / "w" are torch.float8_e4m3fn tensors, "a_scale" / "w_scale" fp32 ones read at
(z / zdiv) * a_scale_zs + m and (z / zdiv) * w_scale_zs + n; v = acc * rs[m] * cs[n] before the bias, the order of epilogue_store.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import torch

# include/mfhip.h: compute / storage codes and activations (the same numbers as reflecting_reality_amd.hip)
MF_F32, MF_BF16, MF_F16X3, MF_BF16X3, MF_FP8, MF_BF16X1, MF_F16 = 0, 1, 2, 3, 4, 5, 6
ACT_NONE, ACT_SILU, ACT_GEGLU4 = 0, 1, 2
TORCH_DT = {MF_F32: torch.float32, MF_BF16: torch.bfloat16, MF_F16: torch.float16}
FP8_DT = torch.float8_e4m3fn
SPLIT_CODES = (MF_F16X3, MF_BF16X3)

# Error bounds, in units of S (the sum of |a_k w_k| after the epilogue's first-order propagation, see reference()).
# 16-bit outputs: fp32 accumulation of K products through MFMA blocks and an fp32 epilogue.  A worst-case recursive sum errs by up
# to K * 2^-24 S; the matrix pipe sums in blocks and trees, and the observed error of such sums grows like sqrt(K) 2^-24 S.  At
# the step's largest K (17280) sqrt(K) = 131 < 2^8, hence 2^-18 S: 64x the typical error, 4 orders below the output ulp for
# |ref| >= 2^-10 S, so the bound is dominated by the 0.5 ulp of the final rounding (which it does not widen).
BOUND16 = 2.0 ** -18
# fp32 outputs (f16x3 / bf16x3 / fp32 codes, or a 16-bit GEMM writing fp32): no final 16-bit rounding to hide behind.  The fp32
# MFMA errs by 0.75-1.5e-7 S at K <= 1024 and 3.5e-7 S at K = 4096 (cdna_hip_programming.md); an f16x3 product drops lo * lo and
# rounds lo to fp16 (2^-22 relative each).  2^-19 S = 1.9e-6 S leaves 5x over the K = 4096 figure for the deepest K of the step.
BOUND32 = 2.0 ** -19
# Approximations the kernels make on purpose are not charged to S but to a separate absolute allowance `a` per element (Ref.a): the
# bound grows by `a`, and the statistics limits by the mean of a / ulp over their elements (a bias of at most that size is allowed).
# GEGLU, gemm_conv_kernel epilogue_store8: erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7) for 16-bit outputs, erff for fp32,
# and 0.5 x (1 + erf) formed in fp32, whose cancellation at x << 0 costs another 2^-24: the gate factor errs by
# <= 0.5 |x| (1.5e-7 + 2^-24) = 1.05e-7 |x| < 2^-22 |x|.
GELU_A = 2.0 ** -22
# GEGLU, tile 70 (csrc/gemm_pers.hip pers_item): Phi from a table of 768 steps of 1/64 with linear interpolation, |error| <= 7.4e-6
# < 2^-17 (the kernel's own figure, h^2 / 8 max |Phi''|): the output errs by <= 2^-17 |v x|.
GELU_LUT_A = 2.0 ** -17
# Folded LayerNorm: mean and rstd come from fp32 sums of the row's values and squares (K / 8 terms per lane, then a lane tree) and
# var = E[a^2] - mean^2.  The relative error of those sums, sqrt(K / 8) 2^-24 at K <= 1280 (< 2^-20), is amplified by the
# cancellation (E[a^2] + |mean| E|a|) / var, and rstd carries it into every output of the row.
LN_A = 2.0 ** -20
# Tile 70, the persistent 128-row GEMM (csrc/gemm_pers.hip, header "Roles"), rounds the fp32 accumulator, after the folded
# LayerNorm, bias and alpha, to the 16-bit storage type in its LDS slab, and adds the residual and applies SiLU / GEGLU to that
# 16-bit value: the reference's own bf16 / fp16 semantics (a Linear's output is a 16-bit tensor before the residual add), not the
# single rounding of gemm_conv_kernel.  The model follows the tile it is given.  Where the exact intermediate lies within
# 2^-18 S of a rounding boundary the kernel may round it the other way: two intermediate ulps (one ulp of the larger binade at a
# binade edge), times the gain of what follows, are then allowed in `a`.
# fp8: the block-scaled MFMA (v_mfma_scale_f32_32x32x64_f8f6f4) sums its 64 products per step with fewer bits than a chain of fp32
# FMAs.  No derivation is at hand; the figure is the project's own (tests/test_fp8_gpu.py: measured 4e-5 ... 7e-5 of the result's
# rms, asserted at 2e-4), made scale-aware: a[m, n] = 2e-4 R rs[m] cs[n] |alpha| with R the float64 rms of the unscaled code product
# q_a q_w^T over the case.  Rows out of the quantiser all have amax 448, so the code product is homogeneous across rows and columns
# and a small rs[m] or cs[n] shrinks the allowance with the output.  It goes into Ref.a and through the epilogue gains like LN_A.
FP8_A = 2e-4
PERS_TILE = 70
SENTINEL = 0x7B          # byte pattern of untouched output memory: bf16 / fp32 1.3e36, fp16 61280 (finite, never a result here)


class NotModelled(Exception):
    """The descriptor uses a field this model does not cover: the audit must fail, not skip."""


@dataclass
class Ref:
    v: torch.Tensor          # float64 [nz, rows, ncols]: the exact output (ncols = n, or n / 2 under GEGLU)
    s: torch.Tensor          # float64 [nz, rows, ncols]: S of every element
    rows: torch.Tensor       # int64 [rows]
    a: torch.Tensor          # float64 [nz, rows, ncols]: absolute allowance for the kernels' deliberate approximations


def check_supported(d) -> None:
    why = []
    if d.dtype not in (MF_F32, MF_BF16, MF_F16, MF_FP8) + SPLIT_CODES:
        why.append(f"compute code {d.dtype}")
    if d.a_dtype != d.dtype and not (d.a_dtype == MF_F32 and d.dtype in (MF_BF16,) + SPLIT_CODES):
        why.append(f"a_dtype {d.a_dtype} with dtype {d.dtype}")
    if (d.a_scale or d.w_scale) and d.dtype != MF_FP8:
        why.append("a_scale / w_scale without the fp8 code")
    if d.dtype == MF_FP8 and (d.ln_colsum or d.vt_out):
        why.append("fp8 with ln_colsum / vt_out (the entry refuses it)")
    if d.w_split and d.dtype not in SPLIT_CODES:
        why.append("w_split with a non-split code")
    if d.nz < 1 or d.zdiv < 1:
        why.append(f"nz {d.nz} / zdiv {d.zdiv}")
    if d.nz > 1 and (d.a1 or d.w_split):
        why.append("z-batching with a second A segment or a pre-split W")
    if d.bias_mode not in (0, 1):
        why.append(f"bias_mode {d.bias_mode}")
    if d.act not in (ACT_NONE, ACT_SILU, ACT_GEGLU4):
        why.append(f"act {d.act}")
    if d.act == ACT_GEGLU4 and d.n % 8:
        why.append("GEGLU with n % 8 != 0")
    if d.upsample not in (0, 1):
        why.append(f"upsample {d.upsample}")
    for name in ("res0", "res1"):
        if getattr(d, name) and getattr(d, name + "_dtype") not in TORCH_DT:
            why.append(f"{name}_dtype {getattr(d, name + '_dtype')}")
    if d.out_dtype not in TORCH_DT:
        why.append(f"out_dtype {d.out_dtype}")
    if d.ln_colsum and (d.kh != 1 or d.kw != 1 or d.a1 or d.nz != 1):
        why.append("folded LayerNorm outside a plain 1x1 GEMM")
    if d.vt_out and (d.vt_n0 <= 0 or d.vt_n0 >= d.n or d.vt_tokens <= 0 or d.act != ACT_NONE):
        why.append("vt_out geometry")
    if d.defer_reduce:
        why.append("defer_reduce (replay with defer_reduce = 0)")
    if why:
        raise NotModelled("; ".join(why))


def m_rows(d) -> int:
    return d.batch * d.h_out * d.w_out


def k_depth(d) -> int:
    return d.kh * d.kw * (d.c0 + d.c1)


def out_cols(d) -> int:
    return d.n // 2 if d.act == ACT_GEGLU4 else d.n


def zoff(z: int, zdiv: int, o: int, i: int) -> int:
    return (z // zdiv) * o + (z % zdiv) * i


def _take(buf: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """buf[idx]; fp8 storage is indexed through its bytes."""
    if buf.dtype == FP8_DT:
        return buf.view(torch.uint8)[idx].view(FP8_DT).float()
    return buf[idx]


def _a_values(d, t: torch.Tensor) -> torch.Tensor:
    """Operand A as the kernel multiplies it: 16-bit storage as is, fp32 storage under a bf16 code rounded to bf16 (RNE), fp32
    under the split and fp32 codes as is."""
    if d.dtype == MF_BF16 and t.dtype == torch.float32:
        t = t.to(torch.bfloat16)
    return t.double()


def gather_a(d, ops, rows: torch.Tensor, z: int = 0) -> torch.Tensor:
    """[rows, K] float64 implicit-GEMM A rows: k = (ky * kw + kx) * (c0 + c1) + c over cat(a0[:c0], a1[:c1]) of the (upsampled)
    input pixel the tap lands on; taps outside the image read 0."""
    hw = d.h_out * d.w_out
    b, rem = rows // hw, rows % hw
    oy, ox = rem // d.w_out, rem % d.w_out
    hin, win = (2 * d.h_in, 2 * d.w_in) if d.upsample else (d.h_in, d.w_in)
    segs = [(ops["a0"], d.c0, d.lda0)] + ([(ops["a1"], d.c1, d.lda1)] if d.c1 else [])
    za = zoff(z, d.zdiv, d.a_zs_o, d.a_zs_i)
    cols = []
    for ky in range(d.kh):
        for kx in range(d.kw):
            iy = oy * d.stride - d.pad_t + ky
            ix = ox * d.stride - d.pad_l + kx
            ok = (iy >= 0) & (iy < hin) & (ix >= 0) & (ix < win)
            sy, sx = iy.clamp(0, hin - 1), ix.clamp(0, win - 1)
            if d.upsample:
                sy, sx = sy // 2, sx // 2
            pix = (b * d.h_in + sy) * d.w_in + sx
            for buf, c, lda in segs:
                idx = za + pix[:, None] * lda + torch.arange(c, device=pix.device)[None, :]
                v = _a_values(d, _take(buf, idx))
                cols.append(torch.where(ok[:, None], v, torch.zeros((), dtype=v.dtype, device=v.device)))
    return torch.cat(cols, 1)


def w_matrix(d, ops, z: int = 0) -> torch.Tensor:
    """[n, K] float64 weight rows as multiplied: 16-bit / fp32 values, or hi + lo of a pre-split row (per 32 k: 32 high halves,
    then 32 low halves; ldw counted in 4-byte units)."""
    k = k_depth(d)
    buf = ops["w"]
    dev = buf.device
    nn = torch.arange(d.n, device=dev)
    if d.w_split:
        kp = (k + 31) // 32 * 32
        kk = torch.arange(kp, device=dev)
        hi_off = (kk // 32) * 64 + kk % 32
        base = nn[:, None] * (2 * d.ldw)
        w = buf[base + hi_off[None, :]].double() + buf[base + hi_off[None, :] + 32].double()
        return w[:, :k]
    wz = zoff(z, d.zdiv, d.w_zs_o, d.w_zs_i)
    return _take(buf, wz + nn[:, None] * d.ldw + torch.arange(k, device=dev)[None, :]).double()


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gelu_d(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def reference(d, ops, rows: torch.Tensor, zs: Optional[List[int]] = None, fp8_allow: float = FP8_A) -> Ref:
    """Exact output and S for output rows `rows` (int64) of every z in `zs` (default all).  fp8_allow: FP8_A above; 0 for cases
    whose products and sums are exact in fp32 (small integer codes, power-of-two scales)."""
    check_supported(d)
    dev = ops["a0"].device
    rows = rows.to(dev)
    zs = list(range(d.nz)) if zs is None else zs
    n = d.n
    ncol = torch.arange(n, device=dev)
    pers = d.tile == PERS_TILE
    if pers and d.out_dtype == MF_F32:
        raise NotModelled("tile 70 with an fp32 output")
    vs, ss, al = [], [], []
    fp8 = d.dtype == MF_FP8
    prods = [(gather_a(d, ops, rows, z), w_matrix(d, ops, z)) for z in zs]
    if fp8:         # R: the rms of the unscaled code product over the case (FP8_A)
        code_rms = math.sqrt(sum(float(((a @ w.T) ** 2).sum()) for a, w in prods) / max(1, len(zs) * len(rows) * n))
    for z, (a, w) in zip(zs, prods):
        acc = a @ w.T
        s = a.abs() @ w.abs().T
        allow = torch.zeros_like(acc)
        if fp8:
            rs = ops["a_scale"][(z // d.zdiv) * d.a_scale_zs + rows].double()[:, None] if d.a_scale else torch.ones((), dtype=torch.float64, device=dev)
            cs = ops["w_scale"][(z // d.zdiv) * d.w_scale_zs + ncol].double()[None, :] if d.w_scale else torch.ones((), dtype=torch.float64, device=dev)
            g = (rs * cs).abs()
            acc, s, allow = acc * rs * cs, s * g, allow + fp8_allow * code_rms * g
        if d.ln_colsum:
            # out = rstd[m] (acc - mean[m] colsum[n]): mean / var of the A row over K (population variance), in the kernel from fp32
            # sums: d(mean) ~ mean|a|, d(var) ~ mean(a^2) + |mean| mean|a| (cancellation of E[a^2] - mean^2), d(rstd)/rstd ~ d(var)/var
            k = a.shape[1]
            mean = a.mean(1, keepdim=True)
            var = a.var(1, unbiased=False, keepdim=True)
            r = 1.0 / torch.sqrt(var + d.ln_eps)
            cs = ops["ln_colsum"][:n].double()[None, :]
            acc = r * (acc - mean * cs)
            amp = ((a * a).mean(1, keepdim=True) + mean.abs() * a.abs().mean(1, keepdim=True)) / (var + d.ln_eps)
            s = r * (s + cs.abs() * a.abs().sum(1, keepdim=True) / k + (mean * cs).abs()) + acc.abs() * amp
            allow = LN_A * acc.abs() * amp
        v = acc
        if d.bias:
            b = ops["bias"].double()
            b = b[rows][:, None] if d.bias_mode else b[:n][None, :]
            v, s = v + b, s + b.abs()
        if d.temb:
            img = rows // (d.h_out * d.w_out)
            t = ops["temb"][img[:, None] * d.ld_temb + ncol[None, :]].double()
            v, s = v + t, s + t.abs()
        v, s, allow = v * d.alpha, s * abs(d.alpha), allow * abs(d.alpha)
        if pers:
            # tile 70's 16-bit slab (PERS_TILE above): the value before the residual / activation is rounded to the storage type
            um = ulp(v, d.out_dtype)
            v16 = v.to(TORCH_DT[d.out_dtype]).double()
            near = (v - v16).abs() >= 0.5 * um - BOUND16 * s - allow
            allow = allow + torch.where(near, 2 * um, torch.zeros_like(um))
            v = v16
        if d.res0:
            r0 = ops["res0"][rows[:, None] * d.ld_res0 + ncol[None, :]].double()
            v, s = v + r0, s + r0.abs()
        if d.res1:
            mm = rows % d.res1_rows if 0 < d.res1_rows < m_rows(d) else rows
            r1 = ops["res1"][mm[:, None] * d.ld_res1 + ncol[None, :]].double()
            v, s = v + r1, s + r1.abs()
        if d.act == ACT_SILU:
            sg = torch.sigmoid(v)
            y = v * sg
            gain = (sg * (1.0 + v * (1.0 - sg))).abs()
            s, allow = gain * s + y.abs(), gain * allow
            v = y
        elif d.act == ACT_GEGLU4:
            # per 8 columns: 4 values then their 4 gates; output column 4 g + j = value 8 g + j times gelu(gate 8 g + 4 + j)
            sh = (len(rows), n // 8, 8)
            vv, sv, av = v.view(sh), s.view(sh), allow.view(sh)
            val, gate = vv[..., :4], vv[..., 4:]
            y = val * _gelu(gate)
            g_val, g_gate = _gelu(gate).abs(), (val * _gelu_d(gate)).abs()
            s = g_val * sv[..., :4] + g_gate * sv[..., 4:] + y.abs()
            allow = g_val * av[..., :4] + g_gate * av[..., 4:] + (GELU_LUT_A if pers else GELU_A) * (val * gate).abs()
            v = y.reshape(len(rows), n // 2)
            s = s.reshape(len(rows), n // 2)
            allow = allow.reshape(len(rows), n // 2)
        vs.append(v)
        ss.append(s)
        al.append(allow)
    return Ref(torch.stack(vs), torch.stack(ss), rows, torch.stack(al))


# ---- comparator -------------------------------------------------------------------------------------------------------------

MANT = {MF_BF16: 7, MF_F16: 10, MF_F32: 23}
EMIN = {MF_BF16: -126, MF_F16: -14, MF_F32: -126}


def ulp(ref: torch.Tensor, code: int) -> torch.Tensor:
    """The spacing of the storage format at |ref| (subnormal spacing below the normal range)."""
    _, e = torch.frexp(ref.abs())
    e = torch.clamp(e.to(torch.int64) - 1, min=EMIN[code])
    return torch.ldexp(torch.ones_like(ref), (e - MANT[code]).to(ref.dtype))


@dataclass
class Verdict:
    ok: bool
    msg: str
    max_ulp: float           # max |got - ref| / ulp_out(ref)
    mean_e: float            # mean of sign(ref) e over the statistics elements (nan if too few)
    rms_e: float
    n_stat: int
    worst: float             # max |got - ref| / bound


def bound(ref: torch.Tensor, s: torch.Tensor, code: int, a: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-element bound: 16-bit outputs 0.5 ulp_out(ref) + 2^-18 S (the correctly rounded exact value, plus what the fp32
    accumulation may have moved it); fp32 outputs 2^-19 S (see BOUND16 / BOUND32); plus the allowance `a` (Ref.a)."""
    b = BOUND32 * s if code == MF_F32 else 0.5 * ulp(ref, code) + BOUND16 * s
    return b if a is None else b + a


def compare(got: torch.Tensor, ref: torch.Tensor, s: torch.Tensor, code: int, what: str = "",
            a: Optional[torch.Tensor] = None) -> Verdict:
    """got: the kernel's stored values (any float dtype); ref / s: float64 from reference().

    Every element: |got - ref| <= bound().  16-bit outputs with N >= 1000 elements where |ref| >= 2^-10 S (there the accumulation
    error is << 1 ulp, so e = (got - ref) / ulp_out(ref) of a correctly rounded result is uniform on [-0.5, 0.5]: mean 0, standard
    deviation 1 / sqrt(12) = 0.2887, e^2 has mean 1/12 and standard deviation sqrt(1/80 - 1/144) = 0.0745):
      |mean(sign(ref) e)| <= 6 * 0.2887 / sqrt(N)        (truncation toward zero: mean -0.25; a dropped K term: a bias of its sign)
      mean(e^2) <= 1/12 + 6 * 0.0745 / sqrt(N)            (a second rounding of an intermediate: mean(e^2) ~ 1/6)
    With an allowance `a` (deliberate approximations, Ref.a) e may move by d = a / ulp: the bias limit grows by mean(d), the
    spread limit by mean(|e0| 2 d + d^2) <= mean(d) / 2 + mean(d^2) (|e0| averages 1/4).
    """
    got = got.double()
    err = (got - ref).abs()
    b = bound(ref, s, code, a)
    u = ulp(ref, code)
    e = (got - ref) / u
    finite = torch.isfinite(got)
    bad = (~finite) | (err > b)
    nbad = int(bad.sum())
    worst = float((err / b.clamp_min(1e-300)).max()) if got.numel() else 0.0
    max_ulp = float(e.abs().max()) if got.numel() else 0.0
    msgs = []
    if nbad:
        i = int(torch.argmax((err / b.clamp_min(1e-300)).masked_fill(~finite, float("inf")).flatten()))
        msgs.append(f"{nbad}/{got.numel()} elements outside the bound (worst at flat {i}: got {float(got.flatten()[i])!r} "
                    f"ref {float(ref.flatten()[i])!r} bound {float(b.flatten()[i]):.3e})")
    mean_e = rms_e = float("nan")
    n_stat = 0
    if code != MF_F32:
        sel = (ref.abs() >= 2.0 ** -10 * s) & (ref != 0) & finite
        n_stat = int(sel.sum())
        if n_stat:
            es = e[sel]
            mean_e = float((torch.sign(ref[sel]) * es).mean())
            rms_e = float((es * es).mean().sqrt())
        if n_stat >= 1000:
            dm = dq = 0.0
            if a is not None:
                dd = a[sel] / u[sel]
                dm, dq = float(dd.mean()), float(0.5 * dd.mean() + (dd * dd).mean())
            lim_m = 6 * 0.2887 / math.sqrt(n_stat) + dm
            lim_q = 1.0 / 12 + 6 * 0.0745 / math.sqrt(n_stat) + dq
            if abs(mean_e) > lim_m:
                msgs.append(f"rounding bias: mean(sign(ref) e) = {mean_e:+.4f} ulp over {n_stat} elements (limit {lim_m:.4f})")
            if rms_e ** 2 > lim_q:
                msgs.append(f"rounding spread: mean(e^2) = {rms_e ** 2:.4f} ulp^2 over {n_stat} elements (limit {lim_q:.4f})")
    else:
        n_stat = got.numel()
        if n_stat:
            es = e.flatten()
            mean_e = float((torch.sign(ref.flatten()) * es).mean())
            rms_e = float((es * es).mean().sqrt())
    return Verdict(not msgs, (what + ": " if what else "") + "; ".join(msgs), max_ulp, mean_e, rms_e, n_stat, worst)


def untouched(buf_bytes: torch.Tensor, region_bytes: torch.Tensor, sentinel: int = SENTINEL) -> int:
    """Number of bytes outside the written region (bool mask, same length) that lost their sentinel."""
    return int(((buf_bytes != sentinel) & ~region_bytes).sum())


def region_mask(numel: int, blocks, device=None) -> torch.Tensor:
    """Element mask of a flat buffer; blocks = [(offset, rows, cols, ld)] written by the launch."""
    mask = torch.zeros(numel, dtype=torch.bool, device=device)
    for off, r, c, ld in blocks:
        if r and c:
            mask.as_strided((r, c), (ld, 1), off).fill_(True)
    return mask


def out_blocks(d):
    """[(element offset, rows, cols, row stride)] of `out` the launch writes (per z), and of `vt_out` (None without it)."""
    m = m_rows(d)
    cols = d.vt_n0 if d.vt_out else out_cols(d)
    out = [(zoff(z, d.zdiv, d.o_zs_o, d.o_zs_i), m, cols, d.ldc) for z in range(d.nz)]
    vt = None
    if d.vt_out:
        nv, imgs = d.n - d.vt_n0, m // d.vt_tokens
        vt = [(0, imgs * nv, d.vt_tokens, d.vt_ld)]
    return out, vt


def sample_rows(m: int, seed: int, block: int = 128, budget: int = 4096, all_below: int = 8192) -> torch.Tensor:
    """Whole `block`-row blocks: all rows when m <= all_below, else the first block, the last (possibly partial) one and seeded
    random blocks up to about `budget` rows."""
    if m <= all_below:
        return torch.arange(m)
    nb = (m + block - 1) // block
    g = torch.Generator().manual_seed(seed)
    pick = {0, nb - 1}
    want = max(budget // block, 2)
    for i in torch.randperm(nb - 2, generator=g)[: max(want - 2, 0)].tolist():
        pick.add(i + 1)
    blocks = sorted(pick)
    return torch.cat([torch.arange(b * block, min((b + 1) * block, m)) for b in blocks])


def check_gn_part(part: torch.Tensor, r: int, groups: int, d, ref: Ref, code: int) -> List[str]:
    """The (sum, sum of squares) per channel (and per group when `groups` > 0) of every R-row block whose rows are all in ref.rows,
    against float64 sums of ref.v.  Tolerance: the sum over the block of each element's bound (times 2|ref| + bound for the
    squares), plus 2^-20 times the block's sum of |ref| (of ref^2): the fp32 summation of at most a few hundred terms."""
    n, m = d.n, m_rows(d)
    v, s = ref.v[0], ref.s[0]
    b = bound(v, s, code, ref.a[0])
    rows = ref.rows.cpu()
    pos = {int(x): i for i, x in enumerate(rows.tolist())}
    part = part.double().cpu()
    fails = []
    for blk in sorted({int(x) // r for x in rows.tolist()}):
        lo, hi = blk * r, min(blk * r + r, m)
        if any(x not in pos for x in range(lo, hi)):
            continue
        idx = torch.tensor([pos[x] for x in range(lo, hi)], device=v.device)
        vb, bb = v[idx], b[idx]
        want = torch.stack([vb.sum(0), (vb * vb).sum(0)], 1).cpu()
        tol = torch.stack([bb.sum(0) + 2.0 ** -20 * vb.abs().sum(0),
                           (bb * (2 * vb.abs() + bb)).sum(0) + 2.0 ** -20 * (vb * vb).sum(0)], 1).cpu()
        got = part[2 * blk * n: 2 * (blk + 1) * n].view(n, 2)
        bad = ((got - want).abs() > tol) | ~torch.isfinite(got)
        if bad.any():
            c = int(bad.any(1).nonzero()[0])
            fails.append(f"gn_part block {blk} (rows {lo}-{hi}): {int(bad.sum())} bad; channel {c} got {got[c].tolist()} "
                         f"want {want[c].tolist()} tol {tol[c].tolist()}")
        if groups:
            cpg = n // groups
            gw = want.view(groups, cpg, 2).sum(1)
            gt = tol.view(groups, cpg, 2).sum(1)
            base = 2 * n * (m // r) + 2 * blk * groups
            gg = part[base: base + 2 * groups].view(groups, 2)
            gbad = ((gg - gw).abs() > gt) | ~torch.isfinite(gg)
            if gbad.any():
                g = int(gbad.any(1).nonzero()[0])
                fails.append(f"gn_part groups block {blk}: {int(gbad.sum())} bad; group {g} got {gg[g].tolist()} want {gw[g].tolist()}")
    return fails


def gather_got(d, out: torch.Tensor, rows: torch.Tensor, vt: Optional[torch.Tensor] = None,
               zs: Optional[List[int]] = None) -> torch.Tensor:
    """The launch's stored values for `rows` of every z, laid out like Ref.v: `out` (and `vt_out`) as flat typed tensors from
    the descriptor's pointers.  Columns n >= vt_n0 are read from vt_out[m / vt_tokens][n - vt_n0][m % vt_tokens]."""
    zs = list(range(d.nz)) if zs is None else zs
    rows = rows.to(out.device)
    cols = out_cols(d)
    res = []
    for z in zs:
        oz = zoff(z, d.zdiv, d.o_zs_o, d.o_zs_i)
        nout = d.vt_n0 if d.vt_out else cols
        got = out[oz + rows[:, None] * d.ldc + torch.arange(nout, device=out.device)[None, :]]
        if d.vt_out:
            nv = d.n - d.vt_n0
            img, tok = rows // d.vt_tokens, rows % d.vt_tokens
            cv = torch.arange(nv, device=out.device)
            g2 = vt[(img[:, None] * nv + cv[None, :]) * d.vt_ld + tok[:, None]]
            got = torch.cat([got, g2.to(got.dtype)], 1)
        res.append(got)
    return torch.stack(res)
