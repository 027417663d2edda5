"""float64 reference, per-element error bound, gradient families and an arithmetic model of the flash-attention BACKWARD
(attn_bwd_kernel<HD, KV, B16> in csrc/attention.hip, behind mf_attention_bwd_f16x3 and mf_attention_bwd_bf16).  A helper: no test
functions here; tests/test_attention_bwd_reference_cpu.py proves on the CPU that the inputs have teeth, tests/test_attention_bwd_gpu.py
holds the kernel to the bound.  The sibling of attention_ref.py, whose reference, input families, storage rounding and units it reuses.

Reference.  s = scale q k^T (natural log), w = softmax(s), o = w v, and for an upstream gradient dO:
    dP = dO v^T,   D_i = sum_c dO_ic o_ic,   dS = w (dP - D),   G = scale dS,
    dQ = G k,      dK = G^T q,               dV = w^T dO.

Bound.  The kernel recomputes P from the caller's lse:  P~ = exp2(fma(T, c, -(lse2 - pshift))), T = q.k accumulated in fp32,
c = fp32(scale log2 e), and forms G~ = scale P~ (U - D), U = dO.v accumulated in fp32 (attention.hip:735-737, 787-794).  For query i,
key k, with lse_i = lse2_i ln 2 (natural log):

    eps_ik = u_S scale sum_c |q_ic| |k_kc| + 2^-22 (|s_ik| + |lse_i|) + 2^-20 [+ the caller's lse error, if it is not the exact one]
    eta_ik = u_S sum_c |dO_ic| |v_kc| + 2^-23 |D_i| + 2^-24 |dP_ik - D_i|      [+ the caller's D error]
    eP_ik  = w_ik (eps_ik + u_P + u_X) + a
    eG_ik  = |G_ik| (eps_ik + u_P + u_X + 2^-22) + scale w_ik eta_ik + a
    B_dq_ij = u_O |dQ_ij| + sum_k eG_ik |k_kj| + n(skv) 2^-24 sum_k |G_ik| |k_kj|
    B_dk_kj = u_O |dK_kj| + sum_i eG_ik |q_ij| + n(sq)  2^-24 sum_i |G_ik| |q_ij|
    B_dv_kj = u_O |dV_kj| + sum_i eP_ik |dO_ij| + n(sq)  2^-24 sum_i w_ik |dO_ij|

eps is the relative error of the unrounded P~:
  u_S     = 2^-20 (attention_ref.units off the MJ head dims: the backward has no Q~ rounding; fp32 accumulation of <= 80 exact products or
          the 22-bit operand split, attention.hip:700-710), times the score's condition number;
  2^-22.. the exponent's argument in fp32: the supplied lse2 is an fp32 number (2^-24 |lse2|), `lse - pshift` rounds once
          (attention.hip:592, 725, 776: 2^-24 (|lse2| + 8)), c rounds scale log2 e (2^-24 |T c|), the fma rounds its result
          (2^-24 (|T c| + |lse2| + 8)); in natural-log units that is at most 2^-22 (|s| + |lse|) + 16 ln 2 2^-24;
  2^-20   those 16 ln 2 2^-24 of pshift <= 8, and one ulp (2^-23) of v_exp_f32 (attention.hip:735, 788).
eta is the absolute error of (U - D): U's fp32 accumulation (u_S again, relative to sum |dO| |v|), the fp32 rounding of the supplied D
and of the subtraction (2^-24 |D| each, 2^-24 |dP - D|: attention.hip:737, 794).
u_P     the rounding of P~ and of G~ to the operand type of the last products (attention.hip:750-753, 806): attention_ref.units' u_P,
        2^-8 bf16, 2^-21 for the two truncated fp16 pieces; 2^-22 more on G for its two fp32 multiplications (attention.hip:737).
u_X     2^-22 on the split form: of the four products hi.hi + hi.lo + lo.hi + lo.lo the three MFMAs leave out lo.lo, two factors of 2^-11
        (attention.hip:843-845, 849-851); 0 on bf16.
a       the ABSOLUTE floor of the split: P~ and G~ are split AFTER the 2^pshift pre-scale, and the low piece is an fp16 toward zero whose
        subnormal spacing is 2^-24: a = 2^-24 2^-pshift with pshift = min(8, floor(log2 skv)) as launch_attn_bwd computes it
        (attention.hip:1128-1130).  bf16 has fp32's exponent range: 0.  (The unfused routes, which split the fp32 P and dS without a shift,
        take attention_ref.units' a_P = 2^-24 of 'f16x3_unfused'.)
n(S)    the fp32 roundings an accumulator goes through: one per MFMA issue, 4 k-steps per 64-row tile and 3 MFMAs per product on the split
        form, 1 on bf16 (attention.hip:830-854): n = m 4 ceil(S / 64), each 2^-24 of a partial sum that sum |terms| bounds.  The unfused
        routes are GEMMs over S terms: n = S.
u_O     the stored gradient: fp32 (2^-23, attention_ref.units' u_O of the fp32 outputs; inv_pscale is a power of two), or 2^-8 for the
        bf16 outputs of out_dtype = MF_BF16 (attention.hip:885-887).
A test passes when |got - ref| <= B for every element of dQ, dK and dV: factor 1, no atol."""
import functools
import math
import types

import torch

import attention_ref as A
from attention_ref import LOG2E, TILE, WAVE, merge_heads, split_heads

FLAVOURS = ("f16x3", "bf16")                         # mf_attention_bwd_f16x3, mf_attention_bwd_bf16
GRADS = ("dense", "aligned", "sparse_rows")
FAULTS = ("no_D", "lse_natural_log", "tail_queries_unmasked", "tail_keys_unmasked", "drop_tile", "pshift_not_undone", "dd_wrong_layout",
          "scale_missing")
F16_MAX = 65504.0
U_S = 2.0 ** -20


# ---- the cases both test files run ---------------------------------------------------------------------------------------------
# A block covers 256 column items, a tile 64 rows (double-buffered), sq % 4 == 0 is required.  (324, 77): 6 query tiles, the last with 4
# rows; two query blocks, the second with 68 items; one key block with 179 ghost lanes; two key tiles.  (68, 300) adds a ragged second
# key block; (256, 256) has no ragged edge anywhere (the bf16 form runs its unmasked path only).
B, HEADS = 2, 3                                      # batch and head strides differ, and batch 0's tile tails see batch 1's rows
ENTRY_DIMS = (("f16x3", 8), ("f16x3", 40), ("bf16", 8), ("bf16", 40), ("bf16", 80))
FAMILIES = ("dense", "peaked", "stairs_up", "stairs_down", "late_spike", "all_negative", "flat")
SHAPES = ((324, 77), (324, 333))
RAGGED = ((324, 77), (324, 333), (68, 300))
EVEN = (256, 256)
GUARD_QUIET = [(d, family, grad, sq, skv) for d in (8, 40) for family in ("all_negative", "flat") for grad in ("dense", "aligned")
               for sq, skv in RAGGED]
GUARD_LOUD = [(d, "peaked", "dense", sq, skv) for d in (8, 40) for sq, skv in ((324, 77), (324, 333))]


@functools.lru_cache(maxsize=12)
def case(flavour, d, family, grad, sq, skv, gain=1.0):
    """Inputs (float64, rounded to the flavour's storage), the float64 reference and the bound of one case, built once.  gain: a power
    of two on dO (exact in every storage)."""
    scale = f32_scale(d)
    seed = 100 * d + 7 * sq + skv
    q, k, v = A.make_inputs(family, B, HEADS, sq, skv, d, seed=seed, rnd=flavour)
    do = make_grad(grad, A.reference(q, k, v, HEADS, scale)[0], HEADS, seed + 1, flavour) * gain
    ref = reference_bwd(q, k, v, do, HEADS, scale)
    return types.SimpleNamespace(q=q, k=k, v=v, do=do, scale=scale, ref=ref, bound=bound_bwd(q, k, v, do, HEADS, scale, ref, flavour),
                                 lse=ref.lse2.float(), dd=ref.D.float())           # what the caller hands over: fp32


def loud_gain(d, family, grad, sq, skv):
    """The power of two on dO that carries the real-pair maximum of the guarded quantity past 4 x 65504."""
    m = real_pair_max(case("f16x3", d, family, grad, sq, skv).ref, f32_scale(d), skv, "f16x3")[0]
    return 2.0 ** (math.floor(math.log2(4.0 * F16_MAX / m)) + 1)


def ratio(got, want, bnd):
    """err / B per element; an error where B is 0 (an exactly zero gradient: q = 0, dO = 0) counts as inf, none as 0."""
    err = (got - want).abs()
    return torch.where(bnd > 0, err / bnd, torch.where(err > 0, math.inf, 0.0).to(err.dtype)).nan_to_num(math.inf)


def f32_scale(d):
    """d^-1/2 as the C entry receives it: a float."""
    return float(torch.tensor(d ** -0.5, dtype=torch.float32))


def pshift_of(skv, flavour):
    """launch_attn_bwd: 2^sh <= skv, at most 2^8; none on bf16."""
    sh = 0
    while flavour == "f16x3" and sh < 8 and (2 << sh) <= skv:
        sh += 1
    return sh


def reference_bwd(q, k, v, do, heads, scale):
    """float64 views of the stored operands, q / do [B, sq, C], k / v [B, skv, C] -> a namespace of dq, dk, dv [B, S, C], o [B, sq, C],
    w, s, dP, dS [B, H, sq, skv], D, lse2 [B, H, sq] (explicit formulas: the module docstring)."""
    o, w, s, lse2 = A.reference(q, k, v, heads, scale)
    q4, k4, v4, do4, o4 = (split_heads(t.double(), heads) for t in (q, k, v, do, o))
    dP = do4 @ v4.transpose(-1, -2)
    D = (do4 * o4).sum(-1)
    dS = w * (dP - D[..., None])
    return types.SimpleNamespace(dq=merge_heads(scale * (dS @ k4)), dk=merge_heads(scale * (dS.transpose(-1, -2) @ q4)),
                                 dv=merge_heads(w.transpose(-1, -2) @ do4), o=o, w=w, s=s, lse2=lse2, dP=dP, D=D, dS=dS)


def make_grad(family, o, heads, seed, rnd):
    """dO [B, sq, C] in float64, already rounded to storage (`rnd`: 'bf16' or 'f16x3', attention_ref.stored) for the exact output `o`."""
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(o.shape, generator=g, dtype=torch.float64)
    if family == "dense":
        do = noise
    elif family == "aligned":
        # along o, head by head: D = dO.o = 4 |o| is large, and on a peaked row dP_ik = dO_i.v_k is as large for the hot key
        o4 = split_heads(o, heads)
        do = merge_heads(4.0 * o4 / o4.norm(dim=-1, keepdim=True)) + 0.1 * noise
    elif family == "sparse_rows":
        do = torch.zeros_like(o)
        do[:, ::37] = noise[:, ::37]
    else:
        raise ValueError(family)
    return A.stored(do, rnd)


def real_pair_max(ref, scale, skv, flavour):
    """float64 max over the real (query, key) pairs of what the range guard looks at, |scale dS| 2^pshift, and of |dS| 2^pshift."""
    m = float(ref.dS.abs().max()) * 2.0 ** pshift_of(skv, flavour)
    return scale * m, m


def bound_bwd(q, k, v, do, heads, scale, ref, flavour, *, out16=False, lse_err=None, d_err=None):
    """(B_dq, B_dk, B_dv) for reference_bwd's `ref` of the same operands.  flavour: 'f16x3' / 'bf16' (the flash kernel), or
    'f16x3_unfused' / 'fp32' / 'bf16_unfused' (the GEMM chain of autograd.record_attention in that precision; the last is the bf16x1
    mode, whose GEMMs round P and dS to bf16 as the flash kernel does).  lse_err [B, H, sq] (natural log) and d_err [B, H, sq]: the
    error of a caller's lse and D that are not the exact ones rounded to fp32 (route_errors)."""
    d = q.shape[-1] // heads
    sq, skv = q.shape[1], k.shape[1]
    flash = flavour in FLAVOURS
    u_p = A.units(flavour.split("_")[0], d)[0]
    a_unfused = 0.0 if flavour == "bf16_unfused" else A.units(flavour, d)[3]
    split = flavour in ("f16x3", "f16x3_unfused")
    u_x = 2.0 ** -22 if split else 0.0
    a = (2.0 ** -24 * 2.0 ** -pshift_of(skv, flavour) if flavour == "f16x3" else 0.0) if flash else a_unfused
    u_o = 2.0 ** -8 if out16 else 2.0 ** -23
    n = (lambda s_: (3 if split else 1) * 4 * -(-s_ // TILE)) if flash else (lambda s_: s_)
    q4, k4, v4, do4 = (split_heads(t.double(), heads).abs() for t in (q, k, v, do))
    w, dpd = ref.w, ref.dP - ref.D[..., None]
    lse = (ref.lse2 / LOG2E).abs()[..., None]
    eps = U_S * scale * (q4 @ k4.transpose(-1, -2)) + 2.0 ** -22 * (ref.s.abs() + lse) + 2.0 ** -20
    if lse_err is not None:
        eps = eps + lse_err[..., None]
    eta = U_S * (do4 @ v4.transpose(-1, -2)) + 2.0 ** -23 * ref.D.abs()[..., None] + 2.0 ** -24 * dpd.abs()
    if d_err is not None:
        eta = eta + d_err[..., None]
    g = scale * (w * dpd).abs()
    e_p = w * (eps + u_p + u_x) + a
    e_g = g * (eps + u_p + u_x + 2.0 ** -22) + scale * w * eta + a
    r = 2.0 ** -24
    b_dq = u_o * ref.dq.abs() + merge_heads(e_g @ k4 + n(skv) * r * (g @ k4))
    b_dk = u_o * ref.dk.abs() + merge_heads(e_g.transpose(-1, -2) @ q4 + n(sq) * r * (g.transpose(-1, -2) @ q4))
    b_dv = u_o * ref.dv.abs() + merge_heads(e_p.transpose(-1, -2) @ do4 + n(sq) * r * (w.transpose(-1, -2) @ do4))
    return b_dq, b_dk, b_dv


def route_errors(q, k, v, do, heads, scale, ref, flavour):
    """(lse_err, d_err) of bound_bwd for ops.attention_train + Tape.backward, where lse and D are the project's own.
    Flash routes ('f16x3', 'bf16'): lse is the forward kernel's, inside attention_ref.bound's B_lse (log2 units: times ln 2), and
    D = mf_rowdot_heads(dO, O) of the forward's output, inside B per element, summed in fp32 over the d channels (d 2^-24 sum |dO| |o|).
    Unfused routes: P is mf_softmax_rows of the score GEMM, its relative error eps of bound_bwd plus that of the row's denominator,
    ebar_i = sum_k w_ik eps_ik — which takes lse_err's place — and D = sum_k P dP inside mf_softmax_bwd (train.hip, softmax_bwd_kernel):
    d_err_i = sum_k w_ik ((eps_ik + ebar_i) |dP_ik| + u_S sum_c |dO_ic| |v_kc|) + 2^-23 sum_k w_ik |dP_ik| (each product rounds to fp32,
    the double sum once more)."""
    d = q.shape[-1] // heads
    q4, k4, v4, do4 = (split_heads(t.double(), heads).abs() for t in (q, k, v, do))
    if flavour in FLAVOURS:
        b_o, b_lse = A.bound(q, k, v, heads, scale, (ref.o, ref.w, ref.s, ref.lse2), flavour)
        o4 = split_heads(ref.o, heads).abs()
        return b_lse * math.log(2.0), (do4 * split_heads(b_o, heads)).sum(-1) + d * 2.0 ** -24 * (do4 * o4).sum(-1)
    lse = (ref.lse2 / LOG2E).abs()[..., None]
    eps = U_S * scale * (q4 @ k4.transpose(-1, -2)) + 2.0 ** -22 * (ref.s.abs() + lse) + 2.0 ** -20
    ebar = (ref.w * eps).sum(-1)
    dp = ref.dP.abs()
    d_err = (ref.w * ((eps + ebar[..., None]) * dp + U_S * (do4 @ v4.transpose(-1, -2)))).sum(-1) + 2.0 ** -23 * (ref.w * dp).sum(-1)
    return ebar, d_err


# ---- arithmetic model ----------------------------------------------------------------------------------------------------------

def _f32(x):
    return x.float().double()


def _split(x):
    """x as the two fp16 pieces of mf_split_f16x2 (each toward zero, v_cvt_pkrtz saturating at the fp16 maximum), summed."""
    hi, lo = A.split_f16(x.clamp(-F16_MAX, F16_MAX).float())
    return hi.double() + lo.double()


def _bf16(x):
    return x.float().to(torch.bfloat16).double()


def transposed(x, ldt, pad=0.0):
    """[B, S, C] -> the transposed plane [B, C, ldt] of the descriptor; pad columns hold +-pad, alternating."""
    b, s, c = x.shape
    t = (pad * (1.0 - 2.0 * (torch.arange(ldt) % 2))).to(x.dtype).expand(b, c, ldt).clone()
    t[:, :, :s] = x.transpose(1, 2)
    return t


def _row_tile(x, t, heads):
    """Tile t of a row-major operand [B, S, C] as the DMA delivers it, [B, H, 64, d]: rows past S are the next batch's (the descriptor
    ends with the last batch: zeros past it)."""
    b, s, c = x.shape
    flat = torch.cat([x.reshape(b * s, c), x.new_zeros(TILE, c)])
    rows = (torch.arange(b)[:, None] * s + t * TILE + torch.arange(TILE)[None, :]).clamp_max(b * s + TILE - 1)
    return flat[rows].view(b, TILE, heads, c // heads).transpose(1, 2)


def _t_tile(xt, t, heads):
    """Tile t of a transposed plane [B, C, ldt], [B, H, d, 64]: 64 consecutive elements from column 64 t of each channel row, running
    on into the next row where ldt ends earlier (zeros past the plane)."""
    b, c, ldt = xt.shape
    flat = torch.cat([xt.reshape(-1), xt.new_zeros(TILE)])
    start = torch.arange(b * c)[:, None] * ldt + t * TILE + torch.arange(TILE)[None, :]
    return flat[start.clamp_max(b * c * ldt + TILE - 1)].view(b, heads, c // heads, TILE)


def _tile_stat(x, t, sq):
    """lse / dd of tile t's 64 rows [B, H, 64]: the descriptor of one (batch, head) ends at sq, rows past it read zeros."""
    out = x.new_zeros(*x.shape[:2], TILE)
    n = max(0, min(TILE, sq - t * TILE))
    out[..., :n] = x[..., t * TILE: t * TILE + n]
    return out


def emulate_bwd(q, k, v, do, lse2, dd, heads, scale, flavour, fault=None, *, ldqt=None, ldkt=None, pad=0.0, out16=False):
    """The kernel's arithmetic in float64 with its rounding points, as a specification: two passes over 64-row tiles against column
    items in waves of 32 (ghost lanes: zero fragments, and lse = D = 0 in the dQ pass), T and U in fp32, P~ = exp2(fma(T, c, -(lse2 -
    pshift))), G~ = (scale P~) (U - D), tail rows zeroed, both rounded to bf16 or truncated to two fp16 pieces, the accumulators
    rounded to fp32 after every tile and scaled by 2^-pshift at the end.  lse2 / dd [B, H, sq]: what the caller supplies (fp32 values).
    ldqt / ldkt / pad: the transposed planes as transposed() lays them out (default: S rounded up to 8, zero pads).
    Returns (dq, dk, dv, guard) with guard = (max |G~| over real column lanes, over ghost column lanes), the per-lane maxima the split
    form's range guard raises its flag from.  `fault`: one of FAULTS, the arithmetic of a kernel with that mistake."""
    assert flavour in FLAVOURS and (fault is None or fault in FAULTS)
    b, sq, c = q.shape
    skv = k.shape[1]
    split = flavour == "f16x3"
    rnd = _split if split else _bf16
    cc = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    sc32 = float(torch.tensor(scale, dtype=torch.float32))
    psh = pshift_of(skv, flavour)
    ldqt, ldkt = ldqt or -(-sq // 8) * 8, ldkt or -(-skv // 8) * 8
    lse2, dd = _f32(lse2), _f32(dd)
    if fault == "lse_natural_log":
        lse2 = _f32(lse2 / LOG2E)
    if fault == "dd_wrong_layout":
        dd = dd.transpose(1, 2).contiguous().view(dd.shape)
    real_max, ghost_max = 0.0, 0.0

    def one_pass(kv):
        nonlocal real_max, ghost_max
        c1, c2, r1, r2 = (k, v, q, do) if kv else (q, do, k, v)
        t1 = transposed(q, ldqt, pad) if kv else transposed(k, ldkt, pad)
        t2 = transposed(do, ldqt, pad) if kv else None
        s_c, s_r = c1.shape[1], r1.shape[1]
        scp = -(-s_c // WAVE) * WAVE
        ghost = torch.arange(scp) >= s_c
        colpad = lambda x: torch.cat([split_heads(x, heads), x.new_zeros(b, heads, scp - s_c, c // heads)], 2)
        f1, f2 = colpad(c1), colpad(c2)
        if not kv:                              # the lane's own query: lse - pshift and D, both 0.0f on a ghost lane
            lane = lambda x: torch.cat([x, x.new_zeros(b, heads, scp - s_c)], -1)[..., None, :]
            lv_c = torch.where(ghost, torch.zeros(()).double(), lane(_f32(lse2 - psh)))
            dv_c = lane(dd)
        acc1 = torch.zeros(b, heads, scp, c // heads, dtype=torch.float64)
        acc2 = torch.zeros_like(acc1)
        for t in range(-(-s_r // TILE)):
            if fault == "drop_tile" and t == 1:
                continue
            T = _f32(_row_tile(r1, t, heads) @ f1.transpose(-1, -2))                       # [B, H, 64 rows, scp lanes]
            U = _f32(_row_tile(r2, t, heads) @ f2.transpose(-1, -2))
            if kv:
                lv, dv = _f32(_tile_stat(lse2, t, sq) - psh)[..., None], _tile_stat(dd, t, sq)[..., None]
            else:
                lv, dv = lv_c, dv_c
            P = _f32(torch.exp2(_f32(T * cc - lv)))
            dead = (t * TILE + torch.arange(TILE) >= s_r)[:, None]
            if fault != ("tail_queries_unmasked" if kv else "tail_keys_unmasked"):
                P = torch.where(dead, torch.zeros_like(P), P)
            diff = U if fault == "no_D" else _f32(U - dv)
            G = _f32(_f32((1.0 if fault == "scale_missing" else sc32) * P) * diff)
            if split:
                ga = G.abs().nan_to_num(0.0, posinf=math.inf)                              # fmaxf drops a NaN
                real_max = max(real_max, float(ga[..., ~ghost].max()))
                if bool(ghost.any()):
                    ghost_max = max(ghost_max, float(ga[..., ghost].max()))
            # what a ghost lane holds is never stored: keep inf / NaN out of the matrix products
            Pr, Gr = (rnd(torch.where(ghost, torch.zeros_like(x), x)).transpose(-1, -2) for x in (P, G))
            acc1 = _f32(acc1 + Gr @ _t_tile(t1, t, heads).transpose(-1, -2))
            if kv:
                acc2 = _f32(acc2 + Pr @ _t_tile(t2, t, heads).transpose(-1, -2))
        inv = 1.0 if fault == "pshift_not_undone" else 2.0 ** -psh
        fin = lambda x: merge_heads((_bf16 if out16 else _f32)(x * inv)[:, :, :s_c])
        return fin(acc1), fin(acc2)

    dk, dv_ = one_pass(True)
    dq, _ = one_pass(False)
    return dq, dk, dv_, (real_max, ghost_max)
