"""float64 reference, per-element error bound, input families and an arithmetic model of the flash-attention kernels
(csrc/attention.hip).  A helper: no test functions here; tests/test_attention_reference_cpu.py proves on the CPU that the inputs
have teeth, tests/test_attention_gpu.py holds the kernels to the bound.

Bound.  For query i, key k, channel j (s: natural-log scores, w: softmax weights, o: the exact output):

    eps_ik  = u_P + u_S * scale * sum_c |q_ic| |k_kc| + 2^-22 (|s_ik| + max_k' |s_ik'|) + 2^-21
    B_ij    = u_O |o_ij| + a_O + sum_k (w_ik eps_ik + a_P wmax_i) (|v_kj| + |o_ij|)
    B_lse_i = sum_k (w_ik eps_ik + a_P wmax_i) / ln 2 + 2^-22 (|lse2_i| + 1)          (sums over the keys the mask leaves)

eps is the relative error of one un-normalised probability as the kernel holds it:
  u_P     the rounding of P to the operand type of the second product (pack_h2 of st[][] / mf_split_f16x2): one ulp, 2^-8 bf16,
          2^-11 fp16, 2^-21 for the two-piece fp16 split and for fp32;
  u_S     the rounding that reaches the score, times the score's condition number sum |q||k| scale: on the MJ head dims (8, 40) of
          the 16-bit flavours the rounding of Q~ = round16(q scale log2 e) (= u_P); elsewhere 2^-20 (fp32 accumulation of <= 512
          exact products, or the 22-bit operand split);
  2^-22.. the fp32 evaluation of the exponent's argument score - offset (both up to max |s| in size), and 2^-21 for v_exp_f32.
a_P is the ABSOLUTE rounding of P where the operand type runs out of exponent (the same pack_h2<F16> / mf_split_f16x2 lines): an fp16 P
below 2^-14 is a subnormal, spacing 2^-24, so a_P = 2^-25 (nearest); the split's low piece, of P * 2^SP_SHIFT = 256 P toward zero, leaves
2^-24 / 256 = 2^-32; bf16 has fp32's exponent range (0).  P is taken against an offset that never exceeds the row's running maximum, so
l >= 1 / wmax_i (wmax: the row's largest weight) and an absolute error a_P of P is at most a_P wmax_i of a weight.  It matters where one
key holds nearly all the weight and |o_j| is small: 76 keys of weight 2^-16 each then carry 2^-10 relative error.  a_O = 2^-25 is the
same spacing for a stored fp16 output below 2^-14.
The UNFUSED f16x3 form (ops.attention_unfused: head dim 160) hands the second GEMM the normalised weights in fp32, and that GEMM
splits its A operand into two fp16 pieces without a shift (gemm_conv_kernel.h, the mf_split_f16x2 of the A fragment): every weight
carries up to 2^-24 of absolute error whatever wmax is ('f16x3_unfused': a_P = 2^-24 and the factor wmax_i dropped).
An error d of a probability moves o_j by w d (v_kj - o_j): |v| + |o| covers the numerator and the denominator whether l sums the
rounded P (head dims with a ones row in V^T) or the unrounded one.  u_O is the rounding of the stored output (2^-8 / 2^-11 / 2^-23).
A test passes when |got - o| <= B for every element: factor 1, no atol."""
import math

import torch

LOG2E = 1.4426950408889634
MJ_DIMS = (8, 40)                 # 16-bit flavours: head dims whose QK^T reduction has three spare k slots (attention.hip `MJ`)
MJ_T = 5.0                        # deferred maximum: the offset moves when a score exceeds it by more than MJ_T exp2 units
TILE = 64                         # keys per tile
WAVE = 32                         # queries per wave (the rescale branches are wave-uniform)
FLAVOURS = ("bf16", "fp16", "f16x3")
FAMILIES = ("dense", "peaked", "stairs_up", "stairs_down", "late_spike", "early_spike", "all_negative", "flat")
FAULTS = ("no_o_rescale", "no_l_rescale", "drop_tile", "tail_unmasked", "causal_off_by_one", "offset_not_updated")
HOT = math.sqrt(40.0)             # a hot key of amplitude a scores a * HOT (natural log units) at every head dim


def units(flavour, d):
    """(u_P, u_S, u_O, a_P, a_O) of the module docstring for one precision and head dim."""
    if flavour in ("bf16", "fp16"):
        u = 2.0 ** -8 if flavour == "bf16" else 2.0 ** -11
        a = 2.0 ** -25 if flavour == "fp16" else 0.0
        return u, (u if d in MJ_DIMS else 2.0 ** -20), u, a, a
    if flavour in ("f16x3", "f16x3_unfused", "fp32"):
        return 2.0 ** -21, 2.0 ** -20, 2.0 ** -23, {"f16x3": 2.0 ** -32, "f16x3_unfused": 2.0 ** -24, "fp32": 0.0}[flavour], 0.0
    raise ValueError(flavour)


def split_heads(x, heads):
    b, s, c = x.shape
    return x.view(b, s, heads, c // heads).transpose(1, 2)            # [B, H, S, d]


def merge_heads(x):
    b, h, s, d = x.shape
    return x.transpose(1, 2).reshape(b, s, h * d)


def reference(q, k, v, heads, scale, causal=False):
    """float64 views of the stored operands, q [B, sq, C], k / v [B, skv, C] -> (o [B, sq, C], w [B, H, sq, skv], s (natural log,
    -inf where masked), lse2 [B, H, sq] = log2 sum_k exp(s_k))."""
    q4, k4, v4 = (split_heads(t.double(), heads) for t in (q, k, v))
    s = (q4 @ k4.transpose(-1, -2)) * scale
    if causal:
        sq, skv = s.shape[-2:]
        i = torch.arange(sq, device=s.device)[:, None]
        j = torch.arange(skv, device=s.device)[None, :]
        s = s.masked_fill(j > i, -math.inf)
    lse = torch.logsumexp(s, -1)
    w = torch.exp(s - lse[..., None])
    return merge_heads(w @ v4), w, s, lse * LOG2E


def bound(q, k, v, heads, scale, ref, flavour):
    """(B [B, sq, C], B_lse [B, H, sq]) for the reference tuple `ref` of the same operands."""
    o, w, s, lse2 = ref
    d = q.shape[-1] // heads
    u_p, u_s, u_o, a_p, a_o = units(flavour, d)
    q4, k4, v4 = (split_heads(t.double(), heads) for t in (q, k, v))
    sa = torch.where(torch.isinf(s), torch.zeros_like(s), s.abs())
    eps = u_p + u_s * scale * (q4.abs() @ k4.abs().transpose(-1, -2)) + 2.0 ** -22 * (sa + sa.amax(-1, keepdim=True)) + 2.0 ** -21
    wmax = 1.0 if flavour == "f16x3_unfused" else w.amax(-1, keepdim=True)
    we = w * eps + a_p * wmax * (~torch.isinf(s))
    o4 = split_heads(o, heads).abs()
    b = u_o * o4 + a_o + we @ v4.abs() + o4 * we.sum(-1, keepdim=True)
    return merge_heads(b), we.sum(-1) / math.log(2.0) + 2.0 ** -22 * (lse2.abs() + 1.0)


# ---- storage rounding ----------------------------------------------------------------------------------------------------------

def split_f16(x):
    """fp32 -> (hi, lo) fp16 planes as mf_split_halves makes them: hi = x toward zero, lo = (x - hi) toward zero."""
    def rtz(t):
        h = t.to(torch.float16)
        over = h.float().abs() > t.abs()
        return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)      # one step toward zero: the magnitude bits - 1
    x = x.float()
    hi = rtz(x)
    return hi, rtz(x - hi.float())


def stored(x, rnd):
    """float64 value the kernel sees for x kept as `rnd`: 'bf16' / 'fp16' storage, 'f32' (fp32 kept whole: the fp32 mode) or
    'f16x3' (fp32 storage, read by the kernel as two fp16 planes)."""
    if rnd == "bf16":
        return x.float().to(torch.bfloat16).double()
    if rnd == "fp16":
        return x.float().to(torch.float16).double()
    if rnd == "f32":
        return x.float().double()
    if rnd == "f16x3":
        hi, lo = split_f16(x.float())
        return hi.double() + lo.double()
    raise ValueError(rnd)


# ---- input families ------------------------------------------------------------------------------------------------------------

def _aim(k4, hot, amp, noise):
    """q = 0.3 noise + sum_n c_n k[hot_n], c_n chosen so that key hot_n alone scores amp_n * HOT at scale = d^-1/2.
    k4 [B, H, skv, d]; hot (long) and amp [B, H, sq, n]."""
    b, h, _, d = k4.shape
    kh = k4[torch.arange(b)[:, None, None, None], torch.arange(h)[None, :, None, None], hot]          # [B, H, sq, n, d]
    coef = amp * HOT * math.sqrt(d) / (kh * kh).sum(-1)
    return 0.3 * noise + (coef[..., None] * kh).sum(-2)


def make_inputs(family, B, heads, sq, skv, d, seed, rnd):
    """(q [B, sq, C], k, v [B, skv, C]) in float64, already rounded to storage (`rnd`: see stored()); scale = d^-1/2 is assumed."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    k4, v4, noise = rn(B, heads, skv, d), rn(B, heads, skv, d), rn(B, heads, sq, d)
    nt = (skv + TILE - 1) // TILE
    last0 = (nt - 1) * TILE                                   # first key of the last (possibly partial) tile
    i = torch.arange(sq)
    if family == "dense":
        q4 = noise
    elif family == "peaked":
        # three hot keys per query, drawn per query (lanes of one wave peak in different tiles); every eighth query's first hot key
        # is pinned to a tile edge
        hot = torch.randint(0, skv, (B, heads, sq, 3), generator=g)
        pins = [p for p in (0, 63, 64, skv - 1, last0) if p < skv]
        for n, p in enumerate(pins):
            hot[:, :, n::8, 0] = p
        amp = 2.0 + 0.2 * torch.rand(B, heads, sq, 3, generator=g, dtype=torch.float64)
        q4 = _aim(k4, hot, amp, noise)
    elif family in ("stairs_up", "stairs_down"):
        # one hot key per tile, amplitude 0.3 .. 2.0 with the tile index; even and odd queries climb in opposite directions
        # (the other keys are kept small, so that each tile's maximum is its hot key's score and not the noise of 63 others)
        t = torch.arange(nt)
        hot = t * TILE + (17 * t + 5) % torch.clamp(skv - t * TILE, max=TILE)
        k4 = 0.4 * k4
        k4[:, :, hot] = torch.sign(k4[:, :, hot])       # hot keys: +-1 in every channel, so that no single product carries the score
        up = 0.3 + 1.7 * (t.double() / max(nt - 1, 1)) if nt > 1 else torch.tensor([2.0], dtype=torch.float64)
        rising = (i % 2 == 0) if family == "stairs_up" else (i % 2 == 1)
        amp = torch.where(rising[:, None], up[None, :], up.flip(0)[None, :])                            # [sq, nt]
        q4 = _aim(k4, hot.expand(B, heads, sq, nt), amp.expand(B, heads, sq, nt), noise)
    elif family in ("late_spike", "early_spike"):
        hot = torch.where(i % 2 == 0, skv - 1, last0) if family == "late_spike" else torch.zeros(sq, dtype=torch.long)
        k4 = 0.4 * k4
        k4[:, :, hot.unique()] = torch.sign(k4[:, :, hot.unique()])
        q4 = _aim(k4, hot[:, None].expand(B, heads, sq, 1), torch.full((B, heads, sq, 1), 2.0, dtype=torch.float64), noise)
    elif family == "all_negative":
        # every key = mu + small noise, every query = -gamma mu: all scores sit near -20
        mu = torch.where(rn(B, heads, 1, d) >= 0, 1.0, -1.0).double()
        k4 = mu + 0.1 * k4
        q4 = -(20.0 / math.sqrt(d)) * mu + 0.1 * noise / math.sqrt(d)
        q4 = q4.expand(B, heads, sq, d)
    elif family == "flat":
        q4 = torch.zeros(B, heads, sq, d, dtype=torch.float64)
    elif family == "forbidden":
        # causal only: the hottest key of query i is i + 1 (masked), the second hottest is i itself: the answer is v_i
        assert sq == skv
        nxt = torch.clamp(i + 1, max=skv - 1)
        hot = torch.stack([nxt, i], -1)
        amp = torch.tensor([3.0, 2.0], dtype=torch.float64).expand(sq, 2).clone()
        amp[sq - 1, 0] = 0.0                                  # the last query has no next key
        q4 = _aim(k4, hot.expand(B, heads, sq, 2), amp.expand(B, heads, sq, 2), noise / 3.0)
    else:
        raise ValueError(family)
    return tuple(stored(merge_heads(t.contiguous()), rnd) for t in (q4, k4, v4))


# ---- arithmetic model ----------------------------------------------------------------------------------------------------------

def _f32(x):
    return x.float().double()


def _r16(x, flavour):
    return x.float().to(torch.bfloat16 if flavour == "bf16" else torch.float16).double()


def _rz22(x):
    """P as two fp16 pieces, each toward zero: 22 bits, truncated."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.trunc(m * 2.0 ** 22) / 2.0 ** 22, e)


def emulate(q, k, v, heads, scale, causal, flavour, fault=None):
    """The kernel's arithmetic in float64 with its rounding points, as a specification: Q~ rounding on the MJ head dims, 64-key
    tiles, the deferred maximum (MJ) or the running maximum, both with wave-uniform (32 queries) rescales, P rounded to the operand
    type of the second product, l from the rounded P where V^T has a ones row (head dim not a multiple of 32) and from the unrounded
    P elsewhere, tail and causal masks, the rounding of the stored output.  Returns (o [B, sq, C], lse2 [B, H, sq]).
    `fault`: one of FAULTS, the arithmetic of a kernel with that mistake."""
    assert fault is None or fault in FAULTS
    B, sq, C = q.shape
    skv, d = k.shape[1], C // heads
    sixteen = flavour in ("bf16", "fp16")
    mj = sixteen and d in MJ_DIMS
    ones = d % 32 != 0
    c = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    q4, k4, v4 = (split_heads(t.double(), heads) for t in (q, k, v))
    sqp, nt = -(-sq // WAVE) * WAVE, -(-skv // TILE)
    pad = lambda t, n: torch.cat([t, t.new_zeros(B, heads, n - t.shape[2], d)], 2)
    q4, k4, v4 = pad(q4, sqp), pad(k4, nt * TILE), pad(v4, nt * TILE)
    qi = torch.arange(sqp)
    qt = _r16(_f32(q4 * c), flavour) if mj else q4
    m = torch.zeros(B, heads, sqp, dtype=torch.float64) if mj else torch.full((B, heads, sqp), -math.inf, dtype=torch.float64)
    m_sub = m.clone()                                    # MJ: the offset held in the Q~ slots, the one the matrix pipe subtracts
    l = torch.zeros(B, heads, sqp, dtype=torch.float64)
    o = torch.zeros(B, heads, sqp, d, dtype=torch.float64)
    any_wave = lambda x: x.view(B, heads, sqp // WAVE, WAVE).any(-1, keepdim=True).expand(-1, -1, -1, WAVE).reshape(B, heads, sqp)
    for t in range(nt):
        if fault == "drop_tile" and t == 1:
            continue
        key = t * TILE + torch.arange(TILE)
        kt, vt = k4[:, :, key], v4[:, :, key]
        dead = (key >= skv)[None, :].expand(sqp, TILE)
        if fault == "tail_unmasked":
            dead = torch.zeros_like(dead)
        if causal:
            dead = dead | (key[None, :] > qi[:, None] + (1 if fault == "causal_off_by_one" else 0))
        s = qt @ kt.transpose(-1, -2)
        if mj:
            st = _f32(s - m_sub[..., None]).masked_fill(dead, -math.inf)
            mx = st.amax(-1)
            fire = torch.ones_like(mx, dtype=torch.bool) if t == 0 else any_wave(mx > MJ_T)
            want = _f32(m + (mx if t == 0 else mx.clamp_min(0.0)))      # three 16-bit pieces hold every fp32 value of this size
            m_new = torch.where(fire, want, m)
            dlt = m_new - m
            if not (fault == "offset_not_updated" and t > 0):
                st = _f32(st - dlt[..., None])
                m_sub = m_new
            alpha = torch.exp2(-dlt) if t > 0 else torch.ones_like(dlt)
            p = torch.exp2(st)
        else:
            s = _f32(s).masked_fill(dead, -math.inf)
            m_new = torch.maximum(m, _f32(s.amax(-1) * c))
            alpha = torch.exp2(m - m_new)
            m_use = m if (fault == "offset_not_updated" and t > 0) else m_new
            p = torch.exp2(_f32(s * c - m_use[..., None]))
        m = m_new
        if fault != "no_l_rescale":
            l = l * alpha
        if fault != "no_o_rescale":
            o = o * alpha[..., None]
        p = _f32(torch.where(dead, torch.zeros_like(p), p))
        pr = _r16(p, flavour) if sixteen else _rz22(p)
        l = _f32(l + (pr if ones else p).sum(-1))
        o = _f32(o + pr @ vt)
    out = _f32(o / l[..., None])
    if sixteen:
        out = _r16(out, flavour)
    return merge_heads(out[:, :, :sq]), (m + torch.log2(l))[:, :, :sq]
