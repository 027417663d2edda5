"""Plain-torch reference of the fp8 (OCP e4m3fn) quantiser, csrc/fp8.hip: no project kernel, runs on the CPU.

e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; normals from 2^-6, subnormals k * 2^-9 (k = 1 ... 7), largest value 448
(0x7E), no infinities, NaN = 0x7F / 0xFF.

`quantize_contract` repeats the kernel's fp32 arithmetic step by step; `quantize_exact` is the same definition in float64.
tests/test_fp8_reference_cpu.py shows the two agree on every code of the GPU test's random inputs, so the contract is no licence
for a sloppy kernel; the GPU test (tests/test_fp8_audit_gpu.py) holds the kernel's bytes to the contract."""
import torch

E4M3_MAX = 448.0
NAN_CODE = 0x7F
INV448 = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(448.0, dtype=torch.float32)          # fl32(1 / 448)
UP_BELOW, UP = 2.0 ** -64, 2.0 ** 64          # rows with amax < 2^-64 are multiplied by 2^64 first (exact): 1 / sc stays finite


def e4m3_spacing(y: torch.Tensor) -> torch.Tensor:
    """The distance between neighbouring e4m3 values at |y| (float64): 2^(e - 3) for |y| in [2^e, 2^(e + 1)), e clamped to
    [-6, 8] (2^-9 through the subnormals, 32 in the top binade and beyond it, where the quantiser saturates)."""
    a = y.double().abs().clamp(min=2.0 ** -6)
    _, e = torch.frexp(a)
    e = torch.clamp(e.to(torch.int64) - 1, min=-6, max=8)
    return torch.ldexp(torch.ones_like(a), (e - 3).to(torch.float64))


def e4m3_round(y: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest e4m3fn value, ties to the even code, saturating at +-448; NaN stays NaN, the sign of zero stays."""
    y = y.double()
    a = y.abs().clamp(max=E4M3_MAX)
    sp = e4m3_spacing(a)
    r = torch.round(a / sp) * sp                # torch.round: half to even; a / sp is exact (sp a power of two)
    r = r.clamp(max=E4M3_MAX)
    return torch.where(torch.isnan(y), y, torch.copysign(r, y))


def codes(v: torch.Tensor) -> torch.Tensor:
    """The e4m3fn bytes of values that e4m3_round returned (they are representable, so the cast is exact)."""
    return v.float().to(torch.float8_e4m3fn).view(torch.uint8)


def decode(c: torch.Tensor) -> torch.Tensor:
    """uint8 codes -> float64."""
    return c.view(torch.float8_e4m3fn).float().double()


def near_tie(y: torch.Tensor, rel: float = 2.0 ** -20) -> torch.Tensor:
    """True where float64 y (already divided by the scale) lies within rel * |y| of the midpoint between two e4m3 codes."""
    a = y.double().abs().clamp(max=E4M3_MAX)
    sp = e4m3_spacing(a)
    lo = torch.floor(a / sp) * sp
    return (a - (lo + 0.5 * sp)).abs() <= rel * a


def one_step(qa: torch.Tensor, qb: torch.Tensor) -> torch.Tensor:
    """True where two code bytes have the same sign and neighbouring magnitudes."""
    return ((qa ^ qb) & 0x80 == 0) & (((qa & 0x7F).to(torch.int16) - (qb & 0x7F).to(torch.int16)).abs() == 1)


def _finish(x, amax, sc, inv, up, one):
    """The shared tail of the two precisions: y, clamp, RNE; non-finite rows: scale NaN, every code NaN."""
    y = (x * up[:, None]) * inv[:, None]
    y = y.clamp(-E4M3_MAX, E4M3_MAX)
    bad = ~torch.isfinite(amax)
    q = codes(e4m3_round(y.double()))
    q = torch.where(bad[:, None], torch.full_like(q, NAN_CODE), q)
    sc = torch.where(bad, torch.full_like(sc, float("nan")), sc)
    return q, sc, y


def _amax(x):
    """Row maximum of |x| that keeps a NaN and an Inf (torch.amax propagates NaN)."""
    return x.abs().amax(1)


def quantize_contract(x: torch.Tensor):
    """(codes uint8 [rows, C], scale fp32 [rows]) by the arithmetic csrc/fp8.hip defines, step by step in torch float32:
    amax = max |x|; up = 2^64 where amax < 2^-64, else 1; scu = (amax * up) * fl(1 / 448); sc = scu / up (1 for an all-zero row);
    inv = 1 / scu; q = RNE_e4m3(clamp((x * up) * inv, -448, 448)).  A row with a NaN or an Inf: sc = NaN, every code 0x7F."""
    x = x.float()
    amax = _amax(x)
    one = torch.ones_like(amax)
    up = torch.where(amax < UP_BELOW, one * UP, one)
    scu = (amax * up) * INV448
    live = amax > 0
    sc = torch.where(live, scu * (1.0 / up), one)
    inv = 1.0 / torch.where(live, scu, one)
    q, sc, _ = _finish(x, amax, sc, inv, up, one)
    return q, sc


def quantize_exact(x: torch.Tensor):
    """The same definition in float64: sc = amax / 448 (1 for an all-zero row), q = RNE_e4m3(clamp(x / sc)).  Returns
    (codes uint8, scale float64, y float64 = x / sc before the rounding)."""
    x = x.double()
    amax = _amax(x)
    one = torch.ones_like(amax)
    live = amax > 0
    sc = torch.where(live, amax / E4M3_MAX, one)
    q, sc, y = _finish(x, amax, sc, 1.0 / sc, one, one)
    return q, sc, y


def ln_quantize(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    """float64 LayerNorm of the stored x, then quantize_exact.  Returns (y64 [rows, C] the LayerNorm output, codes, scale float64,
    delta [rows, C]): delta = 2^-20 (|y - beta| (1 + |mean| / std) + |beta|) is what an fp32 two-pass LayerNorm may move an
    element by — it errs by about 2^-24 |x| per element, which the cancellation x - mean magnifies by |mean| / std; the factor
    16 covers the lane-tree sums up to C = 8192."""
    x = x.double()
    g, b = gamma.double(), beta.double()
    mean = x.mean(1, keepdim=True)
    var = x.var(1, unbiased=False, keepdim=True)
    std = torch.sqrt(var + eps)
    y = (x - mean) / std * g + b
    delta = 2.0 ** -20 * ((y - b).abs() * (1.0 + mean.abs() / std) + b.abs())
    q, sc, _ = quantize_exact(y)
    return y, q, sc, delta


# ---- inputs shared by the CPU and the GPU tests -----------------------------------------------------------------------------------
GAUSS_SHAPES = ((300, 320), (64, 1280), (7, 8192), (130, 5120))


def gauss(rows: int, c: int, seed: int = 71) -> torch.Tensor:
    """Gaussian rows, each with a scale of its own in (0, 4)."""
    g = torch.Generator().manual_seed(seed * 100003 + rows * 8209 + c)
    return torch.randn(rows, c, generator=g) * (torch.rand(rows, 1, generator=g) * 4.0 + 2.0 ** -6)


def tie_values() -> torch.Tensor:
    """Every e4m3 tie (k + 0.5 spacings) of every binade below 448, the subnormal ones included, with alternating signs: all
    representable in bf16 (5 significant bits)."""
    v = [(k + 0.5) * 2.0 ** -9 for k in range(7)]                                       # 0.5, 1.5, ... 6.5 x 2^-9
    for e in range(-6, 9):
        v += [(8 + k + 0.5) * 2.0 ** (e - 3) for k in range(8) if (8 + k + 0.5) * 2.0 ** (e - 3) < E4M3_MAX]
    t = torch.tensor(v, dtype=torch.float64)
    return t * torch.tensor([1.0, -1.0]).repeat(len(v))[: len(v)]


SPECIAL = ("ties", "subnormal_targets", "neg_zero", "zero", "amax_min_normal", "amax_3e38", "2^-20", "2^-10", "2^0", "2^10", "2^20",
           "ties_shifted")


def special_rows(c: int, seed: int = 72) -> torch.Tensor:
    """[len(SPECIAL), c] fp32, every value exact in bf16 where the row's point needs it (ties, subnormal targets, 2^-126)."""
    g = torch.Generator().manual_seed(seed * 7919 + c)
    rows = []
    ties = tie_values().float()
    for name in SPECIAL:
        r = torch.randn(c, generator=g)
        if name in ("ties", "ties_shifted"):           # amax forced to 448: scale 1, the row holds k + 0.5 spacings of every binade
            sh = 0 if name == "ties" else len(ties) // 2
            r = ties.roll(sh).repeat(c // len(ties) + 1)[:c].clone()
            r[c - 1 if name == "ties" else 0] = E4M3_MAX
        elif name == "subnormal_targets":
            r = (torch.tensor([0.5, -1.5, 2.5, -0.5, 1.5, -2.5, 3.5]) * 2.0 ** -9).repeat(c // 7 + 1)[:c].clone()
            r[c // 2] = -E4M3_MAX
        elif name == "neg_zero":
            r[::2] = -0.0
        elif name == "zero":
            r = torch.zeros(c)
        elif name == "amax_min_normal":                 # amax = 2^-126, the smallest normal fp32; the rest denormal or zero
            r = (torch.tensor([1.0, -0.5, 0.25, 0.0, -0.75, -1.0, 0.5, -0.0]) * 2.0 ** -126).repeat(c // 8 + 1)[:c].clone()
        elif name == "amax_3e38":
            r = r / r.abs().max() * 3e38
        else:
            r = r * 2.0 ** int(name[2:])
        rows.append(r.float())
    return torch.stack(rows)
