"""Inputs whose mean dwarfs their spread, float64 references and the bound for the normalisation kernels (no GPU needed).

Every other normalisation test draws randn * s + m with |m| <= s / 2, where var = E[x^2] - mean^2 from fp32 sums is harmless.  The
ladder below walks the ratio |mean| / std up to 6000, in the storage dtype the kernel reads, with a seed and a sign of its own for
every (image, group), so that a kernel which mixes groups or images cannot pass by symmetry.

The yardstick is torch's own fp32 result on the CPU for the same stored values (torch.native_group_norm, F.layer_norm, fp32
autograd), measured against float64 in the metric the kernel is measured in.  bound(): an element passes inside the tolerance the
suite already holds that kernel and output dtype to, or inside FACTOR x the yardstick's own maximum error.  FACTOR = 4: two fp32
evaluations that sum in different orders, compared on an L-inf statistic, scatter up to about 2 x (ENV_K_LINF_SMALL in tests/util.py
is 1.75 for the same reason); the defect this guards against, unshifted fp32 (sum, sum of squares), costs 7 x to 1100 x."""
import functools

import torch
import torch.nn.functional as F

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
EPS = 1e-5
FACTOR = 4.0

# name -> (|mean|, std); the three special rungs are built by hand below
RUNGS = {"base": (0.7, 2.0), "m10": (10.0, 1.0), "m30": (30.0, 1.0), "m100": (100.0, 1.0), "m100_tight": (100.0, 0.1),
         "m300_tight": (300.0, 0.05), "chan_offset": (0.0, 1.0), "outlier": (20.0, 1.0), "constant": (77.7, 0.0)}
LADDER = tuple(RUNGS)
MIN_DISTINCT = 8


def ladder(dtype):
    """The rungs that exist in `dtype`: -300 / 0.05 needs fp32's spacing, and the 1e4 outlier is kept out of fp16."""
    skip = {F32: (), BF16: ("m300_tight",), F16: ("m300_tight", "outlier")}[dtype]
    return tuple(n for n in LADDER if n not in skip)


def spacing(dtype, v):
    """The distance between neighbouring `dtype` values at magnitude v."""
    if v == 0.0:
        return 0.0
    e = torch.frexp(torch.tensor(float(abs(v)), dtype=torch.float64))[1].item() - 1          # |v| in [2^e, 2^(e + 1))
    return 2.0 ** (e - {F32: 23, BF16: 7, F16: 10}[dtype])


def spread(name, dtype):
    """The rung's std in `dtype`: 16-bit storage cannot hold std 0.1 at offset 100, so the spread is at least 3 x the spacing at
    the offset (+-1.5 sigma then covers 9 neighbouring values)."""
    mean, std = RUNGS[name]
    return std if dtype == F32 or std == 0.0 else max(std, 3.0 * spacing(dtype, mean))


def _unit(name, rows, cols, dtype, gen):
    """One normalisation unit ([rows, cols] fp32 values, not yet rounded) of rung `name`, signs and positions drawn from `gen`."""
    mean, _ = RUNGS[name]
    sign = 1.0 if torch.rand((), generator=gen).item() < 0.5 else -1.0
    if name == "constant":
        return torch.full((rows, cols), 77.7)
    x = torch.randn(rows, cols, generator=gen) * spread(name, dtype) + sign * mean
    if name == "chan_offset":
        x[:, int(torch.randint(cols, (), generator=gen))] += sign * 50.0
    if name == "outlier":
        x[int(torch.randint(rows, (), generator=gen)), int(torch.randint(cols, (), generator=gen))] = sign * 1e4
    return x


def distinct_values(x, groups):
    """[B, groups]: the number of distinct stored values of every (image, group) of x [B, HW, C]."""
    b, hw, c = x.shape
    xg = x.float().view(b, hw, groups, c // groups).permute(0, 2, 1, 3).reshape(b, groups, -1)
    return torch.tensor([[xg[i, g].unique().numel() for g in range(groups)] for i in range(b)])


@functools.lru_cache(maxsize=48)
def gn_input(names, b, hw, c, groups, dtype, seed):
    """[B, HW, C] in `dtype` for `groups` groups.  `names`: one rung for every image, or a tuple with a rung per image.  Every
    (image, group) has a generator of its own.  Asserts the ladder's condition: except for `constant`, at least MIN_DISTINCT
    distinct stored values in every group.  The result is shared (cached): do not write to it."""
    names = (names,) * b if isinstance(names, str) else tuple(names)
    assert len(names) == b and c % groups == 0
    cpg = c // groups
    x = torch.empty(b, hw, groups, cpg)
    for i in range(b):
        for g in range(groups):
            gen = torch.Generator().manual_seed((seed * 1000003 + i) * 4099 + g)
            x[i, :, g, :] = _unit(names[i], hw, cpg, dtype, gen)
    x = x.view(b, hw, c).to(dtype)
    nd = distinct_values(x, groups)
    for i, n in enumerate(names):
        if n != "constant":
            assert int(nd[i].min()) >= MIN_DISTINCT, f"{n} in {dtype}: a group holds only {int(nd[i].min())} distinct values"
    return x


@functools.lru_cache(maxsize=48)
def ln_input(name, rows, c, dtype, seed):
    """[rows, C] in `dtype`: every row is a unit of rung `name` with its own sign; `chan_offset` offsets one column of all rows."""
    gen = torch.Generator().manual_seed(seed * 7919 + rows * 31 + c)
    mean, _ = RUNGS[name]
    if name == "constant":
        return torch.full((rows, c), 77.7).to(dtype)
    sign = (torch.rand(rows, 1, generator=gen) < 0.5).float() * 2.0 - 1.0
    x = torch.randn(rows, c, generator=gen) * spread(name, dtype) + sign * mean
    if name == "chan_offset":
        x[:, int(torch.randint(c, (), generator=gen))] += 50.0 * sign[:, 0]
    if name == "outlier":
        x[torch.arange(rows), torch.randint(c, (rows,), generator=gen)] = 1e4 * sign[:, 0]
    x = x.to(dtype)
    if c >= 32:
        assert min(r.unique().numel() for r in x.float()[:: max(1, rows // 16)]) >= MIN_DISTINCT, name
    return x


def params(c, seed):
    gen = torch.Generator().manual_seed(seed + 977)
    return torch.randn(c, generator=gen), torch.randn(c, generator=gen)


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------
def _gn(x, gamma, beta, groups, silu, dt):
    """x [B, HW, C] as stored -> (y [B, HW, C], mean [B, G], rstd [B, G]) evaluated in `dt` by torch on the CPU."""
    b, hw, c = x.shape
    xc = x.to(dt).permute(0, 2, 1).contiguous()
    if dt == torch.float64:
        xg = xc.reshape(b, groups, -1)
        mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + EPS)
        y = ((xg - mean[..., None]) * rstd[..., None]).view(b, c, hw) * gamma.to(dt)[None, :, None] + beta.to(dt)[None, :, None]
    else:
        y, mean, rstd = torch.native_group_norm(xc, gamma.to(dt), beta.to(dt), b, c, hw, groups, EPS)
    y = y.permute(0, 2, 1)
    return (F.silu(y) if silu else y), mean, rstd


@functools.lru_cache(maxsize=32)
def gn_case(names, b, hw, c, groups, dtype, seed, silu):
    """(x, gamma, beta, float64 (y, mean, rstd), torch fp32 (y, mean, rstd)) of one ladder input; shared (cached), do not write to it."""
    x = gn_input(names, b, hw, c, groups, dtype, seed)
    gamma, beta = params(c, seed)
    return x, gamma, beta, _gn(x, gamma, beta, groups, silu, torch.float64), _gn(x, gamma, beta, groups, silu, F32)


def gn_from_sums(x, sums, n, gamma, beta, groups, silu):
    """float64 GroupNorm of x with the statistics taken from handed-over fp32 (sum, sum of squares) per (image, group) [B, G, 2] over
    n elements each: the contract of the producer-fed routes."""
    b, hw, c = x.shape
    s, q = sums[..., 0].double(), sums[..., 1].double()
    mean = s / n
    m2 = (q - s * mean).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(m2 / n + EPS)
    xg = x.double().view(b, hw, groups, -1)
    y = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).view(b, hw, c) * gamma.double() + beta.double()
    return F.silu(y) if silu else y


def gn_grads(x, gy, gamma, beta, groups, silu, dt):
    """(dx [B, HW, C], dgamma, dbeta) by autograd in `dt` on the CPU."""
    xx = x.to(dt).permute(0, 2, 1).contiguous().requires_grad_(True)
    ga, be = gamma.to(dt).requires_grad_(True), beta.to(dt).requires_grad_(True)
    y = F.group_norm(xx, groups, ga, be, EPS)
    y = F.silu(y) if silu else y
    y.backward(gy.to(dt).permute(0, 2, 1).contiguous())
    return xx.grad.permute(0, 2, 1), ga.grad, be.grad


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------
def ln(x, gamma, beta, dt):
    return F.layer_norm(x.to(dt), (x.shape[-1],), gamma.to(dt), beta.to(dt), EPS)


def ln_grads(x, gy, gamma, beta, dt):
    xx = x.to(dt).requires_grad_(True)
    ga, be = gamma.to(dt).requires_grad_(True), beta.to(dt).requires_grad_(True)
    F.layer_norm(xx, (x.shape[-1],), ga, be, EPS).backward(gy.to(dt))
    return xx.grad, ga.grad, be.grad


def softmax_ref(s, cols):
    return torch.softmax(s[..., :cols].double(), -1)


# ---- the bound ---------------------------------------------------------------------------------------------------------------
def rel(got, ref):
    """The scalar metric of tests/test_training_gpu.py: L-inf error over L-inf of the reference."""
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


def bound(existing_atol, existing_rtol, yardstick_err, ref=None, factor=FACTOR):
    """The error an output may show.  With `ref` (elementwise metric): max(existing_atol + existing_rtol * |ref|, factor x the
    yardstick's maximum error), a tensor shaped like ref.  Without (a scalar metric such as rel()): max(existing_atol, factor x
    the yardstick's value).  existing_* are the tolerances the suite already holds the kernel to; a yardstick of 0 leaves them alone."""
    if ref is None:
        return max(float(existing_atol), factor * float(yardstick_err))
    return torch.clamp(existing_atol + existing_rtol * ref.abs().double(), min=factor * float(yardstick_err))


def max_err(got, ref):
    return float((got.double().cpu() - ref.double()).abs().max())


def judge(name, got, ref, yard, atol, rtol, factor=FACTOR, fail=True):
    """Elementwise check of `got` against float64 `ref` under bound(); `yard` is the yardstick's output (or None for a yardstick of
    0).  Prints the kernel's and the yardstick's maximum error and their RATIO; returns (passed, kernel error, yardstick error)."""
    err = (got.double().cpu() - ref.double()).abs()
    ye = max_err(yard, ref) if yard is not None else 0.0
    nan = int(torch.isnan(err).sum())
    bad = int((err > bound(atol, rtol, ye, ref, factor)).sum()) + nan
    e = float(err.max())
    print(f"{name}: hip {e:.3e} yardstick {ye:.3e} RATIO hip/yardstick {e / ye if ye > 0 else float('inf'):.2f} "
          f"|ref|max {float(ref.abs().max()):.3e} bad={bad}/{ref.numel()}")
    if fail:
        assert bad == 0, f"{name}: {bad} elements outside the bound, max err {e:.3e} (yardstick {ye:.3e})"
    return bad == 0, e, ye


def judge_rel(name, got, ref, yard, floor, factor=FACTOR, fail=True):
    """The same for the scalar metric rel()."""
    e, ye = rel(got, ref), rel(yard, ref) if yard is not None else 0.0
    ok = e == e and e <= bound(floor, 0.0, ye, None, factor)
    print(f"{name}: hip {e:.3e} yardstick {ye:.3e} RATIO hip/yardstick {e / ye if ye > 0 else float('inf'):.2f}")
    if fail:
        assert ok, f"{name}: rel error {e:.3e} > max({floor:.1e}, {factor} x {ye:.3e})"
    return ok, e, ye


# ---- the scheme under suspicion, emulated in torch -------------------------------------------------------------------------------
def emulate_sums_groupnorm(x, groups, per=16, shift=False):
    """GroupNorm statistics as `per` rows per thread of fp32 sequential (sum, sum of squares), combined in double: the scheme of the
    own-statistics kernels.  shift: one pivot per (image, group), the value at row 0 / first channel of the group, subtracted before
    accumulating.  x [B, HW, C] fp32 with HW % per == 0 -> (y [B, HW, C] fp32 without affine, mean, rstd)."""
    b, hw, c = x.shape
    cpg = c // groups
    x = x.float()
    piv = x[:, 0].view(b, groups, cpg)[:, :, :1].expand(b, groups, cpg).reshape(b, 1, c) if shift else torch.zeros(b, 1, c)
    xv = x.view(b, hw // per, per, c)
    s = torch.zeros(b, hw // per, c)
    ss = torch.zeros(b, hw // per, c)
    for r in range(per):
        v = xv[:, :, r] - piv
        s = s + v
        ss = ss + v * v
    S = s.double().sum(1).view(b, groups, cpg).sum(-1)
    Q = ss.double().sum(1).view(b, groups, cpg).sum(-1)
    n = hw * cpg
    md = S / n
    m2 = (Q - S * md).clamp(min=0.0)
    mean = (md + piv.view(b, groups, cpg)[:, :, 0].double()).float()
    rstd = (1.0 / torch.sqrt(m2 / n + EPS)).float()
    y = (x.view(b, hw, groups, cpg) - mean[:, None, :, None]) * rstd[:, None, :, None]
    return y.view(b, hw, c), mean, rstd
