"""The normalisation kernels on inputs whose mean dwarfs their spread (tests/norm_conditioning_ref.py: the ladder, the float64
references, torch's fp32 result as the yardstick, and bound()).

Every other normalisation test draws its input within half a standard deviation of zero, where var = E[x^2] - mean^2 from fp32 sums
is harmless.  Here the ratio |mean| / std climbs to 6000.  An element passes inside the tolerance the suite already holds that kernel
and output dtype to (taken from test_groupnorm_streaming_gpu.py, test_ops_gpu.py, test_fp16_gpu.py and test_training_gpu.py), or
inside 4 x the error torch's own fp32 evaluation shows on the same stored values.  Every case prints `RATIO hip/yardstick`.

Findings recorded here (one MI355X; every figure is in profiles/gn_conditioning_ratios.txt):
  * the own-statistics GroupNorm passes (gn_stats_kernel, gn_slab_kernel, the deferred split-K prologue included) and phase 0 of the
    streaming GroupNorm backward summed raw x and x^2 in fp32: with an fp32 output they left the bound at m100 (slab 9 x torch's fp32
    error), m100_tight (25 x ... 111 x) and m300_tight (66 x ... 551 x, errors of 0.07 ... 1.8), the backward's dx at 118 x / 165 x.
    They now sum x - pivot (csrc/norm.hip, csrc/train.hip): every route and rung is at most 1.3 x torch (at most 1.0 x from m10 to m300_tight), dx at most 1.0 x.
  * layernorm_kernel / layernorm8_kernel took the mean from an fp32 sum of raw values: a constant row came out 8.7e-3 from beta (torch:
    exactly beta).  The mean is now pivot + sum(x - pivot) / C.
  * gn_slab_kernel's sum of squares is an explicit fma chain: left to the compiler, the deferred split-K instantiation contracted it
    differently from the plain one and the two no longer agreed bit for bit on these inputs.
  * the producer-fed routes take fp32 (sum, sum of squares): test_groupnorm_from_handed_over_sums holds the kernel to its contract
    (statistics from these sums) and prints how far the whole route is from the true float64 result at every rung.  With the fp32 affine
    y = x * a + (beta - mean * a) the fp32 output missed the contract at m100_tight, m300_tight and constant (2.2e-4, 2.0e-2, 3.8e-3
    against atol 1e-4: the shift rounds a term of size |mean| * rstd * |gamma|); gn_apply_kernel now forms an fp32 output as
    ((x - mean_hi) - mean_lo) * a + beta with the mean carried as two floats, and every rung is within 2.3e-5 of the contract.
  * the folded LayerNorm passes base, m10 and m30 on every tile; at mean / std = 100 (measured only) bf16 stays inside its tolerance
    and fp16 leaves it in the GEGLU case alone: tile 69 max error 4.7e-2 (164 of 5242880 elements out), tile 70 8.7e-2 (753 out)."""
import math

import pytest
import torch
import torch.nn.functional as F

import norm_conditioning_ref as R
from norm_conditioning_ref import BF16, F16, F32

pytestmark = pytest.mark.gpu

from reflecting_reality_amd import hip, ops  # noqa: E402

DEV = "cuda"
B = 3
PAIRS = [(F32, F32), (F32, BF16), (F32, F16), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16)]     # every pair mf_groupnorm accepts
SAME = [(F32, F32), (BF16, BF16), (F16, F16)]
# (atol, rtol) the suite already uses, by output dtype
GN_TOL = {F32: (1e-4, 2e-5), BF16: (1e-1, 2e-2), F16: (4e-3, 4e-3)}        # test_groupnorm_streaming_gpu.py: check()
LN_TOL = {F32: (5e-5, 1e-5), BF16: (1e-1, 2e-2), F16: (4e-3, 2e-3)}        # test_ops_gpu.py::test_layernorm, test_fp16_gpu.py
REL_FLOOR = 2e-5                                                            # test_training_gpu.py: every backward kernel

# route -> [(c0, c1, hw, groups)]: the first shape runs every dtype pair
ROUTES = {
    "slab": [(320, 0, 64, 32), (1280, 1280, 200, 32)],                      # one launch
    "fused": [(640, 0, 1024, 32), (640, 320, 33 * 31, 32)],                 # own statistics, every apply block finalizes
    "separate": [(320, 0, 1100, 32)],                                       # own statistics, a finalize launch (hw > 1024)
    "vec4": [(36, 0, 300, 4)],                                              # 4-channel vectors
}
ROUTE_SHAPES = [(r, i) for r, shapes in ROUTES.items() for i in range(len(shapes))]


# what the library's plan of a call says on each route (hip.GnPlan)
PLAN_OF_ROUTE = {
    "slab": dict(form=0, launches=1, vec=8),
    "fused": dict(form=1, finalize=1, launches=2, vec=8),
    "separate": dict(form=1, finalize=0, launches=3, vec=8),
    "vec4": dict(form=1, vec=4),
}


def on_route(route, x0, gamma, beta, **call):
    """The path is checked, not assumed: the library's own plan of the very call hip.groupnorm makes of these arguments."""
    plan = hip.groupnorm_plan(x0, gamma, beta, **call)
    got = {field: getattr(plan, field) for field in PLAN_OF_ROUTE[route]}
    assert got == PLAN_OF_ROUTE[route], (route, tuple(x0.shape), {f: getattr(plan, f) for f, _ in hip.GnPlan._fields_})
    assert hip.gn_slab_applies(x0.shape[1], x0.shape[2] + (call["x1"].shape[2] if call.get("x1") is not None else 0), call["groups"]) == (route == "slab")


def gn_run(x, c0, gamma, beta, groups, silu, out_dt, route, **kw):
    """x [B, HW, C] on the host, split into the segments (c0, C - c0), on `route`; a repeated launch must give the same bits."""
    x0 = x[..., :c0].contiguous().to(DEV)
    x1 = x[..., c0:].contiguous().to(DEV) if c0 < x.shape[-1] else None
    ga, be = gamma.to(DEV), beta.to(DEV)
    on_route(route, x0, ga, be, groups=groups, eps=R.EPS, silu=silu, out_dtype=out_dt, x1=x1, **kw)
    y = hip.groupnorm(x0, ga, be, groups=groups, eps=R.EPS, silu=silu, out_dtype=out_dt, x1=x1, **kw)
    y2 = hip.groupnorm(x0, ga, be, groups=groups, eps=R.EPS, silu=silu, out_dtype=out_dt, x1=x1, **kw)
    assert torch.equal(y, y2), "a repeated launch gave other bits"
    return y


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("rung", R.LADDER)
@pytest.mark.parametrize("route,which", ROUTE_SHAPES)
def test_groupnorm_forward(route, which, rung, silu):
    c0, c1, hw, groups = ROUTES[route][which]
    for in_dt, out_dt in (PAIRS if which == 0 else SAME):
        if rung not in R.ladder(in_dt):
            continue
        x, gamma, beta, ref, yard = R.gn_case(rung, B, hw, c0 + c1, groups, in_dt, 11, silu)
        y = gn_run(x, c0, gamma, beta, groups, silu, out_dt, route)
        R.judge(f"groupnorm {route}[{c0}+{c1},{hw}] {rung} {in_dt}->{out_dt} silu={silu}", y, ref[0], yard[0], *GN_TOL[out_dt])


@pytest.mark.parametrize("in_dt", [F32, BF16])
@pytest.mark.parametrize("rung", R.LADDER)
@pytest.mark.parametrize("route,which", ROUTE_SHAPES)
def test_groupnorm_stats_out(route, which, rung, in_dt):
    """(mean, rstd) of every group, as mf_groupnorm_bwd takes them, against float64; the yardstick is what torch returns."""
    if rung not in R.ladder(in_dt):
        return
    c0, c1, hw, groups = ROUTES[route][which]
    x, gamma, beta, ref, yard = R.gn_case(rung, B, hw, c0 + c1, groups, in_dt, 11, True)
    st = torch.zeros(B, groups, 2, device=DEV)
    gn_run(x, c0, gamma, beta, groups, True, in_dt, route, stats_out=st)
    for k, what in ((0, "mean"), (1, "rstd")):
        R.judge(f"stats_out {what} {route}[{c0}+{c1},{hw}] {rung} {in_dt}", st[..., k], ref[1 + k], yard[1 + k], *GN_TOL[F32])


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("rung", R.LADDER)
@pytest.mark.parametrize("hw,splits,terms", [(64, 2, "bt"), (256, 5, "b")])
def test_groupnorm_slab_deferred_split_k(hw, splits, terms, rung, dt):
    """The slab form fed by a deferred split-K reduce whose SUM is the ladder input: the same bits as the explicit reduce followed by
    the ordinary call, and inside the bound on the values that reduce would have stored."""
    if rung not in R.ladder(dt):
        return
    c, groups, alpha = 320, 32, 0.75
    assert hip.gn_slab_applies(hw, c, groups)
    x = R.gn_input(rung, B, hw, c, groups, dt, 12).float()
    gamma, beta = R.params(c, 12)
    g = torch.Generator().manual_seed(13)
    sd = max(R.spread(rung, dt), 1e-3)
    bias = (torch.randn(c, generator=g) * 0.25 * sd).to(DEV) if "b" in terms else None
    temb = (torch.randn(B, c, generator=g) * 0.25 * sd).to(DEV) if "t" in terms else None
    ws = (x.view(1, B * hw, c) / (alpha * splits)).repeat(splits, 1, 1).contiguous().to(DEV)
    acc = torch.zeros(B * hw, c, device=DEV)
    for z in range(splits):
        acc = acc + ws[z]
    acc = acc.view(B, hw, c)
    if bias is not None:
        acc = acc + bias
    if temb is not None:
        acc = acc + temb[:, None, :]
    x_ref = (acc * alpha).to(dt)
    ga, be = gamma.to(DEV), beta.to(DEV)
    z_ref = hip.groupnorm(x_ref, ga, be, groups=groups, eps=R.EPS, silu=True, out_dtype=dt)
    for _ in range(2):
        xin = torch.empty(B, hw, c, device=DEV, dtype=dt)          # comes back unwritten from the producing GEMM
        xin._sk_pending = (ws, splits, bias, temb, c, alpha)
        plan = hip.groupnorm_plan(xin, ga, be, groups=groups, eps=R.EPS, silu=True, out_dtype=dt)
        assert plan.form == 0 and plan.launches == 1 and xin._sk_pending is not None
        z = hip.groupnorm(xin, ga, be, groups=groups, eps=R.EPS, silu=True, out_dtype=dt)
        assert xin._sk_pending is None
        assert torch.equal(z, z_ref), f"deferred reduce differs from reduce + GroupNorm by {(z.float() - z_ref.float()).abs().max()}"
    xs = x_ref.cpu()
    if rung != "constant":
        assert int(R.distinct_values(xs, groups).min()) >= R.MIN_DISTINCT
    ref, yard = R._gn(xs, gamma, beta, groups, True, torch.float64), R._gn(xs, gamma, beta, groups, True, F32)
    R.judge(f"deferred split-K slab[{hw},{splits}] {rung} {dt}", z, ref[0], yard[0], *GN_TOL[dt])


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("rung", ["m100_tight", "m300_tight", "outlier", "constant"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_a_well_conditioned_image_keeps_its_bits_beside_an_ill_conditioned_one(route, rung, dt):
    if rung not in R.ladder(dt):
        return
    c0, c1, hw, groups = ROUTES[route][-1]
    c = c0 + c1
    x_mix = R.gn_input(("base", rung, "base"), B, hw, c, groups, dt, 14)
    x_base = R.gn_input("base", B, hw, c, groups, dt, 14)
    assert torch.equal(x_mix[0], x_base[0]) and torch.equal(x_mix[2], x_base[2]) and not torch.equal(x_mix[1], x_base[1])
    gamma, beta = R.params(c, 14)
    y_mix, y_base = gn_run(x_mix, c0, gamma, beta, groups, True, dt, route), gn_run(x_base, c0, gamma, beta, groups, True, dt, route)
    assert torch.equal(y_mix[0], y_base[0]) and torch.equal(y_mix[2], y_base[2]), "an image depends on its neighbour"
    y_one = gn_run(x_mix[1:2].contiguous(), c0, gamma, beta, groups, True, dt, route)
    assert torch.equal(y_mix[1:2], y_one), "an image depends on its place in the batch"
    ref, yard = R._gn(x_mix, gamma, beta, groups, True, torch.float64), R._gn(x_mix, gamma, beta, groups, True, F32)
    R.judge(f"mixed batch {route}[{c0}+{c1},{hw}] base|{rung}|base {dt}", y_mix, ref[0], yard[0], *GN_TOL[dt])


# The first rung at which an fp32 output of a producer-fed route leaves bound() against the TRUE float64 GroupNorm (printed by the test
# below, measured on MI355X at 640 channels x 1024 rows in blocks of 128 rows; include/mfhip.h and DESIGN.md carry it): a property of
# the fp32 (sum, sum of squares) hand-over format, not of the kernel that reads it.
#   per-channel sums (part0): inside at m30 (8.1e-5, 9.7 x torch fp32), outside from m100 (7.3e-4, 19 x)
#   per-group sums (grp0):    inside at m10 (4.6e-5, 11 x), outside from m30 (3.7e-4, 44 x; 546 of 1966080 elements)
HANDED_OVER_SUMS_FIRST_RUNG_OUT = {"part0": "m100", "grp0": "m30"}


@pytest.mark.parametrize("rung", R.LADDER)
@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_groupnorm_from_handed_over_sums(dt, rung):
    """640 channels x 1024 rows with the statistics from per-channel sums of row blocks (part0) and from per-group sums (grp0), faked
    as test_three_statistics_routes fakes them.  The kernel's contract is "statistics from these sums": the reference is the float64
    GroupNorm evaluated FROM the fp32 sums as handed over, at the existing tolerance alone (a yardstick of 0).  The error of the whole
    route against the true float64 result is printed for every rung, not asserted: where it leaves the bound is decided by the
    hand-over format, which this kernel cannot mend.

    Measured on MI355X, fp32, maximum error against the contract (part0 / grp0): base 1.7e-6 / 1.6e-6 ... m100_tight 1.7e-6 / 1.4e-6,
    m300_tight 1.9e-6 / 2.2e-5 (|ref| up to 162 there), outlier 1.3e-5 / 1.3e-5, constant 1.4e-7 / 2.2e-7."""
    if rung not in R.ladder(dt):
        return
    hw, c, groups, rows = 1024, 640, 32, 128
    n = hw * (c // groups)
    x, gamma, beta, ref, yard = R.gn_case(rung, B, hw, c, groups, dt, 15, True)
    xd = x.to(DEV)
    ga, be = gamma.to(DEV), beta.to(DEV)
    v = xd.float().view(-1, rows, c)
    chan = torch.stack([v.sum(1), (v * v).sum(1)], dim=-1)                       # [B * blocks, C, 2] fp32
    grp = chan.view(-1, groups, c // groups, 2).sum(2)                           # [B * blocks, G, 2] fp32
    inside = []
    for route, part, sums in (("part0", (chan.contiguous().view(-1), rows), chan.double().view(B, -1, groups, c // groups, 2).sum((1, 3))),
                              ("grp0", (torch.cat([chan.reshape(-1), grp.reshape(-1)]).contiguous(), rows, groups),
                               grp.double().view(B, -1, groups, 2).sum(1))):
        xd._gn_part = part
        plan = hip.groupnorm_plan(xd, ga, be, groups=groups, eps=R.EPS, silu=True, out_dtype=dt)
        assert (plan.form, plan.launches) == {"part0": (2, 2), "grp0": (3, 1)}[route], (route, plan.form, plan.launches)
        y = hip.groupnorm(xd, ga, be, groups=groups, eps=R.EPS, silu=True, out_dtype=dt)
        y2 = hip.groupnorm(xd, ga, be, groups=groups, eps=R.EPS, silu=True, out_dtype=dt)
        del xd._gn_part
        assert torch.equal(y, y2), route
        R.judge(f"route {route} {rung} {dt} against the true float64 result (not asserted)", y, ref[0], yard[0], *GN_TOL[dt], fail=False)
        contract = R.gn_from_sums(x, sums.cpu(), n, gamma, beta, groups, True)
        inside.append(R.judge(f"route {route} {rung} {dt} against its contract", y, contract, None, *GN_TOL[dt], fail=False))
    assert all(r[0] for r in inside), f"{rung} {dt}: max errors against the contract (part0, grp0) {[r[1] for r in inside]}"


# ---- GroupNorm backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("rung", R.ladder(F32))
@pytest.mark.parametrize("c0,c1,h,w", [(320, 0, 32, 32), (64, 0, 6, 10), (640, 320, 17, 19)])
def test_groupnorm_backward(c0, c1, h, w, rung, silu):
    """dx, dgamma, dbeta of the streaming form, the one-block form (streaming=False) and the streaming form fed the forward kernel's
    (mean, rstd), against float64 autograd in the _rel metric of tests/test_training_gpu.py; the yardstick is fp32 autograd."""
    hw, c, groups = h * w, c0 + c1, 32
    x = R.gn_input(rung, B, hw, c, groups, F32, 16)
    gamma, beta = R.params(c, 16)
    gy = torch.randn(B, hw, c, generator=torch.Generator().manual_seed(17))
    ref, yard = R.gn_grads(x, gy, gamma, beta, groups, silu, torch.float64), R.gn_grads(x, gy, gamma, beta, groups, silu, F32)
    x0 = x[..., :c0].contiguous().to(DEV)
    x1 = x[..., c0:].contiguous().to(DEV) if c1 else None
    ga, be, gyd = gamma.to(DEV), beta.to(DEV), gy.to(DEV)
    stats = torch.empty(B, groups, 2, device=DEV)
    hip.groupnorm(x0, ga, be, groups=groups, eps=R.EPS, silu=silu, out_dtype=F32, x1=x1, stats_out=stats)
    got = {}
    for form, kw in (("streaming", dict(streaming=True)), ("one-block", dict(streaming=False)), ("streaming+stats", dict(streaming=True, stats=stats))):
        dx0, dx1, dg, db = hip.groupnorm_bwd(x0, gyd, ga, be, groups=groups, eps=R.EPS, silu=silu, x1=x1, **kw)
        dx = torch.cat([dx0, dx1], -1) if c1 else dx0
        got[form] = dx
        name = f"groupnorm_bwd {form}[{c0}+{c1},{h}x{w}] {rung} silu={silu}"
        res = [R.judge_rel(f"{name} {what}", g_, r_, y_, REL_FLOOR, fail=False)
               for what, g_, r_, y_ in (("dx", dx, ref[0], yard[0]), ("dgamma", hip.colsum(dg, c)[0], ref[1], yard[1]), ("dbeta", hip.colsum(db, c)[0], ref[2], yard[2]))]
        assert all(r[0] for r in res), f"{name}: (dx, dgamma, dbeta) rel errors {[r[1] for r in res]} against yardsticks {[r[2] for r in res]}"
    # the two forms of the same op directly: each is inside the bound of the reference, so they are within twice the bound of each other
    lim = 2.0 * R.bound(REL_FLOOR, 0.0, R.rel(yard[0], ref[0]))
    d = R.rel(got["streaming"], got["one-block"].cpu())
    print(f"groupnorm_bwd streaming vs one-block [{c0}+{c1},{h}x{w}] {rung} silu={silu}: {d:.3e} (limit {lim:.3e})")
    assert d <= lim


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------
# c % 8 == 4 runs the 4-channel layernorm_kernel (no other test reaches it), c % 8 == 0 layernorm8_kernel; 4 and 2048 are the limits of
# mf_layernorm, 2044 the widest row of the 4-channel kernel, 2040 a row whose last 8-channel pass is partly idle
LN_C4, LN_C8 = (4, 36, 100, 2044), (8, 320, 2040, 2048)
LN_ALL_PAIRS = [(F32, F32), (BF16, BF16), (F16, F16), (BF16, F32), (F16, F32), (F32, BF16), (F32, F16)]


@pytest.mark.parametrize("rung", R.LADDER)
@pytest.mark.parametrize("c", LN_C4 + LN_C8)
def test_layernorm_forward(c, rung):
    assert (c % 8 == 4) == (c in LN_C4)
    pairs = LN_ALL_PAIRS if c in (36, 320) else [(F32, F32), (BF16, BF16), (BF16, F32)]      # bf16 -> fp32: the text encoder's final norm
    gamma, beta = R.params(c, 18)
    for rows in (1, 5, 77, 1003):
        for in_dt, out_dt in pairs:
            if rung not in R.ladder(in_dt):
                continue
            x = R.ln_input(rung, rows, c, in_dt, 18)
            ref, yard = R.ln(x, gamma, beta, torch.float64), R.ln(x, gamma, beta, F32)
            y = hip.layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), R.EPS, out_dt)
            R.judge(f"layernorm[{rows}x{c}] {rung} {in_dt}->{out_dt}", y, ref, yard, *LN_TOL[out_dt])


@pytest.mark.parametrize("rung", R.ladder(F32))
@pytest.mark.parametrize("rows,c", [(130, 320), (5, 32), (77, 96)])
def test_layernorm_backward(rows, c, rung):
    x = R.ln_input(rung, rows, c, F32, 19)
    gamma, beta = R.params(c, 19)
    g = torch.Generator().manual_seed(20)
    gy, add = torch.randn(rows, c, generator=g), torch.randn(rows, c, generator=g)
    ref, yard = R.ln_grads(x, gy, gamma, beta, torch.float64), R.ln_grads(x, gy, gamma, beta, F32)
    dx, dg, db = hip.layernorm_bwd(x.to(DEV), gy.to(DEV), gamma.to(DEV), R.EPS, add=add.to(DEV))
    name = f"layernorm_bwd[{rows}x{c}] {rung}"
    res = [R.judge_rel(f"{name} {what}", g_, r_, y_, REL_FLOOR, fail=False)
           for what, g_, r_, y_ in (("dx + add", dx, ref[0] + add.double(), yard[0] + add), ("dgamma", hip.colsum(dg, c)[0], ref[1], yard[1]),
                                    ("dbeta", hip.colsum(db, c)[0], ref[2], yard[2]))]
    assert all(r[0] for r in res), f"{name}: rel errors {[r[1] for r in res]} against yardsticks {[r[2] for r in res]}"


# ---- LayerNorm folded into the GEMM that consumes it ---------------------------------------------------------------------------------
FOLD_TOL = {"bf16": (3e-2, 2e-2), "fp16": (6e-3, 4e-3)}      # test_linear_with_folded_layernorm, test_persistent_short_k_gemm
FOLD_CASES = ([("bf16", t, 300, 320, 1280, "linear") for t in (0, 48)] + [("bf16", t, 77, 64, 72, "linear") for t in (0, 48)]
              + [(p, t, 256, 320, 1600, "linear") for p in ("bf16", "fp16") for t in (69, 70)]
              + [(p, t, 2048, 320, 2 * 2560, "geglu") for p in ("bf16", "fp16") for t in (69, 70)])


def fold_rows(rung, rows, c, dt, seed):
    """Rows of mean / std of the rung, the mean's sign alternating by row, rounded to the storage dtype."""
    mean, _ = R.RUNGS[rung]
    g = torch.Generator().manual_seed(seed)
    sign = 1.0 - 2.0 * (torch.arange(rows) % 2).float()
    return (torch.randn(rows, c, generator=g) * R.spread(rung, dt) + sign[:, None] * mean).to(dt)


@pytest.mark.parametrize("rung", ["base", "m10", "m30", "m100"])
@pytest.mark.parametrize("prec_name,tile,rows,c,n,mode", FOLD_CASES)
def test_linear_with_folded_layernorm(prec_name, tile, rows, c, n, mode, rung):
    """rstd * (acc - mean * colsum(W gamma)) + (bias + W beta) with rows far from zero: the rank-1 correction carries mean / std times
    the weight of the base case, so a column sum that is not the sum of the ROUNDED W gamma shows.  Reference: float64 LayerNorm ->
    Linear on the rounded rows.  base, m10 and m30 are asserted at the existing tolerances; m100 is measured and printed."""
    from util import report
    prec = ops.Precision.get(prec_name)
    x = fold_rows(rung, rows, c, prec.act, 21)
    g = torch.Generator().manual_seed(22)
    gamma, beta = torch.randn(c, generator=g) * 0.5 + 1.0, torch.randn(c, generator=g) * 0.3
    w = torch.randn(n, c, generator=g) / math.sqrt(c)
    b = torch.randn(n, generator=g)
    xn = F.layer_norm(x.double(), (c,), gamma.double(), beta.double(), R.EPS)
    lin = F.linear(xn, w.double(), b.double())
    if mode == "geglu":
        hh, gate = lin.chunk(2, dim=-1)
        ref = hh * F.gelu(gate)
        y = ops.linear_geglu(x.to(DEV), ops.geglu_weight(w, b, prec, DEV, ln=(gamma, beta, R.EPS)), tile=tile)
    else:
        ref = lin
        y = ops.linear(x.to(DEV), ops.ConvWeight(w, b, prec, DEV, ln=(gamma, beta, R.EPS)), tile=tile)
    atol, rtol = FOLD_TOL[prec_name]
    report(f"folded layernorm {rung} [{prec_name},{mode},{rows}x{c}->{n},tile{tile}]", y, ref, atol, rtol, fail=rung != "m100")


# ---- softmax rows ---------------------------------------------------------------------------------------------------------------
def softmax_scores(rows, cols, ld, seed):
    """Rows offset by +-1e4, the maximum in the last kept column, some entries -inf (never a whole row), pad columns filled with junk."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(rows, ld, generator=g) * 4
    s += (1.0 - 2.0 * (torch.arange(rows) % 2).float())[:, None] * 1e4
    if cols > 1:
        s[:, :cols - 1][torch.rand(rows, cols - 1, generator=g) < 0.2] = -math.inf
    s[:, cols - 1] = s[:, :cols].max(-1).values + 1.5
    return s


def softmax_check(name, p, ref, cols, out_dt):
    got = p[..., :cols].double().cpu()
    if out_dt == F32:
        atol, rtol = 1e-6, 1e-5                                    # test_ops_gpu.py::test_softmax_rows
        bad = int(((got - ref).abs() > atol + rtol * ref.abs()).sum())
    else:                                                          # one ulp of the output type at the reference (probabilities are <= 1)
        mant, emin = (10, -14) if out_dt == F16 else (7, -126)
        e = torch.where(ref > 0, torch.frexp(ref)[1] - 1, torch.full_like(ref, emin, dtype=torch.int32)).clamp(min=emin)       # ref in [2^e, 2^(e + 1))
        ulp = torch.ldexp(torch.ones_like(ref), e - mant)
        bad = int(((got - ref).abs() > ulp).sum())
    print(f"{name}: max_abs_err={float((got - ref).abs().max()):.3e} bad={bad}/{ref.numel()}")
    assert bad == 0 and not bool(torch.isnan(got).any()), name
    if p.shape[-1] > cols:
        assert float(p[..., cols:].float().abs().max()) == 0.0, f"{name}: pad columns are not exactly 0"


@pytest.mark.parametrize("out_dt", [F32, BF16, F16])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 77, 4096])
def test_softmax_rows(cols, out_dt):
    ld = (cols + 7) // 8 * 8
    for rows in (1, 5, 300):
        s = softmax_scores(rows, cols, ld, 23 + cols)
        p = hip.softmax_rows(s.to(DEV), cols, out_dt)
        softmax_check(f"softmax[{rows}x{cols},ld {ld},{out_dt}]", p, R.softmax_ref(s, cols), cols, out_dt)


@pytest.mark.parametrize("out_dt", [F32, BF16, F16])
def test_softmax_rows_causal(out_dt):
    sq = cols = 77
    ld = 80
    s = softmax_scores(2 * sq, cols, ld, 24)
    s[:, 0] = s[:, 0].clamp(min=-2e4)                               # column 0 is all query 0 keeps: never -inf
    p = hip.softmax_rows_causal(s.view(2, sq, ld).to(DEV), cols, sq, out_dt).view(2 * sq, ld)
    ref = torch.zeros(2 * sq, cols, dtype=torch.float64)
    for r in range(2 * sq):
        keep = r % sq + 1
        ref[r, :keep] = torch.softmax(s[r, :keep].double(), -1)
    softmax_check(f"softmax causal[{out_dt}]", p, ref, cols, out_dt)
    for r in range(2 * sq):
        assert float(p[r, r % sq + 1:].float().abs().max() if r % sq + 1 < ld else 0.0) == 0.0
