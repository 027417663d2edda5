"""GroupNorm with the storage dtypes compiled in (csrc/norm.hip: gn_stats_kernel, gn_apply_kernel, gn_slab_kernel).

Every case is compared with F.group_norm (+ F.silu) evaluated in float64 on the values the kernel reads, with the bounds of
tests/test_ops_gpu.py::test_groupnorm (tol = 2e-5 for fp32 output, 2e-2 for bf16 output, as check(..., 5 * tol, tol)) and 4e-3 for fp16
output (as test_groupnorm_from_producer_partial_sums), and is repeated once: the repeat must give the same bits.

The shapes are the smallest at which the loops take another path: whole batches of U = 4 rows plus one and plus U - 1 tail rows with a
short last block, idle lanes (40 threads per row, 12 rows in flight), many rows in flight per block, the 4-channel vector path, two
passes over the columns of a row, two segments with groups across the border; for the one-launch form, fewer than 64 rows, one row per
lane, a last row partly past the end, and the full 4 x 64 rows."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from reflecting_reality_amd import hip  # noqa: E402

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
PAIRS = [(F32, F32), (F32, BF16), (F32, F16), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16)]     # every pair mf_groupnorm accepts
TOL = {F32: 2e-5, BF16: 2e-2}


def check(name, got, ref, out_dt):
    got = got.double().cpu()
    atol, rtol = (4e-3, 4e-3) if out_dt == F16 else (5 * TOL[out_dt], TOL[out_dt])
    err = (got - ref).abs()
    bad = (err > atol + rtol * ref.abs()).sum().item()
    print(f"{name}: max_abs_err={err.max().item():.3e} ref_max={ref.abs().max().item():.3e} bad={bad}/{ref.numel()}")
    assert bad == 0, f"{name}: {bad} elements out of tolerance, max err {err.max().item():.3e}"


def make(b, hw, c0, c1, in_dt, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.randn(b, hw, c0, generator=g) * 2 + 0.7).to(in_dt)
    x1 = (torch.randn(b, hw, c1, generator=g) - 1.0).to(in_dt) if c1 else None
    return x0, x1, torch.randn(c0 + c1, generator=g), torch.randn(c0 + c1, generator=g)


def reference(x0, x1, gamma, beta, groups, silu):
    xc = (torch.cat([x0, x1], -1) if x1 is not None else x0).double()
    ref = F.group_norm(xc.permute(0, 2, 1), groups, gamma.double(), beta.double(), 1e-5).permute(0, 2, 1)
    return F.silu(ref) if silu else ref


def run(x0, x1, gamma, beta, groups, silu, out_dt, **kw):
    a0, a1 = x0.to(DEV), (x1.to(DEV) if x1 is not None else None)
    ga, be = gamma.to(DEV), beta.to(DEV)
    y = hip.groupnorm(a0, ga, be, groups=groups, eps=1e-5, silu=silu, out_dtype=out_dt, x1=a1, **kw)
    y2 = hip.groupnorm(a0, ga, be, groups=groups, eps=1e-5, silu=silu, out_dtype=out_dt, x1=a1, **kw)
    assert torch.equal(y, y2), "a repeated launch gave other bits"
    return y


# (c0, c1, hw, groups): the two-launch form (hw > 256), batch 3
APPLY_SHAPES = [(320, 0, 12 * 4 * 2 + 1, 32), (320, 0, 12 * 4 * 2 + 3 * 12 + 5, 32), (32, 0, 1000, 32), (64, 0, 1000, 32),
                (36, 0, 300, 4), (4608, 0, 300, 32), (640, 320, 33 * 31, 32)]


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("in_dt,out_dt", PAIRS)
def test_apply_every_dtype_pair(in_dt, out_dt, silu):
    c0, c1, hw, groups = APPLY_SHAPES[0]
    x0, x1, gamma, beta = make(3, hw, c0, c1, in_dt, 1)
    y = run(x0, x1, gamma, beta, groups, silu, out_dt)
    check(f"apply[{in_dt}->{out_dt},{c0},{hw},silu={silu}]", y, reference(x0, x1, gamma, beta, groups, silu), out_dt)


@pytest.mark.parametrize("in_dt,out_dt", [(BF16, BF16), (F32, F32), (F16, F16), (F32, BF16)])
@pytest.mark.parametrize("c0,c1,hw,groups", APPLY_SHAPES[1:])
def test_apply_shapes(c0, c1, hw, groups, in_dt, out_dt):
    x0, x1, gamma, beta = make(3, hw, c0, c1, in_dt, 2)
    y = run(x0, x1, gamma, beta, groups, True, out_dt)
    check(f"apply[{in_dt}->{out_dt},{c0}+{c1},{hw}]", y, reference(x0, x1, gamma, beta, groups, True), out_dt)


@pytest.mark.parametrize("c0,c1,hw", [(320, 0, 137), (640, 320, 33 * 31), (320, 0, 65)])
def test_stats_out(c0, c1, hw):
    """(mean, rstd) of every group, as mf_groupnorm_bwd takes them: fp32 results of the same sums as an fp32 output, held to its bound."""
    x0, x1, gamma, beta = make(3, hw, c0, c1, BF16, 3)
    st = torch.zeros(3, 32, 2, device=DEV)
    run(x0, x1, gamma, beta, 32, True, BF16, stats_out=st)
    xc = (torch.cat([x0, x1], -1) if x1 is not None else x0).double().view(3, hw, 32, -1).permute(0, 2, 1, 3).reshape(3, 32, -1)
    ref = torch.stack([xc.mean(-1), 1.0 / torch.sqrt(xc.var(-1, unbiased=False) + 1e-5)], -1)
    check(f"stats_out[{c0}+{c1},{hw}]", st, ref, F32)


@pytest.mark.parametrize("dt", [BF16, F32, F16])
def test_three_statistics_routes(dt):
    """640 channels x 1024 rows: the statistics from the kernel's own pass, from per-channel sums of row blocks (part0) and from
    per-group sums (grp0), the producer's sums faked as tests/test_ops_gpu.py does."""
    b, hw, c, groups, rows = 3, 1024, 640, 32, 128
    x0, _, gamma, beta = make(b, hw, c, 0, dt, 4)
    ref = reference(x0, None, gamma, beta, groups, True)
    x = x0.to(DEV)
    ga, be = gamma.to(DEV), beta.to(DEV)
    v = x.float().view(-1, rows, c)
    chan = torch.stack([v.sum(1), (v * v).sum(1)], dim=-1)
    grp = chan.view(-1, groups, c // groups, 2).sum(2)
    for route, part in (("own", None), ("part0", (chan.contiguous().view(-1), rows)),
                        ("grp0", (torch.cat([chan.reshape(-1), grp.reshape(-1)]).contiguous(), rows, groups))):
        if part is not None:
            x._gn_part = part
        y = hip.groupnorm(x, ga, be, groups=groups, eps=1e-5, silu=True, out_dtype=dt)
        y2 = hip.groupnorm(x, ga, be, groups=groups, eps=1e-5, silu=True, out_dtype=dt)
        assert torch.equal(y, y2), route
        check(f"route {route} [{dt}]", y, ref, dt)
        if part is not None:
            del x._gn_part


@pytest.mark.parametrize("in_dt,out_dt", [(BF16, BF16), (F32, F32), (F16, F16), (BF16, F32), (F32, F16)])
@pytest.mark.parametrize("hw", [25, 64, 65, 200, 256])
@pytest.mark.parametrize("c0,c1", [(320, 0), (1280, 1280)])
def test_slab_form(c0, c1, hw, in_dt, out_dt):
    assert hip.gn_slab_applies(hw, c0 + c1, 32)
    x0, x1, gamma, beta = make(3, hw, c0, c1, in_dt, 5)
    silu = hw != 200
    y = run(x0, x1, gamma, beta, 32, silu, out_dt)
    check(f"slab[{in_dt}->{out_dt},{c0}+{c1},{hw}]", y, reference(x0, x1, gamma, beta, 32, silu), out_dt)


@pytest.mark.parametrize("dt", [BF16, F32, F16])
@pytest.mark.parametrize("hw,splits,terms", [(64, 2, "bt"), (64, 5, "b"), (256, 2, ""), (256, 5, "bt")])
def test_slab_deferred_split_k_input(hw, splits, terms, dt):
    """The input as a deferred split-K reduce (mf_groupnorm_desc.sk_ws): the same bits as the explicit reduce — slabs added in slab
    order, + bias, + temb, * alpha, rounded to the storage dtype — followed by the ordinary call."""
    b, c = 3, 320
    g = torch.Generator().manual_seed(6)
    ws = (torch.randn(splits, b * hw, c, generator=g) * 0.8 + 0.1).to(DEV)
    bias = torch.randn(c, generator=g).to(DEV) if "b" in terms else None
    temb = torch.randn(b, c, generator=g).to(DEV) if "t" in terms else None
    alpha = 0.75
    gamma, beta = torch.randn(c, generator=g).to(DEV), torch.randn(c, generator=g).to(DEV)
    acc = torch.zeros(b * hw, c, device=DEV)
    for z in range(splits):
        acc = acc + ws[z]
    acc = acc.view(b, hw, c)
    if bias is not None:
        acc = acc + bias
    if temb is not None:
        acc = acc + temb[:, None, :]
    x_ref = (acc * alpha).to(dt)
    z_ref = hip.groupnorm(x_ref, gamma, beta, groups=32, eps=1e-5, silu=True, out_dtype=dt)
    for _ in range(2):
        x = torch.empty(b, hw, c, device=DEV, dtype=dt)          # comes back unwritten from the producing GEMM
        x._sk_pending = (ws, splits, bias, temb, c, alpha)
        assert hip.groupnorm_plan(x, gamma, beta, groups=32, eps=1e-5, silu=True, out_dtype=dt).form == 0
        z = hip.groupnorm(x, gamma, beta, groups=32, eps=1e-5, silu=True, out_dtype=dt)
        assert x._sk_pending is None
        assert torch.equal(z, z_ref), f"deferred reduce differs from reduce + GroupNorm by {(z.float() - z_ref.float()).abs().max()}"
    check(f"deferred[{dt},{hw},{splits}]", z, reference(x_ref.cpu(), None, gamma.cpu(), beta.cpu(), 32, True), dt)


@pytest.mark.parametrize("c0,c1,hw", [(320, 0, 137), (640, 320, 33 * 31), (320, 0, 65), (1280, 1280, 200)])
@pytest.mark.parametrize("dt", [BF16, F32])
def test_an_image_does_not_depend_on_its_place_in_the_batch(c0, c1, hw, dt):
    x0, x1, gamma, beta = make(3, hw, c0, c1, dt, 7)
    y3 = run(x0, x1, gamma, beta, 32, True, dt)
    y1 = run(x0[1:2].contiguous(), x1[1:2].contiguous() if x1 is not None else None, gamma, beta, 32, True, dt)
    assert torch.equal(y3[1:2], y1)


@pytest.mark.parametrize("hw", [137, 64])
@pytest.mark.parametrize("in_dt,out_dt", [(F16, BF16), (BF16, F16)])
def test_a_dtype_pair_without_a_kernel_is_an_error(in_dt, out_dt, hw):
    x0, _, gamma, beta = make(2, hw, 320, 0, in_dt, 8)
    with pytest.raises(hip.MfhipError):
        hip.groupnorm(x0.to(DEV), gamma.to(DEV), beta.to(DEV), groups=32, eps=1e-5, silu=True, out_dtype=out_dt)
