"""mf_gemm_conv_plan: what mf_gemm_conv decides on the host (tile, split-K, column ranges, who reduces, where the GroupNorm statistics
come from), asked without a GPU — the plan entry never launches and never reads through a pointer.

The expected values were derived by hand from the conditions of csrc/gemm_conv.hip as they stood before plan and launch were separated
(column ranges double while tiles_m * ranges < 256 and tiles_n % (2 * ranges) == 0; the split-K heuristic; the hand-over rules), not from
the code under test.  The refusal cases follow tests/test_attention_abi_cpu.py: a valid baseline with exactly one mutation, and
mf_gemm_conv itself is only ever called with a fault (a fault-free call would launch on host pointers)."""
import ctypes as C

import pytest
import torch

from reflecting_reality_amd import hip

EINVAL, EALIGN = -1, -3
ACT_GEGLU4 = 2

_BUF = (C.c_char * 4096)()
P16 = (C.addressof(_BUF) + 15) // 16 * 16          # never dereferenced
_INTS = (C.c_int32 * 4)()                          # the descriptor's host out-ints: a plan looks at their null-ness only
HOST_INT = C.addressof(_INTS)


def linear(m, n, k, /, tile=0, dt=hip.MF_BF16, **over):
    """The descriptor of a plain Linear [m, k] -> [m, n] with a per-column bias, as ops.linear builds it."""
    d = hip.GemmDesc(dtype=dt, a_dtype=dt, out_dtype=dt, a0=P16, w=P16, out=P16, bias=P16, c0=k, lda0=k, ldw=k, batch=m, h_in=1, w_in=1,
                     h_out=1, w_out=1, kh=1, kw=1, stride=1, n=n, ldc=n, ld_res0=n, ld_res1=n, nz=1, zdiv=1, alpha=1.0, tile=tile)
    for name, v in over.items():
        setattr(d, name, v)
    return d


def conv(batch, hw, cin, n, kh, tile, **over):
    return linear(0, n, cin, tile, batch=batch, h_in=hw, w_in=hw, h_out=hw, w_out=hw, kh=kh, kw=kh, pad_t=kh // 2, pad_l=kh // 2,
                  ldw=kh * kh * cin, **over)


def plan(d):
    p = hip.GemmPlan()
    rc = hip.load().mf_gemm_conv_plan(C.byref(d), C.byref(p))
    return rc, p


def planned(d):
    rc, p = plan(d)
    assert rc == 0, hip.load().mf_last_error().decode()
    return p


# M, N, K, tiles_per_block, blocks (None: not checked), goes to tile 70 under hip.PERS_MIN_NLOOP = 2
SHAPES = [(8192, 5120, 640, 8, 256, True), (2048, 10240, 1280, 4, 256, True), (32768, 320, 320, 2, 256, True), (128, 960, 128, 3, 2, True),
          (128, 640, 128, 1, None, False), (8192, 640, 640, 1, None, False)]


@pytest.fixture
def default_routing(monkeypatch):
    monkeypatch.setattr(hip, "PREFER_PERS", True)
    monkeypatch.setattr(hip, "PERS_MIN_NLOOP", 2)


def test_plan_layout():
    assert hip.load().mf_sizeof_gemm_plan() == C.sizeof(hip.GemmPlan) == 32


@pytest.mark.parametrize("m,n,k,nloop,blocks,routed", SHAPES)
def test_expected_plans_at_tile_70(m, n, k, nloop, blocks, routed, default_routing):
    p = planned(linear(m, n, k, tile=hip.PERS_TILE))
    assert (p.tile, p.splitk, p.tiles_per_block, p.reduce_launch, p.deferred_splits) == (hip.PERS_TILE, 1, nloop, 0, 0)
    if blocks is not None:
        assert p.blocks == blocks
    d = linear(m, n, k)
    assert hip._route_pers(d) == routed
    assert (d.tile, d.splitk) == ((hip.PERS_TILE, 1) if routed else (0, 0))


@pytest.mark.parametrize("m,n,k,nloop,blocks,routed", SHAPES)
def test_pers_linear_agrees(m, n, k, nloop, blocks, routed, default_routing):
    assert hip.pers_linear(m, n, k, torch.bfloat16) == routed
    assert hip.pers_linear(m, n, k, torch.float16) == routed
    assert not hip.pers_linear(m, n, k, torch.float32)


TILE70_REFUSALS = {
    "M = 64": dict(batch=64),
    "N = 128": dict(n=128, ldc=128, ld_res0=128, ld_res1=128),
    "K = 96": dict(c0=96, lda0=96, ldw=96),
    "K = 64": dict(c0=64, lda0=64, ldw=64),
    "c1 > 0": dict(a1=P16, c1=64, lda1=64, ldw=192),
    "time embedding": dict(temb=P16, ld_temb=960),
    "res1": dict(res1=P16, res1_dtype=hip.MF_BF16),
    "ld_res0 = 964": dict(res0=P16, res0_dtype=hip.MF_BF16, ld_res0=964),
    "out 8 bytes off": dict(out=P16 + 8),
    "fp32 out": dict(out_dtype=hip.MF_F32),
}


@pytest.mark.parametrize("case", TILE70_REFUSALS)
def test_refused_at_tile_70_and_served_elsewhere(case, default_routing):
    fault = TILE70_REFUSALS[case]
    assert planned(linear(128, 960, 128, tile=hip.PERS_TILE)).tiles_per_block == 3          # the baseline goes to tile 70
    rc, _ = plan(linear(128, 960, 128, tile=hip.PERS_TILE, **fault))
    assert rc == EINVAL and b"persistent 128-row GEMM" in hip.load().mf_last_error()
    d = linear(128, 960, 128, **fault)
    assert planned(d).tile not in (0, hip.PERS_TILE)
    assert not hip._route_pers(d) and (d.tile, d.splitk) == (0, 0)


def test_splitk_and_deferral():
    ws = dict(ws=P16, ws_floats=39 * 128 * 1280, defer_reduce=1, deferred_splits=HOST_INT)
    # M 128, N 1280, K 11520: 10 tiles of 128 x 128, 180 K tiles; ceil(394 / 10) = 39 <= 180 / 4 slices of ceil(180 / 39) = 5 K tiles: 36 of them
    p = planned(conv(2, 8, 1280, 1280, 3, 1, **ws))
    assert (p.tile, p.splitk, p.deferred_splits, p.reduce_launch, p.tiles_per_block, p.blocks) == (1, 36, 36, 0, 1, 360)
    p = planned(conv(2, 8, 1280, 1280, 3, 1, res0=P16, res0_dtype=hip.MF_BF16, **ws))
    assert (p.splitk, p.deferred_splits, p.reduce_launch) == (36, 0, 1)


@pytest.mark.parametrize("tile,rows,grouped", [(1, 128, 0), (14, 128, 1), (70, 128, 0)])
def test_gn_part_modes(tile, rows, grouped):
    """128 x 128 columns do not hold whole groups of 10 channels, 160 do; tile 70 has no statistics epilogue (column sums, per channel)."""
    d = conv(2, 32, 320, 320, 1, tile, splitk=1, gn_part=P16, gn_part_floats=2 * 320 * (2048 // 32), gn_part_rows=HOST_INT, gn_groups=32,
             gn_grouped=HOST_INT + 4)
    p = planned(d)
    assert (p.tile, p.splitk, p.gn_part_rows, p.gn_grouped, p.reduce_launch, p.deferred_splits) == (tile, 1, rows, grouped, 0, 0)
    assert list(_INTS) == [0, 0, 0, 0], "a plan writes no host out-int"


_VT = dict(vt_out=P16, vt_tokens=64, vt_ld=64, n=960)
_GN = dict(gn_part=P16, gn_part_floats=1 << 20, gn_part_rows=HOST_INT)
FAULTS = {          # name -> (mutation of linear(128, 960, 128), return code, a word of the message)
    "null a0": (dict(a0=None), EINVAL, "null a0/w/out"),
    "bad dtype": (dict(dtype=9), EINVAL, "bad dtype"),
    "c0 % vec": (dict(c0=132), EINVAL, "channels"),
    "misaligned w": (dict(w=P16 + 8), EALIGN, "16-byte aligned"),
    "ldw < K": (dict(ldw=64), EINVAL, "ldw 64 < K 128"),
    "GEGLU with a residual": (dict(act=ACT_GEGLU4, res0=P16, res0_dtype=hip.MF_BF16), EINVAL, "GEGLU"),
    "vt_n0 % 160": (dict(vt_n0=128, **_VT), EINVAL, "vt_out needs"),
    "gn_part with hw % 32": (dict(batch=2, h_in=8, w_in=6, h_out=8, w_out=6, **_GN), EINVAL, "gn_part needs"),
    "split-K without a workspace": (dict(splitk=2), EINVAL, "needs a workspace"),
    "halo tile on a 1x1 call": (dict(tile=16), EINVAL, "3x3 halo kernel"),
    "tile 27 on fp32 compute": (dict(tile=27, dtype=hip.MF_F32, a_dtype=hip.MF_F32, out_dtype=hip.MF_F32), EINVAL, "16x16x32 MFMA form"),
}


@pytest.mark.parametrize("case", FAULTS)
def test_plan_and_launch_refuse_alike(case):
    fault, want, word = FAULTS[case]
    lib = hip.load()
    assert planned(linear(128, 960, 128)).tile > 0           # the baseline is a valid call (asked of the plan: it would launch)
    if case == "vt_n0 % 160":
        assert planned(linear(128, 960, 128, vt_n0=640, **_VT)).tile > 0
    if case == "gn_part with hw % 32":
        assert planned(linear(128, 960, 128, batch=2, h_in=8, w_in=8, h_out=8, w_out=8, **_GN)).gn_part_rows == 64
    rc_plan, _ = plan(linear(128, 960, 128, **fault))
    msg_plan = lib.mf_last_error().decode()
    rc_conv = lib.mf_gemm_conv(C.byref(linear(128, 960, 128, **fault)), None)
    msg_conv = lib.mf_last_error().decode()
    assert rc_plan == rc_conv == want and msg_plan == msg_conv and word in msg_plan, (rc_plan, msg_plan, rc_conv, msg_conv)


def test_null_arguments():
    lib = hip.load()
    assert lib.mf_gemm_conv_plan(None, C.byref(hip.GemmPlan())) == EINVAL and b"null descriptor" in lib.mf_last_error()
    assert lib.mf_gemm_conv_plan(C.byref(linear(128, 960, 128)), None) == EINVAL and b"null plan" in lib.mf_last_error()
