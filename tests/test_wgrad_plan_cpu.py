"""mf_conv_wgrad_plan: what mf_conv_wgrad decides on the host (kernel form, tile width, pixel split, who sums the slabs, grid, block,
dynamic LDS), asked without a GPU — the plan entry never launches and reads nothing behind the descriptor's pointers.

The expected plans were computed by transcribing the cost model and the conditions of mf_conv_wgrad as they stood BEFORE plan and launch
were separated (rounds of 512 blocks x 32-pixel steps x 2.3 / 3.7 us, the 0.98 hysteresis, the slab traffic term, the split capped at
M / 256 in 1..64 and by the workspace) into Python, in double precision with the same order of operations — not from the code under test.
The refusal cases follow tests/test_gemm_plan_cpu.py: a valid baseline with exactly one mutation, and mf_conv_wgrad itself is only ever
called with a fault (a fault-free call would launch on host pointers)."""
import ctypes as C

import pytest

from reflecting_reality_amd import hip

EINVAL, EALIGN = -1, -3
F32, F16X3, BF16X1, BF16 = hip.MF_F32, hip.MF_F16X3, hip.MF_BF16X1, hip.MF_BF16
WT_PLANE, W160_PLANE, WD_NST = 32 * 256, 32 * 320, 3          # bytes of one 16-bit plane of a 32-pixel stage (128 / 160 columns); DMA stages

_BUF = (C.c_char * 4096)()
P16 = (C.addressof(_BUF) + 15) // 16 * 16          # never dereferenced


def conv(dt, batch, h, w, c0, n, k, /, c1=0, **over):
    """The descriptor of a k x k stride-1 'same' conv's weight gradient as hip.conv_wgrad builds it (the shared 64 Mi-float workspace,
    heuristic split, accumulate)."""
    d = hip.WgradDesc(dtype=dt, a0=P16, a1=P16 if c1 else None, c0=c0, c1=c1, lda0=c0, lda1=c1, batch=batch, h_in=h, w_in=w, h_out=h, w_out=w,
                      kh=k, kw=k, stride=1, pad_t=k // 2, pad_l=k // 2, dy=P16, lddy=n, n=n, dw=P16, lddw=k * k * (c0 + c1), accumulate=1,
                      splitm=0, ws=P16, ws_floats=hip.WGRAD_WS_FLOATS)
    for name, v in over.items():
        setattr(d, name, v)
    return d


def plan(d):
    p = hip.WgradPlan()
    rc = hip.load().mf_conv_wgrad_plan(C.byref(d), C.byref(p))
    return rc, p


def planned(d):
    rc, p = plan(d)
    assert rc == 0, hip.load().mf_last_error().decode()
    return p


def fields(p):
    return {name: getattr(p, name) for name, _ in hip.WgradPlan._fields_}


# (dtype, batch, h, w, c0, n, k) -> form, tiles, splitm, m_per_split, reduce_launch, slabs_xcd
TABLE = [
    ((BF16, 8, 64, 64, 320, 320, 3), (2, 36, 14, 2368, 1, 8)),
    ((F16X3, 8, 64, 64, 320, 320, 3), (2, 36, 14, 2368, 1, 8)),
    ((F16X3, 4, 32, 32, 320, 320, 3), (2, 36, 13, 320, 1, 8)),
    ((BF16, 8, 32, 32, 640, 640, 3), (3, 225, 2, 4096, 1, 0)),
    ((BF16, 8, 16, 16, 1280, 1280, 3), (3, 900, 1, 2048, 0, 0)),
    ((BF16, 8, 8, 8, 1280, 1280, 3, 1280), (3, 1800, 1, 512, 0, 0)),
    ((BF16, 8, 64, 64, 320, 320, 1), (3, 9, 54, 608, 1, 48)),
    ((BF16, 2, 33, 31, 136, 72, 3), (3, 18, 7, 320, 1, 0)),
    ((BF16, 3, 5, 7, 8, 8, 3), (3, 9, 1, 128, 0, 0)),
    ((F16X3, 8, 8, 8, 1280, 1280, 3), (1, 900, 1, 512, 0, 0)),
    ((BF16X1, 2, 16, 16, 160, 160, 3), (1, 36, 2, 256, 1, 0)),
    ((F32, 8, 64, 64, 320, 320, 3), (0, 81, 13, 2528, 1, 8)),
    ((F32, 2, 8, 8, 64, 64, 3), (0, 9, 1, 128, 1, 0)),
]
IDS = ["-".join(map(str, case)) for case, _ in TABLE]


def launch_of(form, dt):
    """(tile_w, threads, dynamic LDS bytes) of a form: what the launch ladder of the entry passed before the plan existed."""
    planes = 2 * 4 if dt == F16X3 else 2 * 2
    return {0: (128, 256, 0), 1: (128, 256, planes * WT_PLANE), 2: (160, 320, planes * W160_PLANE), 3: (128, 256, WD_NST * 2 * WT_PLANE)}[form]


def check(p, dt, want):
    form, tiles, splitm, m_per_split, reduce_launch, slabs_xcd = want
    tile_w, threads, lds = launch_of(form, dt)
    assert fields(p) == dict(form=form, tile_w=tile_w, tiles=tiles, splitm=splitm, m_per_split=m_per_split, reduce_launch=reduce_launch,
                             slabs_xcd=slabs_xcd, blocks=tiles * splitm, threads=threads, lds_bytes=lds)


def test_plan_layout():
    assert hip.load().mf_sizeof_wgrad_plan() == C.sizeof(hip.WgradPlan) == 40


@pytest.mark.parametrize("case,want", TABLE, ids=IDS)
def test_expected_plans(case, want):
    check(planned(conv(*case)), case[0], want)


def test_no_workspace_means_one_slab_on_the_128_tile():
    check(planned(conv(BF16, 8, 64, 64, 320, 320, 3, ws=None, ws_floats=0, accumulate=1)), BF16, (3, 81, 1, 32768, 0, 0))


def test_two_segments_take_the_dma_form_when_the_first_fills_whole_tiles():
    assert planned(conv(BF16, 2, 8, 8, 256, 384, 3, 128)).form == 3


def test_two_segments_with_a_ragged_first_one_stay_register_staged():
    """c0 = 136, c1 = 64 at 2 x 16 x 16, n = 160: M = 512 (cap 2), tiles of 128: 2 x 2 x 9 = 36, of 160: 1 x 2 x 9 = 18; one round either
    way.  128: split 2 costs 8 steps x 2.3 + slabs (2 x 160 x 1800 x 8 / 4e6 + 4 = 5.152) = 23.552 < 0.98 x 16 x 2.3 = 36.064;
    160: split 1 costs 16 x 3.7 = 59.2, split 2 8 x 3.7 + 5.152 = 34.752: the 128 tile wins, and the DMA form is refused (C0 % 128 != 0)."""
    check(planned(conv(BF16, 2, 16, 16, 136, 160, 3, 64)), BF16, (1, 36, 2, 256, 1, 0))


def test_fp32_with_one_slab_adds_through_the_workspace_and_writes_directly():
    check(planned(conv(F32, 2, 8, 8, 64, 64, 3, accumulate=1)), F32, (0, 9, 1, 128, 1, 0))
    check(planned(conv(F32, 2, 8, 8, 64, 64, 3, accumulate=0)), F32, (0, 9, 1, 128, 0, 0))


@pytest.mark.parametrize("case,want", TABLE, ids=IDS)
def test_dma_switch_off_moves_form_3_to_form_1_and_nothing_else(case, want):
    lib = hip.load()
    try:
        lib.mf_debug_set_wgrad_dma(0)
        p = planned(conv(*case))
    finally:
        lib.mf_debug_set_wgrad_dma(1)
    check(p, case[0], ((1 if want[0] == 3 else want[0]),) + want[1:])
    check(planned(conv(*case)), case[0], want)


@pytest.mark.parametrize("case,want", TABLE, ids=IDS)
def test_the_planned_split_fits_the_workspace_query(case, want):
    d = conv(*case)
    n, K = d.n, d.kh * d.kw * (d.c0 + d.c1)
    assert planned(d).splitm * n * K <= hip.load().mf_conv_wgrad_ws_floats(C.byref(d))


def test_split_is_capped_by_the_workspace():
    d = conv(BF16, 8, 64, 64, 320, 320, 1, ws_floats=3 * 320 * 320)
    assert planned(conv(BF16, 8, 64, 64, 320, 320, 1)).splitm == 54
    assert 1 <= planned(d).splitm <= 3


BASE = (BF16, 2, 16, 16, 160, 160, 3)
FAULTS = {          # name -> (baseline arguments, mutation, return code, a word of the message)
    "bad dtype": (BASE, dict(dtype=9), EINVAL, "dtype must be"),
    "MF_BF16 with c0 % 8": (BASE, dict(c0=156, lda0=156, lddw=9 * 156), EINVAL, "multiples of 8"),
    "c0 % 4": ((F16X3,) + BASE[1:], dict(c0=158, lda0=158, lddw=9 * 158), EINVAL, "multiples of 4"),
    "a1 without c1": (BASE, dict(a1=P16), EINVAL, "channel counts / pixel strides"),
    "null dy": (BASE, dict(dy=None), EINVAL, "null a0/dy/dw"),
    "bad geometry": (BASE, dict(stride=0), EINVAL, "bad geometry"),
    "misaligned a0": (BASE, dict(a0=P16 + 8), EALIGN, "16-byte aligned"),
    "lddy % 4": ((F16X3,) + BASE[1:], dict(lddy=162), EALIGN, "lddy a multiple of 4"),
    "M = 2^31": (BASE, dict(batch=32768, h_in=256, w_in=256, h_out=256, w_out=256), EINVAL, "M too large"),
    "lddw < K": (BASE, dict(lddw=1439), EINVAL, "lddw < K"),
    "explicit split without the workspace for it": (BASE, dict(splitm=2, ws_floats=2 * 160 * 1440 - 1), EINVAL, "split-M=2 needs 460800"),
    "accumulate without a workspace": ((F32,) + BASE[1:], dict(ws=None, ws_floats=0), EINVAL, "accumulate needs a workspace"),
}


@pytest.mark.parametrize("case", FAULTS)
def test_plan_and_launch_refuse_alike(case):
    base, fault, want, word = FAULTS[case]
    lib = hip.load()
    planned(conv(*base))          # the baseline is a valid call (asked of the plan: it would launch)
    rc_plan, _ = plan(conv(*base, **fault))
    msg_plan = lib.mf_last_error().decode()
    rc_conv = lib.mf_conv_wgrad(C.byref(conv(*base, **fault)), None)
    msg_conv = lib.mf_last_error().decode()
    assert rc_plan == rc_conv == want and msg_plan == msg_conv and word in msg_plan, (rc_plan, msg_plan, rc_conv, msg_conv)


def test_null_arguments():
    lib = hip.load()
    assert lib.mf_conv_wgrad_plan(None, C.byref(hip.WgradPlan())) == EINVAL and b"null descriptor" in lib.mf_last_error()
    assert lib.mf_conv_wgrad(None, None) == EINVAL and b"null descriptor" in lib.mf_last_error()
    assert lib.mf_conv_wgrad_plan(C.byref(conv(*BASE)), None) == EINVAL and b"null plan" in lib.mf_last_error()
