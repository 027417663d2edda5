"""mf_groupnorm_plan: what mf_groupnorm decides on the host (which of its four forms, how many launches, vector width, who finalizes
the statistics, the chunks that place them in the workspace, grid, block, dynamic LDS), asked without a GPU — the plan entry never
launches and reads nothing behind the descriptor's pointers.

The expected plans were computed by transcribing the conditions of mf_groupnorm as they stood BEFORE plan and launch were separated
(the slab shape rule, the chunking of max(ceil(hw / 64), 16) rows, the fused finalize up to hw 1024 with aligned gamma / beta, the
producers' sums with at most 128 / 64 row blocks, 1024 target blocks of at least 4 rows per thread, the finalize launch's threads per
channel) into Python with its sweep switches at their defaults — not from the code under test.  The refusal cases follow
tests/test_wgrad_plan_cpu.py: a valid baseline with exactly one mutation, and mf_groupnorm itself is only ever called with a fault (a
fault-free call would launch on host pointers)."""
import ctypes as C

import pytest

from reflecting_reality_amd import hip

EINVAL = -1
F32, BF16, F16 = hip.MF_F32, hip.MF_BF16, hip.MF_F16

_BUF = (C.c_char * 4096)()
P16 = (C.addressof(_BUF) + 15) // 16 * 16          # never dereferenced
FIELDS = [name for name, _ in hip.GnPlan._fields_]


def gn(batch, hw, c0, c1=0, /, groups=32, in_dt=BF16, out_dt=BF16, **over):
    """The descriptor of GroupNorm + SiLU over [batch, hw, c0 (+ c1)] as hip.groupnorm builds it: every pointer 16-byte aligned."""
    d = hip.GroupNormDesc(x0=P16, x1=P16 if c1 else None, c0=c0, c1=c1, in_dtype=in_dt, batch=batch, hw=hw, groups=groups, eps=1e-5,
                          gamma=P16, beta=P16, silu=1, out=P16, out_dtype=out_dt, ws=P16)
    for name, v in over.items():
        setattr(d, name, v)
    return d


def plan(d):
    p = hip.GnPlan()
    rc = hip.load().mf_groupnorm_plan(C.byref(d), C.byref(p))
    return rc, p


def planned(d):
    rc, p = plan(d)
    assert rc == 0, hip.load().mf_last_error().decode()
    return p


def fields(p):
    return tuple(getattr(p, name) for name in FIELDS)


PART0 = dict(part0=P16)
PARTS = dict(part0=P16, part1=P16)
BOTH = dict(part0=P16, grp0=P16)
# name -> (descriptor, (form, launches, vec, finalize, centered, chunks, rows_per_chunk, rows_per_block, blocks, threads, lds_bytes, finalize_parts))
TABLE = {
    "slab 3x64x320": (gn(3, 64, 320), (0, 1, 8, 0, 0, 0, 0, 64, 24, 320, 20480, 0)),
    "slab 3x200x1280+1280": (gn(3, 200, 1280, 1280), (0, 1, 8, 0, 0, 0, 0, 64, 96, 640, 40960, 0)),
    "slab 2x25x64+32": (gn(2, 25, 64, 32), (0, 1, 8, 0, 0, 0, 0, 25, 8, 128, 4800, 0)),
    "fused 3x1024x640": (gn(3, 1024, 640), (1, 2, 8, 1, 0, 64, 16, 24, 129, 512, 30720, 0)),
    "fused 3x1024x640, fp32 out": (gn(3, 1024, 640, out_dt=F32), (1, 2, 8, 1, 1, 64, 16, 24, 129, 512, 30720, 0)),
    "fused 3x1023x640+320": (gn(3, 1023, 640, 320), (1, 2, 8, 1, 0, 64, 16, 16, 192, 512, 30720, 0)),
    "separate 3x1100x320": (gn(3, 1100, 320), (1, 3, 8, 0, 0, 62, 18, 48, 69, 512, 30720, 0)),
    "vec4 3x300x36 in 4 groups": (gn(3, 300, 36, groups=4), (1, 2, 4, 1, 0, 19, 16, 224, 6, 512, 16128, 0)),
    "separate 8x4096x320": (gn(8, 4096, 320), (1, 3, 8, 0, 0, 64, 64, 48, 688, 512, 30720, 0)),
    "2x64x3200: 100 channels per group, no slab": (gn(2, 64, 3200), (1, 2, 8, 1, 0, 4, 16, 4, 32, 448, 25600, 0)),
    "3x64x320, gamma 4 bytes off 16: three launches": (gn(3, 64, 320, gamma=P16 + 4), (1, 3, 8, 0, 0, 4, 16, 48, 6, 512, 30720, 0)),
    "3x64x320, x0 8 bytes off 16: no slab, fused": (gn(3, 64, 320, x0=P16 + 8), (1, 2, 8, 1, 0, 4, 16, 48, 6, 512, 30720, 0)),
    "1x16x320 to fp32, beta off 16: one chunk, not centered": (gn(1, 16, 320, out_dt=F32, beta=P16 + 4), (1, 3, 8, 0, 0, 1, 16, 48, 1, 512, 30720, 0)),
    "channel sums 2x4096x320, blocks of 256": (gn(2, 4096, 320, **PART0, part0_rows=256), (2, 2, 8, 0, 0, 64, 64, 48, 172, 512, 7680, 12)),
    "channel sums 2x1024x640+320, blocks of 256 / 128": (gn(2, 1024, 640, 320, **PARTS, part0_rows=256, part1_rows=128),
                                                         (2, 2, 8, 0, 0, 64, 16, 16, 128, 512, 7680, 4)),
    "channel sums 2x1024x640 to fp32: centered": (gn(2, 1024, 640, out_dt=F32, **PART0, part0_rows=128), (2, 2, 8, 0, 1, 64, 16, 24, 86, 512, 7680, 6)),
    "channel sums 2x4096x64 in 2 groups: one slice": (gn(2, 4096, 64, groups=2, **PART0, part0_rows=128), (2, 2, 8, 0, 0, 64, 64, 256, 32, 512, 8192, 8)),
    "2x4096x320, 256 blocks of 16 rows > 128: own statistics": (gn(2, 4096, 320, **PART0, part0_rows=16), (1, 3, 8, 0, 0, 64, 64, 48, 172, 512, 30720, 0)),
    "2x4096x320, second segment without sums: own statistics": (gn(2, 4096, 160, 160, **PART0, part0_rows=64), (1, 3, 8, 0, 0, 64, 64, 48, 172, 512, 30720, 0)),
    "group sums 2x4096x320, blocks of 64": (gn(2, 4096, 320, **BOTH, part0_rows=64, grp0_rows=64), (3, 1, 8, 2, 0, 64, 64, 48, 172, 512, 0, 0)),
    "2x4096x320, 128 blocks of 32 rows > 64: channel sums": (gn(2, 4096, 320, **BOTH, part0_rows=32, grp0_rows=32), (2, 2, 8, 0, 0, 64, 64, 48, 172, 512, 7680, 12)),
    "group sums 2x1024x640 fp32 to fp32": (gn(2, 1024, 640, in_dt=F32, out_dt=F32, **BOTH, part0_rows=128, grp0_rows=128),
                                           (3, 1, 8, 2, 1, 64, 16, 24, 86, 512, 0, 0)),
    "2x1024x640, group sums but gamma off 16: channel sums": (gn(2, 1024, 640, **BOTH, part0_rows=128, grp0_rows=128, gamma=P16 + 4),
                                                               (2, 2, 8, 0, 0, 64, 16, 24, 86, 512, 7680, 6)),
    "slab 3x64x320 with producer sums: still the slab": (gn(3, 64, 320, **BOTH, part0_rows=32, grp0_rows=32), (0, 1, 8, 0, 0, 0, 0, 64, 24, 320, 20480, 0)),
    "slab 3x64x320 from 3 split-K slabs": (gn(3, 64, 320, sk_ws=P16, sk_splits=3, sk_bias=P16, sk_temb=P16, sk_ld_temb=320, sk_alpha=1.0),
                                           (0, 1, 8, 0, 0, 0, 0, 64, 24, 320, 20480, 0)),
}


def test_plan_layout():
    assert hip.load().mf_sizeof_gn_plan() == C.sizeof(hip.GnPlan) == 48


@pytest.mark.parametrize("case", TABLE)
def test_expected_plans(case):
    d, want = TABLE[case]
    assert dict(zip(FIELDS, fields(planned(d)))) == dict(zip(FIELDS, want))


PAIRS = [(F32, F32), (F32, BF16), (F32, F16), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16)]


@pytest.mark.parametrize("in_dt,out_dt", PAIRS)
def test_every_accepted_dtype_pair_plans_the_same_route(in_dt, out_dt):
    """The storage dtypes choose the kernels' template arguments, not the route: only `centered` follows an fp32 output."""
    assert fields(planned(gn(3, 64, 320, in_dt=in_dt, out_dt=out_dt))) == TABLE["slab 3x64x320"][1]
    want = list(TABLE["fused 3x1024x640"][1])
    want[FIELDS.index("centered")] = int(out_dt == F32)
    assert fields(planned(gn(3, 1024, 640, in_dt=in_dt, out_dt=out_dt))) == tuple(want)


SLAB, STREAM = (3, 64, 320), (2, 1024, 640)
SK = dict(sk_ws=P16, sk_splits=3, sk_bias=P16, sk_temb=P16, sk_ld_temb=320, sk_alpha=1.0)
SK_TEXT = ("mf_groupnorm: a deferred split-K input (sk_ws) needs the one-launch form (hw <= 256, channels % 8 == 0, one segment), "
           ">= 2 slabs, 16-byte aligned slabs / bias / temb and no stats_out")
FAULTS = {          # name -> (baseline arguments, baseline keywords, mutation, a word of the message)
    "null x0": (STREAM, {}, dict(x0=None), "null pointer"),
    "null out": (STREAM, {}, dict(out=None), "null pointer"),
    "null gamma": (SLAB, {}, dict(gamma=None), "null pointer"),
    "null beta": (SLAB, {}, dict(beta=None), "null pointer"),
    "null ws": (STREAM, {}, dict(ws=None), "null pointer"),
    "c1 without x1": (STREAM, {}, dict(c1=320), "bad segments"),
    "x1 without c1": (STREAM, {}, dict(x1=P16), "bad segments"),
    "no first segment": (STREAM, {}, dict(c0=0), "bad segments"),
    "C not divisible by groups": (STREAM, {}, dict(groups=7), "C=640 not divisible by groups=7"),
    "no groups": (SLAB, {}, dict(groups=0), "not divisible by groups=0"),
    "channels % 4": (STREAM, {}, dict(c0=642, groups=2), "multiples of 4"),
    "no image": (STREAM, {}, dict(batch=0), "bad batch/hw"),
    "no rows": (SLAB, {}, dict(hw=0), "bad batch/hw"),
    "fp16 in, bf16 out": (STREAM, {}, dict(in_dtype=F16), "fp16 and bf16 operands"),
    "bf16 in, fp16 out": (SLAB, {}, dict(out_dtype=F16), "fp16 and bf16 operands"),
    "128 groups": (STREAM, {}, dict(groups=128), "at most 64 groups"),
    "128 groups on the slab shape": (SLAB, {}, dict(c0=1280, groups=128), "at most 64 groups"),
    "mixed 16-bit dtypes are reported before 128 groups": (STREAM, {}, dict(groups=128, out_dtype=F16), "fp16 and bf16 operands"),
    "C too large for LDS": (STREAM, {}, dict(c0=8256), "C=8256 too large"),
    "a dtype without kernels, streaming": (STREAM, {}, dict(in_dtype=hip.MF_FP8), "no kernel for in_dtype 4 with out_dtype 1"),
    "a dtype without kernels, slab": (SLAB, {}, dict(out_dtype=hip.MF_F16X3), "no kernel for in_dtype 1 with out_dtype 2"),
    "C too large is reported before a dtype without kernels": (STREAM, {}, dict(c0=8256, in_dtype=hip.MF_FP8), "C=8256 too large"),
    "sk_ws at hw 1024": (SLAB, SK, dict(hw=1024), SK_TEXT),
    "sk_ws with two segments": (SLAB, SK, dict(c1=320, x1=P16), SK_TEXT),
    "sk_ws with 1 slab": (SLAB, SK, dict(sk_splits=1), SK_TEXT),
    "sk_ws with stats_out": (SLAB, SK, dict(stats_out=P16), SK_TEXT),
    "sk_ws with a misaligned slab": (SLAB, SK, dict(sk_ws=P16 + 4), SK_TEXT),
    "sk_ws with a misaligned bias": (SLAB, SK, dict(sk_bias=P16 + 8), SK_TEXT),
    "sk_ws with temb rows off 16 bytes": (SLAB, SK, dict(sk_ld_temb=322), SK_TEXT),
    "sk_ws with a misaligned gamma": (SLAB, SK, dict(gamma=P16 + 4), SK_TEXT),
    "sk_ws is refused before a dtype without kernels": (SLAB, SK, dict(sk_splits=1, in_dtype=hip.MF_FP8), SK_TEXT),
}


@pytest.mark.parametrize("case", FAULTS)
def test_plan_and_launch_refuse_alike(case):
    base, kw, fault, word = FAULTS[case]
    lib = hip.load()
    planned(gn(*base, **kw))          # the baseline is a valid call (asked of the plan: it would launch)
    rc_plan, _ = plan(gn(*base, **{**kw, **fault}))
    msg_plan = lib.mf_last_error().decode()
    rc_gn = lib.mf_groupnorm(C.byref(gn(*base, **{**kw, **fault})), None)
    msg_gn = lib.mf_last_error().decode()
    assert rc_plan == rc_gn == EINVAL and msg_plan == msg_gn and word in msg_plan, (rc_plan, msg_plan, rc_gn, msg_gn)
    if word is SK_TEXT:
        assert msg_plan == SK_TEXT          # word for word


def test_null_arguments():
    lib = hip.load()
    assert lib.mf_groupnorm_plan(None, C.byref(hip.GnPlan())) == EINVAL and b"mf_groupnorm: null pointer" in lib.mf_last_error()
    assert lib.mf_groupnorm(None, None) == EINVAL and b"mf_groupnorm: null pointer" in lib.mf_last_error()
    assert lib.mf_groupnorm_plan(C.byref(gn(*SLAB)), None) == EINVAL and b"null plan" in lib.mf_last_error()


def test_the_slab_predicate_is_the_plans_form():
    """mf_groupnorm_slab_applies(hw, c, groups) == (the plan of that shape with aligned pointers is form 0), over the shapes of
    tests/test_host_logic.py::test_gn_slab_predicate_mirrors_the_library; a shape the call refuses has no form."""
    lib = hip.load()
    shapes = [(hw, c, 32) for c in (320, 640, 960, 1280, 1920, 2560) for hw in (64, 256, 1024)] + [(64, 3200, 32), (64, 324, 32), (64, 320, 0)]
    seen = set()
    for hw, c, groups in shapes:
        rc, p = plan(gn(2, hw, c, groups=groups))
        slab = rc == 0 and p.form == 0
        assert bool(lib.mf_groupnorm_slab_applies(hw, c, groups)) == slab, (hw, c, groups)
        seen.add((rc == 0, slab))
    assert seen == {(True, True), (True, False), (False, False)}


def test_the_workspace_query_holds_what_the_plan_places_in_it():
    """Chunk statistics [batch][groups][chunks][2] (the centered triples in the image's own slots: 3 floats per group need 2 chunks),
    then the per-channel affine [batch][2][C] at batch * groups * 64 * 2."""
    for case, (d, _) in TABLE.items():
        p = planned(d)
        assert p.chunks <= 64 and (not p.centered or p.chunks >= 2), case
        assert d.batch * d.groups * 64 * 2 + d.batch * 2 * (d.c0 + d.c1) == hip.load().mf_groupnorm_ws_floats(d.batch, d.groups, d.c0 + d.c1), case
