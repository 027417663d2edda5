"""The argument contract of the 16 attention entries of csrc/attention.hip (11 forward, 2 backward, 3 row-dot), checked without a GPU.

Every check of these entries runs before anything is launched, so a call with one fault returns its code from host buffers alone.  A case
is a valid call (the baseline) with exactly one mutation; the baseline itself is never called, because a fault-free call would launch on
host pointers (this file also runs with the whole suite on GPU machines).  One fault per case leaves the order of the checks free.

The head dims a flavour refuses are the complement of the ops.FLASH_*_HEAD_DIMS tuples; the GPU tests run every dim inside them, and the
two together pin the library's table and the Python tuples to each other."""
import ctypes as C

import pytest

from reflecting_reality_amd import hip, ops

EINVAL, EALIGN = -1, -3

_BUF = (C.c_char * 4096)()
P16 = (C.addressof(_BUF) + 15) // 16 * 16          # never dereferenced: every case is refused before a launch

_16 = "q ldq k ldk vt ldvt out ldo batch heads sq skv head_dim scale stream"
_X3 = "q_hi q_lo ldq k_hi k_lo ldk vt_hi vt_lo ldvt out ldo batch heads sq skv head_dim scale stream"
_IP = {" out": " k_ip ldk_ip vt_ip ldvt_ip out", " skv ": " skv skv_ip ", " scale": " scale ip_scale"}
_IP_X3 = {" out": " k_ip_hi k_ip_lo ldk_ip vt_ip_hi vt_ip_lo ldvt_ip out", " skv ": " skv skv_ip ", " scale": " scale ip_scale"}


def _sub(params, table):
    for old, new in table.items():
        assert params.count(old) == 1
        params = params.replace(old, new)
    return params


# entry -> its parameters in the order of include/mfhip.h
FORWARD = {
    "mf_attention_bf16": _16, "mf_attention_f16": _16, "mf_attention_causal_bf16": _16, "mf_attention_causal_f16": _16,
    "mf_attention_bf16_lse": _sub(_16, {" ldo": " ldo lse"}),
    "mf_attention_f16x3": _X3, "mf_attention_causal_f16x3": _X3, "mf_attention_f16x3_lse": _sub(_X3, {" ldo": " ldo lse"}),
    "mf_attention_ip_bf16": _sub(_16, _IP), "mf_attention_ip_f16": _sub(_16, _IP), "mf_attention_ip_f16x3": _sub(_X3, _IP_X3),
}
FORWARD = {name: params.split() for name, params in FORWARD.items()}
BACKWARD = ("mf_attention_bwd_f16x3", "mf_attention_bwd_bf16")
SPLIT = [e for e in FORWARD if e.endswith(("f16x3", "f16x3_lse"))]          # two planes per operand, fp32 out
CAUSAL = [e for e in FORWARD if "causal" in e]
IP = [e for e in FORWARD if "_ip_" in e]
FP32_OUT = [*SPLIT, *BACKWARD]                 # ldo may be any multiple of 4 (the backward's gradients: in both of its forms)
assert (len(FORWARD), len(SPLIT), len(CAUSAL), len(IP)) == (11, 4, 3, 3)

# rows of 192 elements hold every head dim probed below (up to 160); vt / vt_ip rows hold their keys
_SCALARS = dict(ldq=192, ldk=192, ldvt=64, ldk_ip=192, ldvt_ip=72, ldo=192, batch=1, heads=1, sq=48, skv=48, skv_ip=4, head_dim=8, scale=0.125,
                ip_scale=1.0, stream=None)
_BWD_SCALARS = dict(ldq=192, ldk=192, ldv=192, lddo=192, ldqt=64, ldkt=64, lddot=64, ldo=192, batch=1, heads=1, sq=48, skv=48, head_dim=8,
                    scale=0.125, out_dtype=0)
_BWD_POINTERS = [name for name, kind in hip.AttnBwdDesc._fields_ if kind is C.c_void_p]


def pointers(entry):
    """The pointer arguments an entry checks: lse of the forward may be NULL and is not among them, and the single-plane backward ignores
    the _lo planes."""
    if entry in FORWARD:
        return [p for p in FORWARD[entry] if p not in _SCALARS and p != "lse"]
    return [p for p in _BWD_POINTERS if entry == "mf_attention_bwd_f16x3" or not p.endswith("_lo")]


def leading_dims(entry):
    """The leading dimensions that must be multiples of 8 (an fp32 out, and the backward's gradients, need only 4: see FP32_OUT)."""
    names = FORWARD[entry] if entry in FORWARD else list(_BWD_SCALARS)
    return [p for p in names if p.startswith("ld") and not (p == "ldo" and entry in FP32_OUT)]


def refused(entry, **fault):
    """Call `entry` on the baseline with `fault` applied; returns (return code, message)."""
    assert fault, f"{entry}: a case needs a fault (the baseline would launch)"
    lib = hip.load()
    if entry in FORWARD:
        args = {p: _SCALARS.get(p, P16) for p in FORWARD[entry]}
        assert set(fault) <= set(args), f"{entry} has no {set(fault) - set(args)}"
        args.update(fault)
        rc = getattr(lib, entry)(*args.values())
    else:
        null_desc = fault.pop("d", 0) is None
        d = hip.AttnBwdDesc(**{**{p: P16 for p in _BWD_POINTERS}, **_BWD_SCALARS, **fault})
        rc = getattr(lib, entry)(None if null_desc else C.byref(d), None)
    return rc, lib.mf_last_error().decode()


def check(entry, rc, keyword, **fault):
    got, msg = refused(entry, **fault)
    assert got == rc and keyword in msg, f"{entry}({fault}) returned {got} with {msg!r}; expected {rc} and {keyword!r}"


ENTRIES = [*FORWARD, *BACKWARD]


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers(entry):
    planes = 2 if entry in SPLIT or entry == "mf_attention_bwd_f16x3" else 1
    assert len(pointers(entry)) == (7 * planes + 5 if entry in BACKWARD else (5 if entry in IP else 3) * planes + 1)
    for p in pointers(entry):
        check(entry, EINVAL, "null pointer", **{p: None})
    if entry in BACKWARD:
        check(entry, EINVAL, "null pointer", d=None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_misaligned_pointers(entry):
    for p in pointers(entry):
        check(entry, EALIGN, "aligned", **{p: P16 + 8})


@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_sizes(entry):
    for size in ("batch", "heads", "sq", "skv"):
        check(entry, EINVAL, "bad sizes", **{size: 0})


@pytest.mark.parametrize("entry", ENTRIES)
def test_leading_dims(entry):
    lds = leading_dims(entry)
    assert len(lds) == (7 if entry in BACKWARD else 3 + (entry not in SPLIT) + 2 * (entry in IP))
    for ld in lds:
        check(entry, EINVAL, "leading dims", **{ld: 60})          # 60 is above every sequence of the baseline: the one fault is 60 % 8
    if entry in FP32_OUT:
        check(entry, EINVAL, "leading dims", ldo=62)
    if entry in FORWARD:
        check(entry, EINVAL, "leading dims", sq=64, skv=64, ldvt=56)


@pytest.mark.parametrize("entry", CAUSAL)
def test_causal_needs_square_scores(entry):
    check(entry, EINVAL, "sq == skv", sq=64, skv=80, ldvt=80)


@pytest.mark.parametrize("entry", IP)
def test_ip_segment(entry):
    for n in (0, 65):
        check(entry, EINVAL, "skv_ip", skv_ip=n)
    check(entry, EINVAL, "leading dims", skv_ip=9, ldvt_ip=8)


def head_dims(entry):
    if entry in BACKWARD:
        return ops.FLASH_BWD_HEAD_DIMS if entry == "mf_attention_bwd_f16x3" else ops.FLASH_BWD_BF16_HEAD_DIMS
    return ops.FLASH_CAUSAL_HEAD_DIMS if entry in CAUSAL else ops.FLASH_SPLIT_HEAD_DIMS if entry in SPLIT else ops.FLASH_HEAD_DIMS


@pytest.mark.parametrize("entry", ENTRIES)
def test_unsupported_head_dims(entry):
    """Only the dims outside the tuple are probed (one inside would launch); tests/test_attention_gpu.py and test_training_gpu.py run
    those."""
    have = head_dims(entry)
    assert set(have) <= set(range(8, 161, 8)) and _SCALARS["head_dim"] in have
    for d in range(8, 161, 8):
        if d not in have:
            check(entry, EINVAL, f"unsupported head_dim {d} ", head_dim=d)


@pytest.mark.parametrize("entry", BACKWARD)
def test_backward_transposed_rows_and_sq(entry):
    for fault in (dict(ldqt=40), dict(lddot=40), dict(ldkt=40), dict(sq=62)):
        check(entry, EINVAL, "", **fault)


def test_rowdot_entries():
    lib = hip.load()
    # a, b, out, batch, sq, heads, head_dim, ld, stream
    for fn, b_off in ((lib.mf_rowdot_heads, 8), (lib.mf_rowdot_heads_bf16, 4)):
        assert fn(P16, P16, P16, 1, 48, 2, 6, 64, None) == EINVAL
        assert fn(P16, P16, P16, 1, 48, 1, 4, 6, None) == EINVAL
        assert fn(P16, P16 + b_off, P16, 1, 48, 2, 8, 64, None) == EALIGN
    # a, b16, a16, out, batch, sq, heads, head_dim, stream
    assert lib.mf_rowdot_heads_cast(P16, P16, P16, P16, 1, 48, 2, 12, None) == EINVAL
    assert lib.mf_rowdot_heads_cast(P16, P16, P16 + 8, P16, 1, 48, 2, 8, None) == EALIGN
