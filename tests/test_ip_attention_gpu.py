"""Decoupled cross-attention (mf_attention_ip_bf16 / _f16 / _f16x3, and ops.attention(ip=...)) through the C ABI against float64:
tests/ip_attention_ref.py holds the reference o = o_text + s o_ip, the per-element bound (factor 1, no atol) and the cases;
tests/test_ip_attention_reference_cpu.py shows on the CPU that the cases catch a joint softmax, a dropped ip_scale and an unmasked ip tail.

As in tests/test_attention_gpu.py: B = 2, heads = 3, gap columns on q, k, k_ip and out, a sentinel-filled and guarded output, and every
case is launched twice and must be bit-reproducible.  No case is skipped and no element is excluded."""
import math
import os
import sys

import pytest
import torch

import attention_ref as A
import ip_attention_ref as I
from test_attention_gpu import Buf, Out, cols, planes, rows_tensor, seen, vt_tensor  # noqa: F401  (Buf: the guarded buffers behind Out)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from reflecting_reality_amd import hip, ops  # noqa: E402

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
B, HEADS = I.B, I.HEADS
STORE = {"bf16": torch.bfloat16, "fp16": torch.float16, "f16x3": torch.float32}
FLAVOUR_DIMS = [(fl, d) for fl in A.FLAVOURS for d in I.DIMS[fl]]


def launch(flavour, qp, kp, vp, kip, vip, out, *, ldq, ldk, ldvt, ldk_ip, ldvt_ip, sq, skv, skv_ip, d, s):
    fn = hip.attention_ip_f16x3 if flavour == "f16x3" else hip.attention_ip_bf16
    fn(qp, kp, vp, kip, vip, out.tensor(), ldq=ldq, ldk=ldk, ldvt=ldvt, ldk_ip=ldk_ip, ldvt_ip=ldvt_ip, ldo=out.ldo, batch=B, heads=HEADS,
       sq=sq, skv=skv, skv_ip=skv_ip, head_dim=d, scale=d ** -0.5, ip_scale=s)
    torch.cuda.synchronize()


class Case:
    """Device operands of one (flavour, d, pair, shape) with gap columns, and the float64 values the kernel reads."""

    def __init__(self, flavour, d, pair, sq, skv, skv_ip, k_ip_extra_rows=0, vt_ip_ld=None, hot_next_batch=False):
        self.flavour, self.d, self.sq, self.skv, self.skv_ip = flavour, d, sq, skv, skv_ip
        c = self.c = HEADS * d
        dt = STORE[flavour]
        q64, k64, v64, ki64, vi64 = I.make_inputs(pair, B, HEADS, sq, skv, skv_ip, d, flavour)
        if hot_next_batch:
            # the rows behind batch 0's ip keys inside its 64-key tile ARE batch 1's ip keys: make them score 3 |q| for batch 0's
            # queries (for batch 1 they are ordinary keys).  A tail mask taken from skv instead of skv_ip would let them in.
            hot = 3.0 * math.sqrt(d) * q64 / A.split_heads(q64, HEADS).norm(dim=-1).transpose(1, 2).repeat_interleave(d, -1)
            ki64[1, :] = A.stored(hot[0, :skv_ip], flavour)
        self.ldq, self.ldk, self.ldk_ip = c + 8, c + 16, c + 24
        self.ldvt, self.ldvt_ip = (skv + 7) // 8 * 8, vt_ip_ld or (skv_ip + 7) // 8 * 8
        self.k_ip_t = rows_tensor(ki64, self.ldk_ip, dt, extra_rows=k_ip_extra_rows)
        self.vt_ip_t = vt_tensor(vi64, self.ldvt_ip, dt)
        self.qp, self.kp = planes(rows_tensor(q64, self.ldq, dt), flavour), planes(rows_tensor(k64, self.ldk, dt), flavour)
        self.vp, self.kip, self.vip = planes(vt_tensor(v64, self.ldvt, dt), flavour), planes(self.k_ip_t, flavour), planes(self.vt_ip_t, flavour)
        rows = lambda p, n: seen(cols(p, 0, c), flavour)[: B * n].reshape(B, n, c)
        self.seen = (rows(self.qp, sq), rows(self.kp, skv), seen(self.vp, flavour)[:, :, :skv].transpose(1, 2),
                     rows(self.kip, skv_ip), seen(self.vip, flavour)[:, :, :skv_ip].transpose(1, 2))

    def run(self, s, kip=None, vip=None):
        out = Out(self.flavour, self.sq, self.c)
        launch(self.flavour, self.qp, self.kp, self.vp, kip if kip is not None else self.kip, vip if vip is not None else self.vip, out,
               ldq=self.ldq, ldk=self.ldk, ldvt=self.ldvt, ldk_ip=self.ldk_ip, ldvt_ip=self.ldvt_ip, sq=self.sq, skv=self.skv,
               skv_ip=self.skv_ip, d=self.d, s=s)
        out.untouched()
        return out


def held(name, got, ops64, d, s, units):
    """Failure messages (empty: inside the bound) of `got` against the float64 reference of the operands `ops64`."""
    scale = d ** -0.5
    ref = I.reference(*ops64, HEADS, scale, s)
    bnd = I.bound(*ops64, HEADS, scale, s, ref, units)
    err = (got - ref[0]).abs()
    worst = I.ratio(got, ref[0], bnd)
    print(f"{name}: worst err/B {worst:.3f}, rms err/B {float((err / bnd).pow(2).mean().sqrt()):.3f}, |o|max {float(ref[0].abs().max()):.2f}")
    bad = []
    if not bool((err <= bnd).all()):
        bad.append(f"{name}: {int((~(err <= bnd)).sum())} of {got.numel()} outputs outside B, worst err/B {worst:.3g}")
    if s == 0.0:       # nothing of the ip segment may reach the result: the plain launch's bound and one more output rounding
        plain = I.plain_bound_s0(*ops64[:3], HEADS, scale, ref[1], units)
        if not bool((err <= plain).all()):
            bad.append(f"{name}: ip_scale = 0 leaves the plain bound, worst err/B {I.ratio(got, ref[0], plain):.3g}")
    return bad


@pytest.mark.parametrize("pair", I.PAIRS, ids=lambda p: "-".join(p))
@pytest.mark.parametrize("flavour,d", FLAVOUR_DIMS)
def test_flavours(flavour, d, pair):
    bad = []
    for sq, skv, skv_ip, s in I.SHAPES:
        name = f"ip[{flavour}, d{d}, {pair[0]}+{pair[1]}, {sq}x{skv}+{skv_ip}, s={s}]"
        case = Case(flavour, d, pair, sq, skv, skv_ip)
        o1, o2 = case.run(s), case.run(s)
        got = o1.values().to(DEV)
        bad += held(name, got, case.seen, d, s, flavour)
        if not torch.equal(o1.buf.bytes, o2.buf.bytes):
            bad.append(f"{name}: two launches differ")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("skv_ip", [4, 5, 33])
@pytest.mark.parametrize("flavour,d", [("bf16", 40), ("bf16", 160), ("fp16", 80), ("f16x3", 40), ("f16x3", 64)])
def test_decoys_past_skv_ip(flavour, d, skv_ip):
    """What lies past skv_ip must not count.  (1) Inside batch 0's key tile the rows past skv_ip are batch 1's ip keys, made hot for
    batch 0's queries here: the result must still meet the bound of the float64 reference, which gives batch 0 its own skv_ip keys only
    (a tail mask on skv, or none, fails it).  (2) Rows behind the LAST batch hold NaN (the kernel never reads them: outside the buffer
    descriptor; they must at least not be required) and the pad columns of vt_ip hold 1e30 — in the fp16 operand types, whose largest
    finite value is smaller, 65504: include/mfhip.h asks for finite pad columns; they meet probabilities that are exact zeros.  The
    result of (2) is bit-identical to the clean launch's."""
    sq, skv, s = 130, 74, 0.7
    case = Case(flavour, d, ("peaked", "stairs_up"), sq, skv, skv_ip, k_ip_extra_rows=64, vt_ip_ld=(skv_ip + 64 + 7) // 8 * 8,
                hot_next_batch=True)
    clean = case.run(s)
    big = 1e30 if flavour == "bf16" else 65504.0
    as_planes = lambda t: tuple(t) if isinstance(t, tuple) else (t,)
    kip, vip = tuple(x.clone() for x in as_planes(case.kip)), tuple(x.clone() for x in as_planes(case.vip))
    for x in kip:
        x[B * skv_ip:] = math.nan
    for x in vip:
        x[:, :, skv_ip:] = big
    kip, vip = (kip, vip) if flavour == "f16x3" else (kip[0], vip[0])
    dirty = case.run(s, kip=kip, vip=vip)
    assert not bool(torch.isnan(dirty.values()).any())
    assert torch.equal(clean.buf.bytes, dirty.buf.bytes)
    bad = held(f"decoy[{flavour}, d{d}, +{skv_ip}]", dirty.values().to(DEV), case.seen, d, s, flavour)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("skv_ip", [0, 65])
@pytest.mark.parametrize("flavour", A.FLAVOURS)
def test_skv_ip_out_of_range_is_einval(flavour, skv_ip):
    d, sq, skv = 40, 33, 74
    case = Case(flavour, d, ("peaked", "flat"), sq, skv, 64)
    out = Out(flavour, sq, case.c)
    lib = hip.load()
    tail = (B, HEADS, sq, skv, skv_ip, d, d ** -0.5, 1.0, None)
    if flavour == "f16x3":
        args = (case.qp[0], case.qp[1], case.ldq, case.kp[0], case.kp[1], case.ldk, case.vp[0], case.vp[1], case.ldvt, case.kip[0], case.kip[1],
                case.ldk_ip, case.vip[0], case.vip[1], case.ldvt_ip, out.tensor(), out.ldo)
        fn = lib.mf_attention_ip_f16x3
    else:
        args = (case.qp, case.ldq, case.kp, case.ldk, case.vp, case.ldvt, case.kip, case.ldk_ip, case.vip, case.ldvt_ip, out.tensor(), out.ldo)
        fn = lib.mf_attention_ip_f16 if flavour == "fp16" else lib.mf_attention_ip_bf16
    rc = fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], *tail)
    torch.cuda.synchronize()
    assert rc == -1, f"MF_EINVAL (-1) expected for skv_ip = {skv_ip}, got {rc}"          # include/mfhip.h MF_EINVAL
    assert "skv_ip" in lib.mf_last_error().decode()
    out.untouched()
    assert bool((out.buf.bytes == 0x7B).all()), "a refused launch wrote the output"
    with pytest.raises(hip.MfhipError):
        launch(flavour, case.qp, case.kp, case.vp, case.kip, case.vip, out, ldq=case.ldq, ldk=case.ldk, ldvt=case.ldvt, ldk_ip=case.ldk_ip,
               ldvt_ip=case.ldvt_ip, sq=sq, skv=skv, skv_ip=skv_ip, d=d, s=1.0)


# (precision, head dim, units of the bound): the composition path (two unfused attentions and an fp32 combine) for fp32 and for f16x3 at
# head dim 160, and the fused entries as ops.attention reaches them
DISPATCH = [("fp32", 40, "fp32"), ("fp32", 160, "fp32"), ("f16x3", 160, "f16x3_unfused"), ("f16x3", 40, "f16x3"), ("bf16", 80, "bf16"),
            ("fp16", 160, "fp16")]


@pytest.mark.parametrize("pair", I.PAIRS, ids=lambda p: "-".join(p))
@pytest.mark.parametrize("prec_name,d,units", DISPATCH)
def test_dispatcher(prec_name, d, units, pair):
    prec = ops.Precision.get(prec_name)
    c = HEADS * d
    rnd = {"f16x3": "f16x3", "fp32": "f32", "bf16": "bf16", "fp16": "fp16"}[prec_name]
    bad = []
    for sq, skv, skv_ip, s in I.SHAPES:
        q64, k64, v64, ki64, vi64 = I.make_inputs(pair, B, HEADS, sq, skv, skv_ip, d, rnd)

        def vt_of(v, n):
            t = torch.zeros(B, c, (n + 7) // 8 * 8, dtype=prec.act, device=DEV)
            t[:, :, :n] = v.transpose(1, 2).to(DEV, prec.act)
            return t
        q, k, ki = (t.to(DEV, prec.act) for t in (q64, k64, ki64))
        vt, vti = vt_of(v64, skv), vt_of(vi64, skv_ip)
        o1 = ops.attention(q, k, vt, HEADS, skv, d ** -0.5, prec, ip=(ki, vti, skv_ip, s))
        o2 = ops.attention(q, k, vt, HEADS, skv, d ** -0.5, prec, ip=(ki, vti, skv_ip, s))
        torch.cuda.synchronize()
        assert o1.shape == (B, sq, c) and o1.dtype == (prec.compute if prec.half else torch.float32)
        name = f"dispatch[{prec_name}, d{d}, {pair[0]}+{pair[1]}, {sq}x{skv}+{skv_ip}, s={s}]"
        bad += held(name, o1.double(), (q.double(), k.double(), v64.to(DEV), ki.double(), vi64.to(DEV)), d, s, units)
        if not torch.equal(o1, o2):
            bad.append(f"{name}: two calls differ")
    assert not bad, "\n".join(bad)


def test_dispatcher_refuses_training_and_causal():
    prec = ops.Precision.get("bf16")
    q = torch.zeros(1, 8, 24, dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(1, 24, 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(hip.MfhipError, match="inference only"):
        ops.attention(q, q, vt, 3, 8, 1.0, prec, causal=True, ip=(q, vt, 4, 1.0))
    assert ops.TAPE is None
    ops.TAPE = object()                       # a training step is being recorded: the ip branch has no backward pass
    try:
        with pytest.raises(hip.MfhipError, match="inference only"):
            ops.attention(q, q, vt, 3, 8, 1.0, prec, ip=(q, vt, 4, 1.0))
    finally:
        ops.TAPE = None
    assert ops.attention(q, q, vt, 3, 8, 1.0, prec, ip=(q, vt, 4, 1.0)).shape == (1, 8, 24)
