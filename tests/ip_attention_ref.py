"""float64 reference and per-element bound of decoupled cross-attention (csrc/attention.hip, the IP instantiations of attn_fwd_kernel;
mf_attention_ip_*):

    o = o_text + s o_ip,    o_text = softmax(q k^T scale) v,    o_ip = softmax(q k_ip^T scale) v_ip       (s = ip_scale)

A helper on top of tests/attention_ref.py (`A`): no test functions here.  tests/test_ip_attention_reference_cpu.py shows on the CPU that
the cases below tell a correct kernel from three wrong ones; tests/test_ip_attention_gpu.py holds the kernels to the bound.

Bound, per element, factor 1, no atol:

    B = A.bound(text) + |s| A.bound(ip) + u_O |o| + a_O + 2^-23 (|o_text| + |s o_ip|)

Each segment is an attention of its own, so its error is the one A.bound derives for a launch on those operands (the ip segment's
scaled by |s|).  The sum is formed in fp32: one rounding of s o_ip and one of the sum, each at most 2^-24 of a term no larger than
|o_text| + |s o_ip|, together 2^-23 (|o_text| + |s o_ip|).  The stored result is rounded once more: u_O |o| + a_O (A.units).  This covers
the fused kernel (which rounds to storage once, so it uses less than the bound grants) and the composition of two launches and an
fp32 combine (whose two stored 16-bit results are inside the A.bound terms).  Derived, not tuned."""
import math

import torch

import attention_ref as A

PAIRS = (("peaked", "all_negative"), ("all_negative", "peaked"), ("stairs_up", "late_spike"), ("flat", "early_spike"), ("late_spike", "flat"))
SHAPES = ((33, 74, 4, 1.0), (130, 64, 1, 0.6), (40, 77, 16, -0.5), (128, 65, 64, 1.0), (200, 73, 5, 0.0))       # sq, skv, skv_ip, ip_scale
DIMS = {"bf16": (8, 40, 64, 80, 160), "fp16": (8, 40, 64, 80, 160), "f16x3": (8, 40, 64, 80)}
FAULTS = ("joint_softmax", "ip_scale_dropped", "ip_tail_unmasked")
B, HEADS = 2, 3


def seed_of(d, sq, skv, skv_ip):
    return 11 + 31 * d + 1000 * sq + skv + 100000 * skv_ip


def make_inputs(pair, b, heads, sq, skv, skv_ip, d, rnd):
    """(q, k, v, k_ip, v_ip) float64, rounded to storage: the text segment is family pair[0]; the ip keys and values are the k, v of
    family pair[1] at skv_ip keys under another seed (its queries are not used: q is the text family's)."""
    seed = seed_of(d, sq, skv, skv_ip)
    q, k, v = A.make_inputs(pair[0], b, heads, sq, skv, d, seed, rnd)
    _, k_ip, v_ip = A.make_inputs(pair[1], b, heads, sq, skv_ip, d, seed + 7, rnd)
    return q, k, v, k_ip, v_ip


def reference(q, k, v, k_ip, v_ip, heads, scale, s):
    """(o, ref_text, ref_ip): o float64 [B, sq, C] and the two A.reference tuples."""
    rt, ri = A.reference(q, k, v, heads, scale), A.reference(q, k_ip, v_ip, heads, scale)
    return rt[0] + s * ri[0], rt, ri


def bound(q, k, v, k_ip, v_ip, heads, scale, s, ref, flavour):
    o, rt, ri = ref
    d = q.shape[-1] // heads
    _, _, u_o, _, a_o = A.units(flavour, d)
    bt, _ = A.bound(q, k, v, heads, scale, rt, flavour)
    bi, _ = A.bound(q, k_ip, v_ip, heads, scale, ri, flavour)
    return bt + abs(s) * bi + u_o * o.abs() + a_o + 2.0 ** -23 * (rt[0].abs() + (s * ri[0]).abs())


def plain_bound_s0(q, k, v, heads, scale, ref_text, flavour):
    """ip_scale = 0: the plain launch's bound plus one more rounding of the stored output."""
    d = q.shape[-1] // heads
    _, _, u_o, _, a_o = A.units(flavour, d)
    return A.bound(q, k, v, heads, scale, ref_text, flavour)[0] + u_o * ref_text[0].abs() + a_o


def model(q, k, v, k_ip, v_ip, heads, scale, s, flavour, fault=None):
    """Two emulated launches (A.emulate), an fp32 combine and the storage rounding; `fault`: the arithmetic of a kernel with that mistake."""
    assert fault is None or fault in FAULTS
    if fault == "joint_softmax":          # one softmax over cat(k, k_ip), the ip values scaled
        o, _ = A.emulate(q, torch.cat([k, k_ip], 1), torch.cat([v, s * v_ip], 1), heads, scale, False, flavour)
        return o
    ot, _ = A.emulate(q, k, v, heads, scale, False, flavour)
    oi, _ = A.emulate(q, k_ip, v_ip, heads, scale, False, flavour, fault="tail_unmasked" if fault == "ip_tail_unmasked" else None)
    s_used = 1.0 if fault == "ip_scale_dropped" else s
    f32 = lambda x: x.float().double()
    out = f32(ot + f32(s_used * oi))
    return A._r16(out, flavour) if flavour in ("bf16", "fp16") else out


def ratio(got, ref_o, bnd):
    return float(((got - ref_o).abs() / bnd).nan_to_num(math.inf).max())
