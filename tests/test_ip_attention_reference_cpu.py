"""The cases of tests/ip_attention_ref.py have teeth, shown on the CPU: a float64 model of the decoupled cross-attention (two emulated
launches, an fp32 combine, the storage rounding) stays inside the bound B on every (family pair, shape), and each of three wrong kernels
— one joint softmax over cat(k, k_ip), ip_scale dropped, the ip tile's tail keys left unmasked — leaves B by a factor of 10 or more on at
least one of them, at every flavour and head dim."""
import pytest
import torch

import attention_ref as A
import ip_attention_ref as I

FLAVOUR_DIMS = [(fl, d) for fl in A.FLAVOURS for d in I.DIMS[fl]]
_CASES = {}


def cases(flavour, d):
    """Per (pair, shape): (operands, s, reference, bound), computed once per (flavour, d) and shared by the tests below."""
    key = (flavour, d)
    if key not in _CASES:
        out = []
        for pair in I.PAIRS:
            for sq, skv, skv_ip, s in I.SHAPES:
                ops = I.make_inputs(pair, I.B, I.HEADS, sq, skv, skv_ip, d, flavour)
                ref = I.reference(*ops, I.HEADS, d ** -0.5, s)
                out.append((pair, (sq, skv, skv_ip, s), ops, ref, I.bound(*ops, I.HEADS, d ** -0.5, s, ref, flavour)))
        _CASES[key] = out
    return _CASES[key]


@pytest.mark.parametrize("flavour,d", FLAVOUR_DIMS)
def test_model_inside_bound(flavour, d):
    worst = 0.0
    for pair, shape, ops, ref, bnd in cases(flavour, d):
        r = I.ratio(I.model(*ops, I.HEADS, d ** -0.5, shape[3], flavour), ref[0], bnd)
        worst = max(worst, r)
        assert r <= 1.0, f"{flavour} d{d} {pair} {shape}: the model's err/B is {r:.3f}"
    print(f"model[{flavour}, d{d}]: worst err/B {worst:.3f}")


@pytest.mark.parametrize("fault", I.FAULTS)
@pytest.mark.parametrize("flavour,d", FLAVOUR_DIMS)
def test_fault_outside_bound(flavour, d, fault):
    best = 0.0
    for pair, shape, ops, ref, bnd in cases(flavour, d):
        best = max(best, I.ratio(I.model(*ops, I.HEADS, d ** -0.5, shape[3], flavour, fault=fault), ref[0], bnd))
        if best >= 10.0:
            break
    print(f"{fault}[{flavour}, d{d}]: err/B {best:.1f}")
    assert best >= 10.0, f"{fault} at {flavour} d{d} stays within {best:.2f} B on every case: the cases cannot see it"


def test_scale_zero_is_the_plain_attention():
    """ip_scale = 0: the reference is the text attention alone, and B is at least the plain bound."""
    sq, skv, skv_ip, s = I.SHAPES[4]
    assert s == 0.0
    ops = I.make_inputs(I.PAIRS[0], I.B, I.HEADS, sq, skv, skv_ip, 40, "bf16")
    ref = I.reference(*ops, I.HEADS, 40 ** -0.5, s)
    assert torch.equal(ref[0], ref[1][0])
    plain = I.plain_bound_s0(*ops[:3], I.HEADS, 40 ** -0.5, ref[1], "bf16")
    assert bool((plain <= I.bound(*ops, I.HEADS, 40 ** -0.5, s, ref, "bf16")).all())
