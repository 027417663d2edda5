"""CPU proof that tests/attention_bwd_ref.py has teeth: the arithmetic model of the flash-attention backward stays inside the derived
bound on every case tests/test_attention_bwd_gpu.py runs, each modelled kernel mistake leaves the bound by a factor of 4 or more on a
case named for it, the explicit formulas are autograd's, the input and gradient families are what they say, and the range-guard cases
sit on their side of the fp16 maximum with the stated margin."""
import math

import pytest
import torch

import attention_bwd_ref as R
from attention_bwd_ref import HEADS


def model(flavour, d, family, grad, sq, skv, fault=None, **kw):
    """(max err/B of dq, dk, dv) of the arithmetic model, and its guard maxima."""
    c = R.case(flavour, d, family, grad, sq, skv)
    dq, dk, dv, guard = R.emulate_bwd(c.q, c.k, c.v, c.do, c.lse, c.dd, HEADS, c.scale, flavour, fault, **kw)
    r = [float(R.ratio(g, w, b).max()) for g, w, b in zip((dq, dk, dv), (c.ref.dq, c.ref.dk, c.ref.dv), c.bound)]
    return r, guard, (dq, dk, dv)


@pytest.mark.parametrize("grad", R.GRADS)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("flavour,d", R.ENTRY_DIMS)
def test_correct_model_is_inside_the_bound(flavour, d, family, grad):
    for sq, skv in R.SHAPES:
        r, _, out = model(flavour, d, family, grad, sq, skv)
        assert not any(bool(torch.isnan(t).any()) for t in out)
        print(f"model[{flavour}, d{d}, {family}, {grad}, {sq}x{skv}]: worst err/B dq {r[0]:.3f} dk {r[1]:.3f} dv {r[2]:.3f}")
        assert max(r) <= 1.0


@pytest.mark.parametrize("flavour,d", [("f16x3", 40), ("bf16", 40), ("bf16", 80)])
def test_correct_model_is_inside_the_bound_on_the_other_shapes(flavour, d):
    """(68, 300) and (256, 256), and the decoy layout of test_layout_and_decoys: pads of 1e4 and longer transposed rows change no bit."""
    for sq, skv in (R.RAGGED[2], R.EVEN):
        for family, grad in (("peaked", "dense"), ("all_negative", "aligned")):
            r, _, out = model(flavour, d, family, grad, sq, skv)
            assert max(r) <= 1.0, (sq, skv, family, r)
            ld = lambda s_: -(-s_ // 8) * 8 + 8
            decoy = model(flavour, d, family, grad, sq, skv, ldqt=ld(sq), ldkt=ld(skv), pad=1e4)[2]
            assert all(torch.equal(a, b_) for a, b_ in zip(out, decoy))


# the cases that must expose each fault: (flavour, d, input family, dO family, sq, skv)
FAULT_CASES = {
    "no_D": [("f16x3", 40, "peaked", "aligned", 324, 77), ("bf16", 40, "dense", "aligned", 324, 333)],
    "lse_natural_log": [("f16x3", 8, "all_negative", "dense", 324, 77), ("bf16", 40, "peaked", "dense", 324, 333)],
    "tail_queries_unmasked": [("f16x3", 40, "all_negative", "dense", 324, 77), ("bf16", 8, "flat", "dense", 324, 333)],
    "tail_keys_unmasked": [("f16x3", 40, "all_negative", "dense", 324, 77), ("bf16", 40, "flat", "dense", 324, 333)],
    "drop_tile": [("f16x3", 40, "dense", "dense", 324, 77), ("bf16", 40, "flat", "sparse_rows", 324, 333)],
    "pshift_not_undone": [("f16x3", 8, "dense", "dense", 324, 77), ("f16x3", 40, "peaked", "aligned", 324, 333)],
    "dd_wrong_layout": [("f16x3", 40, "dense", "aligned", 324, 77), ("bf16", 80, "peaked", "aligned", 324, 333)],
    "scale_missing": [("f16x3", 8, "dense", "dense", 324, 77), ("bf16", 40, "all_negative", "sparse_rows", 324, 333)],
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_faults_are_caught(fault):
    assert sorted(FAULT_CASES) == sorted(R.FAULTS)
    for cs in FAULT_CASES[fault]:
        assert cs[:2] in R.ENTRY_DIMS and cs[2] in R.FAMILIES and cs[3] in R.GRADS and cs[4:] in R.SHAPES      # a case the GPU file runs
        r, _, _ = model(*cs, fault=fault)
        print(f"{fault}{list(cs)}: worst err/B dq {r[0]:.3g} dk {r[1]:.3g} dv {r[2]:.3g}")
        assert max(r) >= 4.0, (fault, cs, r)


def test_explicit_formulas_are_autograd():
    for family, grad in (("peaked", "aligned"), ("dense", "dense")):
        c = R.case("bf16", 40, family, grad, 68, 300)
        q, k, v = (t.clone().requires_grad_(True) for t in (c.q, c.k, c.v))
        q4, k4, v4 = (R.split_heads(t, HEADS) for t in (q, k, v))
        o = R.merge_heads(torch.softmax(q4 @ k4.transpose(-1, -2) * c.scale, -1) @ v4)
        o.backward(c.do)
        for name, got, want in (("dq", c.ref.dq, q.grad), ("dk", c.ref.dk, k.grad), ("dv", c.ref.dv, v.grad)):
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name
        assert float((c.ref.o - o.detach()).abs().max()) < 1e-13
        assert float((c.ref.dS.sum(-1)).abs().max()) < 1e-12                       # rows of dS sum to zero: D is the right one


def test_inputs_have_teeth():
    for d in (8, 40):
        for sq, skv in R.SHAPES:
            ref = R.case("f16x3", d, "peaked", "aligned", sq, skv).ref
            wmax, hot = ref.w.max(-1)
            peaked = wmax > 0.9
            frac = float(peaked.double().mean())
            # attention_ref's `peaked` aims every query at THREE keys of nearly equal amplitude, which share the weight unless the keys'
            # own overlap separates them: 0.22 (d 40, 333 keys) to 0.46 (d 8, 77 keys) of the rows are held by one key, not half of them;
            # 60 and more rows of every (batch, head), spread over every wave and tile, is what the peaked-row checks below stand on
            print(f"peaked d{d} {sq}x{skv}: {100 * frac:.0f} % of the rows have a weight above 0.9, |s|max {float(ref.s.abs().max()):.1f}")
            assert frac >= 0.2 and int(peaked.sum(-1).min()) >= 60
            assert float(ref.s.abs().max()) > 15.0
            # aligned: D = dO.o is large and dP - D cancels at the key that holds the row.  (Over ALL keys of a row the median of
            # |dP - D| is |D| itself — the other keys' dP is noise — so the cancellation is looked at where the weight is.)
            at_hot = (ref.dP.gather(-1, hot[..., None])[..., 0] - ref.D).abs()
            margin = ref.D.abs()[peaked] / at_hot[peaked]
            print(f"aligned d{d} {sq}x{skv}: |D| / |dP - D| at the hot key of a peaked row: median {float(margin.median()):.1f}, "
                  f"min {float(margin.min()):.1f}")
            assert float(margin.median()) > 5.0 and float(ref.D.abs()[peaked].min()) > 1.0
            lse2 = R.case("f16x3", d, "all_negative", "dense", sq, skv).ref.lse2
            assert float(lse2.max()) < -15.0
            flat = R.case("f16x3", d, "flat", "dense", sq, skv).ref
            assert float((flat.w - 1.0 / skv).abs().max()) < 1e-15
            sparse = R.case("f16x3", d, "dense", "sparse_rows", sq, skv).do
            assert int((sparse.abs().sum(-1) > 0).sum(-1).max()) == -(-sq // 37)


@pytest.mark.parametrize("d,family,grad,sq,skv", R.GUARD_QUIET)
def test_guard_quiet_cases_are_16x_inside_the_fp16_range(d, family, grad, sq, skv):
    """No real (query, key) pair comes near the range: 2^pshift |dS| (scale left out: the larger figure) is below 65504 / 16 — it is at most
    about 90 — while the model's ghost lanes of the dK / dV pass, which the kernel never stores, hold far more than 65504 on
    all_negative: exp2(pshift - lse2) |D| scale with lse2 near -20."""
    c = R.case("f16x3", d, family, grad, sq, skv)
    scaled, unscaled = R.real_pair_max(c.ref, c.scale, skv, "f16x3")
    _, (real, ghost), _ = model("f16x3", d, family, grad, sq, skv)
    print(f"guard quiet[d{d}, {family}, {grad}, {sq}x{skv}]: real pairs {unscaled:.3g} (with scale {scaled:.3g}, model {real:.3g}), ghost lanes {ghost:.3g}")
    assert unscaled < R.F16_MAX / 16 and real < R.F16_MAX / 16
    assert abs(real - scaled) <= 1e-4 * scaled
    assert skv % 256 != 0
    if family == "all_negative":
        assert ghost > 100 * R.F16_MAX


@pytest.mark.parametrize("d,family,grad,sq,skv", R.GUARD_LOUD)
def test_guard_loud_cases_are_4x_outside_the_fp16_range(d, family, grad, sq, skv):
    """dO times a power of two until the guarded quantity scale 2^pshift |dS| of a REAL pair is past 4 x 65504, while dO itself (an operand
    that is split as well) stays 2 x inside the range."""
    gain = R.loud_gain(d, family, grad, sq, skv)
    c = R.case("f16x3", d, family, grad, sq, skv, gain)
    scaled, _ = R.real_pair_max(c.ref, c.scale, skv, "f16x3")
    print(f"guard loud[d{d}, {family}, {grad}, {sq}x{skv}]: gain {gain:g}, real pairs {scaled:.3g}, |dO| max {float(c.do.abs().max()):.3g}")
    assert math.log2(gain) == int(math.log2(gain))
    assert scaled > 4 * R.F16_MAX
    assert float(c.do.abs().max()) < R.F16_MAX / 2
