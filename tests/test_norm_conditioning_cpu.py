"""The ladder, the yardstick and the bound of tests/norm_conditioning_ref.py, checked without a GPU — and that the bound has teeth:
a torch emulation of "unshifted fp32 (sum, sum of squares) per thread, double combine" (the scheme csrc/norm.hip used for its own
statistics) passes it on well-centred inputs, fails it once the mean dwarfs the spread, and passes everywhere with one pivot per
(image, group) subtracted before accumulating."""
import pytest
import torch

import norm_conditioning_ref as R
from norm_conditioning_ref import BF16, F16, F32

B, HW, C, G = 2, 1024, 640, 32
# fp32 output of mf_groupnorm in tests/test_groupnorm_streaming_gpu.py: check(..., 5 * 2e-5, 2e-5)
ATOL, RTOL = 1e-4, 2e-5


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_ladder_holds_distinct_values_signs_and_seeds(dtype):
    for name in R.ladder(dtype):
        x = R.gn_input(name, B, HW, C, G, dtype, 1)                  # (asserts the distinct-value condition itself)
        assert x.dtype == dtype and x.shape == (B, HW, C) and bool(torch.isfinite(x.float()).all())
        xg = x.float().view(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B * G, -1)
        if name == "constant":
            assert xg.unique().numel() == 1
            continue
        assert int(R.distinct_values(x, G).min()) >= R.MIN_DISTINCT
        assert len({tuple(u[:4].tolist()) for u in xg}) == B * G, "two (image, group) units drew the same values"
        mean, std = R.RUNGS[name]
        if mean and name != "outlier":
            signs = torch.sign(xg.mean(-1))
            assert (signs > 0).any() and (signs < 0).any(), f"{name}: every unit has the same sign of offset"
            ratio = (xg.mean(-1).abs() / xg.std(-1)).median().item()
            assert ratio >= 0.5 * mean / R.spread(name, dtype), f"{name} in {dtype}: |mean| / std = {ratio}"
    assert ("m300_tight" in R.ladder(dtype)) == (dtype == F32) and ("outlier" in R.ladder(dtype)) == (dtype != F16)
    rows = R.ln_input("m100", 77, 100, dtype, 2).float()
    assert (rows.mean(-1) > 0).any() and (rows.mean(-1) < 0).any()


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_yardstick_is_inside_the_bound_with_factor_one(dtype, silu):
    for name in R.ladder(dtype):
        x, gamma, beta, ref, yard = R.gn_case(name, B, HW, C, G, dtype, 1, silu)
        ok, e, ye = R.judge(f"yardstick {name} [{dtype}]", yard[0], ref[0], yard[0], ATOL, RTOL, factor=1.0)
        assert ok and e == ye
        for k in (1, 2):
            R.judge_rel(f"yardstick {name} stat {k}", yard[k], ref[k], yard[k], 2e-6, factor=1.0)
    x = R.ln_input("m100_tight", 77, 320, dtype, 3)
    gamma, beta = R.params(320, 3)
    R.judge("yardstick layernorm", R.ln(x, gamma, beta, F32), R.ln(x, gamma, beta, torch.float64), R.ln(x, gamma, beta, F32), 5e-5, 1e-5,
            factor=1.0)


def _emulated(name, shift):
    x, _, _, ref, yard = R.gn_case(name, B, HW, C, G, F32, 1, False)
    one, zero = torch.ones(C), torch.zeros(C)
    ref1 = R._gn(x, one, zero, G, False, torch.float64)
    yard1 = R._gn(x, one, zero, G, False, F32)
    y, _, _ = R.emulate_sums_groupnorm(x, G, per=16, shift=shift)
    return R.judge(f"emulated {'shifted' if shift else 'unshifted'} sums, {name}", y, ref1[0], yard1[0], ATOL, RTOL, fail=False)


def test_the_bound_has_teeth():
    for name in ("base", "m10"):
        assert _emulated(name, False)[0], f"unshifted sums should pass {name}"
    for name in ("m100_tight", "m300_tight"):
        ok, e, ye = _emulated(name, False)
        assert not ok and e > R.FACTOR * ye, f"unshifted sums should fail {name}: {e} vs yardstick {ye}"
    for name in R.ladder(F32):
        assert _emulated(name, True)[0], f"pivot-shifted sums should pass {name}"


def test_bound_arithmetic():
    ref = torch.tensor([0.0, 10.0, -100.0])
    assert torch.equal(R.bound(1e-4, 1e-5, 0.0, ref), torch.tensor([1e-4, 2e-4, 1.1e-3], dtype=torch.float64))
    assert torch.allclose(R.bound(1e-4, 1e-5, 1e-4, ref), torch.tensor([4e-4, 4e-4, 1.1e-3], dtype=torch.float64))
    assert R.bound(2e-5, 0.0, 1e-7) == 2e-5 and R.bound(2e-5, 0.0, 1e-5) == 4e-5
    assert R.spacing(BF16, 100.0) == 0.5 and R.spacing(F16, 100.0) == 2.0 ** -4 and R.spacing(F32, 300.0) == 2.0 ** -15
    ok, _, _ = R.judge("nan", torch.tensor([float("nan")]), torch.tensor([1.0]), None, 1.0, 1.0, fail=False)
    assert not ok
