"""tests/fp8_ref.py, the reference tests/test_fp8_audit_gpu.py holds csrc/fp8.hip to, checked here without a GPU: the e4m3
rounding against torch's own cast, the fp32 contract against the float64 definition, and the non-finite contract."""
import pytest
import torch

import fp8_ref as R


def test_e4m3_round_matches_torch_cast_on_every_bf16_pattern():
    """All 2^16 bf16 bit patterns, clamped to +-448 (torch's cast is round-to-nearest-even but does not saturate): value and sign
    of zero, NaN to NaN."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.bfloat16).float()
    xc = x.clamp(-448.0, 448.0)                                    # NaN stays NaN
    want = xc.to(torch.float8_e4m3fn)
    got = R.e4m3_round(x.double())
    nan = torch.isnan(x)
    assert bool(torch.isnan(got[nan]).all()) and bool(torch.isnan(want.float()[nan]).all())
    assert torch.equal(R.codes(got[~nan]), want.view(torch.uint8)[~nan])
    # every finite code is a fixed point, and decode inverts codes
    allc = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    fin = (allc & 0x7F) != 0x7F
    assert torch.equal(R.codes(R.e4m3_round(R.decode(allc[fin]))), allc[fin])


def test_e4m3_round_exact_ties_subnormals_and_saturation():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)          # noqa: E731
    assert R.e4m3_round(t(17.0, 19.0, -17.0, -19.0)).tolist() == [16.0, 20.0, -16.0, -20.0]
    assert R.e4m3_round(t(2.0 ** -10, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 2.0 ** -10 * (1 + 2.0 ** -30))).tolist() == \
        [0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -9]
    assert R.e4m3_round(t(448.0, 449.0, 464.0, 1e30, -1e30, float("inf"))).tolist() == [448.0, 448.0, 448.0, 448.0, -448.0, 448.0]
    assert R.e4m3_round(t(7.5 * 2.0 ** -9, 2.0 ** -6 * 1.0625)).tolist() == [2.0 ** -6, 2.0 ** -6]     # subnormal -> normal edge
    z = R.e4m3_round(t(-0.0, -2.0 ** -11))
    assert torch.equal(torch.signbit(z), torch.tensor([True, True])) and z.abs().max() == 0
    assert R.e4m3_spacing(t(0.0, 2.0 ** -7, 2.0 ** -6, 1.0, 1.99, 256.0, 448.0, 1e9)).tolist() == \
        [2.0 ** -9, 2.0 ** -9, 2.0 ** -9, 0.125, 0.125, 32.0, 32.0, 32.0]
    # every tie of tie_values() lies exactly between two codes and goes to the even one
    ties = R.tie_values()
    r = R.e4m3_round(ties)
    assert bool(((r - ties).abs() == 0.5 * R.e4m3_spacing(ties)).all())
    assert bool(((R.codes(r) & 1) == 0).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_contract_agrees_with_float64_on_the_gpu_tests_random_inputs(dt):
    """quantize_contract (fp32, the kernel's steps) against quantize_exact (float64) on every Gaussian input of the GPU test:
    with fp32 inputs no code differs (900 864 elements), the scales agree to 2^-22.  bf16 inputs have 8 significant bits, so
    x / amax * 448 lands EXACTLY on a tie for about one element in a thousand (999 here), and there the fp32 quotient, 1e-7 off,
    may fall to the other side: those differences, and only those, are allowed — one step, at an exact tie of the float64 y."""
    ndiff = total = 0
    worst = 0.0
    for rows, c in R.GAUSS_SHAPES:
        x = R.gauss(rows, c).to(dt)
        q, s = R.quantize_contract(x)
        qe, se, y = R.quantize_exact(x)
        d = q != qe
        ndiff += int(d.sum())
        total += q.numel()
        worst = max(worst, float(((s.double() - se) / se).abs().max()))
        assert bool(R.one_step(q[d], qe[d]).all()) and bool(R.near_tie(y[d], 2.0 ** -40).all())
    print(f"contract vs float64 ({dt}): {ndiff} of {total} codes differ, scales differ by {worst:.2e} relative")
    assert total == 900864
    assert ndiff == 0 if dt == torch.float32 else ndiff <= 2e-3 * total
    assert worst <= 2.0 ** -22


@pytest.mark.parametrize("c", [8, 264, 2056, 4104])
def test_contract_on_the_special_rows(c):
    x = R.special_rows(c)
    q, s = R.quantize_contract(x)
    qe, se, y = R.quantize_exact(x)
    name = {n: i for i, n in enumerate(R.SPECIAL)}
    for n in ("ties", "ties_shifted", "subnormal_targets"):
        i = name[n]
        assert float(s[i]) == 1.0, n                               # amax 448: 448 * fl(1 / 448) rounds to 1
        assert torch.equal(q[i], qe[i]) and torch.equal(R.decode(q[i]), R.e4m3_round(x[i].double()))
        assert bool(((q[i] & 1) == 0).all()), n                   # every element a tie (or +-448): all codes even
    i = name["zero"]
    assert float(s[i]) == 1.0 and int(q[i].max()) == 0
    i = name["neg_zero"]
    assert bool((q[i][::2] == 0x80).all())
    i = name["amax_min_normal"]                                    # 2^-126 -> +-448, halves and quarters follow; zeros stay zeros
    assert bool(torch.isfinite(s[i])) and float(s[i]) > 0
    assert R.decode(q[i][:8]).tolist() == [448.0, -224.0, 112.0, 0.0, -320.0, -448.0, 224.0, -0.0]
    i = name["amax_3e38"]
    assert bool(torch.isfinite(s[i])) and int(R.decode(q[i]).abs().max()) == 448
    # the fp32 contract may differ from float64 only at a near-tie; on these rows nowhere except where the scale itself is denormal
    keep = torch.tensor([n != "amax_min_normal" for n in R.SPECIAL])
    assert torch.equal(q[keep], qe[keep])
    bf = x.to(torch.bfloat16)
    for n in ("ties", "ties_shifted", "subnormal_targets", "amax_min_normal", "zero"):
        assert torch.equal(bf[name[n]].float(), x[name[n]]), f"{n} is not exact in bf16"


def test_contract_non_finite_rows():
    x = R.gauss(6, 64).clone()
    x[1, 5] = float("nan")
    x[3, 63] = float("inf")
    x[4, 0] = float("-inf")
    q, s = R.quantize_contract(x)
    qe, se, _ = R.quantize_exact(x)
    assert torch.isnan(s).tolist() == [False, True, False, True, True, False] == torch.isnan(se).tolist()
    assert bool((q[[1, 3, 4]] == R.NAN_CODE).all()) and bool((qe[[1, 3, 4]] == R.NAN_CODE).all())
    clean = R.quantize_contract(R.gauss(6, 64))
    assert torch.equal(q[[0, 2, 5]], clean[0][[0, 2, 5]]) and torch.equal(s[[0, 2, 5]], clean[1][[0, 2, 5]])


def test_ln_quantize_is_layer_norm_then_quantize():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(9, 320, generator=g) * 3 + 40
    gamma, beta = torch.randn(320, generator=g), torch.randn(320, generator=g)
    y, q, s, delta = R.ln_quantize(x, gamma, beta, 1e-5)
    want = torch.nn.functional.layer_norm(x.double(), (320,), gamma.double(), beta.double(), 1e-5)
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(s, want.abs().amax(1) / 448.0, rtol=1e-14, atol=0)
    assert bool(((R.decode(q) * s[:, None] - y).abs() <= 0.5 * R.e4m3_spacing(y / s[:, None]) * s[:, None] * (1 + 1e-12)).all())
    assert bool((delta > 0).all()) and float(delta.max()) < 1e-3
