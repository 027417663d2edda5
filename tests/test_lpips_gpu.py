"""LPIPS on the HIP path: the new kernels of csrc/lpips.hip one by one, the first conv's geometry through the existing GEMM tiles, the
[B, 7] table end to end in the four precisions, and the Python surface (metrics.compute_metrics, inference.validate).  The yardstick is
tests/lpips_ref.py, the plain-torch restatement of torchmetrics' LPIPS (net_type="squeeze"), evaluated on the CPU.

Tolerances (none taken from the device's results):
  * mf_lpips_prepare, mf_relu, mf_maxpool3s2_ceil: bit for bit (the same roundings in the same order; the 16-bit outputs are the fp32
    value rounded once).
  * conv1's geometry: per output |got - float64| <= ((K + 2) 2^-24 + s) * (sum_k |x_k| |w_k| + |bias|), K = 27 products accumulated in
    fp32, s what the mode adds.  fp32: 0.  f16x3: 2^-19 — the activation is split in registers toward zero (high half within 2^-10, low
    half within 2^-10 of the rest: 2^-20), the weight ahead of time to nearest (2^-22), the low x low product is dropped (2^-21), and
    the low halves of small operands are fp16 subnormals (below 2^-22 of the magnitude sum here): 1.75 * 2^-20 + 2^-22, rounded up.
    bf16 / fp16: the operands are rounded first and the float64 reference takes the rounded operands (their products are exact in
    fp32), so s is the one rounding of the stored result, 2^-8 / 2^-11.
  * mf_lpips_layer + mf_lpips_finish: relative deviation from float64 <= 4 x the fp32 restatement's own relative deviation on the same
    inputs, the largest over all cases of the module (pooled, so one lucky case does not set the bar).  Equal halves: exactly 0.
  * end to end, per layer: the relative deviation of every pair from the float64 table <= 4 x (fp32) / 16 x (f16x3) the fp32
    restatement's, <= 2 x the restatement's own in bf16 / fp16; the restatement's deviation is the largest over every case of the
    module for that layer.  4 x: the same arithmetic in another summation order; 16 x: two of fp32's 24 significand bits dropped per
    operand (4 x) times the same 4 x — the margins the CLIP towers are held to.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import lpips_ref as R  # noqa: E402
from reflecting_reality_amd import hip, inference, metrics, ops  # noqa: E402
from reflecting_reality_amd.lpips import LPIPS, stage_shapes, tiles_by_rule  # noqa: E402

DEV = "cuda"
K_FP32, K_F16X3, K_HALF = 4.0, 16.0, 2.0
DT = {"fp32": torch.float32, "f16x3": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SIZES = ((64, 64), (66, 70))            # 64: every pool window whole; 66 x 70: partial windows at all three pools on H, at the first and third on W
REGIONS = (None, "mask", "mirror")


def dev(a):
    return None if a is None else torch.as_tensor(np.array(a)).to(DEV)


# ---- mf_lpips_prepare -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("norm_range", [(-1, 1), (0, 1)])
@pytest.mark.parametrize("region", REGIONS)
def test_prepare_bitwise(batch, norm_range, region):
    pred, gt, mask = R.images(5, batch, 33, 35)
    assert (mask == 255).any() and (mask == 0).any()
    got = hip.lpips_prepare(dev(pred), dev(gt), dev(mask) if region else None, region, list(norm_range) == [0, 1], torch.float32)
    assert got.shape == (2 * batch, 33, 35, 8) and got.dtype == torch.float32
    want = torch.cat([R.network_input(R.blacken(x, mask, region), norm_range, torch.float32) for x in (pred, gt)]).permute(0, 2, 3, 1)
    assert torch.equal(got[..., :3].cpu(), want), f"{int((got[..., :3].cpu() != want).sum())} values differ from torch's fp32 formula"
    assert float(got[..., 3:].abs().max()) == 0.0
    for dt in (torch.bfloat16, torch.float16):
        g16 = hip.lpips_prepare(dev(pred), dev(gt), dev(mask) if region else None, region, list(norm_range) == [0, 1], dt)
        assert g16.dtype == dt and torch.equal(g16, got.to(dt))                       # the fp32 value rounded once


# ---- mf_relu ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_relu_bitwise_on_a_strided_block(dt):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 37, 40, generator=g).to(dt)                                  # 111 rows, 40 apart; the block is columns 8 .. 31
    d = x.to(DEV)
    out = hip.relu_(d[..., 8:32])
    assert out.data_ptr() == d[..., 8:32].data_ptr()
    want = x.clone()
    want[..., 8:32] = F.relu(x[..., 8:32].float()).to(dt)
    assert torch.equal(d.cpu(), want)                                               # the block clamped, its neighbours untouched
    big = torch.randn(1100, 136, generator=g).to(dt)                                # more than one block of threads, a contiguous tensor
    assert torch.equal(hip.relu_(big.to(DEV)).cpu(), F.relu(big.float()).to(dt))
    with pytest.raises(hip.MfhipError):
        hip.relu_(d[:, ::2, :8])                                                     # rows two strides apart


# ---- mf_maxpool3s2_ceil -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(32, 34), (31, 31), (8, 10)])
@pytest.mark.parametrize("c", [16, 136])
def test_maxpool_bitwise(h, w, c):
    g = torch.Generator().manual_seed(h * 100 + c)
    x = torch.randn(2, h, w, c, generator=g) - 0.5                                    # signed: mostly negative windows exist
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        xd = x.to(dt)
        want = F.max_pool2d(xd.float().permute(0, 3, 1, 2), 3, 2, ceil_mode=True).permute(0, 2, 3, 1).to(dt)
        got = hip.maxpool3s2_ceil(xd.to(DEV))
        assert got.shape == want.shape and got.is_contiguous() and torch.equal(got.cpu(), want), (h, w, c, dt)
    assert tuple(got.shape[1:3]) == (-(-(h - 3) // 2) + 1, -(-(w - 3) // 2) + 1)


# ---- conv1's geometry through the existing tiles ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "f16x3", "bf16", "fp16"])
@pytest.mark.parametrize("h,w,batch", [(66, 70, 3), (68, 70, 1)])        # -> 32 x 34 (the network's case: M = 3264 = 64 * 51) and 33 x 34: M = 1122 = 2 * 3 * 11 * 17
def test_conv1_geometry_against_float64(prec, h, w, batch):
    P = ops.Precision.get(prec)
    g = torch.Generator().manual_seed(h)
    wt = torch.randn(64, 3, 3, 3, generator=g) * 0.3
    bias = torch.randn(64, generator=g) * 0.1
    x = torch.zeros(batch, h, w, 8)
    x[..., :3] = torch.randn(batch, h, w, 3, generator=g) * 2
    cw = ops.ConvWeight(wt, bias, P, DEV, cin_pad=8)
    with tiles_by_rule(True):                         # the route LPIPS takes: the library's own tile rule, nothing timed
        got = ops.conv2d(x.to(DEV, P.act), cw, stride=2, padding=0).double().cpu()
    ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    assert got.shape == (batch, ho, wo, 64) and (batch * ho * wo) % 128 != 0 and (h != 68 or (batch * ho * wo) % 16 != 0)      # no whole number of tiles
    xr, wr = (x.to(P.act).double(), wt.to(P.compute).double()) if P.half else (x.double(), wt.double())
    xn = xr[..., :3].permute(0, 3, 1, 2)
    ref = F.conv2d(xn, wr, bias.double(), stride=2).permute(0, 2, 3, 1)
    mag = F.conv2d(xn.abs(), wr.abs(), bias.double().abs(), stride=2).permute(0, 2, 3, 1)
    s = {"fp32": 0.0, "f16x3": 2.0 ** -19, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}[prec]
    bound = (29 * 2.0 ** -24 + s) * mag
    err = (got - ref).abs()
    print(f"conv1[{prec}, {h} x {w} x {batch}]: max |err| {float(err.max()):.3e}, largest err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# ---- mf_lpips_layer + mf_lpips_finish ---------------------------------------------------------------------------------------------------
LAYER_CASES = [(c, p) for c in (64, 128, 256, 384, 512) for p in (1, 255, 1023)]


@functools.lru_cache(maxsize=None)
def layer_case(c, p):
    """Two image pairs of p pixels: non-negative features (they follow a ReLU), one pixel all zero on the first side only, weights >= 0."""
    g = torch.Generator().manual_seed(c * 7 + p)
    feat = F.relu(torch.randn(4, p, c, generator=g) + 0.3)
    feat[2:] = feat[:2] + 0.5 * F.relu(torch.randn(2, p, c, generator=g))
    feat[0, p // 2] = 0.0                                            # n(a) = sqrt(1e-8): the epsilon decides this pixel
    w = torch.randn(c, generator=g).abs() / c ** 0.5
    nchw = lambda t, dt: t.to(dt).permute(0, 2, 1)[..., None]        # [B, C, p, 1]
    ref = {dt: R.layer_distance(nchw(feat[:2], dt), nchw(feat[2:], dt), w.to(dt).reshape(1, c, 1, 1)).double().numpy()
           for dt in (torch.float64, torch.float32)}
    return feat, w, ref


@functools.lru_cache(maxsize=None)
def layer_yardstick():
    """The fp32 restatement's largest relative deviation from float64 over every case of the module."""
    return max(float(R.relative_deviation(layer_case(c, p)[2][torch.float32], layer_case(c, p)[2][torch.float64]).max()) for c, p in LAYER_CASES)


def run_layer(feat, w, layer=0):
    b = feat.shape[0] // 2
    ws = hip.lpips_ws(b, DEV)
    f4 = feat.reshape(2 * b, -1, 1, feat.shape[-1]).contiguous()
    for l in range(7):                                               # every slot is written before the finish reads it
        hip.lpips_layer(f4, w, l, ws)
    rows = hip.lpips_finish(ws, b)
    return rows


@pytest.mark.parametrize("c,p", LAYER_CASES)
def test_layer_distance_against_float64(c, p):
    feat, w, ref = layer_case(c, p)
    rows = run_layer(feat.to(DEV), w.to(DEV))
    assert rows.shape == (2, 7) and rows.dtype == torch.float32
    got = rows.cpu().double().numpy() / p
    assert all(np.array_equal(got[:, 0], got[:, l]) for l in range(7))          # the seven slots hold the same sums
    devn = float(R.relative_deviation(got[:, 0], ref[torch.float64]).max())
    yard = layer_yardstick()
    print(f"lpips_layer[C {c}, {p} pixels]: relative deviation {devn:.3e} (fp32 restatement, pooled: {yard:.3e}; RATIO {devn / yard:.2f}, bound {K_FP32})")
    assert devn <= K_FP32 * yard
    assert torch.equal(rows, run_layer(feat.to(DEV), w.to(DEV)))                 # a fixed summation order: the same bits again
    same = torch.cat([feat[:2], feat[:2]]).to(DEV)
    assert float(run_layer(same, w.to(DEV)).abs().max()) == 0.0                  # equal halves: exactly 0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_layer_distance_reads_16_bit_features(dt):
    """The arithmetic is fp32 whatever the storage: on features that are exact in the 16-bit type the fp32 tolerance holds unchanged."""
    feat, w, _ = layer_case(128, 255)
    f16 = feat.to(dt)
    nchw = lambda t: t.double().permute(0, 2, 1)[..., None]
    ref = R.layer_distance(nchw(f16[:2]), nchw(f16[2:]), w.double().reshape(1, -1, 1, 1)).numpy()
    got = run_layer(f16.to(DEV), w.to(DEV)).cpu().double().numpy()[:, 0] / 255
    devn = float(R.relative_deviation(got, ref).max())
    print(f"lpips_layer[{dt}]: relative deviation {devn:.3e} (bound {K_FP32} x {layer_yardstick():.3e})")
    assert devn <= K_FP32 * layer_yardstick()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_tables():
    """{(h, w, region): {dtype: [3, 7] table}} of the restatement on the CPU, computed once, and per dtype the per-layer yardstick: the
    largest relative deviation from float64 over every case and pair."""
    sd = R.weights(R.WEIGHT_SEED)
    tables = {}
    for h, w in SIZES:
        pred, gt, mask = R.inputs_for(h, w)
        for region in REGIONS:
            tables[(h, w, region)] = {dt: R.table(pred, gt, sd, dt, mask, region) for dt in (torch.float64, torch.float32, torch.bfloat16, torch.float16)}
    yard = {dt: np.max([R.relative_deviation(t[dt], t[torch.float64]).max(axis=0) for t in tables.values()], axis=0)
            for dt in (torch.float32, torch.bfloat16, torch.float16)}
    return tables, yard


@functools.lru_cache(maxsize=None)
def model_of(prec):
    m = LPIPS(precision=prec, device=DEV)
    m.load_state_dict(R.weights(R.WEIGHT_SEED))
    return m


@pytest.mark.parametrize("prec", ["fp32", "f16x3", "bf16", "fp16"])
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("batch", [1, 3])
def test_table_end_to_end(prec, h, w, batch):
    """Largest per-layer ratios measured on the MI355X over all cases (the device's relative deviation / the restatement's pooled deviation
    of that layer): fp32 1.56 (bound 4), f16x3 1.87 (bound 16), bf16 1.59 and fp16 1.25 (bound 2).  The bounds stay the derived ones."""
    tables, yard = reference_tables()
    model = model_of(prec)
    pred, gt, mask = R.inputs_for(h, w, batch)
    counts = np.array([a * b for a, b in stage_shapes(h, w)], np.float64)
    k, y = {"fp32": (K_FP32, yard[torch.float32]), "f16x3": (K_F16X3, yard[torch.float32]), "bf16": (K_HALF, yard[torch.bfloat16]),
            "fp16": (K_HALF, yard[torch.float16])}[prec]
    fails = []
    for region in REGIONS:
        rows = metrics.lpips_rows(dev(pred), dev(gt), model, dev(mask) if region else None, region)
        assert rows.shape == (batch, 7) and rows.dtype == torch.float32 and rows.is_cuda
        got = rows.cpu().double().numpy() / counts
        ref = tables[(h, w, region)][torch.float64][:batch]
        d = R.relative_deviation(got, ref).max(axis=0)
        ratio = d / y
        print(f"lpips[{prec}, {h} x {w}, batch {batch}, {region}]: per-layer relative deviation {np.array2string(d, precision=2)}; RATIO to the "
              f"restatement's {np.array2string(ratio, precision=2)} (bound {k}); largest {ratio.max():.2f}")
        assert not np.isnan(got).any()
        if not (ratio <= k).all():
            fails.append(f"{region}: ratios {np.array2string(ratio, precision=2)}")
        total = metrics.lpips(dev(pred), dev(gt), model, dev(mask) if region else None, region)
        assert total == float(metrics.lpips_finish(rows.cpu().numpy(), h, w).mean())
        assert torch.equal(rows, metrics.lpips_rows(dev(pred), dev(gt), model, dev(mask) if region else None, region))      # bit-reproducible
    assert not fails, f"lpips[{prec}, {h} x {w}, batch {batch}] outside {k} x the restatement's deviation: " + "; ".join(fails)


def test_identical_images_score_zero_and_norm_ranges_differ():
    model = model_of("fp32")
    pred, gt, mask = R.inputs_for(66, 70, 1)
    assert metrics.lpips(dev(pred), dev(pred), model) == 0.0
    a, b = metrics.lpips(dev(pred), dev(gt), model), metrics.lpips(dev(pred), dev(gt), model, norm_range=[0, 1])
    sd = R.weights(R.WEIGHT_SEED)
    want_a, want_b = R.score(pred, gt, sd), R.score(pred, gt, sd, norm_range=(0, 1))
    # (the per-layer test above holds fp32 to 4 x the restatement's ~1e-6; this only shows that the range reaches the network)
    assert a != b and abs(a - want_a) <= 1e-4 * want_a and abs(b - want_b) <= 1e-4 * want_b


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------
def test_compute_metrics_and_the_calculator_score_lpips():
    from PIL import Image
    model = model_of("fp32")
    pred, gt, mask = (a[0] for a in R.inputs_for(66, 70, 1))
    plain = metrics.compute_metrics(pred, gt)
    got = metrics.compute_metrics(pred, gt, lpips_model=model)
    assert set(got) == {"lpips", "ssim", "psnr"} and all(type(v) is float for v in got.values())
    assert got["lpips"] == metrics.lpips(pred, gt, model) and (got["ssim"], got["psnr"]) == (plain["ssim"], plain["psnr"])
    assert metrics.compute_metrics(Image.fromarray(pred), dev(gt), lpips_model=model) == got
    calc = metrics.MetricsCalculator(["PSNR", "LPIPS", "LPIPS_mask", "LPIPS_mirror"], DEV, lpips_model=model)
    gt_data = {"image": gt, "mask": mask, "masked_image": R.blacken(gt, mask, "mask")}
    sd = R.weights(R.WEIGHT_SEED)
    for name, region in (("LPIPS", None), ("LPIPS_mask", "mask"), ("LPIPS_mirror", "mirror")):
        v = calc.compute_metric(name, Image.fromarray(pred), gt_data, "a caption")
        assert v == metrics.lpips(pred, gt, model, mask if region else None, region)
        want = R.score(pred[None], gt[None], sd, mask=mask[None], region=region)
        assert abs(v - want) <= 1e-4 * want, (name, v, want)
    assert calc.calculate_lpips(pred, gt) == got["lpips"] and calc.compute_metric("PSNR", pred, gt_data, None) == plain["psnr"]


def test_validate_keeps_the_smallest_lpips_per_sample():
    """inference.validate(..., lpips_model=) on the tiny pipeline: per image the number metrics.lpips gives on the image run_sharded returns,
    per sample the MINIMUM over its images (train_brushnet_mirror.py:250), and every other key as in a run without the model."""
    from reflecting_reality_amd import synth
    from test_pipeline_gpu import _tiny_pipe
    pipe = _tiny_pipe()
    model = model_of("fp32")
    samples = []
    for s in range(2):
        inp = synth.pipeline_inputs(1, 32, 32, seed=70 + s, cross_dim=32, vae_scale=2)
        kw = dict(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"],
                  mask=inp["mask"], depth=inp["depth"], height=32, width=32, conditioning_noise=inp["vae_noise"])
        gt = np.random.default_rng(s).integers(0, 256, (32, 32, 3), dtype=np.uint8)
        m = np.zeros((32, 32), np.uint8)
        m[8:24, 6:20] = 255
        samples.append({**kw, "gt_image": gt, **({"gt_mask": m} if s == 1 else {})})
    common = dict(seed=5, num_images_per_validation=3, num_inference_steps=2, rank=0, world=1)
    plain = inference.validate(pipe, samples, **common)
    res = inference.validate(pipe, samples, lpips_model=model, **common)
    for key in plain:
        if key not in ("per_image", "images"):
            assert res[key] == plain[key], key
    assert set(res) - set(plain) == {"lpips", "mean_lpips", "lpips_mask", "mean_lpips_mask", "lpips_mirror", "mean_lpips_mirror"}
    for i in (0, 1):
        for k in range(3):
            assert torch.equal(res["images"][i][k], plain["images"][i][k])
            got = res["per_image"][i][k]
            assert {key: v for key, v in got.items() if not key.startswith("lpips")} == plain["per_image"][i][k]
            assert got["lpips"] == metrics.lpips(res["images"][i][k], samples[i]["gt_image"], model) > 0
        assert res["lpips"][i] == min(r["lpips"] for r in res["per_image"][i]) < max(r["lpips"] for r in res["per_image"][i])
        assert res["psnr"][i] == max(r["psnr"] for r in res["per_image"][i])
    assert "lpips_mask" not in res["per_image"][0][0]
    last = res["per_image"][1][2]
    for region in ("mask", "mirror"):
        assert last["lpips_" + region] == metrics.lpips(res["images"][1][2], samples[1]["gt_image"], model, samples[1]["gt_mask"], region)
        assert res["lpips_" + region] == [min(r["lpips_" + region] for r in res["per_image"][1])]
    assert res["mean_lpips"] == sum(res["lpips"]) / 2
