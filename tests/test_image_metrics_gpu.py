"""mf_image_metrics (csrc/metrics.hip) on the device against the float64 restatement of tests/image_metrics_ref.py, and the Python
surface on top of it (metrics.compute_metrics, inference.validate).

What holds for every launch below: the squared-error sum and the four extrema are numpy's integers; PSNR finished from them is the
float64 value to 1e-12 relative; |SSIM - float64| <= 4 x max(|fp32 restatement - float64|, 1e-6), a bound computed from the two CPU
restatements alone (image_metrics_ref.bound), never from the device's result."""
import numpy as np
import pytest
import torch

import image_metrics_ref as R
from reflecting_reality_amd import hip, metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 32                         # csrc/metrics.hip MT: SSIM positions per tile edge; a tile reads TILE + 10 pixels per edge


def dev(a):
    return None if a is None else torch.as_tensor(np.array(a)).to(DEV)           # (a copy: the shared cases are read-only)


def rows_of(pred, gt, mask=None, region=None, data_range=0.0):
    """numpy [B]HWC images (a single image gets its batch axis) -> (host rows, the raw bytes of the device rows)."""
    pred, gt = (a[None] if a.ndim == 3 else a for a in (pred, gt))
    if mask is not None and mask.ndim == 2:
        mask = mask[None]
    raw = hip.image_metrics(dev(pred), dev(gt), dev(mask), region, data_range)
    return hip.metrics_rows(raw), raw.cpu().numpy().tobytes()


def check_row(row, pred, gt, name, bound=None, data_range=None):
    """One device row against numpy's integers and the float64 restatement (pred / gt: the images AFTER the region step)."""
    assert int(row["sq_err"]) == R.sq_err_sum(pred, gt), name
    assert (int(row["pred_min"]), int(row["pred_max"]), int(row["target_min"]), int(row["target_max"])) == \
        (int(pred.min()), int(pred.max()), int(gt.min()), int(gt.max())), name
    assert int(row["count"]) == (pred.shape[0] - 10) * (pred.shape[1] - 10) * pred.shape[2], name
    got = metrics.finish(row, pred.size, data_range)
    want_psnr = R.psnr(pred, gt, data_range)
    if np.isinf(want_psnr):
        assert got["psnr"] == want_psnr, name
    else:
        assert abs(got["psnr"] - want_psnr) <= 1e-12 * abs(want_psnr), (name, got["psnr"], want_psnr)
    ref, bnd, fdev = R.bound(pred, gt, data_range) if bound is None else bound
    err = abs(got["ssim"] - ref)
    print(f"{name}: SSIM device {got['ssim']:.9f} float64 {ref:.9f} |diff| {err:.3e} (fp32 restatement {fdev:.3e}, bound {bnd:.3e}); "
          f"PSNR {got['psnr']:.6f}")
    assert err <= bnd, f"{name}: |SSIM - float64| = {err:.3e} > {bnd:.3e}"


@pytest.mark.parametrize("name", list(R.cases()))
def test_every_case_through_the_entry(name):
    pred, gt, _ = R.cases()[name]
    rows, _ = rows_of(pred, gt)
    check_row(rows[0], pred, gt, name, bound=R.case_bound(name))
    if name == "identical":
        assert metrics.finish(rows[0], pred.size)["psnr"] == float("inf") and int(rows[0]["sq_err"]) == 0


# H and W at one tile - 1, one tile, one tile + 1 (plus the 10-pixel halo), two tiles + 1 with an odd W, 1 .. 4 channels
EDGES = [(TILE - 1 + 10, TILE + 1 + 10, 3), (TILE + 10, TILE + 10, 3), (TILE + 1 + 10, TILE - 1 + 10, 1), (TILE + 10, TILE + 1 + 10, 1),
         (2 * TILE + 1 + 10, 2 * TILE + 10 - 1, 3), (TILE + 1 + 10, 2 * TILE + 1 + 10, 1), (TILE + 10, 37, 2), (29, TILE + 1 + 10, 4)]


@pytest.mark.parametrize("h,w,c", EDGES)
def test_shapes_at_the_tile_edges(h, w, c):
    pred, gt = R.smooth_pair(h, w, c=c, seed=100 + h + 3 * w + c)
    rows, _ = rows_of(pred, gt)
    check_row(rows[0], pred, gt, f"{h}x{w}x{c}")
    # the same bytes at an odd address (a view one byte into a buffer): rows and images off every dword boundary
    off_p, off_g = torch.empty(pred.size + 1, dtype=torch.uint8, device=DEV), torch.empty(gt.size + 3, dtype=torch.uint8, device=DEV)
    off_p[1:].copy_(dev(pred).flatten())
    off_g[3:].copy_(dev(gt).flatten())
    raw = hip.image_metrics(off_p[1:].view(1, h, w, c), off_g[3:].view(1, h, w, c))
    assert raw.cpu().numpy().tobytes() == rows.tobytes(), "the result depends on the buffers' alignment"
    rr, _ = rows_of(pred, gt, data_range=255.0)
    check_row(rr[0], pred, gt, f"{h}x{w}x{c} data_range 255", data_range=255.0)


def test_batch_rows_equal_single_image_rows():
    pairs = [R.smooth_pair(43, 75, seed=s, lo=lo, hi=hi) for s, lo, hi in ((21, 0, 255), (22, 30, 200), (23, 0, 120))]
    mask = np.stack([R.rect_mask(43, 75, seed=s) for s in (21, 22, 23)])
    pred, gt = np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])
    for region, dr in ((None, 0.0), ("mask", 0.0), ("mirror", 0.0), (None, 255.0), ("mirror", 255.0)):
        rows, raw = rows_of(pred, gt, mask if region else None, region, dr)
        size = len(raw) // 3
        for i in range(3):
            one, raw1 = rows_of(pred[i], gt[i], mask[i] if region else None, region, dr)
            assert raw[i * size:(i + 1) * size] == raw1, f"image {i} of the batch, region {region}, data_range {dr}"
        if region is None and dr == 0.0:
            for i in range(3):                       # each image keeps its own data_range (the second is confined to 30 .. 200)
                check_row(rows[i], pred[i], gt[i], f"batch image {i}")


@pytest.mark.parametrize("name", ["96x80_mask", "512x512"])
def test_regions_equal_premasked_copies(name):
    pred, gt, mask = R.cases()[name]
    for region in ("mask", "mirror"):
        mp, mg = R.apply_region(pred, mask, region), R.apply_region(gt, mask, region)
        for dr in ((0.0, 255.0) if name == "96x80_mask" else (0.0,)):        # (the given-range path rides its statistics in the tile pass)
            rows, raw = rows_of(pred, gt, mask, region, dr)
            _, raw0 = rows_of(mp, mg, None, None, dr)
            assert raw == raw0, f"{name}: region {region!r} (data_range {dr}) differs from a call on pre-masked copies"
            check_row(rows[0], mp, mg, f"{name}/{region}/data_range {dr}", bound=R.case_bound(name, region, dr or None),
                      data_range=dr or None)


def test_two_calls_return_identical_bytes():
    pred, gt, mask = R.cases()["512x512"]
    p, g, m = dev(np.stack([pred, gt, pred])), dev(np.stack([gt, pred, pred])), dev(np.stack([mask] * 3))
    for region, dr in ((None, 0.0), ("mask", 0.0), ("mirror", 255.0)):
        a = hip.image_metrics(p, g, m if region else None, region, dr).cpu().numpy().tobytes()
        b = hip.image_metrics(p, g, m if region else None, region, dr).cpu().numpy().tobytes()
        assert a == b


def test_compute_metrics_takes_every_input_form():
    from PIL import Image
    pred, gt, mask = R.cases()["96x80_mask"]
    f01 = dev(pred).permute(2, 0, 1).float().div(255.0).unsqueeze(0)           # the pipeline's output_type="pt"
    assert np.array_equal(hip.postprocess(f01, denormalize=False, uint8=True)[0].cpu().numpy(), pred)
    want = metrics.compute_metrics(pred, gt)
    assert set(want) == {"ssim", "psnr"} and all(type(v) is float for v in want.values())
    for form in (dev(pred[None]), dev(pred), f01, f01[0], Image.fromarray(pred), torch.as_tensor(pred.copy())):
        assert metrics.compute_metrics(form, Image.fromarray(gt)) == want
    assert abs(want["psnr"] - R.psnr(pred, gt)) <= 1e-12 * R.psnr(pred, gt)
    assert abs(want["ssim"] - R.case_bound("96x80_mask")[0]) <= R.case_bound("96x80_mask")[1]
    seen = []
    with_lpips = metrics.compute_metrics(pred, gt, lpips_fn=lambda a, b: seen.append((a, b)) or 0.25)
    assert with_lpips == {**want, "lpips": 0.25}
    a, b = seen[0]
    # get_normalised_tensor's x / 127.5 - 1 (the device's fp32 division may round the last bit differently from the host's)
    assert a.shape == (1, 3, 96, 80) and torch.allclose(a.cpu(), torch.as_tensor(pred.copy()).permute(2, 0, 1)[None].float() / 127.5 - 1, rtol=0, atol=2e-7)
    assert torch.allclose(b.cpu(), torch.as_tensor(gt.copy()).permute(2, 0, 1)[None].float() / 127.5 - 1, rtol=0, atol=2e-7)
    # the six numbers of the paper's tables, and the reference's MetricsCalculator surface on the same data
    six = metrics.score_regions(pred, gt, mask)
    assert (six["psnr"], six["ssim"]) == (want["psnr"], want["ssim"])
    calc = metrics.MetricsCalculator(["PSNR", "SSIM", "PSNR_mask", "SSIM_mask", "PSNR_mirror", "SSIM_mirror"], DEV)
    gt_data = {"image": gt, "mask": mask, "masked_image": R.apply_region(gt, mask, "mask")}
    for name in calc.metrics_to_compute:
        key = name.lower()
        assert calc.compute_metric(name, Image.fromarray(pred), gt_data, "a caption") == six[key], name
    for region in ("mask", "mirror"):
        mp, mg = R.apply_region(pred, mask, region), R.apply_region(gt, mask, region)
        assert abs(six["psnr_" + region] - R.psnr(mp, mg)) <= 1e-12 * R.psnr(mp, mg)
        ref, bnd, _ = R.case_bound("96x80_mask", region)
        assert abs(six["ssim_" + region] - ref) <= bnd


def test_validate_scores_what_run_sharded_returns():
    """inference.validate on the tiny pipeline: per image the numbers of compute_metrics on the image run_sharded returns with the same
    seed; per sample the best of the n images, max for PSNR and max for SSIM; the means of those."""
    from reflecting_reality_amd import inference, synth
    from test_pipeline_gpu import _tiny_pipe
    pipe = _tiny_pipe()
    samples, plain = [], []
    for s in range(2):
        inp = synth.pipeline_inputs(1, 16, 16, seed=70 + s, cross_dim=32, vae_scale=2)
        kw = dict(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"],
                  mask=inp["mask"], depth=inp["depth"], height=16, width=16, conditioning_noise=inp["vae_noise"])
        gt = np.random.default_rng(s).integers(0, 256, (16, 16, 3), dtype=np.uint8)
        plain.append(kw)
        samples.append({**kw, "gt_image": gt, **({"gt_mask": R.rect_mask(16, 16, seed=s)} if s == 1 else {})})
    common = dict(seed=5, num_images_per_validation=3, num_inference_steps=2, rank=0, world=1)
    res = inference.validate(pipe, samples, **common)
    imgs = inference.run_sharded(pipe, plain, output_type="pt", **common)
    assert sorted(res["per_image"]) == [0, 1] and all(len(v) == 3 for v in res["per_image"].values())
    for i in (0, 1):
        assert len(imgs[i]) == 3 and not torch.equal(imgs[i][0], imgs[i][1])
        for k in range(3):
            assert torch.equal(res["images"][i][k], imgs[i][k])
            want = metrics.compute_metrics(imgs[i][k], samples[i]["gt_image"])
            got = res["per_image"][i][k]
            assert (got["psnr"], got["ssim"]) == (want["psnr"], want["ssim"])
        assert res["psnr"][i] == max(r["psnr"] for r in res["per_image"][i])
        assert res["ssim"][i] == max(r["ssim"] for r in res["per_image"][i])
    assert res["mean_psnr"] == sum(res["psnr"]) / 2 and res["mean_ssim"] == sum(res["ssim"]) / 2
    assert "psnr_mask" not in res["per_image"][0][0]
    six = metrics.score_regions(imgs[1][2], samples[1]["gt_image"], samples[1]["gt_mask"])
    assert res["per_image"][1][2] == six and res["ssim_mirror"] == [max(r["ssim_mirror"] for r in res["per_image"][1])]
