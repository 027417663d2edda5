"""Image scoring without a GPU: the two CPU restatements of tests/image_metrics_ref.py against each other, the named mistakes against
the bound the device kernel is held to, and the host side of the new entries (ABI, argument errors, the Python surface's refusals)."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_header
import image_metrics_ref as R
from reflecting_reality_amd import hip, program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(R.cases())
# every case but the identical pair, where s = 1 at every position whatever the window, the crop or the constants
MOVING = [n for n in CASES if n != "identical"]
MASKED = [n for n in CASES if R.cases()[n][2] is not None]
# |fp32 restatement - float64| of SSIM as recorded when the check was specified (11 x 11: one position per channel; flat 255: the variance
# of a flat window cancels completely); the restatement must stay within 4 x max(that, 1e-6) — the very margin the device gets
RECORDED = {"11x11": 5.4e-6, "flat255": 2.7e-6, "512x512": 1.5e-6}
RECORDED_OTHER = 1.1e-6
LEAVE = 30.0          # a named mistake must move the value by at least this many bounds


@pytest.mark.parametrize("name", CASES)
def test_fp32_restatement_against_float64(name):
    """The arithmetic torchmetrics runs (every operation in fp32) stays within 4 x max(its recorded deviation, 1e-6) of the definition; the
    deviation itself is recomputed here and is what the device bound is built from (image_metrics_ref.bound)."""
    ref, bound, dev = R.case_bound(name)
    print(f"{name}: SSIM float64 {ref:.9f}, fp32 deviation {dev:.3e}, device bound {bound:.3e}")
    assert dev <= 4.0 * max(RECORDED.get(name, RECORDED_OTHER), 1e-6)
    assert bound == 4.0 * max(dev, 1e-6)
    if name != "64x64_noise":
        assert ref > 0.5, "the smooth cases must sit well away from 0"


def _left(name, wrong, region=None, what=""):
    ref, bound, _ = R.case_bound(name, region)
    print(f"{what} on {name}{'/' + region if region else ''}: moved by {abs(wrong - ref):.3e} = {abs(wrong - ref) / bound:.0f} bounds")
    assert abs(wrong - ref) >= LEAVE * bound, f"{what} on {name}: {wrong} is within {LEAVE} x {bound:.1e} of {ref}"


@pytest.mark.parametrize("name", MOVING)
def test_mistake_no_crop(name):
    pred, gt, _ = R.cases()[name]
    _left(name, R.ssim(pred, gt, keep_padded_border=True), what="reflect-padded border kept")


@pytest.mark.parametrize("name", MOVING)
def test_mistake_uniform_window(name):
    pred, gt, _ = R.cases()[name]
    _left(name, R.ssim(pred, gt, win=np.full(R.WIN, 1.0 / R.WIN)), what="uniform window")


@pytest.mark.parametrize("name", MOVING)
def test_mistake_sigma_one(name):
    pred, gt, _ = R.cases()[name]
    _left(name, R.ssim(pred, gt, win=R.window(sigma=1.0)), what="sigma 1.0")


def test_mistake_data_range_255():
    pred, gt, _ = R.cases()["33x29_30to200"]
    assert (int(gt.min()), int(gt.max()), int(pred.min()), int(pred.max())) == (30, 200, 30, 200)
    _left("33x29_30to200", R.ssim(pred, gt, data_range=255.0), what="data_range fixed at 255")


def test_mistake_one_data_range_per_batch():
    """Two image pairs of one size in a batch, the first confined to 30 .. 200: a range taken over the whole batch is the second's."""
    pred, gt, _ = R.cases()["33x29_30to200"]
    pred2, gt2 = R.smooth_pair(33, 29, seed=14)
    batch_range = float(max(int(np.stack([pred, pred2]).max()) - int(np.stack([pred, pred2]).min()),
                            int(np.stack([gt, gt2]).max()) - int(np.stack([gt, gt2]).min())))
    assert batch_range > R.ssim_data_range(pred, gt) == 170.0
    _left("33x29_30to200", R.ssim(pred, gt, data_range=batch_range), what="one data_range for the batch")


def test_mistake_psnr_range_255():
    pred, gt, _ = R.cases()["33x29_30to200"]
    ref, wrong = R.psnr(pred, gt), R.psnr(pred, gt, data_range=255.0)
    print(f"PSNR {ref:.4f} dB, with data_range 255: {wrong:.4f} dB")
    assert abs((wrong - ref) - 20.0 * np.log10(255.0 / 170.0)) < 1e-9              # 3.52 dB
    assert abs(wrong - ref) >= LEAVE * 1e-12 * abs(ref)


@pytest.mark.parametrize("name", MASKED)
def test_mistake_region_test_greater_than_zero(name):
    """`mask > 0` blacks out the rim and the specks of 1 / 77 / 128 / 254 too; `mask == 255` leaves them."""
    pred, gt, mask = R.cases()[name]
    assert ((mask > 0) & (mask < 255)).sum() > 0
    wp, wg = pred.copy(), gt.copy()
    wp[mask > 0] = 0
    wg[mask > 0] = 0
    _left(name, R.ssim(wp, wg), region="mask", what="region test > 0")
    right_p, right_g = R.apply_region(pred, mask, "mask"), R.apply_region(gt, mask, "mask")
    assert R.sq_err_sum(wp, wg) != R.sq_err_sum(right_p, right_g)


@pytest.mark.parametrize("name", MASKED)
def test_mistake_regions_swapped(name):
    pred, gt, mask = R.cases()[name]
    for region, other in (("mask", "mirror"), ("mirror", "mask")):
        wrong = R.ssim(R.apply_region(pred, mask, other), R.apply_region(gt, mask, other))
        _left(name, wrong, region=region, what=f"{other!r} in place of {region!r}")


# ---- ABI and host behaviour ---------------------------------------------------------------------------------------------------------------
NEW = ("mf_image_metrics", "mf_image_metrics_ws_bytes", "mf_sizeof_metrics_row")


def test_new_entries_in_header_table_and_library():
    lib = hip.load()
    declared, protos = abi_header.declared_names(), abi_header.prototypes()
    for name in NEW:
        assert name in declared and name in protos and name in hip.SIGNATURES and hasattr(lib, name)
        ret, _, params = hip.SIGNATURES[name].partition(":")
        assert (ret, list(params)) == protos[name]
    assert hip.SIGNATURES["mf_image_metrics"].endswith("p") and len(hip.SIGNATURES["mf_image_metrics"]) == 2 + 12
    assert lib.mf_abi_version() == 23 == hip.ABI_VERSION
    assert re.search(r"#define MF_ABI_VERSION 23\b", open(abi_header.HEADER).read())
    assert (hip.MetricsRow, "mf_sizeof_metrics_row") in hip._LAYOUTS
    assert lib.mf_sizeof_metrics_row() == ctypes.sizeof(hip.MetricsRow) == 40 == np.dtype(hip.MetricsRow).itemsize


def test_new_entries_are_in_neither_replay_table():
    hip_text = open(os.path.join(ROOT, "reflecting-reality_amd", "csrc", "program.hip")).read()
    for name in NEW:
        assert name not in program._REPLAYABLE and name not in program._REPLAYABLE_CALL
        assert name not in program.SIGNATURES and name not in program.SIGNATURES_CALL
        assert name not in hip_text
    src = os.path.join(ROOT, "reflecting-reality_amd", "csrc", "metrics.hip")
    assert os.path.exists(src) and "metrics.hip" in __import__("reflecting_reality_amd._build", fromlist=["SOURCES"]).SOURCES


def test_argument_errors_without_a_gpu():
    lib = hip.load()
    buf = (ctypes.c_uint8 * 4096)()
    a = ctypes.addressof(buf) & ~7
    a += 8
    ok = dict(pred=a, target=a + 1024, mask=None, region=0, batch=1, h=16, w=16, c=3, dr=0.0, rows=a + 2048, ws=a + 2560)

    def call(**kw):
        v = {**ok, **kw}
        return lib.mf_image_metrics(v["pred"], v["target"], v["mask"], v["region"], v["batch"], v["h"], v["w"], v["c"], v["dr"], v["rows"],
                                    v["ws"], None)
    for kw, what in ((dict(pred=None), b"null pointer"), (dict(target=None), b"null pointer"), (dict(rows=None), b"null pointer"),
                     (dict(ws=None), b"null pointer"), (dict(h=10), b"at least 11"), (dict(w=10), b"at least 11"),
                     (dict(c=0), b"channels"), (dict(c=5), b"channels"), (dict(region=1), b"needs a mask"), (dict(region=2), b"needs a mask"),
                     (dict(region=3, mask=a), b"region 3"), (dict(batch=0), b"batch 0"), (dict(rows=a + 2052), b"8-byte aligned")):
        assert call(**kw) == -1, kw
        assert what in lib.mf_last_error(), (kw, lib.mf_last_error())
    assert lib.mf_image_metrics_ws_bytes(1, 10, 64, 3) == -1 and lib.mf_image_metrics_ws_bytes(1, 64, 64, 5) == -1
    one, four = lib.mf_image_metrics_ws_bytes(1, 512, 512, 3), lib.mf_image_metrics_ws_bytes(4, 512, 512, 3)
    assert 0 < one and four == 4 * one and one % 8 == 0
    with pytest.raises(ctypes.ArgumentError):          # data_range is a float, h an int32_t
        lib.mf_image_metrics(a, a, None, 0, 1, 16.0, 16, 3, 0.0, a, a, None)


def test_metrics_calculator_refuses_the_unbuilt_names():
    from reflecting_reality_amd import metrics
    for name in ("LPIPS", "LPIPS_mask", "CLIP_Similarity", "Aesthetic_Score", "Image_Reward", "HPS_V2.1", "PSNR_obj", "SSIM_obj", "IoU",
                 "FID"):
        with pytest.raises(NotImplementedError, match=r"metrics\.py:\d+"):
            metrics.MetricsCalculator(["PSNR", name], "cuda")
    calc = metrics.MetricsCalculator(["PSNR", "SSIM", "PSNR_mask", "SSIM_mask", "PSNR_mirror", "SSIM_mirror"], "cuda")
    assert [calc.region_of(n) for n in calc.metrics_to_compute] == [None, None, "mask", "mask", "mirror", "mirror"]
    with pytest.raises(NotImplementedError):
        calc.compute_metric("LPIPS", None, {}, "")


def test_compute_metrics_refuses_images_below_the_window():
    from reflecting_reality_amd import metrics
    for shape in ((10, 64, 3), (64, 10, 3), (5, 5, 3)):
        z = np.zeros(shape, dtype=np.uint8)
        with pytest.raises(ValueError, match="11"):
            metrics.compute_metrics(z, z)
    with pytest.raises(ValueError):
        R.ssim(np.zeros((10, 64, 3), np.uint8), np.zeros((10, 64, 3), np.uint8))
    import torch
    with pytest.raises(ValueError, match="11"):
        metrics.compute_metrics(torch.zeros(1, 3, 8, 64), torch.zeros(1, 3, 8, 64))


def test_finish_is_the_float64_formula():
    """metrics.finish on a row built from numpy's integers reproduces the float64 restatement's PSNR to the last bits."""
    from reflecting_reality_amd import metrics
    for name in CASES:
        pred, gt, _ = R.cases()[name]
        row = {"sq_err": R.sq_err_sum(pred, gt), "count": 1, "ssim_sum": 0.5, "target_min": int(gt.min()), "target_max": int(gt.max()),
               "pred_min": int(pred.min()), "pred_max": int(pred.max())}
        got, want = metrics.finish(row, pred.size)["psnr"], R.psnr(pred, gt)
        assert got == want or abs(got - want) <= 1e-12 * abs(want)
    assert metrics.finish({**row, "sq_err": 0}, 10)["psnr"] == float("inf")
