"""PSNR and SSIM as the reference's evaluation side computes them (metrics/metrics.py:51-67,108-165: torchmetrics'
peak_signal_noise_ratio and structural_similarity_index_measure with their defaults on the images as floats 0 .. 255), restated in
numpy — torchmetrics is not installed where the tests run.  A plain helper module, like attention_ref.py.

  float64   the definition: what the device kernel (csrc/metrics.hip) is held to.
  float32   the same formulas, every operation in np.float32 (the filter, s and the mean): the arithmetic torchmetrics itself runs.
            Its own distance from float64 is the yardstick of the device bound (bound()).

Inputs are uint8 [H][W][C]; one image per call, as the reference scores them.

  region (dataset.py:62-68, both images, before anything else): "mask": pixels with mask == 255 -> 0; "mirror": pixels with mask == 0 -> 0.
  psnr = 10 log10(R^2 / mean((pred - gt)^2)), R = gt.max() - gt.min() (the target only); a zero error gives inf.
  ssim: window = outer product of w[d] = exp(-(d / 1.5)^2 / 2), d = -5 .. 5, normalised; R = max(range(pred), range(gt));
        c1 = (0.01 R)^2, c2 = (0.03 R)^2; E = windowed mean; mu_p = E[p], var_p = max(E[p^2] - mu_p^2, 0), cov = E[pt] - mu_p mu_t;
        s = (2 mu_p mu_t + c1)(2 cov + c2) / ((mu_p^2 + mu_t^2 + c1)(var_p + var_t + c2)); mean of s over the (H - 10)(W - 10) C positions
        whose window lies inside the image (torchmetrics reflect-pads by 5, filters and crops 5 again: the padding reaches no kept position).
The keyword knobs of ssim() exist for tests/test_image_metrics_cpu.py, which shows that each named mistake leaves the bound."""
import numpy as np

WIN, SIGMA = 11, 1.5


def window(size=WIN, sigma=SIGMA, dtype=np.float64):
    d = np.arange(size, dtype=dtype) - dtype((size - 1) / 2)
    g = np.exp(-((d / dtype(sigma)) ** 2) / dtype(2))
    return (g / g.sum()).astype(dtype)


def apply_region(img, mask, region):
    """region None / "mask" / "mirror" on a uint8 [H][W][C] image with a uint8 [H][W] mask."""
    if region in (None, "", "none"):
        return img
    out = img.copy()
    if region == "mask":
        out[mask == 255] = 0
    elif region == "mirror":
        out[mask == 0] = 0
    else:
        raise ValueError(region)
    return out


def sq_err_sum(pred, gt):
    d = pred.astype(np.int64) - gt.astype(np.int64)
    return int((d * d).sum())


def psnr(pred, gt, data_range=None):
    """float64; data_range None: the target's own range."""
    r = float(int(gt.max()) - int(gt.min())) if data_range is None else float(data_range)
    se = sq_err_sum(pred, gt)
    if se == 0:
        return float("inf")
    return float(10.0 * np.log10(np.float64(r) * np.float64(r) / (np.float64(se) / np.float64(pred.size))))


def ssim_data_range(pred, gt):
    return float(max(int(pred.max()) - int(pred.min()), int(gt.max()) - int(gt.min())))


def _filter_separable(maps, w):
    """valid 11-tap filter along W then H of [M][H][W][C] maps, tap by tap in the maps' own dtype (the window is an outer product)."""
    n = len(w)
    hh, ww = maps.shape[1] - n + 1, maps.shape[2] - n + 1
    a = sum(w[d] * maps[:, :, d:d + ww] for d in range(n))
    return sum(w[d] * a[:, d:d + hh] for d in range(n))


def ssim(pred, gt, data_range=None, dtype=np.float64, win=None, keep_padded_border=False):
    """dtype float64: the definition; float32: the arithmetic torchmetrics runs.  win: other 1-D weights; keep_padded_border: the
    'no crop' mistake (reflect-pad by 5, filter, keep all H x W positions)."""
    h, w_, _ = pred.shape
    if h < WIN or w_ < WIN:
        raise ValueError(f"SSIM needs at least {WIN} pixels per edge, got {h} x {w_}")
    f = np.dtype(dtype).type
    r = f(ssim_data_range(pred, gt) if data_range is None else data_range)
    c1, c2 = (f(0.01) * r) ** 2, (f(0.03) * r) ** 2
    wts = window(dtype=dtype) if win is None else np.asarray(win, dtype=dtype)
    p, t = pred.astype(dtype), gt.astype(dtype)
    if keep_padded_border:
        pad = ((WIN // 2, WIN // 2), (WIN // 2, WIN // 2), (0, 0))
        p, t = np.pad(p, pad, mode="reflect"), np.pad(t, pad, mode="reflect")
    maps = np.stack([p, t, p * p, t * t, p * t])
    e = _filter_separable(maps, wts)
    mu_p, mu_t = e[0], e[1]
    var_p, var_t = np.maximum(e[2] - mu_p * mu_p, f(0)), np.maximum(e[3] - mu_t * mu_t, f(0))
    cov = e[4] - mu_p * mu_t
    with np.errstate(invalid="ignore", divide="ignore"):
        s = ((f(2) * mu_p * mu_t + c1) * (f(2) * cov + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (var_p + var_t + c2))
    assert s.dtype == dtype
    return float(s.mean(dtype=dtype))


def bound(pred, gt, data_range=None):
    """(float64 SSIM, the device bound): 4 x max(|fp32 restatement - float64|, 1e-6).  From the two CPU restatements only; the factor 4
    covers another order of the sums and FMA contraction."""
    ref = ssim(pred, gt, data_range)
    dev = abs(ssim(pred, gt, data_range, dtype=np.float32) - ref)
    return ref, 4.0 * max(dev, 1e-6), dev


# ---- seeded cases: smooth fields plus noise (pure noise would put SSIM near 0, where a wrong window changes nothing) ---------------
# The fields wave at 0.3 .. 0.9 rad / pixel with a third of the range as amplitude: structure both images share inside every 11 x 11
# window, so SSIM sits at 0.8 .. 0.9 and the window's shape matters.
def smooth_pair(h, w, c=3, seed=0, lo=0, hi=255, noise=12.0, shift=6.0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.empty((h, w, c))
    for ch in range(c):
        fy, fx, ph = rng.uniform(0.3, 0.9, 2).tolist() + [rng.uniform(0, 6.28)]
        base[:, :, ch] = 0.5 + 0.3 * np.sin(fy * yy + ph) * np.cos(fx * xx - ph) + 0.15 * np.sin(0.5 * fx * (xx + yy))
    base = lo + (hi - lo) * np.clip(base, 0.0, 1.0)
    gt = base + noise * rng.standard_normal(base.shape)
    pred = base + shift * np.sin(0.11 * xx + 0.07 * yy)[:, :, None] + noise * rng.standard_normal(base.shape)
    q = lambda a: np.clip(np.rint(a), lo, hi).astype(np.uint8)
    return q(pred), q(gt)


def rect_mask(h, w, seed=0):
    """A rectangle of 255 on 0 with a rim of other values (1, 128, 254) and a few of them inside: `== 255` and `== 0` are not `> 0`."""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), dtype=np.uint8)
    y0, y1, x0, x1 = h // 5, h // 5 + h // 2, w // 4, w // 4 + w // 2
    m[y0:y1, x0:x1] = 255
    m[y0:y1, x0:x0 + 3] = 128
    m[y0, x0:x1] = 1
    m[y1 - 1, x0:x1] = 254
    ys, xs = rng.integers(y0, y1, 40), rng.integers(x0, x1, 40)
    m[ys, xs] = rng.choice(np.array([1, 77, 128, 254], dtype=np.uint8), 40)
    return m


_CASES = None


def cases():
    """name -> (pred, gt, mask or None); built once, shared and never written to."""
    global _CASES
    if _CASES is None:
        c = {}
        c["11x11"] = smooth_pair(11, 11, seed=1) + (None,)
        c["12x37"] = smooth_pair(12, 37, seed=2) + (None,)
        c["43x75"] = smooth_pair(43, 75, seed=3) + (None,)
        c["33x29_30to200"] = smooth_pair(33, 29, seed=4, lo=30, hi=200) + (None,)
        rng = np.random.default_rng(5)
        c["64x64_noise"] = (rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), None)
        c["96x80_mask"] = smooth_pair(96, 80, seed=6) + (rect_mask(96, 80, seed=6),)
        flat = np.full((40, 40, 3), 255, dtype=np.uint8)
        dot = flat.copy()
        dot[17, 23] = 0
        c["flat255"] = (flat, dot, None)             # the dot in the target: its range, PSNR's, is 255
        p, _ = smooth_pair(48, 40, seed=7)
        c["identical"] = (p, p.copy(), None)
        c["512x512"] = smooth_pair(512, 512, seed=8) + (rect_mask(512, 512, seed=8),)
        for v in c.values():
            for a in v:
                if a is not None:
                    a.setflags(write=False)
        _CASES = c
    return _CASES


_BOUNDS = {}


def case_bound(name, region=None, data_range=None):
    """bound() of a case, computed once per (case, region, data_range)."""
    key = (name, region, data_range)
    if key not in _BOUNDS:
        pred, gt, mask = cases()[name]
        _BOUNDS[key] = bound(apply_region(pred, mask, region), apply_region(gt, mask, region), data_range)
    return _BOUNDS[key]
