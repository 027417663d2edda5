"""LPIPS (net_type="squeeze", normalize=False) restated in plain torch: torchmetrics' learned_perceptual_image_patch_similarity over
torchvision's squeezenet1_1.features, as the specification of the device path.  Runs on the CPU in float64, fp32, bf16 and fp16 and returns
the [B, 7] table of per-layer distances (spatial means), so a broken layer cannot hide in the sum.

  input      x / 127.5 - 1 ([-1, 1]) or x / 255 ([0, 1]) in fp32 (get_normalised_tensor, metrics/metrics.py:24-48), after the region's
             blackening (HDF5Dataset.get_masked_image), then the scaling layer (v - shift) / scale
  backbone   features.0 conv 3 -> 64, 3 x 3, stride 2; ReLU; MaxPool2d(3, 2, ceil_mode=True) at 2, 5, 8; Fire modules elsewhere
  taps       after indices 1, 4, 7, 9, 10, 11, 12
  distance   n(x) = sqrt(1e-8 + sum_c x_c^2);  d_l = mean over pixels of sum_c w_c (a_c / n(a) - b_c / n(b))^2
"""
import numpy as np
import torch
import torch.nn.functional as F

from reflecting_reality_amd import synth
from reflecting_reality_amd.lpips import LPIPS

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
FIRE_IDS = (3, 4, 6, 7, 9, 10, 11, 12)
POOL_IDS = (2, 5, 8)
TAP_IDS = (1, 4, 7, 9, 10, 11, 12)
# The seeds of the test inputs.  A random SqueezeNet forgets its input with depth, so with most seeds the last layers carry well under 1 %
# of the score; these were chosen, on this restatement in float64 alone, so that every layer carries at least 3.8 % of every pair's total
# at 64 x 64 and 66 x 70, on the frame and both regions: a broken layer cannot hide in the sum (tests/test_lpips_cpu.py asserts 2 %).
WEIGHT_SEED, IMAGE_SEED = 24, 14


def weights(seed: int):
    """synth's key-seeded state dict with the conv weights scaled by sqrt(2) (seventeen ReLUs would otherwise halve the signal's power
    each) and the lin weights made non-negative, as the published ones are."""
    sd = synth.state_dict_for(LPIPS.param_shapes(), seed)
    for k in sd:
        if k.startswith("features.") and k.endswith(".weight"):
            sd[k] = sd[k] * (2.0 ** 0.5)
        elif k.startswith("lin"):
            sd[k] = sd[k].abs()
    return sd


def images(seed: int, batch: int, h: int, w: int):
    """(pred, gt, mask) as uint8 numpy arrays: two different seeded images per pair and a mask with a mirror rectangle of 255."""
    gt = synth.images_u8(seed, batch, h, w)
    rng = np.random.default_rng(seed + 1)
    pred = np.clip(gt.astype(np.int32) + rng.integers(-48, 49, gt.shape), 0, 255).astype(np.uint8)
    pred[:, h // 3: h // 3 + h // 4, w // 5: w // 5 + w // 3] = synth.images_u8(seed + 2, batch, h // 4, w // 3)   # a patch that differs outright
    mask = np.zeros((batch, h, w), np.uint8)
    mask[:, h // 4: h // 4 + h // 2, w // 3: w // 3 + w // 2] = 255
    return pred, gt, mask


def inputs_for(h: int, w: int, batch: int = 3):
    """The module's inputs: the first `batch` pairs of ONE seeded set of three, so batch 1 is a sub-case of batch 3."""
    pred, gt, mask = images(IMAGE_SEED, 3, h, w)
    return pred[:batch], gt[:batch], mask[:batch]


def blacken(u8: np.ndarray, mask: np.ndarray, region) -> np.ndarray:
    """HDF5Dataset.get_masked_image: "mask" blackens the mirror pixels (mask == 255), "mirror" everything else (mask == 0)."""
    if not region:
        return u8
    out = u8.copy()
    out[mask == 255 if region == "mask" else mask == 0] = 0
    return out


def network_input(u8: np.ndarray, norm_range, dtype) -> torch.Tensor:
    """uint8 [B, H, W, 3] -> the scaled [B, 3, H, W] tensor: the normalisation in fp32 as the reference evaluates it (float64 for the
    float64 run), then cast to the run's dtype."""
    base = torch.float64 if dtype == torch.float64 else torch.float32
    x = torch.from_numpy(u8).permute(0, 3, 1, 2).to(base)
    if list(norm_range) == [-1, 1]:
        x = x / 127.5 - 1
    elif list(norm_range) == [0, 1]:
        x = x / 255.0
    else:
        raise ValueError("Unsupported normalization range. Use [-1, 1] or [0, 1].")
    shift = torch.tensor(SHIFT, dtype=base)[None, :, None, None]
    scale = torch.tensor(SCALE, dtype=base)[None, :, None, None]
    return ((x - shift) / scale).to(dtype)


def features(x: torch.Tensor, sd, dtype):
    p = lambda k: sd[k].to(dtype)
    taps = []
    x = F.relu(F.conv2d(x, p("features.0.weight"), p("features.0.bias"), stride=2))
    taps.append(x)
    for i in range(2, 13):
        if i in POOL_IDS:
            x = F.max_pool2d(x, 3, 2, ceil_mode=True)
        else:
            f = f"features.{i}."
            s = F.relu(F.conv2d(x, p(f + "squeeze.weight"), p(f + "squeeze.bias")))
            x = torch.cat([F.relu(F.conv2d(s, p(f + "expand1x1.weight"), p(f + "expand1x1.bias"))),
                           F.relu(F.conv2d(s, p(f + "expand3x3.weight"), p(f + "expand3x3.bias"), padding=1))], dim=1)
        if i in TAP_IDS:
            taps.append(x)
    return taps


def unit(x: torch.Tensor) -> torch.Tensor:
    return x / torch.sqrt(1e-8 + torch.sum(x ** 2, dim=1, keepdim=True))


def layer_distance(a: torch.Tensor, b: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """[B, C, h, w] features and a [1, C, 1, 1] weight -> [B]: the 1 x 1 conv of the squared difference, then the spatial mean."""
    return F.conv2d((unit(a) - unit(b)) ** 2, w).mean(dim=(2, 3)).reshape(-1)


def table(pred_u8, gt_u8, sd, dtype=torch.float64, mask=None, region=None, norm_range=(-1, 1)) -> np.ndarray:
    """The [B, 7] table of per-layer distances as float64 numpy, computed in `dtype`."""
    a = network_input(blacken(pred_u8, mask, region), norm_range, dtype)
    b = network_input(blacken(gt_u8, mask, region), norm_range, dtype)
    with torch.no_grad():
        fa, fb = features(a, sd, dtype), features(b, sd, dtype)
        cols = [layer_distance(x, y, sd[f"lin{l}.model.1.weight"].to(dtype)) for l, (x, y) in enumerate(zip(fa, fb))]
    return torch.stack(cols, dim=1).double().numpy()


def score(pred_u8, gt_u8, sd, **kw) -> float:
    """reduction="mean": the mean over the pairs of the sum over the layers."""
    return float(table(pred_u8, gt_u8, sd, **kw).sum(axis=1).mean())


def relative_deviation(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """|got - ref| / |ref| per entry of a [B, 7] table (every layer's distance is positive on the test inputs)."""
    return np.abs(np.asarray(got, np.float64) - ref) / np.abs(ref)
