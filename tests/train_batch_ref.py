"""Reference of the training batch (a plain helper module, like gemm_ref.py): examples/brushnet/dataset/dataset.py:61-96, 216-221 and
examples/brushnet/train_brushnet_mirror.py:1351-1449 minus the networks, restated on the CPU with explicit index arithmetic.

The dataset module itself cannot be imported here (h5py / torchvision are absent); tests/test_train_batch_cpu.py pins these
restatements against the ATen / numpy operations the script calls (F.interpolate nearest and antialiased bicubic, torch.cat,
Tensor.repeat, alphas_cumprod[timesteps], np.fliplr).  The example side is fp32 (what the dataset computes); the batch side takes the VAE
moments as input and is float64, with the error bounds of the fp32 kernel next to every value."""
import numpy as np
import torch
import torch.nn.functional as F


# ---- dataset.py:61-96, 216-221 ---------------------------------------------------------------------------------------------------------
def resize_geometry(h, w, resolution):
    """transforms.Resize(int) (the smaller edge becomes `resolution`, the other int(resolution * long / short)) and
    CenterCrop(resolution) (offsets int(round((size - resolution) / 2)))."""
    nh, nw = (resolution, int(resolution * w / h)) if h <= w else (int(resolution * h / w), resolution)
    return (nh, nw), (int(round((nh - resolution) / 2.0)), int(round((nw - resolution) / 2.0)))


def get_masked_image(image, mask, invert=True):
    out = image.copy()
    out[(mask == 255) if invert else (mask == 0)] = 0
    return out


def fliplr(a):
    """np.fliplr, written out: column x of the result is column W - 1 - x of the input."""
    a = np.asarray(a)
    return a[:, np.arange(a.shape[1] - 1, -1, -1)]


def _resize_crop(planes, resolution):
    """Resize(BICUBIC) on a tensor in torchvision 0.18 = F.interpolate(bicubic, antialias=True, align_corners=False); then the crop."""
    _, h, w = planes.shape
    (nh, nw), (top, left) = resize_geometry(h, w, resolution)
    if (nh, nw) != (h, w):
        planes = F.interpolate(planes[None], size=(nh, nw), mode="bicubic", align_corners=False, antialias=True)[0]
    return planes[:, top:top + resolution, left:left + resolution]


def apply_transforms_rgb(image, resolution):
    x = torch.tensor(np.copy(image), dtype=torch.float32).permute(2, 0, 1) / 255.0
    return (_resize_crop(x, resolution) - 0.5) / 0.5


def apply_transforms_mask(mask, resolution):
    return _resize_crop((torch.tensor(np.copy(mask), dtype=torch.float32) / 255.0).unsqueeze(0), resolution)


def example(image, mask, flip, resolution):
    """One sample of __getitem__: (pixel_values [3, R, R], conditioning_pixel_values [3, R, R], masks [1, R, R]), fp32."""
    masked = get_masked_image(image, mask)
    if flip:
        image, mask, masked = fliplr(image), fliplr(mask), fliplr(masked)
    return apply_transforms_rgb(image, resolution), apply_transforms_rgb(masked, resolution), apply_transforms_mask(mask, resolution)


def example_planes(image, mask, flip):
    """The [0, 1] planes ahead of the resize: (image / 255 [3, H, W], masked image / 255, mask / 255 [1, H, W])."""
    masked = get_masked_image(image, mask)
    if flip:
        image, mask, masked = fliplr(image), fliplr(mask), fliplr(masked)
    f = lambda a: torch.tensor(np.copy(a), dtype=torch.float32) / 255.0
    return f(image).permute(2, 0, 1), f(masked).permute(2, 0, 1), f(mask).unsqueeze(0)


# ---- train_brushnet_mirror.py:1351-1449 ----------------------------------------------------------------------------------------------
def nearest_index(n_in, n_out):
    """F.interpolate(mode='nearest'): source index min(floor(dst * (float)n_in / (float)n_out), n_in - 1), the scale and the product in fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def nearest(planes, h, w):
    planes = np.asarray(planes)
    return planes[..., nearest_index(planes.shape[-2], h)[:, None], nearest_index(planes.shape[-1], w)[None, :]]


def repeat3(planes):
    """depths.repeat(1, 3, 1, 1) for one-channel planes [B, 1, H, W]"""
    return np.asarray(planes)[:, [0, 0, 0]]


def cat_channels(parts):
    parts = [np.asarray(p) for p in parts]
    out = np.empty((parts[0].shape[0], sum(p.shape[1] for p in parts)) + parts[0].shape[2:], dtype=parts[0].dtype)
    at = 0
    for p in parts:
        out[:, at:at + p.shape[1]] = p
        at += p.shape[1]
    return out


def posterior(moments_nhwc, noise, c, scaling):
    """DiagonalGaussianDistribution.sample() * scaling_factor in float64 from NHWC moments [B, h, w, ld]: -> (z [B, c, h, w],
    A = (|mean| + |std * noise|) * scaling, the magnitude the fp32 error bounds scale with)."""
    m = np.asarray(moments_nhwc.float() if isinstance(moments_nhwc, torch.Tensor) else moments_nhwc, dtype=np.float64)
    mean, logvar = m[..., :c].transpose(0, 3, 1, 2), np.clip(m[..., c:2 * c].transpose(0, 3, 1, 2), -30.0, 20.0)
    std, n, s = np.exp(0.5 * logvar), np.asarray(noise, dtype=np.float64), float(np.float32(scaling))
    return (mean + std * n) * s, (np.abs(mean) + np.abs(std * n)) * s


def assemble(moments, posterior_noise, c, scaling, noise, timesteps, alphas_cumprod, masks, depths=None, normals=None, v_prediction=False,
             snr_gamma=None):
    """moments / posterior_noise: [image, conditioning image, depth or None, normals or None].  Returns float64 arrays: latents,
    noisy_latents, target, conditioning_latents, timesteps_f32, loss_weights (snr_gamma) and bound_latents / bound_noisy / bound_target:
      |z - z64| <= 2^-21 A;  |noisy - noisy64| <= 2^-20 (sqrt(a) A + sqrt(1 - a) |eps|);  v target: 2^-20 (sqrt(a) |eps| + sqrt(1 - a) A)
    (0.5 * logvar exact, expf <= 2 ulp, half an ulp for every other rounding, doubled)."""
    z, A = posterior(moments[0], posterior_noise[0], c, scaling)
    h, w = z.shape[-2:]
    eps = np.asarray(noise, dtype=np.float64)
    ts = np.asarray(timesteps, dtype=np.int64)
    a = np.asarray(alphas_cumprod, dtype=np.float64)[ts]                       # alphas_cumprod[timesteps]
    sa, sb = np.sqrt(a)[:, None, None, None], np.sqrt(1.0 - a)[:, None, None, None]
    out = {"latents": z, "bound_latents": 2.0 ** -21 * A, "noisy_latents": sa * z + sb * eps, "bound_noisy": 2.0 ** -20 * (sa * A + sb * np.abs(eps)),
           "target": sa * eps - sb * z if v_prediction else eps,
           "bound_target": 2.0 ** -20 * (sa * np.abs(eps) + sb * A) if v_prediction else np.zeros_like(eps),
           "timesteps_f32": ts.astype(np.float64)}
    parts = [posterior(moments[1], posterior_noise[1], c, scaling)[0], nearest(np.asarray(masks, dtype=np.float64), h, w)]
    if depths is not None:
        parts.append(nearest(np.asarray(depths, dtype=np.float64), h, w))
    elif len(moments) > 2 and moments[2] is not None:
        parts.append(posterior(moments[2], posterior_noise[2], c, scaling)[0])
    if normals is not None:
        parts.append(nearest(np.asarray(normals, dtype=np.float64), h, w))
    elif len(moments) > 3 and moments[3] is not None:
        parts.append(posterior(moments[3], posterior_noise[3], c, scaling)[0])
    out["conditioning_latents"] = cat_channels(parts)
    if snr_gamma is not None:                                                  # :1437-1449
        snr = a / (1.0 - a)
        wgt = np.minimum(snr, snr_gamma)
        out["loss_weights"] = wgt / (snr + 1.0) if v_prediction else wgt / snr
    return out
