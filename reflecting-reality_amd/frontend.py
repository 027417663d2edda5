"""Dataset-side transforms of the reference on the device: examples/brushnet/dataset/dataset.py.

`apply_transforms_depth` (:98-166): normalisation "max_scene_depth" (scene depth = maximum depth under the mirror mask +
`delta`, or the given `max_scene_depth`; one masked max reduction + one streaming pass) or "percentile" (clip to the
[2 %, 98 %] percentiles: a two-level radix select finds the four order statistics np.percentile interpolates between — no
sort), then torchvision's Resize(resolution, BICUBIC) + CenterCrop as ONE bicubic kernel evaluated inside the crop window.
`apply_transforms_normals` (:168-192, the map-valued modes): HWC -> CHW, the same resize / crop, Normalize([0.5], [0.5]).
All on the GPU (csrc/frontend.hip), no host round trip.
`apply_transforms_rgb` / `apply_transforms_mask` / `get_masked_image` (:61-96) and `training_example` — `__getitem__` (:233-271) minus the
tokeniser, flip (:216-221) included: a decoded sample to the dataset's tensors, the uint8 bytes read once (csrc/train_batch.hip).

Bicubic: the reference pins torchvision 0.18 (MirrorFusion/README.md:34), where transforms.Resize defaults to
antialias=True and, for a tensor, hands it to torch.nn.functional.interpolate at EVERY scale (torchvision/transforms/
_functional_tensor.py `resize`): ATen's antialiased bicubic (Keys kernel a = -0.5 stretched by max(scale, 1), normalised
weights) — `antialias=None` / `True` here, mf_bicubic_aa_resize_crop.  `antialias=False` is the plain kernel (A = -0.75:
torchvision < 0.17's default for tensors), mf_bicubic_resize_crop.  SynMirror renders are 512 x 512 = `resolution`, where
Resize + CenterCrop are the identity in both.  The resize is checked against torch's own CPU interpolate (the arithmetic
torchvision calls; torchvision itself is absent from this image).  The reference MODULE imports h5py / torchvision / cv2 and
cannot be imported here, so the numpy statements around the resize (percentile / max-scene-depth normalisation) are checked
against the oracle's restatement of dataset.py:98-192 (oracle/mirrorfusion_ref.py, PARITY UNPINNED for those lines) — see
tests/test_frontend_gpu.py."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import hip


def _resize_geometry(h: int, w: int, resolution: int):
    """torchvision Resize(int): the smaller edge becomes `resolution`, the other keeps the aspect ratio (truncated);
    CenterCrop((resolution, resolution)): offsets int(round((size - resolution) / 2))."""
    if h <= w:
        nh, nw = resolution, int(resolution * w / h)
    else:
        nh, nw = int(resolution * h / w), resolution
    return (nh, nw), (int(round((nh - resolution) / 2.0)), int(round((nw - resolution) / 2.0)))


def _resize_crop(planes: torch.Tensor, resolution: int, antialias: Optional[bool], a: float = 1.0, b: float = 0.0) -> torch.Tensor:
    _, h, w = planes.shape
    (nh, nw), (top, left) = _resize_geometry(h, w, resolution)
    if (nh, nw) == (h, w) == (resolution, resolution):
        return planes if (a, b) == (1.0, 0.0) else hip.axpby_affine(planes, a, b)
    # antialias None = the reference's pinned torchvision (0.18): True, at every scale
    return hip.bicubic_resize_crop(planes, (nh, nw), (top, left), (resolution, resolution), a, b, antialias=antialias is not False)


def apply_transforms_depth(depth_map, mask=None, normalization_method: str = "max_scene_depth", max_scene_depth: float = 5.0,
                           norm_range: Sequence[float] = (-1, 1), delta: float = 0.5, resolution: int = 512, device="cuda",
                           antialias: Optional[bool] = None, **kwargs) -> torch.Tensor:
    """Returns the [1, resolution, resolution] fp32 device tensor the reference's dataset hands to the collate function."""
    if normalization_method not in ("percentile", "max_scene_depth"):
        raise ValueError("Unsupported normalization method. Use 'percentile' or 'max_scene_depth'.")
    rng = [float(v) for v in norm_range]
    if rng not in ([0.0, 1.0], [-1.0, 1.0]):
        raise ValueError("Unsupported normalization range. Use [0, 1] or [-1, 1].")
    d = torch.as_tensor(np.ascontiguousarray(depth_map) if isinstance(depth_map, np.ndarray) else depth_map).to(device, torch.float32)
    if d.dim() != 2:
        raise ValueError("apply_transforms_depth takes an [H, W] depth map")
    signed = rng == [-1.0, 1.0]
    if normalization_method == "percentile":
        out = hip.depth_percentile_normalize(d.contiguous(), signed_range=signed)                  # :115-127
    else:
        m = None
        if mask is not None:
            m = torch.as_tensor(np.ascontiguousarray(mask) if isinstance(mask, np.ndarray) else mask)
            if m.dim() == 3:
                m = m[:, :, 0]                                                    # dataset.py:111-112
            m = m.to(device, torch.float32).contiguous()
        out = hip.depth_normalize(d.contiguous(), m, max_scene_depth=max_scene_depth, delta=delta, signed_range=signed)
    return _resize_crop(out.unsqueeze(0), resolution, antialias)                                    # :150-164


def apply_transforms_normals(normals_map, resolution: int = 512, mask=None, normals_conditioning_mode: str = "concat", device="cuda",
                             antialias: Optional[bool] = None, **kwargs) -> torch.Tensor:
    """dataset.py:168-192 for the map-valued modes: [H, W, 3] -> [3, resolution, resolution], (x - 0.5) / 0.5.  The
    'ip_adapter' mode returns one mean normal vector instead of a map: that is mean_normal_over_mask below."""
    if normals_conditioning_mode == "ip_adapter":
        raise NotImplementedError("normals_conditioning_mode='ip_adapter' yields one [1, 3] vector, not a map: use "
                                  "frontend.mean_normal_over_mask(normals_map, mask) and frontend.NormalEmbedder")
    x = torch.as_tensor(np.ascontiguousarray(normals_map) if isinstance(normals_map, np.ndarray) else normals_map).to(device, torch.float32)
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError("apply_transforms_normals takes an [H, W, 3] normals map")
    h, w, _ = x.shape
    if (h, w) == (resolution, resolution):
        return hip.hwc_to_chw_affine(x, 2.0, -1.0)                                                   # Normalize([0.5], [0.5])
    return _resize_crop(hip.hwc_to_chw_affine(x, 1.0, 0.0), resolution, antialias, 2.0, -1.0)


# ---- the rest of HDF5Dataset.__getitem__ (dataset.py:61-96, 205-271): a decoded sample -> the tensors of one training example -------------
def _u8_host_checked(a, what: str, ndims: Sequence[int]):
    """A uint8 array / tensor as a tensor WHERE IT LIES; its dtype and rank are checked before anything is uploaded."""
    t = torch.as_tensor(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a numpy array or a tensor, got {type(a).__name__}")
    if t.dtype != torch.uint8:
        raise ValueError(f"{what} must be uint8 (the decoded pixels), got {t.dtype}")
    if t.dim() not in ndims:
        raise ValueError(f"{what}: {' or '.join(str(n) for n in ndims)} dimensions, got shape {tuple(t.shape)}")
    return t


def _image_and_mask(image, mask):
    """-> (image [B, H, W, 3], mask [B, H, W], batched) as uint8 tensors where they lie, shapes checked."""
    img = _u8_host_checked(image, "image", (3, 4))
    if img.shape[-1] != 3:
        raise ValueError(f"image: [H, W, 3] or [B, H, W, 3], got shape {tuple(img.shape)}")
    m = _u8_host_checked(mask, "mask", (img.dim() - 1, img.dim()))
    if m.dim() == img.dim():
        if m.shape[-1] != 1:
            raise ValueError(f"mask: one channel, got shape {tuple(m.shape)}")
        m = m[..., 0]
    if tuple(m.shape) != tuple(img.shape[:-1]):
        raise ValueError(f"mask shape {tuple(m.shape)} does not match the image's {tuple(img.shape[:-1])}")
    batched = img.dim() == 4
    return (img if batched else img[None]), (m if batched else m[None]), batched


def _flip_flags(flip, batch: int) -> list:
    flags = [bool(flip)] * batch if isinstance(flip, (bool, int, np.bool_)) else [bool(f) for f in flip]
    if len(flags) != batch:
        raise ValueError(f"flip: one flag per sample ({batch}), got {len(flags)}")
    return flags


def _flips_on_device(flags: list, device) -> Optional[torch.Tensor]:
    """The int32 device flags mf_train_example_u8 reads, or None when no sample is flipped."""
    return torch.tensor(flags, dtype=torch.int32).to(device) if any(flags) else None


def _example_planes(img: torch.Tensor, m: torch.Tensor, flips: Optional[torch.Tensor], resolution: int, antialias: Optional[bool]):
    """uint8 device image [B, H, W, 3] / mask [B, H, W] -> (pixel_values, conditioning_pixel_values, masks) at `resolution`: one launch
    when the sample already has that size, else the [0, 1] planes of that launch through the bicubic resize + crop (2x - 1 on the images)."""
    b, h, w, _ = img.shape
    (nh, nw), (top, left) = _resize_geometry(h, w, resolution)
    if (nh, nw) == (h, w) == (resolution, resolution):
        return hip.train_example_u8(img, m, flips, normalize=True)
    pix, cond, masks = hip.train_example_u8(img, m, flips, normalize=False)
    rs = lambda t, a, c: hip.bicubic_resize_crop(t.reshape(-1, h, w), (nh, nw), (top, left), (resolution, resolution), a, c,
                                                 antialias=antialias is not False).reshape(b, -1, resolution, resolution)
    return rs(pix, 2.0, -1.0), rs(cond, 2.0, -1.0), rs(masks, 1.0, 0.0)


def get_masked_image(image, mask, invert: bool = True, device="cuda") -> torch.Tensor:
    """dataset.py:61-68 on the device: uint8 [H, W, 3] (or [B, H, W, 3]) in, uint8 out; the pixels where mask == 255 (invert, the dataset's
    call) or mask == 0 are zeroed.  training_example does not need it (its kernel blackens while it converts): a helper for callers."""
    img, m, batched = _image_and_mask(image, mask)
    out = hip.masked_image_u8(img.to(device), m.to(device), invert)
    return out if batched else out[0]


def apply_transforms_rgb(image, resolution: int = 512, flip: bool = False, device="cuda", antialias: Optional[bool] = None) -> torch.Tensor:
    """dataset.py:71-83: uint8 [H, W, 3] -> fp32 [3, resolution, resolution] = Normalize([0.5], [0.5])(CenterCrop(Resize(x / 255))).
    `flip`: np.fliplr first (extract_data_from_hdf5, :219-221)."""
    img = _u8_host_checked(image, "image", (3,))
    if img.shape[-1] != 3:
        raise ValueError(f"image: [H, W, 3], got shape {tuple(img.shape)}")
    img = img.to(device)[None]
    return _example_planes(img, torch.zeros(img.shape[:3], dtype=torch.uint8, device=img.device), _flips_on_device([bool(flip)], device),
                           resolution, antialias)[0][0]


def apply_transforms_mask(mask, resolution: int = 512, flip: bool = False, device="cuda", antialias: Optional[bool] = None) -> torch.Tensor:
    """dataset.py:85-96: uint8 [H, W] -> fp32 [1, resolution, resolution] = CenterCrop(Resize(mask / 255)) (no Normalize)."""
    m = _u8_host_checked(mask, "mask", (2,)).to(device)
    planes = hip.u8_to_planes(m[None, :, :, None])[0]                                                # [1, H, W], a true division
    if flip:
        planes = hip.fliplr(planes, channels=1)
    return _resize_crop(planes, resolution, antialias)


def training_example(data: dict, resolution: int = 512, flip=False, depth: bool = False, normals_conditioning_mode: Optional[str] = None,
                     device="cuda", antialias: Optional[bool] = None, **depth_kwargs) -> dict:
    """HDF5Dataset.__getitem__ (dataset.py:233-271) minus `input_ids`, on the device: `data` is what extract_data_from_hdf5 returns
    BEFORE its flip ("image" uint8 [H, W, 3], "mask" uint8 [H, W], and — when asked for — "depth" [H, W], "normals" [H, W, 3]); the
    result holds "pixel_values" [3, R, R], "conditioning_pixel_values" [3, R, R] (the image blackened where mask == 255), "masks"
    [1, R, R], "depths" [1, R, R] (depth=True) and "normals" ([3, R, R], or the [1, 3] mean mirror normal for 'ip_adapter') as fp32 device
    tensors.  `flip` stands for the dataset's flip_horizontal: every map is read right to left.  Batched form: "image" [B, H, W, 3],
    "mask" [B, H, W], "depth" / "normals" with a leading B, `flip` one flag per sample; the results get a leading B.  `depth_kwargs`
    are apply_transforms_depth's (normalization_method, max_scene_depth, norm_range, delta).
    Host Python by design, the caller's concern: reading the HDF5 / PNG file, tokenising the caption (`input_ids`),
    `proportion_empty_prompts`, and the flip coin (`random.random() < 0.5`)."""
    if "image" not in data or "mask" not in data:
        raise ValueError("training_example: data needs 'image' and 'mask'")
    img, m, batched = _image_and_mask(data["image"], data["mask"])
    if normals_conditioning_mode not in (None, False, "concat", "latents", "ip_adapter"):
        raise ValueError(f"normals_conditioning_mode {normals_conditioning_mode!r}: 'concat', 'latents' or 'ip_adapter'")
    b = img.shape[0]
    for key, want in (("depth", depth), ("normals", normals_conditioning_mode)):
        if want and key not in data:
            raise ValueError(f"training_example: data has no {key!r}")
    flags = _flip_flags(flip, b)
    img, m = img.to(device), m.to(device)
    pix, cond, masks = _example_planes(img, m, _flips_on_device(flags, device), resolution, antialias)
    out = {"pixel_values": pix, "conditioning_pixel_values": cond, "masks": masks}
    per_sample = lambda a: a if batched else [a]
    as_f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(device, torch.float32).contiguous()
    if depth or normals_conditioning_mode:
        # the mirror mask at the sample's own size, flipped with it: what the dataset hands apply_transforms_depth / _normals
        mask_f = hip.u8_to_planes(m[..., None])[:, 0]
        mask_f = [hip.fliplr(mask_f[i], channels=1) if flags[i] else mask_f[i] for i in range(b)]
    if depth:
        ds = []
        for i, d in enumerate(per_sample(data["depth"])):
            d = as_f32(d)
            ds.append(apply_transforms_depth(hip.fliplr(d, channels=1) if flags[i] else d, mask=mask_f[i], resolution=resolution,
                                             device=device, antialias=antialias, **depth_kwargs))
        out["depths"] = torch.stack(ds)
    if normals_conditioning_mode:
        ns = []
        for i, n in enumerate(per_sample(data["normals"])):
            n = as_f32(n)
            n = hip.fliplr(n, channels=3) if flags[i] else n
            ns.append(mean_normal_over_mask(n, mask_f[i], device=device) if normals_conditioning_mode == "ip_adapter"
                      else apply_transforms_normals(n, resolution=resolution, normals_conditioning_mode=normals_conditioning_mode,
                                                    device=device, antialias=antialias))
        out["normals"] = torch.stack(ns)
    return out if batched else {k: v[0] for k, v in out.items()}


# ---- CLIPImageProcessor on the device (mf_clip_preprocess) -------------------------------------------------------------------------------
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)          # transformers.utils.constants OPENAI_CLIP_MEAN / OPENAI_CLIP_STD
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_PRECISION_BITS = 32 - 8 - 2                             # PIL Resample.c: coefficients in 22-bit fixed point
_clip_tables: dict = {}


def _bicubic_pil(x: np.ndarray) -> np.ndarray:
    """PIL's bicubic_filter (Resample.c, a = -0.5), in float64."""
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def clip_resize_table(in_size: int, out_size: int):
    """The table of one pass of PIL's Image.resize(BICUBIC) on 8-bit pixels (Resample.c precompute_coeffs + normalize_coeffs_8bpc) for
    in_size -> out_size samples: (bounds int32 [out_size, 2] = (first source index, tap count), coefficients int32 [out_size, ksize]), all
    from float64 on the host.  An output sample is clip8((2^21 + sum_j src[xmin + j] * k[j]) >> 22)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    j = np.arange(ksize, dtype=np.int64)[None, :]
    w = _bicubic_pil((j + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fs))
    w = np.where(j < count[:, None], w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for t in range(ksize):                                # the C loop's order of additions
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.trunc(np.where(w < 0, -0.5, 0.5) + w * float(1 << _PRECISION_BITS)).astype(np.int32)
    return np.stack([xmin, count], axis=1).astype(np.int32), k


def clip_resize_geometry(h: int, w: int, size: int, crop: int):
    """CLIPImageProcessor: the shortest edge becomes `size`, the other int(size * long / short); the centre crop's offsets are
    (h1 - crop) // 2 and (w1 - crop) // 2.  -> ((h1, w1), (top, left))."""
    if h <= w:
        h1, w1 = size, int(size * w / h)
    else:
        h1, w1 = int(size * h / w), size
    return (h1, w1), ((h1 - crop) // 2, (w1 - crop) // 2)


def _clip_device_tables(h: int, w: int, size: int, crop: int, device):
    key = (h, w, size, str(device))
    ent = _clip_tables.get(key)
    if ent is None:
        (h1, w1), _ = clip_resize_geometry(h, w, size, crop)
        ent = []
        for n_in, n_out in ((w, w1), (h, h1)):            # horizontal first, then vertical; a pass whose size does not change is skipped
            if n_in == n_out:
                ent += [None, 0]
            else:
                bounds, k = clip_resize_table(n_in, n_out)
                ent += [torch.from_numpy(np.concatenate([bounds.ravel(), k.ravel()])).to(device), k.shape[1]]
        _clip_tables[key] = ent = tuple(ent)
    return ent


def clip_preprocess(images, size: int = 224, crop: Optional[int] = None, mean=CLIP_MEAN, std=CLIP_STD, out_dtype=torch.float32, patch: int = 14,
                    return_u8: bool = False, device=None):
    """CLIPImageProcessor (PIL backend: bicubic shortest-edge resize on uint8, centre crop, rescale, normalise) and the unfold of the patch
    embedding on the device: images as metrics.to_u8_nhwc takes them (a uint8 NHWC device tensor is read where it lies) -> the patch matrix
    [B, (crop / patch)^2, K8] in out_dtype, K8 = 3 patch^2 rounded up to 8 with zero pad columns (and, return_u8, the cropped uint8 image
    [B, crop, crop, 3]).  The integer resize tables are built here in float64, once per (height, width, size), and kept on the device."""
    from .metrics import to_u8_nhwc
    crop = size if crop is None else crop
    x = to_u8_nhwc(images, device)
    if x.shape[-1] != 3:
        raise ValueError(f"clip_preprocess takes RGB images, got {x.shape[-1]} channels")
    if crop > size or crop % patch:
        raise ValueError(f"clip_preprocess: crop {crop} must not exceed size {size} and must be a multiple of the patch size {patch}")
    htab, hk, vtab, vk = _clip_device_tables(x.shape[1], x.shape[2], size, crop, x.device)
    out, u8 = hip.clip_preprocess(x, size, crop, patch, htab, hk, vtab, vk, mean, std, out_dtype, want_u8=return_u8)
    return (out, u8) if return_u8 else out


def mean_normal_over_mask(normals_map, mask, device="cuda") -> torch.Tensor:
    """dataset.py:173-180 (`apply_transforms_normals(..., "ip_adapter")`): the mean of normals_map [H, W, 3] over the pixels where
    mask [H, W] > 0, L2-normalised, as a [1, 3] fp32 device tensor — one reduction on the device (mf_masked_mean_normal)."""
    as_dev = lambda a: torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(device, torch.float32)
    x, m = as_dev(normals_map), as_dev(mask)
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError("mean_normal_over_mask takes an [H, W, 3] normals map")
    if m.dim() == 3 and m.shape[-1] == 1:
        m = m[:, :, 0]
    if tuple(m.shape) != tuple(x.shape[:2]):
        raise ValueError(f"mean_normal_over_mask: the mask must be [H, W] = {tuple(x.shape[:2])}, got {tuple(m.shape)}")
    return hip.masked_mean_normal(x.contiguous(), m.contiguous())


class NormalEmbedder:
    """The 'ip_adapter' normals branch of MirrorFusionModel.forward (train_brushnet_mirror.py:868-871, 1085-1098): FreqEncoder(input_dim=3,
    max_freq_log2=5, N_freqs=32, log sampling, no input copy, (sin, cos)) -> [.., 192], then NormalProjModel = Linear(192,
    cross_attention_dim) + erf-GELU (ip_adapter/ip_adapter.py:50-112; checkpoint keys "proj.0.weight" / "proj.0.bias", the "image_proj"
    dict of an ip-adapter.bin).  normal [B, 1, 3] -> one prompt token [B, 1, cross_attention_dim] in the model's storage dtype."""

    N_FREQS, MAX_FREQ_LOG2, INPUT_DIM = 32, 5.0, 3

    def __init__(self, cross_attention_dim: int, device="cuda", precision="bf16"):
        from . import ops
        self.cross_attention_dim, self.device = cross_attention_dim, torch.device(device)
        self.prec = ops.Precision.get(precision) if isinstance(precision, str) else precision
        self.proj = None

    @property
    def embed_dim(self) -> int:
        return 2 * self.N_FREQS * self.INPUT_DIM

    def load_state_dict(self, image_proj) -> "NormalEmbedder":
        from . import ops
        w, b = image_proj["proj.0.weight"], image_proj["proj.0.bias"]
        if tuple(w.shape) != (self.cross_attention_dim, self.embed_dim) or tuple(b.shape) != (self.cross_attention_dim,):
            raise ValueError(f"image_proj: proj.0.weight must be [{self.cross_attention_dim}, {self.embed_dim}], got {tuple(w.shape)}")
        self._src = {"proj.0.weight": w.detach().float().cpu().clone(), "proj.0.bias": b.detach().float().cpu().clone()}
        # the token is computed once per image from an fp32 encoding: the projection stays fp32 (f16x3 in that mode) whatever the storage dtype
        self._pprec = ops.Precision.get("f16x3" if self.prec.name == "f16x3" else "fp32")
        self.proj = ops.ConvWeight(self._src["proj.0.weight"], self._src["proj.0.bias"], self._pprec, self.device)
        return self

    def state_dict(self):
        return dict(self._src)

    def __call__(self, normal: torch.Tensor) -> torch.Tensor:
        from . import ops
        if self.proj is None:
            raise RuntimeError("NormalEmbedder has no parameters loaded (load_state_dict(image_proj))")
        if normal.shape[-1] != self.INPUT_DIM:
            raise ValueError(f"a normal is [..., {self.INPUT_DIM}], got {tuple(normal.shape)}")
        x = normal.to(self.device, torch.float32).contiguous()
        enc = hip.freq_encode(x, self.N_FREQS, self.MAX_FREQ_LOG2)
        y = ops.linear(enc, self.proj, out_dtype=torch.float32)
        y = hip.act(y, hip.ACT_GELU_ERF, out=y)
        return y if self.prec.act == torch.float32 else y.to(self.prec.act)
