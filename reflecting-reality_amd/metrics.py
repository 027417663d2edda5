"""The reference's evaluation side on the device: metrics/metrics.py (`compute_metrics` :51-67, `MetricsCalculator.compute_metric`
:108-165), which scores a generated image against its ground truth with torchmetrics' peak_signal_noise_ratio and
structural_similarity_index_measure (defaults, images as floats 0 .. 255), on the whole frame and on the two regions of the paper's tables:
`*_mask` (mirror pixels, mask == 255, blacked out in both images: HDF5Dataset.get_masked_image, dataset.py:62-68) and `*_mirror`
(everything but the mirror, mask == 0, blacked out).

One launch sequence of csrc/metrics.hip (mf_image_metrics) over the uint8 NHWC bytes gives every number of an image: the squared-error
sum and the extrema as exact integers, the sum of the per-position SSIM values; PSNR and the SSIM mean are finished here in float64 from
that row.  An image that is already uint8 NHWC in device memory is scored where it lies: no copy, no host round trip before the row is read.

`CLIP_Similarity` (metrics.py:156-157: torchmetrics' clip_score on openai/clip-vit-large-patch14) is scored on the device too once the
caller brings the network: clip_score() runs the uint8 image through mf_clip_preprocess, the vision tower of image_encoder.CLIPModel,
the caption through its text tower, and mf_clip_score; the mean over the pairs and the clamp at 0 are finished here in float64.  The
weights are something the reference downloads, so `MetricsCalculator(..., clip_model=, clip_tokenizer=)` takes them from the caller.

`LPIPS` (metrics.py:150-151, :202-204: torchmetrics' learned_perceptual_image_patch_similarity with net_type="squeeze") is scored on the
device as well once the caller brings the weights (lpips.LPIPS: torchvision's squeezenet1_1 and the `lpips` package's linear layers):
lpips_rows() runs the uint8 pair through mf_lpips_prepare, the network and mf_lpips_layer / mf_lpips_finish and leaves a [B, 7] row of
per-layer sums on the device; the division by the pixel counts, the sum over the layers and the mean over the pairs are finished here
in float64.  `compute_metrics(..., lpips_model=m)` and `MetricsCalculator(..., lpips_model=m)` take the model.

Not built (the constructor of MetricsCalculator refuses them by name): LPIPS and CLIP similarity without a model, aesthetic score,
ImageReward, HPS and the SAM-based `obj` / IoU scores — their networks and weights are not part of this package.
`compute_metrics(..., lpips_fn=f)` still calls a caller-supplied LPIPS with the normalised tensors the reference builds (metrics.py:60-64)."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import hip

WINDOW = 11          # structural_similarity_index_measure's default kernel_size: smaller images leave no valid position


def _device(device=None) -> torch.device:
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _check_window(h: int, w: int) -> None:
    if h < WINDOW or w < WINDOW:
        raise ValueError(f"SSIM's {WINDOW} x {WINDOW} window needs at least {WINDOW} pixels per edge, got {h} x {w}")


def to_u8_nhwc(image, device=None) -> torch.Tensor:
    """PIL image, uint8 [H, W(, C)] / [B, H, W, C] numpy array or tensor, or float [0, 1] [(B,) C, H, W] tensor (the pipeline's
    output_type="pt") -> uint8 [B, H, W, C] on the device.  A uint8 NHWC device tensor is returned as it is; floats go through
    mf_postprocess' uint8 output, bit for bit what np.array(pil_image) holds ((x * 255).round())."""
    if isinstance(image, torch.Tensor) and image.is_floating_point():
        x = image if image.dim() == 4 else image.unsqueeze(0)
        if x.dim() != 4:
            raise ValueError(f"a float image is [C, H, W] or [B, C, H, W] in [0, 1], got {tuple(image.shape)}")
        _check_window(x.shape[2], x.shape[3])
        dev = x.device if x.is_cuda else _device(device)
        return hip.postprocess(x.to(dev, torch.float32), denormalize=False, uint8=True)
    if not isinstance(image, (torch.Tensor, np.ndarray)):
        image = np.array(image)                                        # PIL (metrics.py:109)
    if isinstance(image, np.ndarray):                                  # (torch refuses to wrap a read-only array quietly)
        image = np.ascontiguousarray(image) if image.flags.writeable else image.copy()
    x = torch.as_tensor(image)
    if x.dtype != torch.uint8:
        raise ValueError(f"an image is uint8 [H, W, C] (or float [0, 1] [C, H, W]), got {x.dtype}")
    if x.dim() == 2:
        x = x.unsqueeze(-1)
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4 or not 1 <= x.shape[-1] <= 4:
        raise ValueError(f"an image is uint8 [H, W, C] or [B, H, W, C] with 1 .. 4 channels, got {tuple(x.shape)}")
    _check_window(x.shape[1], x.shape[2])                              # (before any upload: refused without a device too)
    return x if x.is_cuda else x.to(_device(device))


def _mask_u8(mask, like: torch.Tensor) -> torch.Tensor:
    m = mask if isinstance(mask, (torch.Tensor, np.ndarray)) else np.array(mask)
    if isinstance(m, np.ndarray):
        m = np.ascontiguousarray(m) if m.flags.writeable else m.copy()
    m = torch.as_tensor(m)
    if m.dtype != torch.uint8:
        raise ValueError(f"a mask is uint8 (255 = mirror), got {m.dtype}")
    if m.dim() == 3 and m.shape[-1] in (1, 3) and tuple(m.shape[:2]) == tuple(like.shape[1:3]):
        m = m[:, :, 0]                                                  # dataset.py:111-112: a three-channel mask carries one plane
    if m.dim() == 2:
        m = m.unsqueeze(0)
    if tuple(m.shape) != tuple(like.shape[:3]):
        raise ValueError(f"the mask must be [{like.shape[1]}, {like.shape[2]}], got {tuple(mask.shape) if hasattr(mask, 'shape') else m.shape}")
    return m.to(like.device).contiguous()


def _check_pair(pred: torch.Tensor, gt: torch.Tensor) -> None:
    if pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")


def finish(row, elements: int, data_range: Optional[float] = None) -> Dict[str, float]:
    """One mf_metrics_row -> {"psnr", "ssim"} in float64.  psnr = 10 log10(R^2 / mean squared error), R the target's range (or the
    given one); a zero error gives inf.  ssim = the sum over the valid positions / their count."""
    r = np.float64(int(row["target_max"]) - int(row["target_min"]) if not data_range or data_range <= 0 else data_range)
    se = int(row["sq_err"])
    with np.errstate(divide="ignore", invalid="ignore"):
        psnr = float("inf") if se == 0 else float(10.0 * np.log10(r * r / (np.float64(se) / np.float64(elements))))
        ssim = float(np.float64(row["ssim_sum"]) / np.float64(int(row["count"])))
    return {"psnr": psnr, "ssim": ssim}


def score(pred, gt, mask=None, region=None, data_range: float = 0.0, device=None) -> List[Dict[str, float]]:
    """{"psnr", "ssim"} of every image of a batch, each scored on its own (region: None, "mask" or "mirror")."""
    p = to_u8_nhwc(pred, device)
    g = to_u8_nhwc(gt, p.device)
    _check_pair(p, g)
    m = None if mask is None else _mask_u8(mask, p)
    rows = hip.metrics_rows(hip.image_metrics(p, g, m, region, data_range))
    n = p.shape[1] * p.shape[2] * p.shape[3]
    return [finish(r, n, data_range) for r in rows]


def _normalised(u8: torch.Tensor, norm_range) -> torch.Tensor:
    x = u8.permute(0, 3, 1, 2).float()                                  # get_normalised_tensor, metrics.py:22-48
    if list(norm_range) == [-1, 1]:
        return x / 127.5 - 1
    if list(norm_range) == [0, 1]:
        return x / 255.0
    raise ValueError("Unsupported normalization range. Use [-1, 1] or [0, 1].")


def compute_metrics(pred, gt, norm_range=[-1, 1], lpips_fn: Optional[Callable] = None, device=None, lpips_model=None) -> Dict[str, float]:
    """metrics.py:51-67 for one image pair: {"ssim", "psnr"} as Python floats, and "lpips" when the caller brings the network: an
    lpips.LPIPS as `lpips_model` (scored on the device, lpips()), or a callable `lpips_fn(pred_normalised, gt_normalised)` of their own."""
    if lpips_fn is not None and lpips_model is not None:
        raise ValueError("compute_metrics: give lpips_model or lpips_fn, not both")
    p = to_u8_nhwc(pred, device)
    g = to_u8_nhwc(gt, p.device)
    _check_pair(p, g)
    if p.shape[0] != 1:
        raise ValueError(f"compute_metrics scores one image per call, got a batch of {p.shape[0]} (metrics.score takes a batch)")
    rows = hip.image_metrics(p, g)
    out = {}
    if lpips_model is not None:
        out["lpips"] = lpips(p, g, lpips_model, norm_range=norm_range)
    if lpips_fn is not None:
        v = lpips_fn(_normalised(p, norm_range), _normalised(g, norm_range))
        out["lpips"] = float(v)
    r = finish(hip.metrics_rows(rows)[0], p.shape[1] * p.shape[2] * p.shape[3])
    out["ssim"], out["psnr"] = r["ssim"], r["psnr"]
    return out


REGION_KEYS = ("", "_mask", "_mirror")


def score_regions(pred, gt, mask, device=None, rows_only: bool = False):
    """All six numbers of one image pair — psnr, ssim, psnr_mask, ssim_mask, psnr_mirror, ssim_mirror — from one upload: the three
    launch sequences read the same device bytes and their rows come back in one copy.  rows_only: the [3, row] device tensor, nothing
    read yet (rows_to_regions() finishes it)."""
    p = to_u8_nhwc(pred, device)
    g = to_u8_nhwc(gt, p.device)
    _check_pair(p, g)
    if p.shape[0] != 1:
        raise ValueError(f"score_regions scores one image per call, got a batch of {p.shape[0]}")
    m = _mask_u8(mask, p)
    rows = torch.empty(3, hip.C.sizeof(hip.MetricsRow), dtype=torch.uint8, device=p.device)
    for i, region in enumerate((None, "mask", "mirror")):
        hip.image_metrics(p, g, m if region else None, region, out=rows[i:i + 1])
    return rows if rows_only else rows_to_regions(rows, p.shape[1] * p.shape[2] * p.shape[3])


def rows_to_regions(rows: torch.Tensor, elements: int) -> Dict[str, float]:
    out = {}
    for key, r in zip(REGION_KEYS, hip.metrics_rows(rows)):
        f = finish(r, elements)
        out["psnr" + key], out["ssim" + key] = f["psnr"], f["ssim"]
    return out


# ---- CLIP_Similarity -------------------------------------------------------------------------------------------------------------------
def clip_finish(row) -> float:
    """torchmetrics' CLIPScore.compute from the per-pair scores: max(mean over the pairs, 0), in float64 on the host."""
    r = np.asarray(row, dtype=np.float64).reshape(-1)
    return float(max(r.sum() / np.float64(r.size), 0.0))


def clip_score_rows(images, captions, model, tokenizer, device=None):
    """100 cos(image feature, text feature) of every (image, caption) pair as an fp32 [B] DEVICE tensor, and the [B, 2] norms
    (mf_clip_score); nothing is read back.  `model`: image_encoder.CLIPModel; `images`: what to_u8_nhwc takes (a uint8 NHWC device tensor
    is read where it lies; a list is a batch of equally sized images); `tokenizer`: a CLIPTokenizer-like callable."""
    if isinstance(captions, str):
        captions = [captions]
    captions = list(captions)
    dev = model.device if device is None else device
    if isinstance(images, (list, tuple)):
        x = torch.cat([to_u8_nhwc(im, dev) for im in images])
    else:
        x = to_u8_nhwc(images, dev)
    if x.shape[0] != len(captions):
        raise ValueError(f"clip_score: {x.shape[0]} images but {len(captions)} captions")
    enc = tokenizer(captions, padding="max_length", max_length=model.text.config["max_position_embeddings"], truncation=True,
                    return_tensors="pt")
    ids = enc["input_ids"] if isinstance(enc, dict) else enc.input_ids
    img = model.get_image_features(images=x)
    txt = model.get_text_features(ids.to(model.device))
    return hip.clip_score(img, txt)


def clip_score(images, captions, model, tokenizer, device=None) -> float:
    """torchmetrics.functional.multimodal.clip_score (metrics.py:156-157 calculate_clip_similarity): the features of the two projections,
    each L2-normalised, 100 * their dot product per pair, and max(mean over the pairs, 0).  Captions are tokenised to
    max_position_embeddings with truncation=True.  Under the causal mask the pooled row (the end-of-text position) sees nothing after
    its own position, so padding needs no attention_mask.  The mean and the clamp are finished on the host in float64 from the row
    the device wrote, like finish() for PSNR / SSIM."""
    rows, _ = clip_score_rows(images, captions, model, tokenizer, device)
    return clip_finish(rows.cpu().numpy())


def _load_clip(clip_model, clip_tokenizer, device):
    if isinstance(clip_model, (str, bytes)) or hasattr(clip_model, "__fspath__"):
        from .image_encoder import CLIPModel
        path = str(clip_model)
        if clip_tokenizer is None:
            from transformers import CLIPTokenizer                       # (the checkpoint directory's own vocabulary files)
            clip_tokenizer = CLIPTokenizer.from_pretrained(path, local_files_only=True)
        clip_model = CLIPModel.from_pretrained(path, device=device if device is not None else "cuda")
    if clip_tokenizer is None:
        raise ValueError("clip_model needs its clip_tokenizer (a CLIPTokenizer of the same checkpoint)")
    return clip_model, clip_tokenizer


# ---- LPIPS ---------------------------------------------------------------------------------------------------------------------------------
def lpips_rows(pred, gt, model, mask=None, region=None, norm_range=[-1, 1], device=None) -> torch.Tensor:
    """The fp32 [B, 7] DEVICE row of an lpips.LPIPS: per pair and tapped layer the sum over the pixels of the weighted squared difference
    of the channel-normalised features; nothing is read back.  Images as to_u8_nhwc takes them (RGB), region None / "mask" / "mirror"
    with a uint8 mask: the pixels are blackened in both images before normalising, as HDF5Dataset.get_masked_image does."""
    dev = model.device if device is None else device
    p = to_u8_nhwc(pred, dev)
    g = to_u8_nhwc(gt, p.device)
    _check_pair(p, g)
    if p.shape[-1] != 3:
        raise ValueError(f"LPIPS scores RGB images, got {p.shape[-1]} channels")
    model.stage_shapes(p.shape[1], p.shape[2])                           # (a small side is refused before any upload of the mask)
    if region and mask is None:
        raise ValueError(f"region {region!r} needs a mask")
    m = _mask_u8(mask, p) if region else None
    return model(p, g, m, region, norm_range)


def lpips_finish(rows, h: int, w: int, stage_shapes=None):
    """The [B, 7] row -> the B LPIPS values in float64: every layer's sum divided by its pixel count (the spatial mean), then the sum over
    the layers."""
    if stage_shapes is None:
        from .lpips import stage_shapes
    counts = np.array([a * b for a, b in stage_shapes(h, w)], dtype=np.float64)
    return (np.asarray(rows, dtype=np.float64).reshape(-1, counts.size) / counts).sum(axis=1)


def lpips(pred, gt, model, mask=None, region=None, norm_range=[-1, 1], device=None) -> float:
    """torchmetrics.functional.image.learned_perceptual_image_patch_similarity(pred, gt, net_type="squeeze", reduction="mean",
    normalize=False) on the normalised tensors of get_normalised_tensor (metrics.py:24-48), from the uint8 images."""
    p = to_u8_nhwc(pred, model.device if device is None else device)
    rows = lpips_rows(p, gt, model, mask, region, norm_range, device)
    per_pair = lpips_finish(rows.cpu().numpy(), p.shape[1], p.shape[2], model.stage_shapes)
    return float(per_pair.sum() / np.float64(per_pair.size))


# what compute_metric dispatches on besides PSNR / SSIM, and where the reference does it (metrics/metrics.py).  CLIP_Similarity leaves the
# list when the caller supplies the model, and so does LPIPS (lpips_model=).  Aesthetic_Score stays: the reference feeds floats 0 .. 255
# through open_clip's transforms (metrics.py:86-102), and neither open_clip nor torchvision exists here to pin that path against, so it is
# refused, not guessed.
_UNBUILT = (("LPIPS", "metrics.py:150-151 (calculate_lpips: torchmetrics' LPIPS network)"),
            ("CLIP_Similarity", "metrics.py:156-157 (calculate_clip_similarity: a CLIP model)"),
            ("Aesthetic_Score", "metrics.py:86-102,158-159 (the LAION aesthetic head on open_clip ViT-L-14)"),
            ("Image_Reward", "metrics.py:104-106,160-161 (ImageReward-v1.0)"),
            ("HPS", "metrics.py:162-163 (hpsv2)"),
            ("obj", "metrics.py:79-84,111-122 (SAM segmentation of the object)"),
            ("IoU", "metrics.py:79-84,124-137 (SAM masks of both images)"))


class MetricsCalculator:
    """metrics.py:70-165 for the metrics this package computes: names that hold "PSNR" or "SSIM", on the frame or — with "mask" /
    "mirror" in the name — on a region; and, with `clip_model` (an image_encoder.CLIPModel or a checkpoint directory) and its
    `clip_tokenizer`, names that hold "CLIP_Similarity"; with `lpips_model` (an lpips.LPIPS), names that hold "LPIPS", on the frame or
    a region.  Every other name of the reference is refused at construction."""

    def __init__(self, metrics_to_compute: Sequence[str], device=None, data_dir=None, cache_dir=None, ckpt_path="data/ckpt",
                 norm_range=[-1, 1], clip_model=None, clip_tokenizer=None, lpips_model=None) -> None:
        self.device = device                                                # (resolved at the first upload)
        self.metrics_to_compute = list(metrics_to_compute)
        self.norm_range, self.data_dir, self.cache_dir = norm_range, data_dir, cache_dir
        self.clip_model = self.clip_tokenizer = None
        self.lpips_model = lpips_model
        if clip_model is not None:
            self.clip_model, self.clip_tokenizer = _load_clip(clip_model, clip_tokenizer, device)
        for name in self.metrics_to_compute:
            with_lpips = False
            for key, where in _UNBUILT:
                if key == "LPIPS" and key in name and self.lpips_model is not None:
                    with_lpips = True                                       # (the other names stay refused: the loop goes on)
                    continue
                if key == "CLIP_Similarity" and key in name and self.clip_model is not None:
                    break
                if key in name:
                    raise NotImplementedError(f"metric {name!r}: {key} is not built here (the reference: {where}); its network and "
                                              "weights are not part of this package")
            else:
                if with_lpips or "PSNR" in name or "SSIM" in name:
                    continue
                raise NotImplementedError(f"metric {name!r}: only PSNR and SSIM (frame, *mask*, *mirror*) are built; the reference "
                                          "dispatches at metrics.py:150-165")

    @staticmethod
    def region_of(metric_name: str) -> Optional[str]:
        return "mask" if "mask" in metric_name else ("mirror" if "mirror" in metric_name else None)      # metrics.py:139-146, in that order

    def compute_metric(self, metric_name: str, gen_image, gt_data, caption=None) -> float:
        if metric_name not in self.metrics_to_compute:                      # the same refusals for a name the constructor never saw
            MetricsCalculator([metric_name], self.device, clip_model=self.clip_model, clip_tokenizer=self.clip_tokenizer,
                              lpips_model=self.lpips_model)
        if "CLIP_Similarity" in metric_name:
            if not caption:
                raise ValueError(f"metric {metric_name!r} scores the image against its caption: compute_metric(..., caption=) is required")
            return clip_score(gen_image, [caption], self.clip_model, self.clip_tokenizer, device=self.device)
        region = self.region_of(metric_name)
        # "mask": the reference takes the dataset's masked_image as the target (:140) and masks the generated image (:141); the region step
        # on that target is the identity (its mirror pixels are black already).  "mirror": both from the full image (:144-145).
        gt_image = gt_data["masked_image"] if region == "mask" else gt_data["image"]
        if "LPIPS" in metric_name:
            return lpips(gen_image, gt_image, self.lpips_model, gt_data["mask"] if region else None, region, self.norm_range, self.device)
        r = score(gen_image, gt_image, gt_data["mask"] if region else None, region, device=self.device)
        if len(r) != 1:
            raise ValueError("compute_metric scores one image per call")
        return r[0]["psnr" if "PSNR" in metric_name else "ssim"]

    @staticmethod
    def calculate_psnr(pred_img, gt_img) -> float:
        return score(pred_img, gt_img)[0]["psnr"]

    @staticmethod
    def calculate_ssim(pred_img, gt_img) -> float:
        return score(pred_img, gt_img)[0]["ssim"]

    def calculate_lpips(self, pred_img, gt_img, net_type="squeeze") -> float:
        """metrics.py:202-204 on the uint8 images (the reference's is a staticmethod that downloads the network; this one needs the model
        the calculator was built with)."""
        if self.lpips_model is None:
            raise NotImplementedError("calculate_lpips needs MetricsCalculator(..., lpips_model=): an lpips.LPIPS with its weights")
        if net_type != "squeeze":
            raise NotImplementedError(f"net_type {net_type!r}: only 'squeeze' is built")
        return lpips(pred_img, gt_img, self.lpips_model, norm_range=self.norm_range, device=self.device)
