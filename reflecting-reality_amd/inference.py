"""The inference harness of examples/brushnet/test_brushnet.py on the HIP pipeline: the sample list is split statically
between the ranks (accelerate's `PartialState().split_between_processes`, :163-168), every rank runs its samples through
its own pipeline replica with ONE generator seeded once per rank (`torch.Generator("cuda").manual_seed(args.seed)`, :166)
and draws `num_images_per_validation` images per sample from it in sequence (:247-266); checkpoints are enumerated the
way `--all_ckpt` does (:271-285).  No data-path collective: each image is an independent unit.

`validate` is the scoring loop of `log_validation` (examples/brushnet/train_brushnet_mirror.py:200-250) on top of it: every image is
scored against the sample's ground truth as it is produced (metrics.py, on the device) and the best of the n images of a sample is kept."""
from __future__ import annotations

import os
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import torch

from . import distributed as D


def list_checkpoints(brushnet_path: str, ckpt_modulo: Optional[int] = None) -> List[str]:
    """`checkpoint-N` folders in ascending N, optionally every `ckpt_modulo` steps (test_brushnet.py:271-285)."""
    cps = [d for d in os.listdir(brushnet_path) if d.startswith("checkpoint")]
    cps = sorted(cps, key=lambda x: int(x.split("-")[1]))
    if ckpt_modulo is not None:
        cps = [c for c in cps if int(c.split("-")[1]) % ckpt_modulo == 0]
    return [os.path.join(brushnet_path, c) for c in cps]


def run_sharded(pipe, samples: Sequence[Dict], *, seed: int = 0, num_images_per_validation: int = 4,
                num_inference_steps: int = 50, guidance_scale: float = 7.5, brushnet_conditioning_scale: float = 1.0,
                output_type: str = "pt", rank: Optional[int] = None, world: Optional[int] = None,
                on_result: Optional[Callable[[int, List], None]] = None, generator_device: Optional[str] = None,
                on_image: Optional[Callable[[int, int, object], None]] = None) -> Dict[int, List]:
    """Runs this rank's share of `samples` (dicts of pipeline kwargs: image, mask, depth / normals, prompt_embeds, ...).
    Returns {sample index: [images]} for the samples this rank owns; `on_result(index, images)` is called as each sample
    finishes (the script saves its image grid there), `on_image(index, k, image)` as each of its images is produced
    (validate() scores it there).  generator_device: "cuda" / "cpu" for a torch.Generator there (default: the pipeline's device), or
    "philox" for a rng.PhiloxGenerator: conditioning noise and latents then both come from it, on the device."""
    if rank is None or world is None:
        rank, world, _ = D.env_rank_world()
    lo, hi = D.shard_range(len(samples), rank, world)
    gdev = generator_device or (str(pipe.device) if torch.device(pipe.device).type == "cuda" else "cpu")
    if gdev == "philox":                                                     # the library's own stream (rng.PhiloxGenerator), drawn on the device
        from .rng import PhiloxGenerator
        generator = PhiloxGenerator(seed, pipe.device)
    else:
        generator = torch.Generator(gdev).manual_seed(seed)                  # one generator per rank, drawn from in sequence
    out: Dict[int, List] = {}
    for i in range(lo, hi):
        kw = dict(samples[i])
        images = []
        for _ in range(num_images_per_validation):
            res = pipe(num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, generator=generator,
                       brushnet_conditioning_scale=float(brushnet_conditioning_scale), output_type=output_type, **kw)
            images.append(res.images[0])
            if on_image is not None:
                on_image(i, len(images) - 1, images[-1])
        out[i] = images
        if on_result is not None:
            on_result(i, images)
    return out


def validate(pipe, samples: Sequence[Dict], *, num_images_per_validation: int = 4, seed: int = 0, num_inference_steps: int = 50,
             guidance_scale: float = 7.5, brushnet_conditioning_scale: float = 1.0, gt_key: str = "gt_image", mask_key: str = "gt_mask",
             rank: Optional[int] = None, world: Optional[int] = None, generator_device: Optional[str] = None,
             on_result: Optional[Callable[[int, List], None]] = None, lpips_model=None) -> Dict:
    """train_brushnet_mirror.py:200-250; LPIPS when the caller brings the network (`lpips_model`: an lpips.LPIPS).  A sample is the pipeline's kwargs plus `gt_key`: its ground-truth image (PIL,
    uint8 HWC array or device tensor) and optionally `mask_key`: its uint8 mirror mask — then every image is also scored on the "mask" and
    "mirror" regions (keys psnr_mask, ssim_mask, psnr_mirror, ssim_mirror; with `lpips_model` also lpips, lpips_mask, lpips_mirror).  The images are produced as [0, 1] device tensors and scored
    as they appear: the launches are queued behind the decode, the rows are read once per sample.  Returns
      "per_image"  {sample index: [{"psnr", "ssim", ...} per image]}
      "psnr", "ssim" (and the region keys)  the per-sample best (max) in sample order: what the reference appends to all_metrics (:246-247)
      "lpips" (and its region keys)         the per-sample best, which for LPIPS is the MINIMUM (:250)
      "mean_psnr", "mean_ssim", ...         their means over this rank's samples: what it logs (:258-262)
      "images"     run_sharded's {sample index: [images]}"""
    from . import hip, metrics as M
    stripped = [{k: v for k, v in s.items() if k not in (gt_key, mask_key)} for s in samples]
    dev = torch.device(pipe.device)
    pending: Dict[int, List] = {}
    gts: Dict[int, tuple] = {}
    per_image: Dict[int, List[Dict[str, float]]] = {}
    lp_pending: Dict[int, List] = {}

    def on_image(i: int, k: int, image) -> None:
        if i not in gts:
            gt = M.to_u8_nhwc(samples[i][gt_key], dev)                     # one upload per sample
            gts[i] = (gt, samples[i].get(mask_key))
        gt, mask = gts[i]
        pred = M.to_u8_nhwc(image, dev)
        if mask is None:
            M._check_pair(pred, gt)
            pending.setdefault(i, []).append(hip.image_metrics(pred, gt))
        else:
            pending.setdefault(i, []).append(M.score_regions(pred, gt, mask, rows_only=True))
        if lpips_model is not None:                                        # queued behind the decode like the rows above; read per sample
            regions = (None,) if mask is None else (None, "mask", "mirror")
            lp_pending.setdefault(i, []).append([M.lpips_rows(pred, gt, lpips_model, mask, r) for r in regions])

    def finish_sample(i: int, images: List) -> None:
        gt = gts.pop(i)[0]
        n = gt.shape[1] * gt.shape[2] * gt.shape[3]
        per_image[i] = [M.rows_to_regions(r, n) for r in pending.pop(i)]
        for scores, rows in zip(per_image[i], lp_pending.pop(i, [])):
            for key, r in zip(M.REGION_KEYS, rows):
                scores["lpips" + key] = float(M.lpips_finish(r.cpu().numpy(), gt.shape[1], gt.shape[2], lpips_model.stage_shapes)[0])
        if on_result is not None:
            on_result(i, images)

    images = run_sharded(pipe, stripped, seed=seed, num_images_per_validation=num_images_per_validation,
                         num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                         brushnet_conditioning_scale=brushnet_conditioning_scale, output_type="pt", rank=rank, world=world,
                         on_result=finish_sample, generator_device=generator_device, on_image=on_image)
    out: Dict = {"per_image": per_image, "images": images}
    keys = sorted({k for rows in per_image.values() for r in rows for k in r})
    for key in keys:
        pick = min if key.startswith("lpips") else max                     # train_brushnet_mirror.py:246-250
        best = [pick(r[key] for r in per_image[i]) for i in sorted(per_image) if all(key in r for r in per_image[i])]
        out[key] = best
        out["mean_" + key] = float(sum(best) / len(best)) if best else float("nan")
    return out
