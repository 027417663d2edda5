"""reflecting-reality_amd — MI355X-native MirrorFusion (SD1.5 + BrushNet) denoising hot path.

The directory name carries a hyphen (it is the project name), so the package is imported under the
module name ``reflecting_reality_amd`` through the shim ``reflecting_reality_amd.py`` at the repo root.
Sub-modules:
  hip        ctypes binding of libmfhip.so (include/mfhip.h) — the only compute backend, no fallback
  ops        layer-level operators (conv2d / linear / attention / norms) over NHWC tensors
  models     BrushNetModel, UNet2DConditionModel, AutoencoderKL with the reference call surface
  schedulers DDIMScheduler, PNDMScheduler, UniPCMultistepScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler,
             EulerAncestralDiscreteScheduler, LCMScheduler, DDPMScheduler (forward process only)
  autograd   the tape of hand-written vector-Jacobian products behind the training step
  training   MirrorFusionModel, training_loss, train_step (backward + clip + AdamW), checkpoint save / load hooks
  distributed  batch sharding for inference, bucketed gradient all-reduce (RCCL) for training
  inference  run_sharded: the examples/brushnet/test_brushnet.py harness (sample list split over ranks, N seeds each); validate
  metrics    compute_metrics, MetricsCalculator, score_regions, clip_score, lpips: PSNR / SSIM / LPIPS (frame, mask, mirror) and CLIP similarity on the device
  pipeline   StableDiffusionBrushNetPipeline, StableDiffusionXLBrushNetPipeline
  text_encoder  CLIPTextModel, CLIPTextModelWithProjection (the prompt encoders of both pipelines)
  image_encoder  CLIPVisionModel, CLIPVisionModelWithProjection, CLIPModel (the scorer of CLIP_Similarity)
  lpips      LPIPS (net_type="squeeze": squeezenet1_1.features and the seven layer distances)
  rng        randn_tensor (torch generators, as the reference draws) and PhiloxGenerator, the library's own counter-based stream
"""
__version__ = "0.1.0"

_LAZY = {
    "BrushNetModel": "models", "UNet2DConditionModel": "models", "AutoencoderKL": "models",
    "BrushNetOutput": "models", "DDIMScheduler": "schedulers", "PNDMScheduler": "schedulers", "UniPCMultistepScheduler": "schedulers", "DPMSolverMultistepScheduler": "schedulers", "EulerDiscreteScheduler": "schedulers", "EulerAncestralDiscreteScheduler": "schedulers", "LCMScheduler": "schedulers", "DDPMScheduler": "schedulers",
    "MirrorFusionModel": "training", "compute_snr": "training", "training_loss": "training", "train_step": "training",
    "AdamW": "training", "save_state": "training", "load_state": "training", "run_sharded": "inference",
    "BatchFrontEnd": "training", "PreparedBatch": "training", "train_step_prepared": "training", "GraphedTrainStep": "training",
    "MfhipAttnProcessor": "attn_processor", "MfhipIPAttnProcessor": "attn_processor", "StableDiffusionBrushNetPipeline": "pipeline", "StableDiffusionXLBrushNetPipeline": "pipeline", "StableDiffusionPipelineOutput": "pipeline",
    "VaeImageProcessor": "pipeline", "Precision": "ops", "CLIPTextModel": "text_encoder", "CLIPTextModelWithProjection": "text_encoder",
    "CLIPVisionModel": "image_encoder", "CLIPVisionModelWithProjection": "image_encoder", "CLIPModel": "image_encoder",
    "LPIPS": "lpips", "PhiloxGenerator": "rng", "randn_tensor": "rng",
}


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module(f"{__name__}.{_LAZY[name]}"), name)
    raise AttributeError(name)
