"""StableDiffusionBrushNetPipeline with the reference call surface on the HIP models.

Reference: MirrorFusion/src/diffusers/pipelines/brushnet/pipeline_brushnet.py — __init__ :185-233,
check_inputs :573-693, prepare_image :741-774, prepare_latents :777-791, __call__ :848-1363 (hot loop
:1250-1332), and image_processor.py:446-610 (VaeImageProcessor).

Result-preserving shortcuts relative to the reference:
  * the masked image is VAE-encoded once for B images; the reference encodes the CFG-duplicated 2B batch
    (:771-772, :1188) whose two halves have identical moments and differ only in the posterior noise — the
    noise is still drawn for 2B so both halves match the reference;
  * classifier-free guidance and the DDIM update run as one kernel.
CLIP text encoding is outside the accelerated path: pass `prompt_embeds` / `negative_prompt_embeds`, or give
the pipeline a transformers `text_encoder` + `tokenizer` pair.
"""
from __future__ import annotations

import contextlib
import gc
import inspect
import json
import os
import time

from collections import OrderedDict
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Union

import numpy as np
import torch

from . import hip
from . import lora as _lora
from .models import AutoencoderKL, BrushNetModel, UNet2DConditionModel
from .rng import PhiloxGenerator, is_philox, randn_tensor
from .schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, LCMScheduler, PNDMScheduler,
                         UniPCMultistepScheduler, device_plan)

try:
    import PIL.Image
except Exception:  # pragma: no cover
    PIL = None


@dataclass
class StableDiffusionPipelineOutput:
    images: Any
    nsfw_content_detected: Optional[List[bool]]


class VaeImageProcessor:
    """image_processor.py:446-610 for the formats the BrushNet pipeline feeds it (host side, once per image)."""

    def __init__(self, vae_scale_factor: int = 8, do_resize: bool = True, do_normalize: bool = True,
                 do_convert_rgb: bool = False):
        self.vae_scale_factor = vae_scale_factor
        self.do_resize, self.do_normalize, self.do_convert_rgb = do_resize, do_normalize, do_convert_rgb

    def preprocess(self, image, height: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
        supported = (torch.Tensor, np.ndarray) + ((PIL.Image.Image,) if PIL is not None else ())
        if isinstance(image, supported):
            image = [image]
        elif not (isinstance(image, list) and all(isinstance(i, supported) for i in image)):
            raise ValueError(f"Input is in incorrect format: {[type(i) for i in image]}. Currently, we only support "
                             "PIL.Image.Image, np.ndarray, torch.Tensor")
        first = image[0]
        if PIL is not None and isinstance(first, PIL.Image.Image):
            if self.do_resize and height is not None:
                image = [i.resize((width, height), resample=PIL.Image.LANCZOS) for i in image]
            if self.do_convert_rgb:
                image = [i.convert("RGB") for i in image]
            arr = np.stack([np.array(i).astype(np.float32) / 255.0 for i in image], axis=0)
            if arr.ndim == 3:
                arr = arr[..., None]
            t = torch.from_numpy(arr.transpose(0, 3, 1, 2))
        elif isinstance(first, np.ndarray):
            arr = np.concatenate(image, axis=0) if first.ndim == 4 else np.stack(image, axis=0)
            if arr.ndim == 3:
                arr = arr[..., None]
            t = torch.from_numpy(arr.transpose(0, 3, 1, 2)).float()
        else:
            t = torch.cat(image, dim=0) if first.ndim == 4 else torch.stack(image, dim=0)
            if t.shape[1] == 4:                                             # already latents (:532-533)
                return t
        t = t.float()
        if t.is_cuda:
            # device tensors stay on the device and go through the front-end kernels (csrc/frontend.hip): nearest resize
            # (F.interpolate's default, :resize()), then 2x - 1 unless the tensor already holds negatives — the min is
            # reduced on the device and read by the normalising kernel, the host never waits for it
            if self.do_resize and height is not None and tuple(t.shape[-2:]) != (height, width):
                t = hip.nearest_resize(t, height, width)
            return hip.image_normalize(t) if self.do_normalize else t
        if self.do_resize and height is not None and tuple(t.shape[-2:]) != (height, width):
            t = torch.nn.functional.interpolate(t, size=(height, width))    # :resize() for tensors (host, once)
        if self.do_normalize and t.min() >= 0:                              # negatives pass through un-normalised
            t = 2.0 * t - 1.0
        return t

    def postprocess(self, image: torch.Tensor, output_type: str = "pil", do_denormalize=None):
        if output_type not in ("latent", "pt", "np", "pil"):
            output_type = "np"
        if output_type == "latent":
            return image
        if do_denormalize is None:
            do_denormalize = [self.do_normalize] * image.shape[0]
        if image.is_cuda and image.dtype == torch.float32 and (all(do_denormalize) or not any(do_denormalize)):
            if output_type == "pil":       # straight to uint8 HWC on the device: the host only copies bytes
                arr = hip.postprocess(image, denormalize=all(do_denormalize), uint8=True).cpu().numpy()
                if arr.shape[-1] == 1:
                    return [PIL.Image.fromarray(a.squeeze(), mode="L") for a in arr]
                return [PIL.Image.fromarray(a) for a in arr]
            image = hip.postprocess(image, denormalize=all(do_denormalize))
        else:
            image = torch.stack([(image[i] / 2 + 0.5).clamp(0, 1) if do_denormalize[i] else image[i]
                                 for i in range(image.shape[0])])
        if output_type == "pt":
            return image
        arr = image.cpu().permute(0, 2, 3, 1).float().numpy()
        if output_type == "np":
            return arr
        arr = (arr * 255).round().astype("uint8")
        if arr.shape[-1] == 1:
            return [PIL.Image.fromarray(a.squeeze(), mode="L") for a in arr]
        return [PIL.Image.fromarray(a) for a in arr]


# ---- the scheduler update of ONE call: __call__ picks one of the three forms, once; the loops and the exporter only talk to the object ----
# `eager`: a step of the eager loop.  For the captured step: `key` is the form's part of the graph-cache key, `attach` puts its static
# buffers into the kept state, `load(i)` is the per-step copy before a replay, `launch` ends one_step, `after_replay` / `finish` are the
# host's part, `export` gives a step program its io buffers and tables, and `result` is its meta's sentence about what a run leaves.
# `sample(lat)` is the sample after a step, what a callback_on_step_end sees and the loop returns; `replace(new, lat)` goes on with the
# callback's own.  Both are `lat` itself except under the Euler family, where `lat` holds the MODEL INPUT of the step about to run
# (sample / sqrt(sigma^2 + 1)) and the sample is the update object's own: a slot of the plan's state, or a tensor of _HostStep.
class _FusedDDIM:
    """DDIM with eta == 0 and no rescale: classifier-free guidance and the update are one kernel, reading the step's four
    coefficients from a row of a [steps, 4] table."""
    result = "latents (DDIM update inside)"

    def __init__(self, pipe, g):
        cfg = pipe.scheduler.config
        self.sched, self.g = pipe.scheduler, float(g)
        self.clip = float(cfg["clip_sample_range"]) if cfg["clip_sample"] else 0.0
        self.ptype = 0 if cfg["prediction_type"] == "epsilon" else 1
        self.key = ("ddim", self.ptype, self.clip)

    def attach(self, st, lat, ts):
        self.coef_cur = st.setdefault("coef_cur", torch.empty(4, dtype=torch.float32, device=lat.device))
        self.coefs = torch.tensor([self.sched.step_coefficients(int(t))[:4] for t in ts], dtype=torch.float32).to(lat.device)

    def eager(self, eu, ec, t, latents): return self.sched.step(None, t, latents, return_dict=False, _cfg=(eu, ec, self.g))[0]
    def load(self, i): self.coef_cur.copy_(self.coefs[i])
    def launch(self, eu, ec, lat): hip.cfg_ddim_step_dev(eu, ec, self.g, lat, self.coef_cur, self.ptype, self.clip, out=lat)
    def after_replay(self, t, lat): pass
    def sample(self, lat): return lat
    def replace(self, new, lat): lat.copy_(new)
    def finish(self): pass
    def export(self): return dict(coef4=self.coef_cur), {"table.coef4": self.coefs.contiguous()}


class _DevicePlan:
    """PNDM / UniPC / DPM-Solver++ inside the captured step: mf_sched_step_dev runs the step's row of schedulers.device_plan (a trace of
    their own step()) on a state buffer that keeps their history; the scheduler gets its end state from it after the loop.  A plan that
    reads a step's noise (DPM-Solver++ SDE) takes a rng.PhiloxGenerator: mf_sched_step_noise_dev draws the noise in the kernel from the
    generator's device state and mf_philox_advance moves that state, both inside the graph; the host pair follows per replayed step.
    Euler / Euler-ancestral: the plan keeps the sample in slot `plan.x_slot` and every row ends by writing the next step's model input
    into the latents; attach() starts the run (x0 into the slot, x0 * plan.first_scale into the latents: one launch).
    LCM: a noisy plan whose last row reads no noise (plan.draws); the one captured step still draws and advances there, so the host pair
    stays where the host's step() leaves it and the generator's device state is brought level again on its next use.  Without
    classifier-free guidance launch() gets ec=None and hands the kernels g < 0: register 0 is the noise prediction as the UNet wrote it."""

    def __init__(self, pipe, g, nsteps, generator=None):
        self.sched, self.g = pipe.scheduler, float(g)
        self.plan = device_plan(self.sched, steps=nsteps)
        name = type(self.sched).__name__
        self.key = (name, "device", self.plan.nslots)
        self.result = f"latents ({name} update inside: mf_sched_step_dev; history in sched_state)"
        self.gen, self.meta = None, {}
        if self.plan.noise_reg >= 0:
            if not isinstance(generator, PhiloxGenerator):
                raise hip.MfhipError("a device plan that draws noise needs a rng.PhiloxGenerator")
            self.gen = generator
            generator.device = generator.device or torch.device(pipe.device)
            # taken HERE, outside the capture; its address is part of the graph's key (another generator's state: another graph)
            self.rng_state = generator.device_state()
            self.key += (self.plan.noise_reg, self.rng_state.data_ptr())
            self.result = f"latents ({name} update inside: mf_sched_step_noise_dev + mf_philox_advance; history in sched_state)"
        if self.plan.x_slot >= 0:
            self.key += ("x", self.plan.x_slot)
            self.result = self.result[:-1] + f"; latents hold the model input, sched_state slot {self.plan.x_slot} the sample)"
            # a host starts a run with x0 in that slot and x0 * first_input_scale in latents
            self.meta = dict(sample_slot=self.plan.x_slot, first_input_scale=float(self.plan.first_scale))

    def attach(self, st, lat, ts):
        if "state" not in st:                     # the step's mf_sched_row, and the scheduler's history (persists between steps)
            st["row_cur"] = torch.empty(self.plan.rows.shape[1], dtype=torch.int32, device=lat.device)
            st["state"] = torch.empty((max(self.plan.nslots, 1),) + tuple(lat.shape), dtype=torch.float32, device=lat.device)
        self.row_cur, self.state, self.rows = st["row_cur"], st["state"], self.plan.rows.to(lat.device)
        if self.gen is not None:
            self.per = lat[0].numel()
            self.blocks = hip.philox_normal_blocks(lat.shape[0], self.per)           # what one step's draw consumes
            self.meta = dict(self.meta, philox=dict(per_sample=self.per, first_sample=0, global_batch=int(lat.shape[0]),
                                                    blocks_per_step=self.blocks, noise_reg=self.plan.noise_reg))
            self.rng_state = self.gen.device_state()       # (level with the host pair again: prepare_latents drew since __init__)
        self.x = None
        if self.plan.x_slot >= 0:
            self.x = self.state[self.plan.x_slot].copy_(lat)
            hip.axpby_n([self.x], [self.plan.first_scale], out=lat)
            self.sched.model_input_prescaled = True          # (scale_model_input inside the step body: the identity; finish() clears it)

    def load(self, i):
        self.i = i
        self.row_cur.copy_(self.rows[i])

    def launch(self, eu, ec, lat):
        g = self.g if ec is not None else -1.0    # (no classifier-free guidance: the kernels' g < 0 form, eps_c is not read)
        if self.gen is None:
            hip.sched_step_dev(eu, ec, g, lat, self.state, self.row_cur)
        else:                                     # (same stream: the advance runs after the kernel has read the state)
            hip.sched_step_noise_dev(eu, ec, g, lat, self.state, self.row_cur, self.plan.noise_reg, rng_state=self.rng_state)
            hip.philox_advance(self.rng_state, self.blocks)

    def after_replay(self, t, lat):
        if self.gen is not None:
            if self.plan.draws[self.i]:
                self.gen.note_advanced(self.blocks, on_device=True)
            else:                                 # the row read no noise: the host pair stays, the device state has moved past it
                self.gen.device_moved()

    def sample(self, lat): return lat if self.x is None else self.x

    def replace(self, new, lat):
        if self.x is None:
            lat.copy_(new)
        else:
            raise hip.MfhipError("a device plan of the Euler family steps without a callback_on_step_end")

    def finish(self): self.plan.finish(self.sched, self.state)    # the counters and history the host's step() would have left

    # (the host copies the step's row in like coef4, and the history slots stay in "sched_state" between runs)
    # (the generator's device state of a noise-drawing plan is one more io buffer, bound once like sched_state)
    def export(self):
        io = dict(sched_row=self.row_cur, sched_state=self.state)
        if self.gen is not None:
            io["philox_state"] = self.rng_state
        return io, {"table.sched_row": self.rows.contiguous()}


class _HostStep:
    """Everything else: the guided noise prediction goes to the host's scheduler.step (a handful of mf_axpby_n launches; multistep
    schedulers keep host-side state between steps, scheduling_pndm.py:321-390).  The captured step ends with it in `eps`."""
    result = "eps (guided noise prediction; the scheduler update is the host's)"

    def __init__(self, pipe, g, rescale, eta, generator):
        self.pipe, self.g, self.rescale = pipe, float(g), rescale
        params = inspect.signature(pipe.scheduler.step).parameters
        self.extra = {k: v for k, v in (("eta", eta), ("generator", generator)) if k in params}
        self.key = (type(pipe.scheduler).__name__, "host")
        self.scaled, self.x = bool(getattr(pipe.scheduler, "scales_model_input", False)), None

    def eager(self, eu, ec, t, latents):
        noise_pred = eu if ec is None else hip.cfg_combine(eu, ec, self.g)                          # :1310-1312
        if ec is not None and self.rescale > 0.0:
            # rescale_noise_cfg (pipeline_brushnet_sd_xl.py:1478-1480; pipeline_stable_diffusion.py:59-70): one standard
            # deviation per image and two scalings — a non-default switch outside the timed path, on torch's device ops
            dims, r = list(range(1, ec.ndim)), self.rescale
            std_text, std_cfg = ec.float().std(dim=dims, keepdim=True), noise_pred.float().std(dim=dims, keepdim=True)
            noise_pred = (r * (noise_pred.float() * (std_text / std_cfg)) + (1.0 - r) * noise_pred.float()).to(noise_pred.dtype)
        return self.pipe._sched_step(noise_pred, t, latents, self.extra)

    def attach(self, st, lat, ts):
        self.eps = st.setdefault("eps", torch.empty_like(lat))
        if self.scaled:                           # Euler family: the sample is this object's, `lat` gets the first step's model input
            sched = self.pipe.scheduler
            self.x = lat.clone()
            hip.axpby_n([self.x], [sched._input_scale(sched.index_for_timestep(ts[0]) if sched.begin_index is None else sched.begin_index)],
                        out=lat)
            sched.model_input_prescaled = True    # (scale_model_input inside the step body: the identity; finish() clears it)

    def load(self, i): pass
    def launch(self, eu, ec, lat): self.eps.copy_(eu if ec is None else hip.cfg_combine(eu, ec, self.g))    # :1310-1312

    # (multistep schedulers keep references to their inputs (ets, last_sample): hand them copies, not the graph's static buffers)
    def after_replay(self, t, lat):
        if self.scaled:
            self.replace(self.pipe._sched_step(self.eps.clone(), t, self.x, self.extra), lat)
        else:
            lat.copy_(self.pipe._sched_step(self.eps.clone(), t, lat.clone(), self.extra))          # :1315

    def sample(self, lat): return self.x if self.scaled else lat

    def replace(self, new, lat):
        if self.scaled:                           # the sample, and the model input of the step that follows
            self.x = new
            hip.axpby_n([new.contiguous()], [self.pipe.scheduler._input_scale(self.pipe.scheduler.step_index)], out=lat)
        else:
            lat.copy_(new)

    def finish(self):
        if self.scaled:
            self.pipe.scheduler.model_input_prescaled = False
    def export(self): return dict(eps=self.eps), {}


class StableDiffusionBrushNetPipeline:
    _callback_tensor_inputs = ["latents", "prompt_embeds", "negative_prompt_embeds"]

    def __init__(self, vae: AutoencoderKL, text_encoder, tokenizer, unet: UNet2DConditionModel,
                 brushnet: BrushNetModel, scheduler, safety_checker=None, feature_extractor=None, image_encoder=None,
                 requires_safety_checker: bool = True, depth_conditioning_mode=None, normals_conditioning_mode=None):
        if safety_checker is not None and feature_extractor is None:
            raise ValueError("Make sure to define a feature extractor when loading the pipeline if you want to use "
                             "the safety checker. If you do not want to use the safety checker, you can pass "
                             "`'safety_checker=None'` instead.")
        if safety_checker is not None:
            raise NotImplementedError("the safety checker (a CLIP vision model) is outside the accelerated path; "
                                      "pass safety_checker=None as examples/brushnet/test_brushnet.py:150 does")
        for nm, mode in (("depth", depth_conditioning_mode), ("normals", normals_conditioning_mode)):
            if nm == "normals" and mode == "ip_adapter":
                # train_brushnet_mirror.py:752-756, 868-871: the mirror normal enters as ONE extra prompt token of the UNet (decoupled
                # cross-attention, MfhipIPAttnProcessor on every attn2); no normals map joins the BrushNet conditioning
                if type(self).__name__ != "StableDiffusionBrushNetPipeline":
                    raise NotImplementedError("normals_conditioning_mode='ip_adapter' is built for the SD1.5 pipeline")
                continue
            if mode not in (None, "concat", "latents"):
                raise ValueError(f"{nm}_conditioning_mode must be None, 'concat' or 'latents'" + (" or 'ip_adapter'" if nm == "normals" else "")
                                 + f", got {mode!r}")
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.unet, self.brushnet, self.scheduler = unet, brushnet, scheduler
        self.safety_checker, self.feature_extractor, self.image_encoder = safety_checker, feature_extractor, image_encoder
        self.vae_scale_factor = 2 ** (len(self.vae.config.block_out_channels) - 1)
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor, do_convert_rgb=True)
        self.depth_conditioning_mode = depth_conditioning_mode
        self.normals_conditioning_mode = normals_conditioning_mode
        self.config = dict(requires_safety_checker=requires_safety_checker)
        self._progress_bar_config: Dict[str, Any] = {}
        self._guidance_scale = 7.5
        self._num_timesteps = 0
        self.use_hip_graph = True        # capture the denoise step into a hipGraph when the scheduler allows it
        self.overlap_brushnet = True     # BrushNet on a second HIP stream, ordered against the UNet by per-residual events
        self.share_brushnet_cfg = True   # BrushNet evaluated once when both CFG halves get identical inputs (_brushnet_shareable)
        # opt-in deviation from pipeline_brushnet.py:1188: draw ONE VAE-posterior sample of the conditioning latents and use
        # it for both classifier-free-guidance halves (the reference draws one per half); each half's distribution is
        # unchanged, BrushNet then runs once per image
        self.cfg_shared_conditioning_sample = False
        self._brushnet_once = False
        self._side_stream = None
        self.overlap_aux = False         # UNet shortcut convs / V projections on a third stream: measured 0.8 % slower
                                         # (18.15 vs 18.0 ms per step, tools/bench_aux.py), so off by default
        # both nets' time embeddings + fused time_emb_proj for the whole schedule in one batched pass before the loop
        # (graph path): 8 dependent launches fewer at the head of every step; A/B switch for tools/
        self.precompute_time_embedding = os.environ.get("MFHIP_NO_TEMB_TABLE") != "1"
        # opt-in: the 15 BrushNet zero-convs whose residual lands on a Transformer2DModel.proj_out run INSIDE that GEMM (models.LazyResidual)
        # measured on MI355X (gpurun_out/r03c): 16.75 ms per step with it, 16.56 without — the fused K = 2C GEMM lands on the
        # UNet's stream (the critical one) while the zero-conv it replaces ran in BrushNet's slack: OFF by default
        self.fold_zero_convs = os.environ.get("MFHIP_ZC_FOLD") == "1"
        self._graph_state = None         # the captured step and its static buffers, kept across calls (_denoise_graph)
        self.normal_embedder = None      # 'ip_adapter' normals mode: a frontend.NormalEmbedder turns `normals=` [B, 1, 3] into the ip token

    # ---- loading / saving (pipelines/pipeline_utils.py:148-296 save_pretrained, :465-919 from_pretrained) ---------
    _scheduler_classes = ("DDIMScheduler", "PNDMScheduler", "UniPCMultistepScheduler", "DPMSolverMultistepScheduler",
                          "EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler", "LCMScheduler")

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, torch_dtype=None, device="cuda", **kwargs):
        """The reference's calling convention (examples/brushnet/test_brushnet.py:146-155): `__init__` parameters without
        a default are modules — taken from kwargs, else loaded from the sub-folder `model_index.json` names (`brushnet`
        is never in an SD1.5 index, so it must be passed, like in the reference); parameters with a default
        (`depth_conditioning_mode`, ...) are plain kwargs.  `unet=None` means "load it from the base directory".
        `text_encoder/` is loaded into the HIP CLIPTextModel (text_encoder.py) when the folder exists and no `text_encoder=` was
        passed.  The tokenizer is string processing and stays the caller's object; `tokenizer/` is loaded through
        transformers.CLIPTokenizer when transformers is importable, else left None."""
        from . import schedulers as S
        root = pretrained_model_name_or_path
        index = {}
        if os.path.exists(os.path.join(root, "model_index.json")):
            with open(os.path.join(root, "model_index.json")) as f:
                index = json.load(f)
        mods = {}
        for name, klass in (("vae", AutoencoderKL), ("unet", UNet2DConditionModel), ("brushnet", BrushNetModel)):
            obj = kwargs.pop(name, None)
            if obj is None:
                if not os.path.isdir(os.path.join(root, name)):
                    raise ValueError(f"Pipeline {cls.__name__} expected {{'{name}'}}, but it was neither passed nor "
                                     f"found under {root!r}.")
                obj = klass.from_pretrained(root, subfolder=name, torch_dtype=torch_dtype, device=device)
            mods[name] = obj
        sched = kwargs.pop("scheduler", None)
        if sched is None:
            with open(os.path.join(root, "scheduler", "scheduler_config.json")) as f:
                scfg = json.load(f)
            sname = scfg.get("_class_name") or (index.get("scheduler") or [None, "PNDMScheduler"])[1]
            if sname not in cls._scheduler_classes:
                raise NotImplementedError(f"scheduler {sname} is outside the MirrorFusion path (have {cls._scheduler_classes})")
            sched = getattr(S, sname).from_config(scfg)
        if kwargs.pop("safety_checker", None) is not None:
            raise NotImplementedError("the safety checker is outside the accelerated path; pass safety_checker=None")
        kwargs.pop("low_cpu_mem_usage", None)
        text_encoder, tokenizer = kwargs.pop("text_encoder", None), kwargs.pop("tokenizer", None)
        if text_encoder is None and os.path.isdir(os.path.join(root, "text_encoder")):
            from .text_encoder import CLIPTextModel
            text_encoder = CLIPTextModel.from_pretrained(root, subfolder="text_encoder", torch_dtype=torch_dtype, device=device)
        if tokenizer is None and os.path.isdir(os.path.join(root, "tokenizer")):
            try:
                from transformers import CLIPTokenizer
            except ImportError:
                CLIPTokenizer = None
            if CLIPTokenizer is not None:
                tokenizer = CLIPTokenizer.from_pretrained(root, subfolder="tokenizer")
        return cls._assemble(root, mods, sched, text_encoder, tokenizer, torch_dtype, device, kwargs)

    @classmethod
    def _assemble(cls, root, mods, sched, text_encoder, tokenizer, torch_dtype, device, kwargs):
        """from_pretrained's last step: the constructor call (the XL subclass has another constructor)."""
        return cls(vae=mods["vae"], text_encoder=text_encoder, tokenizer=tokenizer,
                   unet=mods["unet"], brushnet=mods["brushnet"], scheduler=sched, safety_checker=None,
                   feature_extractor=kwargs.pop("feature_extractor", None),
                   requires_safety_checker=kwargs.pop("requires_safety_checker", False),
                   depth_conditioning_mode=kwargs.pop("depth_conditioning_mode", None),
                   normals_conditioning_mode=kwargs.pop("normals_conditioning_mode", None))

    def save_pretrained(self, save_directory: str, **unused):
        """`model_index.json` + one sub-folder per module in the reference's on-disk format (config.json +
        diffusion_pytorch_model.safetensors with the reference's key names; scheduler/scheduler_config.json)."""
        os.makedirs(save_directory, exist_ok=True)
        index = {"_class_name": type(self).__name__, "_diffusers_version": "0.27.0.dev0"}
        for name in ("vae", "unet", "brushnet"):
            m = getattr(self, name)
            m.save_pretrained(os.path.join(save_directory, name))
            index[name] = ["diffusers", m._class_name]
        self.scheduler.save_config(os.path.join(save_directory, "scheduler"))
        index["scheduler"] = ["diffusers", type(self.scheduler).__name__]
        for name in ("text_encoder", "tokenizer", "safety_checker", "feature_extractor"):
            index[name] = [None, None]
        from .text_encoder import CLIPTextModel
        if isinstance(self.text_encoder, CLIPTextModel):
            self.text_encoder.save_pretrained(os.path.join(save_directory, "text_encoder"))
            index["text_encoder"] = ["transformers", self.text_encoder._class_name]
        index.update(requires_safety_checker=False, depth_conditioning_mode=self.depth_conditioning_mode,
                     normals_conditioning_mode=self.normals_conditioning_mode)
        with open(os.path.join(save_directory, "model_index.json"), "w") as f:
            json.dump(index, f, indent=2)

    # ---- DiffusionPipeline surface ----------------------------------------------------------------
    @property
    def device(self):
        return self.unet.device

    _execution_device = device

    def to(self, *args, **kwargs):
        from .models import HipModel
        for m in (self.vae, self.unet, self.brushnet, self.text_encoder, getattr(self, "text_encoder_2", None)):
            if isinstance(m, HipModel):
                m.to(*args, **kwargs)
        return self

    def set_progress_bar_config(self, **kwargs):
        self._progress_bar_config = kwargs

    # Memory-saving switches of DiffusionPipeline (pipelines/pipeline_utils.py:940-1683).  The offload, attention-slicing and
    # xformers ones never change a result in the reference; with 288 GB of HBM per GPU the modules simply stay resident, so they
    # are accepted and do nothing (test_brushnet.py:160 carries a commented-out enable_model_cpu_offload()).
    def enable_model_cpu_offload(self, gpu_id=None, device="cuda"):
        return None

    def enable_sequential_cpu_offload(self, gpu_id=None, device="cuda"):
        return None

    def enable_attention_slicing(self, slice_size="auto"):
        return None

    def disable_attention_slicing(self):
        return None

    # The two VAE switches are forwarded (pipeline_utils / pipeline_brushnet.py enable_vae_slicing .. disable_vae_tiling call the
    # VAE's): tiling changes the result above the VAE's tile threshold, exactly as in the reference.
    def _vae_switch(self, name: str) -> None:
        fn = getattr(self.vae, name, None)
        if callable(fn):
            fn()

    def enable_vae_slicing(self):
        self._vae_switch("enable_slicing")

    def disable_vae_slicing(self):
        self._vae_switch("disable_slicing")

    def enable_vae_tiling(self):
        self._vae_switch("enable_tiling")

    def disable_vae_tiling(self):
        self._vae_switch("disable_tiling")

    def enable_xformers_memory_efficient_attention(self, attention_op=None):
        return None

    def disable_xformers_memory_efficient_attention(self):
        return None

    def progress_bar(self, total):
        try:
            from tqdm.auto import tqdm
            return tqdm(total=total, **self._progress_bar_config)
        except Exception:  # pragma: no cover
            class _N:
                def __enter__(s): return s
                def __exit__(s, *a): return False
                def update(s, *a): pass
            return _N()

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def do_classifier_free_guidance(self):
        """pipeline_brushnet.py:~835: a UNet with `time_cond_proj_dim` (guidance-distilled, LCM) takes the guidance scale as an embedding
        and never runs the doubled batch."""
        return self._guidance_scale > 1 and self.unet.config.get("time_cond_proj_dim") is None

    def get_guidance_scale_embedding(self, w: torch.Tensor, embedding_dim: int = 512, dtype=torch.float32) -> torch.Tensor:
        """pipeline_brushnet.py:795-822 (https://github.com/google-research/vdm model_vdm.py#L298): the sinusoidal embedding
        [len(w), embedding_dim] of the guidance scales `w` (1-D), zero-padded by one column when embedding_dim is odd.  Host arithmetic,
        once per call."""
        assert len(w.shape) == 1
        w = w * 1000.0
        half_dim = embedding_dim // 2
        emb = torch.log(torch.tensor(10000.0)) / (half_dim - 1)
        emb = torch.exp(torch.arange(half_dim, dtype=dtype) * -emb)
        emb = w.to(dtype)[:, None] * emb[None, :]
        emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=1)
        if embedding_dim % 2 == 1:
            emb = torch.nn.functional.pad(emb, (0, 1))
        assert emb.shape == (w.shape[0], embedding_dim)
        return emb

    @property
    def num_timesteps(self):
        return self._num_timesteps

    # ---- input validation (pipeline_brushnet.py:573-693) -------------------------------------------
    def check_inputs(self, prompt, image, mask, callback_steps, negative_prompt=None, prompt_embeds=None,
                     negative_prompt_embeds=None, brushnet_conditioning_scale=1.0, control_guidance_start=0.0,
                     control_guidance_end=1.0, callback_on_step_end_tensor_inputs=None, depth=None, normals=None):
        if callback_steps is not None and (not isinstance(callback_steps, int) or callback_steps <= 0):
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type {type(callback_steps)}.")
        if callback_on_step_end_tensor_inputs is not None and not all(
                k in self._callback_tensor_inputs for k in callback_on_step_end_tensor_inputs):
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`. Please make sure to only forward one of the two.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        if prompt is not None and not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError("Cannot forward both `negative_prompt` and `negative_prompt_embeds`.")
        if prompt_embeds is not None and negative_prompt_embeds is not None \
                and prompt_embeds.shape != negative_prompt_embeds.shape:
            raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, "
                             f"but got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds` {negative_prompt_embeds.shape}.")
        for nm, im in (("image", image), ("mask", mask)):
            if im is None:
                raise TypeError(f"`{nm}` must be passed (PIL image, numpy array, torch tensor or a list of those)")
        if self.depth_conditioning_mode is not None and depth is None:
            raise ValueError(f"depth_conditioning_mode={self.depth_conditioning_mode!r} needs a `depth` input")
        if self.normals_conditioning_mode not in (None, "ip_adapter") and normals is None:
            raise ValueError(f"normals_conditioning_mode={self.normals_conditioning_mode!r} needs a `normals` input")
        if not isinstance(brushnet_conditioning_scale, float):
            raise TypeError("For single brushnet: `brushnet_conditioning_scale` must be type `float`.")
        starts = control_guidance_start if isinstance(control_guidance_start, (tuple, list)) else [control_guidance_start]
        ends = control_guidance_end if isinstance(control_guidance_end, (tuple, list)) else [control_guidance_end]
        if len(starts) != len(ends):
            raise ValueError(f"`control_guidance_start` has {len(starts)} elements, but `control_guidance_end` has {len(ends)} elements.")
        for s, e in zip(starts, ends):
            if s >= e:
                raise ValueError(f"control guidance start: {s} cannot be larger or equal to control guidance end: {e}.")
            if s < 0.0:
                raise ValueError(f"control guidance start: {s} can't be smaller than 0.")
            if e > 1.0:
                raise ValueError(f"control guidance end: {e} can't be larger than 1.0.")

    # ---- prompt --------------------------------------------------------------------------------------
    def encode_prompt(self, prompt, num_images_per_prompt, do_cfg, negative_prompt=None, prompt_embeds=None,
                      negative_prompt_embeds=None, clip_skip: Optional[int] = None):
        """pipeline_brushnet.py:271-450 without LoRA / textual inversion.  clip_skip (:352-370): the hidden state clip_skip layers
        before the last one, through the text model's final LayerNorm (the text encoder is the caller's torch module: outside the
        accelerated path, or text_encoder.CLIPTextModel: the same calls on the HIP kernels)."""
        if prompt_embeds is None:
            if self.text_encoder is None or self.tokenizer is None:
                raise ValueError("pass `prompt_embeds` or construct the pipeline with a text_encoder and tokenizer")
            def enc(txt):
                ids = self.tokenizer(txt, padding="max_length", max_length=self.tokenizer.model_max_length,
                                     truncation=True, return_tensors="pt").input_ids
                ids = ids.to(next(self.text_encoder.parameters()).device)
                with torch.no_grad():
                    if clip_skip is None:
                        return self.text_encoder(ids)[0]
                    out = self.text_encoder(ids, output_hidden_states=True)
                    return self.text_encoder.text_model.final_layer_norm(out[-1][-(clip_skip + 1)])
            plist = [prompt] if isinstance(prompt, str) else prompt
            prompt_embeds = enc(plist)
            if do_cfg and negative_prompt_embeds is None:
                neg = negative_prompt if negative_prompt is not None else [""] * len(plist)
                neg = [neg] * len(plist) if isinstance(neg, str) else neg
                negative_prompt_embeds = enc(neg)
        b, s, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.float().repeat(1, num_images_per_prompt, 1).view(b * num_images_per_prompt, s, -1)
        if do_cfg:
            if negative_prompt_embeds is None:
                raise ValueError("classifier-free guidance needs `negative_prompt_embeds` when `prompt_embeds` is given")
            negative_prompt_embeds = negative_prompt_embeds.float().repeat(1, num_images_per_prompt, 1).view(
                b * num_images_per_prompt, s, -1)
        return prompt_embeds, negative_prompt_embeds

    def prepare_image(self, image, width, height, batch_size, num_images_per_prompt, do_cfg=False):
        """pipeline_brushnet.py:741-774 — WITHOUT the CFG duplication (done after the VAE, see module docstring)."""
        image = self.image_processor.preprocess(image, height=height, width=width).to(dtype=torch.float32)
        repeat_by = batch_size if image.shape[0] == 1 else num_images_per_prompt
        return image if repeat_by == 1 else image.repeat_interleave(repeat_by, dim=0)

    def prepare_latents(self, batch_size, num_channels_latents, height, width, generator, latents=None):
        shape = (batch_size, num_channels_latents, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an "
                             f"effective batch size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None and isinstance(generator, PhiloxGenerator):
            # the library's stream: drawn on the device, init_noise_sigma applied by the draw itself (one rounding, as axpby_n's)
            generator.device = generator.device or torch.device(self.device)
            noise = generator.randn(shape, scale=float(self.scheduler.init_noise_sigma))
            return noise, noise
        if latents is None:
            noise = randn_tensor(shape, generator, self.device)      # on the generator's device, like randn_tensor
        else:
            noise = latents
        noise = noise.to(self.device, torch.float32)
        if self.scheduler.init_noise_sigma != 1.0:
            noise = hip.axpby_n([noise.contiguous()], [float(self.scheduler.init_noise_sigma)])
        return noise.contiguous(), noise

    def build_conditioning(self, image, mask, depth, height, width, batch, num_images_per_prompt, do_cfg,
                           conditioning_noise=None, normals=None, generator=None):
        """pipeline_brushnet.py:1116-1215: [masked-image latents | mask | depth | normals] at latent resolution.
        `conditioning_noise`: the VAE posterior noise of the CFG-duplicated batch — one tensor (image) or a sequence
        (image, depth, normals) for the 'latents' modes; None draws them in the reference's order from the global RNG, or, with a
        rng.PhiloxGenerator (or a list of them, one per sample) as `generator`, from it on the device."""
        return self._conditioning(image, mask, depth, height, width, batch, num_images_per_prompt, do_cfg, conditioning_noise,
                                  normals, generator)[0]

    def _conditioning(self, image, mask, depth, height, width, batch, num_images_per_prompt, do_cfg, conditioning_noise=None,
                      normals=None, generator=None, shared: Optional[bool] = None):
        """build_conditioning, and with it whether both classifier-free-guidance halves got identical VAE posterior samples (what
        _brushnet_shareable asks).  `shared`: the caller has decided that already (export_conditioning)."""
        img = self.prepare_image(image, width, height, batch, num_images_per_prompt)
        m3 = self.prepare_image(mask, width, height, batch, num_images_per_prompt)
        original_mask = hip.mask_keep(m3) if m3.is_cuda else (m3.sum(1)[:, None, :, :] < 0).to(torch.float32)   # :1139 (1 = keep)
        height, width = img.shape[-2:]
        hl, wl = height // self.vae_scale_factor, width // self.vae_scale_factor
        dup = 2 if do_cfg else 1
        lat_c = self.vae.config["latent_channels"]
        sf = float(self.vae.config["scaling_factor"])
        noises = list(conditioning_noise) if isinstance(conditioning_noise, (list, tuple)) else [conditioning_noise]
        noises += [None] * (3 - len(noises))

        def encode_sample(x_host, noise):
            """vae.encode(x).latent_dist.sample() * scaling_factor for the CFG-duplicated batch: B images are encoded
            once and sampled once per CFG half (the reference encodes the duplicated batch, :1188)."""
            nonlocal identical
            moments = self.vae._moments(x_host)
            if noise is None and philox:
                # the same shapes and order as the global-RNG draws below; a list of generators draws each half sample by sample
                if dup == 2 and self.cfg_shared_conditioning_sample:
                    noise = randn_tensor((batch, lat_c, hl, wl), generator, self.device).repeat(2, 1, 1, 1)
                elif isinstance(generator, (list, tuple)) and len(generator) > 1:
                    noise = torch.cat([randn_tensor((batch, lat_c, hl, wl), generator, self.device) for _ in range(dup)])
                    identical = False
                else:
                    noise = randn_tensor((dup * batch, lat_c, hl, wl), generator, self.device)
                    identical = False
            elif noise is None:
                if dup == 2 and self.cfg_shared_conditioning_sample:
                    noise = torch.randn(batch, lat_c, hl, wl, dtype=torch.float32).repeat(2, 1, 1, 1)
                else:
                    noise = torch.randn(dup * batch, lat_c, hl, wl, dtype=torch.float32)   # global RNG, like vae.py:782-791
                    identical = False     # two independent draws: never identical
            if noise.shape[0] != dup * batch:
                raise ValueError(f"conditioning_noise must have batch {dup * batch}")
            if dup == 2 and identical:
                # whether both CFG halves get the same sample is decided HERE, from how the noise was made (a host compare of a
                # host tensor; a device tensor costs one read-back) — not by comparing the built conditioning on the device
                # (export_conditioning decides before it records: the compare is a torch kernel a program cannot hold)
                identical = bool(torch.equal(noise[:batch], noise[batch:])) if shared is None else bool(shared)
            noise = noise.to(self.device, torch.float32)
            return [hip.vae_sample(moments, noise[i * batch:(i + 1) * batch].contiguous(), lat_c, sf) for i in range(dup)]

        philox = is_philox(generator)
        identical = dup == 2
        halves = encode_sample(img, noises[0])
        parts = [[h] for h in halves]
        mask_l = hip.nearest_resize(hip.h2d(original_mask, self.device), hl, wl)                   # :1189-1195
        for ps in parts:
            ps.append(mask_l)
        if self.depth_conditioning_mode is not None:
            d = self.prepare_image(depth, width, height, batch, num_images_per_prompt)
            if self.depth_conditioning_mode == "concat":
                dl = hip.nearest_resize(hip.h2d(d, self.device), hl, wl)                           # :1198-1202
                for ps in parts:
                    ps.append(dl)
            else:
                for ps, h in zip(parts, encode_sample(d.repeat(1, 3, 1, 1), noises[1])):           # :1203-1206
                    ps.append(h)
        if self.normals_conditioning_mode not in (None, "ip_adapter"):
            nrm = self.prepare_image(normals, width, height, batch, num_images_per_prompt)
            if self.normals_conditioning_mode == "concat":
                nl = hip.nearest_resize(hip.h2d(nrm, self.device), hl, wl)                         # :1208-1212
                for ps in parts:
                    ps.append(nl)
            else:
                for ps, h in zip(parts, encode_sample(nrm, noises[2])):                            # :1213-1215
                    ps.append(h)
        # torch.cat along channels of each CFG half (:1196-1215) by the front-end kernel; stacking the halves is a copy
        return torch.cat([hip.concat_channels(ps, batch) for ps in parts], 0).contiguous(), identical

    # ---- the call --------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt=None, image=None, mask=None, depth=None, normals=None, height: Optional[int] = None,
                 width: Optional[int] = None, num_inference_steps: int = 50, timesteps: List[int] = None,
                 guidance_scale: float = 7.5, negative_prompt=None, num_images_per_prompt: Optional[int] = 1,
                 eta: float = 0.0, generator=None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                 ip_adapter_image=None, ip_adapter_image_embeds=None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, cross_attention_kwargs=None,
                 brushnet_conditioning_scale: Union[float, List[float]] = 1.0, guess_mode: bool = False,
                 control_guidance_start: Union[float, List[float]] = 0.0,
                 control_guidance_end: Union[float, List[float]] = 1.0, clip_skip: Optional[int] = None,
                 callback_on_step_end: Optional[Callable] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"],
                 conditioning_noise: Optional[torch.Tensor] = None, _timing: Optional[dict] = None, _export: Optional[dict] = None,
                 _added: Optional[dict] = None, _end: Optional[float] = None, _rescale: float = 0.0, **kwargs):
        # private keywords, all call-scoped: `_timing` (bench.py), `_export` (export_denoise_step's request; its result comes back in it), and
        # from the XL subclass `_added` (added_cond_kwargs of the CFG-duplicated batch), `_end` (denoising_end), `_rescale` (guidance_rescale)
        callback = kwargs.pop("callback", None)
        callback_steps = kwargs.pop("callback_steps", None)
        ip_mode = self.normals_conditioning_mode == "ip_adapter"
        if ip_adapter_image is not None:
            raise NotImplementedError("ip_adapter_image (the CLIP vision tower of an image-prompt IP-Adapter) is not built")
        if ip_adapter_image_embeds is not None and not ip_mode:
            raise NotImplementedError("ip_adapter_image_embeds are taken in normals_conditioning_mode='ip_adapter' only (the mirror normal's token)")
        if ip_mode and not getattr(self.unet, "_ip_procs", None):
            raise ValueError("normals_conditioning_mode='ip_adapter' needs IP-Adapter processors on the UNet: unet.load_ip_adapter(...) or "
                             "unet.set_attn_processor({...attn2.processor: MfhipIPAttnProcessor(...)})")
        lora_models = self._lora_models()
        if cross_attention_kwargs and not lora_models:
            raise NotImplementedError("cross_attention_kwargs (LoRA scale) are not built")
        if lora_models:                      # adapters are always merged: this call's scale is merged here, before anything is captured
            lora_scale = _lora.scale_of(cross_attention_kwargs)
            for m in lora_models:
                m.set_lora_scale(1.0 if lora_scale is None else lora_scale)
                m._lora_sync()
        if timesteps is not None and "timesteps" not in inspect.signature(self.scheduler.set_timesteps).parameters:
            # retrieve_timesteps (pipeline_brushnet.py:113-119): the reference's DDIM / PNDM / UniPC `set_timesteps` take no custom
            # schedule either and the reference raises exactly this (LCMScheduler's takes one: below)
            raise ValueError(f"The current scheduler class {self.scheduler.__class__}'s `set_timesteps` does not support custom"
                             f" timestep schedules. Please check whether you are using the correct scheduler.")
        if guess_mode and type(self) is not StableDiffusionBrushNetPipeline:
            raise NotImplementedError("guess_mode is built for the SD1.5 pipeline")
        if isinstance(control_guidance_start, list) or isinstance(control_guidance_end, list):
            control_guidance_start = control_guidance_start[0] if isinstance(control_guidance_start, list) else control_guidance_start
            control_guidance_end = control_guidance_end[0] if isinstance(control_guidance_end, list) else control_guidance_end
        self.check_inputs(prompt, image, mask, callback_steps, negative_prompt, prompt_embeds, negative_prompt_embeds,
                          brushnet_conditioning_scale, control_guidance_start, control_guidance_end,
                          callback_on_step_end_tensor_inputs, depth=depth, normals=normals)
        self._guidance_scale = guidance_scale
        guard = self.unet.prec.name == "f16x3" and self.device.type == "cuda"
        if guard:
            hip.split_overflow(reset=True)       # the range guard of the fp16 split precision counts this call only
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None:
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        do_cfg = self.do_classifier_free_guidance
        # (the SD1.5 form by name: the XL subclass has its own encode_prompt and hands this loop finished embeddings)
        prompt_embeds, negative_prompt_embeds = StableDiffusionBrushNetPipeline.encode_prompt(
            self, prompt, num_images_per_prompt, do_cfg, negative_prompt, prompt_embeds, negative_prompt_embeds, clip_skip=clip_skip)
        pe = torch.cat([negative_prompt_embeds, prompt_embeds]) if do_cfg else prompt_embeds         # :1103
        pe = pe.to(self.device)
        nb = batch_size * num_images_per_prompt
        # what the UNet reads: the 'ip_adapter' normals mode appends its token (BrushNet keeps the text's 77)
        pe_u = self._append_normal_token(pe, batch_size, num_images_per_prompt, do_cfg, normals, ip_adapter_image_embeds) if ip_mode else pe
        if ip_mode:
            normals = None                    # a [B, 1, 3] vector, consumed above: no normals map enters the conditioning

        first = image[0] if isinstance(image, list) else image
        if height is None or width is None:
            if torch.is_tensor(first) or isinstance(first, np.ndarray):
                hh, ww = (first.shape[-2:] if torch.is_tensor(first) else first.shape[-3:-1] if first.ndim == 4 else first.shape[:2])
            else:
                ww, hh = first.size
            height, width = height or int(hh), width or int(ww)
        # guess_mode (:771-772, 1260-1264): the conditioning is NOT doubled, BrushNet sees the conditional batch only
        cond, identical = self._conditioning(image, mask, depth, height, width, nb, num_images_per_prompt, do_cfg and not guess_mode,
                                             conditioning_noise, normals, generator)
        once = self._brushnet_once = (not guess_mode) and self._brushnet_shareable(cond, nb, do_cfg, identical)

        if timesteps is not None:                                                                   # retrieve_timesteps :113-125
            self.scheduler.set_timesteps(timesteps=timesteps, device=self.device)
            num_inference_steps = len(self.scheduler.timesteps)
        else:
            self.scheduler.set_timesteps(num_inference_steps, device=self.device)                   # :1171
        ts = self.scheduler.timesteps
        if _end is not None and isinstance(_end, float) and 0.0 < _end < 1.0:                        # pipeline_brushnet_sd_xl.py:1376-1391
            ntrain = int(self.scheduler.config["num_train_timesteps"])
            cutoff = int(round(ntrain - _end * ntrain))
            num_inference_steps = len([t for t in ts.tolist() if t >= cutoff])
            ts = ts[:num_inference_steps]
        self._num_timesteps = len(ts)
        latents, _ = self.prepare_latents(nb, self.unet.config["in_channels"], height, width, generator, latents)
        timestep_cond = None                 # :1218-1223: the guidance scale as an embedding, for the UNet only (BrushNet never sees it, :1277)
        if self.unet.config.get("time_cond_proj_dim") is not None:
            timestep_cond = self.get_guidance_scale_embedding(torch.tensor(self.guidance_scale - 1).repeat(nb),
                                                              embedding_dim=self.unet.config["time_cond_proj_dim"]).to(self.device, torch.float32)

        keep = [1.0 - float(i / len(ts) < control_guidance_start or (i + 1) / len(ts) > control_guidance_end)
                for i in range(len(ts))]                                                             # :1236-1242
        rescale = float(_rescale or 0.0)
        num_warmup = len(ts) - num_inference_steps * self.scheduler.order
        if _timing is not None:          # HIP events on the launch stream around the denoise loop (bench.py)
            _timing["host_before_denoise"] = time.perf_counter()
            _timing["denoise_start"] = torch.cuda.Event(enable_timing=True)
            _timing["denoise_end"] = torch.cuda.Event(enable_timing=True)
            _timing["denoise_start"].record()
        fused_ddim = do_cfg and isinstance(self.scheduler, DDIMScheduler) and eta == 0.0 and rescale == 0.0
        # (without classifier-free guidance the captured step serves LCMScheduler, whose calls run there by design; the other samplers'
        # unguided calls keep the eager loop they have always had)
        use_graph = (self.use_hip_graph and (do_cfg or isinstance(self.scheduler, LCMScheduler)) and callback is None
                     and (fused_ddim or eta == 0.0) and rescale == 0.0
                     and all(k == 1.0 for k in keep) and len(ts) > 2 and not guess_mode)
        # THE place that decides how a step ends.  PNDM / UniPC / DPM-Solver++ / Euler update on the device (one plan row per step) unless
        # a callback may read the scheduler between steps, or an eps-form step program is being exported; the eager loop always steps them
        # on the host.  The SDE type of DPM-Solver++ and Euler-ancestral draw noise at every step: on the device only from ONE
        # rng.PhiloxGenerator (the library's stream, which the kernel can draw); a torch.Generator, none, or a list of generators steps on
        # the host.  LCM draws too (every step but the last).
        sde = isinstance(self.scheduler, (EulerAncestralDiscreteScheduler, LCMScheduler)) or (
            isinstance(self.scheduler, DPMSolverMultistepScheduler) and self.scheduler.config["algorithm_type"] == "sde-dpmsolver++")
        if fused_ddim:
            update = _FusedDDIM(self, guidance_scale)
        elif (use_graph and callback_on_step_end is None and not (_export is not None and _export["scheduler"] == "host")
              and isinstance(self.scheduler, (PNDMScheduler, UniPCMultistepScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler,
                                              LCMScheduler))
              and (not sde or isinstance(generator, PhiloxGenerator))):
            update = _DevicePlan(self, guidance_scale, len(ts), generator if sde else None)
        else:
            update = _HostStep(self, guidance_scale, rescale, eta, generator)

        def step_end(i, t, lat):           # callback_on_step_end: the latents to go on with (its own, if it returns some)
            if callback_on_step_end is None:
                return lat
            avail = dict(latents=lat, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds)
            new = (callback_on_step_end(self, i, t, {k: avail[k] for k in callback_on_step_end_tensor_inputs}) or {}).pop("latents", None)
            return lat if new is None else new

        with self.progress_bar(total=num_inference_steps) as bar:
            if use_graph:
                latents = self._denoise_graph(latents, ts, pe, pe_u, cond, nb, guidance_scale, float(brushnet_conditioning_scale), once,
                                              _added, update, step_end, bar, _export, do_cfg, timestep_cond)
                ts = []
            for i, t in enumerate(ts):                                                               # :1250 HOT LOOP
                # step 0 autotunes GEMM tiles: keep its timings undisturbed; guess_mode re-packs the residuals on this
                # stream (the per-residual events are keyed by the tensors BrushNet returned)
                self._overlap(i > 0 and not guess_mode)
                eu, ec = self._predict_noise(latents, t, pe, pe_u, cond, nb, float(brushnet_conditioning_scale) * keep[i], do_cfg, once,
                                             guess_mode, _added, timestep_cond=timestep_cond)
                latents = step_end(i, t, update.eager(eu, ec, t, latents))
                if i == len(ts) - 1 or ((i + 1) > num_warmup and (i + 1) % self.scheduler.order == 0):
                    bar.update()
                    if callback is not None and callback_steps and i % callback_steps == 0:
                        callback(i // getattr(self.scheduler, "order", 1), t, latents)

        self._overlap(False)
        if _timing is not None:
            _timing["denoise_end"].record()
            _timing["host_after_denoise"] = time.perf_counter()
        if output_type != "latent":
            sf = float(self.vae.config["scaling_factor"])
            z = hip.axpby_n([latents.contiguous()], [1.0 / sf])                                     # :1342
            img = self.vae.decode(z, return_dict=False)[0]
        else:
            img = latents
        img = self.image_processor.postprocess(img, output_type=output_type, do_denormalize=[True] * img.shape[0])
        if guard:
            raised = hip.split_overflow(reset=True)
            if raised:
                raise hip.SplitRangeError(
                    f"f16x3: an activation exceeded the fp16 range (|x| > 65504, flags {raised:#x}) during this call; its products "
                    "were computed from saturated halves, so the result is not returned.  Run this input with precision "
                    "'bf16x3' (fp32 range) or 'fp32'.")
        if not return_dict:
            return (img, None)
        return StableDiffusionPipelineOutput(images=img, nsfw_content_detected=None)

    def _append_normal_token(self, pe: torch.Tensor, batch: int, per_prompt: int, do_cfg: bool, normals, embeds) -> torch.Tensor:
        """MirrorFusionModel.forward (train_brushnet_mirror.py:868-871): encoder_hidden_states = cat([text, ip_tokens], dim=1) for the UNet
        only.  `embeds`: [t] with t [2B or B, 1, C], what the reference's get_normal_embeds returns (:75-88: the same token in both
        classifier-free-guidance halves); or `normals` [B, 1, 3] through self.normal_embedder.  B is the number of prompts.  `pe` is [negative | positive], each half prompt-major (p0, p0, p1, p1 for two images per prompt:
        encode_prompt's repeat + view), so the token of prompt i is repeated in place for its images, never tiled across prompts."""
        if embeds is not None:
            tok = embeds[0] if isinstance(embeds, (list, tuple)) else embeds
        else:
            if normals is None or self.normal_embedder is None:
                raise ValueError("normals_conditioning_mode='ip_adapter' takes ip_adapter_image_embeds=[token], or normals=[B, 1, 3] with "
                                 "pipe.normal_embedder set (frontend.NormalEmbedder)")
            nv = torch.as_tensor(normals, dtype=torch.float32)
            if nv.dim() == 2:
                nv = nv[:, None, :]
            tok = self.normal_embedder(nv)
        tok = tok.to(pe.device, pe.dtype)
        if tok.dim() != 3 or tok.shape[1] != 1 or tok.shape[2] != pe.shape[2]:
            raise ValueError(f"the normal token must be [B, 1, {pe.shape[2]}], got {tuple(tok.shape)}")
        rows = tok.shape[0]
        if rows == batch:                             # one token per prompt: the same in every guidance half
            parts = [tok] * (2 if do_cfg else 1)
        elif do_cfg and rows == 2 * batch:            # get_normal_embeds' [unconditional | conditional] stack
            parts = [tok[:batch], tok[batch:]]
        else:
            raise ValueError(f"the normal token's batch is {rows}: expected one token per prompt ({batch})"
                             + (f" or the two guidance halves stacked ({2 * batch})" if do_cfg else ""))
        return torch.cat([pe, torch.cat([t.repeat_interleave(per_prompt, dim=0) for t in parts])], 1).contiguous()

    def _predict_noise(self, latents, t, pe, pe_u, cond, nb, cond_scale, do_cfg, once, guess_mode, added, temb=(None, None), lazy=None,
                       timestep_cond=None):
        """The body of a denoise step up to the scheduler update (pipeline_brushnet.py:1256-1296), for the eager loop and for the
        captured step alike: BrushNet, the UNet with its residuals, and the noise prediction's (unconditional, conditional) halves —
        (eps, None) without classifier-free guidance.  `once` / `guess_mode`: BrushNet sees one half of the batch (the halves are identical
        / the conditional one, :1260-1264); `pe_u`: the UNet's own prompt embeddings; `temb`: the step's rows of the (UNet's, BrushNet's)
        time-embedding tables; `lazy`: unet.lazy_injection_names(); `timestep_cond`: the UNet's guidance-scale embedding (a `temb` row block
        holds it already)."""
        x_in = torch.cat([latents] * 2) if do_cfg else latents                                       # :1256
        x_in = self.scheduler.scale_model_input(x_in, t)          # (returns its input for DDIM / PNDM / UniPC: no launch)
        cond_only = guess_mode and do_cfg
        down, mid, up = self.brushnet(x_in[nb:] if cond_only else x_in[:nb] if once else x_in, t,
                                      encoder_hidden_states=pe[nb:] if cond_only else pe[:nb] if once else pe,
                                      brushnet_cond=cond[:nb] if (once or cond_only) else cond, conditioning_scale=cond_scale,
                                      added_cond_kwargs=added, guess_mode=guess_mode, return_dict=False, _temb=temb[1], _lazy=lazy)   # :1277
        if cond_only:                       # zeros keep the unconditional half unchanged (:1287-1293); copies only, eager loop only
            down = [torch.cat([torch.zeros_like(d), d]) for d in down]
            mid = torch.cat([torch.zeros_like(mid), mid])
            up = [torch.cat([torch.zeros_like(u), u]) for u in up]
        eps = self.unet(x_in, t, encoder_hidden_states=pe_u, down_block_add_samples=down, mid_block_add_sample=mid,
                        up_block_add_samples=up, added_cond_kwargs=added, return_dict=False, _temb=temb[0],
                        timestep_cond=timestep_cond if temb[0] is None else None)[0]                                                 # :1296
        return (eps[:nb], eps[nb:]) if do_cfg else (eps, None)

    def _brushnet_shareable(self, cond: torch.Tensor, nb: int, do_cfg: bool, identical: Optional[bool] = None) -> bool:
        """Under classifier-free guidance the reference feeds BrushNet the duplicated batch (pipeline_brushnet.py:1256-1277:
        torch.cat([latents] * 2), [negative | positive] prompt embeddings, the conditioning latents of the duplicated image
        batch).  The BrushNet built by from_unet is attention-free (brushnet.py:484-486), so it never reads the prompt
        embeddings: its two halves differ ONLY through the conditioning latents, whose VAE posterior the reference samples
        independently per half (:1188 on the image doubled at :771-772).  When the two halves of `cond` are bit-identical
        (conditioning_noise with equal halves, or cfg_shared_conditioning_sample) both halves are the same function of the
        same inputs: BrushNet is evaluated once per image and the UNet's injection adds read each residual for both
        halves (mf_gemm_desc.res1_rows).  Never when an added embedding depends on the prompt (SDXL's pooled text
        embedding enters BrushNet-XL's time embedding)."""
        if not (do_cfg and self.share_brushnet_cfg and self.brushnet.config.get("addition_embed_type") is None
                and self.brushnet.config.get("class_embed_type") is None):
            return False
        # identical halves <=> every VAE posterior sample that went into `cond` was the same for both halves (mask, depth and
        # normals maps are deterministic functions of the inputs): `identical`, as _conditioning returned it with `cond` — no device
        # compare / sync; a caller that holds the tensor alone pays for one
        return bool(torch.equal(cond[:nb], cond[nb:]) if identical is None else identical)

    def _overlap(self, on: bool):
        """Turn the BrushNet || UNet stream overlap (models._RESIDUAL_EVENTS) on or off for the next forward calls."""
        if on and self.overlap_brushnet and self.device.type == "cuda":
            # torch hands streams out of a pool of 32 per device, round robin: the 33rd torch.cuda.Stream of a process IS the first.
            # A side stream that is the stream it forks from (torch.cuda.graph's capture stream is a pool stream too) would put
            # BrushNet and the UNet back on one stream — no overlap, and a recorded step program with one stream — so pick again.
            cur = torch.cuda.current_stream(self.device).cuda_stream
            if self._side_stream is None or self._side_stream.device != self.device or cur in (self._side_stream.cuda_stream, self._aux_stream.cuda_stream):
                taken = {cur}
                for name in ("_side_stream", "_aux_stream"):
                    for _ in range(64):
                        stream = torch.cuda.Stream(device=self.device)
                        if stream.cuda_stream not in taken:
                            break
                    taken.add(stream.cuda_stream)
                    setattr(self, name, stream)
            self.brushnet.side_stream = self._side_stream
            # an auxiliary stream for UNet launches off its critical path (shortcut convs, V projections).  BrushNet
            # keeps a single stream: a fork of the already forked side stream segfaults in hipStreamEndCapture
            # (ROCm 7.2), and its shortcut convs already overlap the UNet
            self.unet.aux_stream = self._aux_stream if self.overlap_aux else None
        else:
            self.brushnet.side_stream = None
            self.unet.aux_stream = self.brushnet.aux_stream = None

    def _denoise_graph(self, latents, ts, pe, pe_u, cond, nb, guidance_scale, cond_scale, once, added, update, step_end, bar, export=None,
                       do_cfg=True, timestep_cond=None):
        """The hot loop as ONE captured hipGraph replayed per timestep (BrushNet + UNet + CFG + what `update` launches, ~800
        kernels on two streams): launch overhead disappears and the host only refreshes two tiny device buffers
        (timestep, the update's row) between replays.  DDIM's update is inside the graph (_FusedDDIM); so is that of the multistep
        schedulers (_DevicePlan), unless a callback_on_step_end may read the scheduler between steps or an eps-form step program is
        exported: then they get the guided noise prediction from the graph and step eagerly (_HostStep).  `export`: the request of
        export_denoise_step, the capture of step 1 is recorded as a program too.  The first step runs eagerly: it autotunes GEMM tiles,
        binds the prompt (cross-attention K/V cache) and sizes every scratch buffer before anything is captured.  `do_cfg`: False runs the
        step on the undoubled batch (LCMScheduler's calls at guidance_scale <= 1 or on a guidance-distilled UNet, whose `timestep_cond`
        enters the UNet's time-embedding table) and hands the update ec=None; part of the graph's key."""
        dev = latents.device
        tvals = ts.to(torch.float32).to(dev)
        ip = pe_u is not pe                                   # the 'ip_adapter' normals mode: the UNet reads its own embeddings
        # The captured graph (and every buffer it reads) is kept across calls with the same shapes and scalars:
        # new inputs are copied INTO the static buffers, so repeated calls pay no capture / instantiate cost.  The key
        # carries each model's weights generation: load_state_dict / .to() rebuild every weight tensor (and the UNet's
        # cross-attention K/V cache), so a graph captured before that points at freed buffers and must not be replayed.
        key = (tuple(latents.shape), tuple(pe.shape), tuple(cond.shape), float(guidance_scale), cond_scale, update.key,
               str(dev), id(self.unet), self.unet._weights_gen, id(self.brushnet), self.brushnet._weights_gen, once,
               tuple((k, tuple(v.shape)) for k, v in sorted(added.items())) if added else None,
               tuple(pe_u.shape) if ip else None, self.unet.ip_signature() if hasattr(self.unet, "ip_signature") else None,
               bool(do_cfg), timestep_cond is not None)
        st = self._graph_state if self._graph_state is not None and self._graph_state["key"] == key else None
        if st is None:
            st = dict(key=key, graph=None, lat=torch.empty_like(latents), pe=torch.empty_like(pe),
                      cond=torch.empty_like(cond), t_cur=torch.empty(1, dtype=torch.float32, device=dev))
            if added:
                st["added"] = {k: torch.empty(v.shape, dtype=torch.float32, device=dev) for k, v in added.items()}
            if ip:
                st["pe_unet"] = torch.empty_like(pe_u)
            self._graph_state = st
        lat, t_cur = st["lat"].copy_(latents), st["t_cur"]
        update.attach(st, lat, ts)
        added = {k: st["added"][k].copy_(v) for k, v in added.items()} if added else added      # (the static buffers, refilled)
        pe, cond = st["pe"].copy_(pe), st["cond"].copy_(cond)
        pe_u = st["pe_unet"].copy_(pe_u) if ip else pe
        # every timestep is known here: both nets' time embeddings and the fused time_emb_proj GEMM run ONCE for
        # the whole schedule (4 batched launches per net) instead of 8 dependent launches at the head of every step; the
        # graph reads one row block per step from a static buffer.  Kept across calls with the same schedule.
        tkey = (tuple(float(t) for t in ts.tolist()), self.unet._weights_gen, self.brushnet._weights_gen,
                float(guidance_scale) if timestep_cond is not None else None)
        if self.precompute_time_embedding and (st.get("temb_key") != tkey or added):
            nrows_b = nb if once else pe.shape[0]
            st["temb_tab"] = (self.unet.time_embedding_table(tvals, pe.shape[0], added, timestep_cond),
                              self.brushnet.time_embedding_table(tvals, nrows_b, added))
            st["temb_key"] = tkey
            if "temb_cur" not in st or any(c.shape != t.shape[1:] for c, t in zip(st["temb_cur"], st["temb_tab"])):
                if st["graph"] is not None:
                    raise RuntimeError("time-embedding table changed shape under a captured graph")
                st["temb_cur"] = tuple(torch.empty_like(t[0]) for t in st["temb_tab"])
        temb_u, temb_b = st["temb_cur"] if self.precompute_time_embedding else (None, None)

        # residuals that land on a proj_out are never computed: their zero-conv becomes a second K segment of that GEMM
        lazy = self.unet.lazy_injection_names() if (self.fold_zero_convs and not once and do_cfg) else None

        def one_step():
            eu, ec = self._predict_noise(lat, t_cur, pe, pe_u, cond, nb, cond_scale, do_cfg, once, False, added, (temb_u, temb_b), lazy,
                                         timestep_cond)
            update.launch(eu, ec, lat)

        # A graph captured by an earlier call with this key serves every step, the first included: what depends on the
        # prompt alone (its device copy, the cross-attention K / V^T) is recomputed into the buffers the graph reads.
        if export is not None:
            st["graph"] = None                                    # (a graph kept from an earlier call is captured again)
        replay_all = (export is None and st["graph"] is not None and os.environ.get("MFHIP_EAGER_FIRST") != "1"      # A/B switch
                      and self.unet.bind_prompt(pe_u))
        for i in range(len(ts)):
            t_cur.copy_(tvals[i:i + 1])
            update.load(i)
            if temb_u is not None:
                temb_u.copy_(st["temb_tab"][0][i])
                temb_b.copy_(st["temb_tab"][1][i])
            if i == 0 and not replay_all:
                one_step()                                   # eager: tunes GEMMs, binds the prompt K/V, sizes scratch
            else:
                if st["graph"] is None:                      # capture does not execute: replay below runs this step
                    st["graph"] = self._capture(one_step) if export is None else self._export_capture(
                        one_step, export, update, st, lat, temb_u, temb_b, cond, len(ts), i, guidance_scale, cond_scale, once)
                st["graph"].replay()
            update.after_replay(ts[i], lat)
            cur = update.sample(lat)
            new = step_end(i, ts[i], cur)
            if new is not cur:
                update.replace(new, lat)
            bar.update()
        update.finish()
        return update.sample(lat).clone()

    def _capture(self, one_step, rec=None):
        """Capture one_step() into a hipGraph (nothing executes) and return it.  `rec`: a program.Recorder(capture=True) that ALSO
        writes the captured pass down as a step program (program.py)."""
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        self._overlap(True)                      # the side stream forks from / joins the capture stream
        # No automatic garbage collection inside the capture: a collection that falls into it runs the destructors of
        # whatever cyclic garbage the process holds (graphs, memory pools, events of earlier calls), and a HIP call made
        # from one of them while the stream captures ends the process.  torch.cuda.graph collects once on entry; what
        # becomes garbage during the capture waits until it has ended.
        gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            # (thread_local: with an initialised process group its watchdog thread may poll events while this thread captures)
            with torch.cuda.graph(graph, capture_error_mode="thread_local" if (torch.distributed.is_available() and torch.distributed.is_initialized()) else "global"):
                self._overlap(True)              # (again, now that the capture stream is current: never the side stream itself)
                with rec if rec is not None else contextlib.nullcontext():
                    one_step()
        except Exception:
            if rec is not None and rec.error is not None:
                raise rec.error                  # (not the "unjoined work" the aborted capture reports on top of it)
            raise
        finally:
            if gc_was_enabled:
                gc.enable()
            self._overlap(False)
        return graph

    def _export_capture(self, one_step, export, update, st, lat, temb_u, temb_b, cond, nsteps, step, guidance_scale, cond_scale, once):
        """_capture with ONE denoise step (the loop body of pipeline_brushnet.py:1250-1332) recorded inside the hipGraph capture of that
        step: the program carries the capture's forks and joins (BrushNet || UNet), replayed by mf_denoise_step_fused."""
        from . import program
        if temb_u is None:
            raise NotImplementedError("export_denoise_step needs precompute_time_embedding (the step reads one row block of the schedule's table)")
        io, tables = update.export()
        rec = program.Recorder(dict(latents=lat, temb_unet=temb_u, temb_brushnet=temb_b, cond=cond, **io),
                               {"table.temb_unet": st["temb_tab"][0].contiguous(), "table.temb_brushnet": st["temb_tab"][1].contiguous(), **tables},
                               capture=True)
        graph = self._capture(one_step, rec)
        rec.finish(graph.pool())                  # (nothing ran: the buffers still hold what they held BEFORE the recorded step)
        meta = dict(entry="mf_denoise_step_fused", reference="pipelines/brushnet/pipeline_brushnet.py:1250-1332", precision=self.unet.prec.name,
                    result=update.result, latents=list(lat.shape), steps=nsteps, recorded_step=step, guidance_scale=float(guidance_scale),
                    conditioning_scale=cond_scale if isinstance(cond_scale, (int, float)) else list(cond_scale),
                    temb_unet=list(temb_u.shape), temb_brushnet=list(temb_b.shape), brushnet_once=bool(once), **getattr(update, "meta", {}))
        export["info"] = rec.save(export["path"], meta=json.dumps(meta))
        export["info"]["meta"] = meta
        return graph

    def export_denoise_step(self, path: str, scheduler: str = "host", **call_kwargs) -> dict:
        """Run the pipeline once and write the denoise step's program to `path` (see program.py / include/mfhip.h "step programs").
        `call_kwargs`: what __call__ takes; the program is specialised on their shapes, the prompt (its cross-attention K / V^T are
        constants of the file), the guidance and conditioning scales, and the schedule (its tables travel as named constants).
        `scheduler` (PNDM, UniPC, DPM-Solver++, Euler): "host" ends the step with the guided noise prediction in the io buffer "eps" for the host's own
        scheduler; "device" records the update too (mf_sched_step_dev: io buffers "sched_row" / "sched_state", table "table.sched_row"),
        so that mf_denoise_step_fused alone runs a whole step.  DDIM's update is inside either way.  DPM-Solver++ exports like UniPC; its SDE
        type needs generator=rng.PhiloxGenerator(seed) for "device" (mf_sched_step_noise_dev + mf_philox_advance on the io buffer
        "philox_state", the generator's device pair; meta["philox"] holds per_sample, global_batch and the blocks a step consumes).  Euler and
        Euler-ancestral (the latter like the SDE type) keep the sample in slot meta["sample_slot"] of "sched_state" and the model input in
        "latents": a host starts a run by writing x0 (noise * init_noise_sigma) into that slot and x0 * meta["first_input_scale"] into
        "latents"; after the last step of a full schedule the two are equal."""
        if self.device.type != "cuda":
            raise hip.MfhipError("export_denoise_step needs the device: a program is a recording of real launches")
        if scheduler not in ("host", "device"):
            raise ValueError(f"export_denoise_step: scheduler must be 'host' or 'device', not {scheduler!r}")
        if scheduler == "device" and not isinstance(self.scheduler, (DDIMScheduler, PNDMScheduler, UniPCMultistepScheduler,
                                                                     DPMSolverMultistepScheduler, EulerDiscreteScheduler, LCMScheduler)):
            raise NotImplementedError(f"{type(self.scheduler).__name__} has no device update")
        if (scheduler == "device" and not isinstance(call_kwargs.get("generator"), PhiloxGenerator)
                and (getattr(self.scheduler, "config", {}).get("algorithm_type") == "sde-dpmsolver++"
                     or isinstance(self.scheduler, (EulerAncestralDiscreteScheduler, LCMScheduler)))):
            raise NotImplementedError("a step program of the DPM-Solver++ SDE / Euler-ancestral / LCM update draws its noise in the kernel: pass "
                                      "generator=rng.PhiloxGenerator(seed), or export with scheduler='host'")
        self._refuse_unguided_export("export_denoise_step", call_kwargs)
        from . import program
        program.refuse_ip_processors(self.unet)      # before anything is captured (the recorder would refuse in the middle of a two-stream capture)
        request = dict(path=path, scheduler=scheduler, info=None)       # travels with the call; _denoise_graph leaves the result in it
        call_kwargs.setdefault("output_type", "latent")
        out = self(**call_kwargs, _export=request)
        if request["info"] is None:
            raise hip.MfhipError("export_denoise_step: the call did not reach a second denoise step on the graph path (num_inference_steps >= 2, "
                                 "use_graph left on)")
        request["info"]["result"] = out
        return request["info"]

    def _refuse_unguided_export(self, what: str, call_kwargs: dict) -> None:
        """Before any file is written: the captured step without classifier-free guidance (LCMScheduler at guidance_scale <= 1, or a UNet
        with time_cond_proj_dim) has no step-program form yet.  Other schedulers' unguided calls never reach the captured step."""
        distilled = self.unet.config.get("time_cond_proj_dim") is not None
        if (isinstance(self.scheduler, LCMScheduler) or distilled) and (distilled or float(call_kwargs.get("guidance_scale", 7.5)) <= 1):
            raise NotImplementedError(f"{what} without classifier-free guidance ("
                                      + ("the UNet has time_cond_proj_dim" if distilled else "guidance_scale <= 1 under LCMScheduler")
                                      + "): a step program's hosts feed the doubled batch and both halves of the noise prediction; export "
                                      "under guidance_scale > 1, or run the call through the pipeline")

    # ---- the two ends of a call as step programs (program.py; include/mfhip.h "step programs") --------------------------------
    def _refuse_vae_switches(self, what: str, batch: int, height: int, width: int, decode: bool = True) -> None:
        """NotImplementedError if VAE tiling / slicing is on and would apply to the exported encode (pixels) or decode (latents)."""
        refuse = getattr(self.vae, "refuse_export", None)
        if refuse is None:
            return
        refuse(what, batch, int(height), int(width), latents=False)
        if decode:
            refuse(what, batch, int(height) // self.vae_scale_factor, int(width) // self.vae_scale_factor, latents=True)

    def _u8_pixels(self, x, name: str) -> torch.Tensor:
        from . import program
        t = torch.as_tensor(np.asarray(x)) if not torch.is_tensor(x) else x
        if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
            raise program.ProgramError(f"`{name}` is uint8 pixels [B, H, W, 3] (what a host holds after decoding an image file), "
                                       f"got {t.dtype} {tuple(t.shape)}")
        return (t[None] if t.dim() == 3 else t).to(self.device).contiguous()

    def export_conditioning(self, path: str, image=None, mask=None, depth=None, conditioning_noise=None, height: Optional[int] = None,
                            width: Optional[int] = None, num_images_per_prompt: int = 1) -> dict:
        """build_conditioning (pipeline_brushnet.py:1116-1215) under classifier-free guidance as a program for mf_build_conditioning,
        preceded by the uint8 ingest (mf_u8_to_planes): io buffers "image_u8" / "mask_u8" (uint8 [B, H, W, 3]), "depth" (fp32
        [B, 1, H, W] in [-1, 1], as `pipe(depth=)` takes it; only with depth_conditioning_mode='concat'), "cond_noise" (the VAE posterior
        noise) and "cond" (the denoise step's conditioning buffer).  `conditioning_noise` of batch B, or of 2B with bit-identical halves,
        exports the SHARED form (one draw for both guidance halves: "cond_noise" holds B images and the step runs BrushNet once);
        otherwise "cond_noise" holds 2B.  The meta records which, and the `brushnet_once` a step exported from the same call carries.
        Whatever the recorder cannot express (another depth / normals mode, several images per prompt: torch kernels between the
        launches) raises ProgramError here, and no file is written."""
        from . import program
        if self.device.type != "cuda":
            raise hip.MfhipError("export_conditioning needs the device: a program is a recording of real launches")
        if type(self) is not StableDiffusionBrushNetPipeline:
            raise NotImplementedError("export_conditioning is built for the SD1.5 pipeline")
        if conditioning_noise is None or isinstance(conditioning_noise, (list, tuple)):
            raise program.ProgramError("export_conditioning takes ONE conditioning_noise tensor: random numbers stay the caller's")
        image_u8, mask_u8 = self._u8_pixels(image, "image"), self._u8_pixels(mask, "mask")
        if image_u8.shape != mask_u8.shape:
            raise program.ProgramError(f"image {tuple(image_u8.shape)} and mask {tuple(mask_u8.shape)} differ in shape")
        nb = image_u8.shape[0] * int(num_images_per_prompt)
        height, width = height or int(image_u8.shape[1]), width or int(image_u8.shape[2])
        self._refuse_vae_switches("export_conditioning", nb, height, width, decode=False)
        noise = conditioning_noise.to(self.device, torch.float32).contiguous()
        if noise.shape[0] not in (nb, 2 * nb):
            raise ValueError(f"conditioning_noise must have batch {nb} (one draw shared by both guidance halves) or {2 * nb}")
        shared = noise.shape[0] == nb or bool(torch.equal(noise[:nb], noise[nb:]))
        noise = noise[:nb].contiguous() if shared else noise
        named = dict(image_u8=image_u8, mask_u8=mask_u8, cond_noise=noise)
        if self.depth_conditioning_mode is not None:
            if depth is None:
                raise ValueError(f"depth_conditioning_mode={self.depth_conditioning_mode!r} needs a `depth` input")
            depth = torch.as_tensor(depth).to(self.device, torch.float32).contiguous()
            named["depth"] = depth

        def run():                                # (`shared` is decided above: the compare is a torch kernel a program cannot hold)
            img, msk = hip.u8_to_planes(image_u8), hip.u8_to_planes(mask_u8)
            return self._conditioning(img, msk, depth, height, width, nb, num_images_per_prompt, True,
                                      torch.cat([noise, noise]) if shared else noise, None, shared=shared)
        run()                                     # warm: tiles tuned, scratch sized
        with program.Recorder(named) as rec:
            cond, identical = run()
            rec.output("cond", cond)
        once = self._brushnet_shareable(cond, nb, True, identical)
        meta = dict(entry="mf_build_conditioning", reference="pipelines/brushnet/pipeline_brushnet.py:1116-1215", precision=self.vae.prec.name,
                    depth_conditioning_mode=self.depth_conditioning_mode, cond_noise_batch=int(noise.shape[0]), batch=nb,
                    shared_conditioning_sample=bool(shared), brushnet_once=bool(once), layouts=rec.layouts)
        info = rec.save(path, meta=json.dumps(meta))
        info["meta"] = meta
        return info

    # -- LoRA adapters (pipeline_brushnet.py:128-145 LoraLoaderMixin; lora.py) ---------------------------------------------------------
    def _lora_models(self) -> list:
        """The UNet / HIP text encoder that hold adapters."""
        return [m for m in (self.unet, self.text_encoder) if hasattr(m, "_lora_state") and m._lora_state() is not None]

    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, adapter_name: Optional[str] = None, weight_name: Optional[str] = None,
                          **kwargs) -> None:
        """LoraLoaderMixin.load_lora_weights: a diffusers, legacy attention-processor or kohya LoRA (dict, .safetensors file or a directory
        holding pytorch_lora_weights.safetensors).  `unet.` / `lora_unet_` keys (and keys without a prefix) bind to the UNet,
        `text_encoder.` / `lora_te_` keys to the HIP text encoder.  Both models are checked before either is changed."""
        if kwargs:
            raise NotImplementedError(f"load_lora_weights: {sorted(kwargs)} are not built")
        self._lora_refuse_xl("load_lora_weights")
        groups = _lora.group_keys(_lora.read_state_dict(pretrained_model_name_or_path_or_dict, weight_name))
        unet_entries = OrderedDict(list(groups["unet"].items()) + list(groups[""].items()))
        te_entries = groups["text_encoder"]
        if not unet_entries and not te_entries:
            raise ValueError("load_lora_weights: the state dict holds no LoRA weights")
        if te_entries:
            from .text_encoder import CLIPTextModel
            if not isinstance(self.text_encoder, CLIPTextModel):
                raise NotImplementedError("the file holds text-encoder LoRA keys: they load into the HIP text encoder (text_encoder.CLIPTextModel), "
                                          "which this pipeline was not built with")
        name = adapter_name or f"default_{max([len(m._lora_state().adapters) for m in self._lora_models()] or [0])}"
        for model, entries in ((self.unet, unet_entries), (self.text_encoder, te_entries)):      # check everything before anything is changed
            if entries:
                model._lora_guard()
                _lora.resolve(entries, model.param_shapes(), model.lora_modules())
                if model._lora_state() is not None and name in model._lora_state().adapters:
                    raise ValueError(f"adapter_name {name!r} is already loaded: unload_lora_weights() or pick another name")
        for model, entries in ((self.unet, unet_entries), (self.text_encoder, te_entries)):
            if entries:
                model.load_lora(None, adapter_name=name, _entries=entries)

    def set_adapters(self, adapter_names, adapter_weights=None) -> None:
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        models = self._lora_models()
        known = {n for m in models for n in m._lora_state().adapters}
        for n in names:
            if n not in known:
                raise ValueError(f"set_adapters: adapter {n!r} is not loaded (have {sorted(known)})")
        if adapter_weights is None or isinstance(adapter_weights, (int, float)):
            adapter_weights = [1.0 if adapter_weights is None else float(adapter_weights)] * len(names)
        if len(adapter_weights) != len(names):
            raise ValueError(f"set_adapters: {len(names)} names and {len(adapter_weights)} weights")
        for m in models:                      # an adapter may touch one of the two models only
            have = [(n, w) for n, w in zip(names, adapter_weights) if n in m._lora_state().adapters]
            m.set_adapters([n for n, _ in have], [w for _, w in have])

    def get_active_adapters(self) -> List[str]:
        out: List[str] = []
        for m in self._lora_models():
            out += [n for n in m.active_adapters() if n not in out]
        return out

    def fuse_lora(self, fuse_unet: bool = True, fuse_text_encoder: bool = True, lora_scale: float = 1.0, safe_fusing: bool = False) -> None:
        self._lora_refuse_xl("fuse_lora")
        for m, on in ((self.unet, fuse_unet), (self.text_encoder, fuse_text_encoder)):
            if on and m in self._lora_models():
                m.fuse_lora(lora_scale=lora_scale, safe_fusing=safe_fusing)

    def unfuse_lora(self, unfuse_unet: bool = True, unfuse_text_encoder: bool = True) -> None:
        for m, on in ((self.unet, unfuse_unet), (self.text_encoder, unfuse_text_encoder)):
            if on and m in self._lora_models():
                m.unfuse_lora()

    def unload_lora_weights(self) -> None:
        for m in self._lora_models():
            m.unload_lora()

    def _lora_refuse_xl(self, what: str) -> None:
        if type(self) is not StableDiffusionBrushNetPipeline:
            raise NotImplementedError(f"{type(self).__name__}.{what}: LoRA loading is built for the SD1.5 pipeline (SDXL's two text encoders and "
                                      "SGM key maps are not); at the model level a diffusers-format adapter loads into the SDXL UNet")

    def export_call(self, directory: str, **call_kwargs) -> dict:
        """Run the pipeline once and write the whole call as five programs plus manifest.json / manifest.txt into `directory`:
        encode_prompt.mfprog (mf_encode_prompt), bind_prompt.mfprog, conditioning.mfprog (mf_build_conditioning), step.mfprog
        (mf_denoise_step_fused, scheduler="device": DDIM, PNDM and UniPC are one loop for the host) and decode.mfprog (mf_decode_image).
        `call_kwargs`: what __call__ takes, with `prompt` (and optionally `negative_prompt`) as text for the pipeline's tokenizer,
        `image` / `mask` as uint8 pixels [B, H, W, 3], `depth` as the normalised fp32 map and `conditioning_noise` given (tokenisation,
        file decoding and random numbers stay the caller's).  examples/c_host/inpaint_host.c runs the directory without Python."""
        from . import program
        from .text_encoder import CLIPTextModel
        if isinstance(self.scheduler, EulerDiscreteScheduler):       # before any file is written
            raise NotImplementedError(f"export_call under {type(self.scheduler).__name__}: the exported call's host loop feeds the sample "
                                      "to the step, the Euler family's step reads the scaled model input (export_denoise_step carries it)")
        self._refuse_unguided_export("export_call", call_kwargs)
        program.refuse_ip_processors(self.unet)
        for m in self._lora_models():
            if m._lora_state().pinned is None:
                raise NotImplementedError("export_call with LoRA adapters loaded but not fused: the exported programs hold one set of weights; "
                                          "call fuse_lora(lora_scale=...) first")
        if type(self) is not StableDiffusionBrushNetPipeline:
            raise NotImplementedError("export_call is built for the SD1.5 pipeline (SDXL's pooled text embedding feeds export-time tables)")
        if self.normals_conditioning_mode is not None or call_kwargs.get("guess_mode"):
            raise program.ProgramError("export_call: normals conditioning and guess_mode are outside the exported call")
        kw = dict(call_kwargs)
        if float(kw.get("guidance_scale", 7.5)) <= 1:
            raise program.ProgramError("export_call: the exported call runs under classifier-free guidance (guidance_scale > 1)")
        px = kw.get("image")
        if px is not None:                                   # before any file is written: no partial export
            shape = tuple(px.shape) if torch.is_tensor(px) else np.asarray(px).shape
            if len(shape) in (3, 4):
                self._refuse_vae_switches("export_call", (1 if len(shape) == 3 else shape[0]) * int(kw.get("num_images_per_prompt", 1) or 1),
                                          kw.get("height") or shape[-3], kw.get("width") or shape[-2])
        if not isinstance(self.text_encoder, CLIPTextModel) or self.tokenizer is None or kw.get("prompt") is None:
            raise program.ProgramError("export_call needs the HIP text encoder (text_encoder.CLIPTextModel), a tokenizer and `prompt`")
        prompt, nipp = kw.pop("prompt"), int(kw.get("num_images_per_prompt", 1) or 1)
        plist = [prompt] if isinstance(prompt, str) else list(prompt)
        neg = kw.pop("negative_prompt", None)
        neg = [""] * len(plist) if neg is None else [neg] * len(plist) if isinstance(neg, str) else list(neg)
        ids = self.tokenizer(neg + plist, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                             return_tensors="pt").input_ids.to(self.device, torch.int32).contiguous()
        image_u8, mask_u8 = self._u8_pixels(kw.pop("image", None), "image"), self._u8_pixels(kw.pop("mask", None), "mask")
        noise, depth, clip_skip = kw.get("conditioning_noise"), kw.get("depth"), kw.get("clip_skip")
        os.makedirs(directory, exist_ok=True)
        files = dict(encode_prompt="encode_prompt.mfprog", bind_prompt="bind_prompt.mfprog", conditioning="conditioning.mfprog",
                     step="step.mfprog", decode="decode.mfprog")
        path = {k: os.path.join(directory, v) for k, v in files.items()}
        self._graph_state = None
        step = self.export_denoise_step(path["step"], scheduler="device", prompt=plist, negative_prompt=neg,
                                        image=hip.u8_to_planes(image_u8), mask=hip.u8_to_planes(mask_u8), **kw)
        latents = step["result"].images
        infos = dict(step=step, bind_prompt=program.export_bind_prompt(self.unet, path["bind_prompt"]),
                     encode_prompt=program.export_encode_prompt(self.text_encoder, path["encode_prompt"], ids, clip_skip=clip_skip),
                     conditioning=self.export_conditioning(path["conditioning"], image=image_u8, mask=mask_u8, depth=depth,
                                                           conditioning_noise=noise, height=kw.get("height"), width=kw.get("width"),
                                                           num_images_per_prompt=nipp),
                     decode=program.export_vae_decode(self.vae, path["decode"], latents, postprocess=True))
        cm, sm = infos["conditioning"]["meta"], step["meta"]
        if cm["brushnet_once"] != sm["brushnet_once"]:
            raise program.ProgramError("export_call: the conditioning program and the step disagree on brushnet_once")
        manifest = dict(abi_version=hip.ABI_VERSION, precision=self.unet.prec.name, scheduler=type(self.scheduler).__name__,
                        steps=int(sm["steps"]), batch=int(cm["batch"]), brushnet_once=bool(sm["brushnet_once"]),
                        cond_noise_batch=int(cm["cond_noise_batch"]), depth=self.depth_conditioning_mode is not None,
                        init_noise_sigma=float(self.scheduler.init_noise_sigma), files=files,
                        io={k: {n: dict(shape=l["shape"], dtype=l["dtype"]) for n, l in v["meta"]["layouts"].items()} for k, v in infos.items()
                            if "layouts" in v["meta"]},
                        shared_buffers=dict(prompt_embeds=["encode_prompt", "bind_prompt"], cond=["conditioning", "step"],
                                            latents=["step", "decode"]))
        manifest["io"]["step"] = dict(latents=dict(shape=list(sm["latents"]), dtype="float32"))
        program.write_manifest(directory, manifest)
        return dict(directory=directory, manifest=manifest, programs=infos, result=step["result"])

    def _sched_step(self, noise_pred, t, latents, extra):
        """The host's scheduler step.  `extra`: the eta / generator keywords its step() takes, decided once per call (_HostStep)."""
        return self.scheduler.step(noise_pred, t, latents, **extra, return_dict=False)[0]


class StableDiffusionXLBrushNetPipeline(StableDiffusionBrushNetPipeline):
    """pipelines/brushnet/pipeline_brushnet_sd_xl.py:936-1535 on the same engine: the SDXL UNet / BrushNet-XL add the
    'text_time' embedding (pooled text embedding + Fourier features of original size / crop / target size) to the time
    embedding; conditioning is [masked-image latents | mask] (5 channels, :1301-1310); everything else is the
    SD1.5 loop.  Prompts go through encode_prompt (text_encoder.CLIPTextModel / CLIPTextModelWithProjection, or the caller's
    torch modules); prompt_embeds / pooled_prompt_embeds are taken as they are."""

    def __init__(self, vae, text_encoder, text_encoder_2, tokenizer, tokenizer_2, unet, brushnet, scheduler,
                 force_zeros_for_empty_prompt: bool = True, add_watermarker=None, feature_extractor=None,
                 image_encoder=None):
        super().__init__(vae=vae, text_encoder=text_encoder, tokenizer=tokenizer, unet=unet, brushnet=brushnet,
                         scheduler=scheduler, safety_checker=None, feature_extractor=feature_extractor,
                         image_encoder=image_encoder, requires_safety_checker=False)
        if add_watermarker:
            raise NotImplementedError("the invisible watermark is outside the accelerated path")
        self.text_encoder_2, self.tokenizer_2 = text_encoder_2, tokenizer_2
        self.config.update(force_zeros_for_empty_prompt=force_zeros_for_empty_prompt)

    @classmethod
    def _assemble(cls, root, mods, sched, text_encoder, tokenizer, torch_dtype, device, kwargs):
        """`text_encoder_2/` goes into the HIP CLIPTextModelWithProjection when the folder exists and none was passed; `tokenizer_2`
        stays the caller's object."""
        text_encoder_2 = kwargs.pop("text_encoder_2", None)
        if text_encoder_2 is None and os.path.isdir(os.path.join(root, "text_encoder_2")):
            from .text_encoder import CLIPTextModelWithProjection
            text_encoder_2 = CLIPTextModelWithProjection.from_pretrained(root, subfolder="text_encoder_2", torch_dtype=torch_dtype, device=device)
        return cls(vae=mods["vae"], text_encoder=text_encoder, text_encoder_2=text_encoder_2, tokenizer=tokenizer,
                   tokenizer_2=kwargs.pop("tokenizer_2", None), unet=mods["unet"], brushnet=mods["brushnet"], scheduler=sched,
                   force_zeros_for_empty_prompt=kwargs.pop("force_zeros_for_empty_prompt", True),
                   feature_extractor=kwargs.pop("feature_extractor", None))

    def _get_add_time_ids(self, original_size, crops_coords_top_left, target_size, text_encoder_projection_dim):
        """pipeline_brushnet_sd_xl.py:_get_add_time_ids, including its consistency check against add_embedding."""
        ids = list(original_size) + list(crops_coords_top_left) + list(target_size)
        passed = self.unet.config["addition_time_embed_dim"] * len(ids) + text_encoder_projection_dim
        expected = self.unet.config["projection_class_embeddings_input_dim"]
        if expected != passed:
            raise ValueError(f"Model expects an added time embedding vector of length {expected}, but a vector of {passed} "
                             "was created. The model has an incorrect config. Please check "
                             "`unet.config.time_embedding_type` and `text_encoder_2.config.projection_dim`.")
        return torch.tensor([ids], dtype=torch.float32)

    @torch.no_grad()
    def encode_prompt(self, prompt, prompt_2=None, device=None, num_images_per_prompt: int = 1,
                      do_classifier_free_guidance: bool = True, negative_prompt=None, negative_prompt_2=None, prompt_embeds=None,
                      negative_prompt_embeds=None, pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None,
                      lora_scale=None, clip_skip: Optional[int] = None):
        """pipeline_brushnet_sd_xl.py:213-420 without LoRA / textual inversion: returns (prompt_embeds, negative_prompt_embeds,
        pooled_prompt_embeds, negative_pooled_prompt_embeds), fp32 on the pipeline's device.  Either text encoder may be None
        when the other exists (:299-302)."""
        device = device or self.device
        if lora_scale is not None:
            raise NotImplementedError("LoRA layers of the text encoders are outside the accelerated path")
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt) if prompt is not None else prompt_embeds.shape[0]
        tokenizers = [self.tokenizer, self.tokenizer_2] if self.tokenizer is not None else [self.tokenizer_2]
        text_encoders = [self.text_encoder, self.text_encoder_2] if self.text_encoder is not None else [self.text_encoder_2]
        if prompt_embeds is None or (do_classifier_free_guidance and negative_prompt_embeds is None):
            if any(m is None for m in tokenizers + text_encoders):
                raise ValueError("pass `prompt_embeds` / `pooled_prompt_embeds` or construct the pipeline with text encoders and tokenizers")

        def encode(texts, tokenizer, text_encoder, max_length):
            ids = tokenizer(texts, padding="max_length", max_length=max_length, truncation=True, return_tensors="pt").input_ids
            return text_encoder(ids.to(device), output_hidden_states=True)

        if prompt_embeds is None:
            prompt_2 = prompt_2 or prompt
            prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
            embeds_list = []
            for texts, tokenizer, text_encoder in zip([prompt, prompt_2], tokenizers, text_encoders):
                out = encode(texts, tokenizer, text_encoder, tokenizer.model_max_length)
                pooled_prompt_embeds = out[0]           # "We are only ALWAYS interested in the pooled output of the final text encoder"
                embeds_list.append(out.hidden_states[-2] if clip_skip is None else out.hidden_states[-(clip_skip + 2)])
            prompt_embeds = torch.concat(embeds_list, dim=-1)
        zero_out_negative_prompt = negative_prompt is None and self.config["force_zeros_for_empty_prompt"]
        if do_classifier_free_guidance and negative_prompt_embeds is None and zero_out_negative_prompt:
            negative_prompt_embeds = torch.zeros_like(prompt_embeds)
            negative_pooled_prompt_embeds = torch.zeros_like(pooled_prompt_embeds)
        elif do_classifier_free_guidance and negative_prompt_embeds is None:
            negative_prompt = negative_prompt or ""
            negative_prompt_2 = negative_prompt_2 or negative_prompt
            negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
            negative_prompt_2 = batch_size * [negative_prompt_2] if isinstance(negative_prompt_2, str) else negative_prompt_2
            if prompt is not None and type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                                f" {type(prompt)}.")
            elif batch_size != len(negative_prompt):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`:"
                                 f" {prompt} has batch size {batch_size}. Please make sure that passed `negative_prompt` matches"
                                 " the batch size of `prompt`.")
            embeds_list = []
            for texts, tokenizer, text_encoder in zip([negative_prompt, negative_prompt_2], tokenizers, text_encoders):
                out = encode(texts, tokenizer, text_encoder, prompt_embeds.shape[1])
                negative_pooled_prompt_embeds = out[0]
                embeds_list.append(out.hidden_states[-2])
            negative_prompt_embeds = torch.concat(embeds_list, dim=-1)
        bs_embed, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.to(device, torch.float32).repeat(1, num_images_per_prompt, 1).view(
            bs_embed * num_images_per_prompt, seq_len, -1)
        if do_classifier_free_guidance:
            seq_len = negative_prompt_embeds.shape[1]
            negative_prompt_embeds = negative_prompt_embeds.to(device, torch.float32).repeat(1, num_images_per_prompt, 1).view(
                batch_size * num_images_per_prompt, seq_len, -1)
        pooled_prompt_embeds = pooled_prompt_embeds.to(device, torch.float32).repeat(1, num_images_per_prompt).view(
            bs_embed * num_images_per_prompt, -1)
        if do_classifier_free_guidance:
            negative_pooled_prompt_embeds = negative_pooled_prompt_embeds.to(device, torch.float32).repeat(
                1, num_images_per_prompt).view(bs_embed * num_images_per_prompt, -1)
        return prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds

    @torch.no_grad()
    def __call__(self, prompt=None, prompt_2=None, image=None, mask=None, height=None, width=None,
                 num_inference_steps: int = 50, denoising_end=None, guidance_scale: float = 5.0, negative_prompt=None,
                 negative_prompt_2=None, num_images_per_prompt: int = 1, eta: float = 0.0, generator=None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_pooled_prompt_embeds=None, output_type="pil", return_dict: bool = True,
                 cross_attention_kwargs=None, guidance_rescale: float = 0.0, brushnet_conditioning_scale=1.0,
                 guess_mode: bool = False, control_guidance_start=0.0, control_guidance_end=1.0, original_size=None,
                 crops_coords_top_left=(0, 0), target_size=None, negative_original_size=None,
                 negative_crops_coords_top_left=(0, 0), negative_target_size=None, clip_skip=None,
                 callback_on_step_end=None, callback_on_step_end_tensor_inputs=("latents",), conditioning_noise=None,
                 **kwargs):
        if prompt is not None or prompt_2 is not None or negative_prompt is not None or negative_prompt_2 is not None:
            # pipeline_brushnet_sd_xl.py:1283-1302: prompts (and whichever embeddings were passed) through encode_prompt once, for ONE
            # image per prompt: the shared path below does the per-image repeats exactly as it does for passed-in embeddings
            if prompt is not None and prompt_embeds is not None:
                raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`. Please make sure to only forward one of the two.")
            if prompt is None and prompt_embeds is None:
                raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
            prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds = self.encode_prompt(
                prompt, prompt_2, self.device, 1, guidance_scale > 1, negative_prompt, negative_prompt_2, prompt_embeds=prompt_embeds,
                negative_prompt_embeds=negative_prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                negative_pooled_prompt_embeds=negative_pooled_prompt_embeds, clip_skip=clip_skip)
        if prompt_embeds is None or pooled_prompt_embeds is None:
            raise ValueError("If `prompt_embeds` are provided, `pooled_prompt_embeds` also have to be passed. Make sure to "
                             "generate `pooled_prompt_embeds` from the same text encoder that was used to generate `prompt_embeds`.")
        do_cfg = guidance_scale > 1
        if do_cfg and (negative_prompt_embeds is None or negative_pooled_prompt_embeds is None):
            raise ValueError("If `negative_prompt_embeds` are provided, `negative_pooled_prompt_embeds` also have to be passed.")
        ih, iw = self.image_processor.preprocess(image).shape[-2:]
        height, width = height or ih, width or iw
        original_size = original_size or (ih, iw)                                                   # :1330-1334
        target_size = target_size or (height, width)
        b = prompt_embeds.shape[0]
        nb = b * num_images_per_prompt
        pooled = pooled_prompt_embeds.float().repeat(1, num_images_per_prompt).view(nb, -1)         # encode_prompt :483-486
        proj_dim = int(pooled.shape[-1])
        ids = self._get_add_time_ids(original_size, crops_coords_top_left, target_size, proj_dim)
        if negative_original_size is not None and negative_target_size is not None:
            nids = self._get_add_time_ids(negative_original_size, negative_crops_coords_top_left, negative_target_size, proj_dim)
        else:
            nids = ids
        if do_cfg:
            npooled = negative_pooled_prompt_embeds.float().repeat(1, num_images_per_prompt).view(nb, -1)
            text = torch.cat([npooled, pooled], 0)
            ids = torch.cat([nids, ids], 0)
        else:
            text = pooled
        ids = ids.repeat(nb, 1)                                              # :1372 (sic: interleaves neg/pos rows)
        # denoising_end (pipeline_brushnet_sd_xl.py:1376-1391) and guidance_rescale (:1478-1480) are read by the shared loop
        return super().__call__(image=image, mask=mask, height=height, width=width, num_inference_steps=num_inference_steps,
                                guidance_scale=guidance_scale, num_images_per_prompt=num_images_per_prompt, eta=eta, generator=generator,
                                latents=latents, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                                output_type=output_type, return_dict=return_dict, cross_attention_kwargs=cross_attention_kwargs,
                                brushnet_conditioning_scale=brushnet_conditioning_scale, guess_mode=guess_mode,
                                control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end, clip_skip=clip_skip,
                                callback_on_step_end=callback_on_step_end, conditioning_noise=conditioning_noise,
                                callback_on_step_end_tensor_inputs=list(callback_on_step_end_tensor_inputs), _end=denoising_end, _rescale=guidance_rescale,
                                _added=dict(text_embeds=text.to(self.device), time_ids=ids.to(self.device)), **kwargs)
