"""DDIMScheduler and PNDMScheduler with the reference call surface, stepping on the device.

Reference: MirrorFusion/src/diffusers/schedulers/scheduling_ddim.py (set_timesteps :299-342, step :344-470,
add_noise :473-497) and scheduling_pndm.py (set_timesteps :168-226, step_prk :261-319, step_plms :321-390,
_get_prev_sample :407-448).  The scalar coefficients are computed on the host exactly like the reference
does (fp32 0-dim tensor arithmetic on the alphas_cumprod table); the per-element update is one HIP kernel
(mf_cfg_ddim_step / mf_axpby_n).  Latents stay fp32 whatever the model precision.  device_plan (end of the file) turns a PNDM /
UniPC / DPM-Solver++ / Euler / LCM schedule into rows for mf_sched_step_dev, the whole update of a step in one launch with device-resident coefficients.
EulerDiscreteScheduler / EulerAncestralDiscreteScheduler (scheduling_euler_discrete.py, scheduling_euler_ancestral_discrete.py) are the two
classes whose scale_model_input is not the identity: their plans keep the sample in a state slot and write the model input to the latents.
"""
from __future__ import annotations

import copy
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import hip
from .models import FrozenConfig


@dataclass
class SchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: Optional[torch.Tensor] = None


@dataclass
class LCMSchedulerOutput:
    prev_sample: torch.Tensor
    denoised: Optional[torch.Tensor] = None


def _betas(cfg) -> torch.Tensor:
    n = cfg["num_train_timesteps"]
    if cfg.get("trained_betas") is not None:
        return torch.tensor(cfg["trained_betas"], dtype=torch.float32)
    sch = cfg["beta_schedule"]
    if sch == "linear":
        return torch.linspace(cfg["beta_start"], cfg["beta_end"], n, dtype=torch.float32)
    if sch == "scaled_linear":
        return torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, n, dtype=torch.float32) ** 2
    raise NotImplementedError(f"{sch} is not implemented (reference supports it; outside the MirrorFusion path)")


class _SchedulerBase:
    order = 1
    _defaults: dict = {}

    def __init__(self, **kwargs):
        cfg = dict(self._defaults)
        unknown = [k for k in kwargs if k not in cfg]
        cfg.update({k: v for k, v in kwargs.items() if k in cfg})
        # configuration_utils.py register_to_config: remember which keys were left at their defaults, so that
        # from_config into another scheduler class falls back to THAT class's defaults for them
        cfg["_use_default_values"] = [k for k in self._defaults if k not in kwargs]
        self.config = FrozenConfig(cfg)
        self._unknown = unknown
        self.betas = _betas(cfg)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if cfg.get("set_alpha_to_one", True) else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps: Optional[int] = None
        self.timesteps = torch.from_numpy(np.arange(0, cfg["num_train_timesteps"])[::-1].copy().astype(np.int64))

    @classmethod
    def from_config(cls, config, **kwargs):
        """configuration_utils.py:~250: keys the target class does not know are dropped; keys the source left at
        its default fall back to the TARGET's defaults (`_use_default_values`)."""
        cfg = {k: v for k, v in dict(config).items() if not k.startswith("_")}
        use_default = dict(config).get("_use_default_values", [])
        cfg = {k: v for k, v in cfg.items() if k not in use_default}
        cfg.update(kwargs)
        return cls(**{k: v for k, v in cfg.items() if k in cls._defaults})

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    config_name = "scheduler_config.json"

    def save_config(self, path: str):
        """configuration_utils.py save_config: `scheduler_config.json` with `_class_name` (explicitly set keys only
        are what a later from_config into another class keeps; the rest is re-defaulted there)."""
        import json
        import os
        os.makedirs(path, exist_ok=True)
        cfg = {k: v for k, v in dict(self.config).items() if not k.startswith("_")}
        cfg["_class_name"] = type(self).__name__
        cfg["_diffusers_version"] = "0.27.0.dev0"
        with open(os.path.join(path, self.config_name), "w") as f:
            json.dump(cfg, f, indent=2, sort_keys=True)

    save_pretrained = save_config

    @classmethod
    def from_pretrained(cls, path: str, subfolder=None, **kwargs):
        import json
        import os
        d = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(d, cls.config_name)) as f:
            cfg = json.load(f)
        return cls.from_config(cfg, **kwargs)

    def __len__(self):
        return self.config["num_train_timesteps"]

    def _alpha(self, t: int) -> torch.Tensor:
        return self.alphas_cumprod[t] if t >= 0 else self.final_alpha_cumprod

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        """scheduling_ddim.py:473-497 (== DDPM): sqrt(a_t) x + sqrt(1 - a_t) eps, per-sample t."""
        ts = timesteps.cpu().long().reshape(-1)
        a = self.alphas_cumprod[ts]
        sa, sb = a ** 0.5, (1 - a) ** 0.5
        outs = []
        for i in range(original_samples.shape[0]):
            k = i if ts.numel() > 1 else 0
            outs.append(hip.axpby_n([original_samples[i].float().contiguous(), noise[i].float().contiguous()],
                                    [float(sa[k]), float(sb[k])]))
        return torch.stack(outs)

    def get_velocity(self, sample: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        """scheduling_ddpm.py:527-546: v = sqrt(a_t) eps - sqrt(1 - a_t) x, per-sample t."""
        ts = timesteps.cpu().long().reshape(-1)
        a = self.alphas_cumprod[ts]
        sa, sb = a ** 0.5, (1 - a) ** 0.5
        outs = []
        for i in range(sample.shape[0]):
            k = i if ts.numel() > 1 else 0
            outs.append(hip.axpby_n([noise[i].float().contiguous(), sample[i].float().contiguous()],
                                    [float(sa[k]), -float(sb[k])]))
        return torch.stack(outs)


class DDPMScheduler(_SchedulerBase):
    """The training script's noise scheduler (train_brushnet_mirror.py:957): only the forward-process half
    (`add_noise`, `get_velocity`, `alphas_cumprod`) is used there; sampling with it is not part of the path."""
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, variance_type="fixed_small", clip_sample=True, prediction_type="epsilon",
                     thresholding=False, dynamic_thresholding_ratio=0.995, clip_sample_range=1.0,
                     sample_max_value=1.0, timestep_spacing="leading", steps_offset=0,
                     rescale_betas_zero_snr=False)

    def set_timesteps(self, num_inference_steps: int, device=None):
        raise NotImplementedError("DDPMScheduler here is the training-side noise scheduler; sample with DDIM/PNDM/UniPC")

    def step(self, *args, **kwargs):
        raise NotImplementedError("DDPMScheduler here is the training-side noise scheduler; sample with DDIM/PNDM/UniPC")


class DDIMScheduler(_SchedulerBase):
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                     prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     clip_sample_range=1.0, sample_max_value=1.0, timestep_spacing="leading",
                     rescale_betas_zero_snr=False)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c["thresholding"] or c["rescale_betas_zero_snr"]:
            raise NotImplementedError("thresholding / rescale_betas_zero_snr are outside the MirrorFusion path")
        if c["prediction_type"] not in ("epsilon", "v_prediction"):
            raise NotImplementedError(f"prediction_type {c['prediction_type']}")

    def set_timesteps(self, num_inference_steps: int, device=None):
        c = self.config
        if num_inference_steps > c["num_train_timesteps"]:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                             f"`self.config.train_timesteps`: {c['num_train_timesteps']}")
        self.num_inference_steps = num_inference_steps
        sp = c["timestep_spacing"]
        if sp == "linspace":
            ts = np.linspace(0, c["num_train_timesteps"] - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        elif sp == "leading":
            ratio = c["num_train_timesteps"] // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
            ts += c["steps_offset"]
        elif sp == "trailing":
            ratio = c["num_train_timesteps"] / num_inference_steps
            ts = np.round(np.arange(c["num_train_timesteps"], 0, -ratio)).astype(np.int64) - 1
        else:
            raise ValueError(f"{sp} is not supported. Please make sure to choose one of 'leading' or 'trailing'.")
        self.timesteps = torch.from_numpy(ts)           # kept on the host: the loop indexes coefficient tables

    def _get_variance(self, timestep, prev_timestep):
        a_t, a_p = self._alpha(int(timestep)), self._alpha(int(prev_timestep))
        return ((1 - a_p) / (1 - a_t)) * (1 - a_t / a_p)

    def step_coefficients(self, timestep: int, eta: float = 0.0) -> Tuple[float, float, float, float, float]:
        """(sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sigma) as the reference computes them."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        timestep = int(timestep)
        prev_t = timestep - self.config["num_train_timesteps"] // self.num_inference_steps
        a_t, a_p = self._alpha(timestep), self._alpha(prev_t)
        b_t = 1 - a_t
        std = eta * self._get_variance(timestep, prev_t) ** 0.5 if eta > 0 else torch.tensor(0.0)
        return (float(a_t ** 0.5), float(b_t ** 0.5), float(a_p ** 0.5), float((1 - a_p - std ** 2) ** 0.5), float(std))

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, eta: float = 0.0,
             use_clipped_model_output: bool = False, generator=None, variance_noise: Optional[torch.Tensor] = None,
             return_dict: bool = True, _cfg: Optional[Tuple[torch.Tensor, torch.Tensor, float]] = None):
        """scheduling_ddim.py:344-470.  `_cfg=(eps_uncond, eps_cond, guidance)` fuses the guidance combine
        (pipeline_brushnet.py:1310-1312) into the same kernel."""
        if use_clipped_model_output:
            raise NotImplementedError("use_clipped_model_output")
        sa, sb, sp, dirc, std = self.step_coefficients(timestep, eta)
        c = self.config
        clip = float(c["clip_sample_range"]) if c["clip_sample"] else 0.0
        ptype = 0 if c["prediction_type"] == "epsilon" else 1
        x = sample.float().contiguous()
        if _cfg is not None:
            eu, ec, g = _cfg
            prev = hip.cfg_ddim_step(eu, ec, float(g), x, sa, sb, sp, dirc, pred_type=ptype, clip=clip)
        else:
            prev = hip.cfg_ddim_step(model_output.float().contiguous(), None, -1.0, x, sa, sb, sp, dirc,
                                     pred_type=ptype, clip=clip)
        if eta > 0:
            if variance_noise is None:
                from .rng import randn_tensor
                variance_noise = randn_tensor(model_output.shape, generator, prev.device)   # scheduling_ddim.py:455-458
            prev = hip.axpby_n([prev, variance_noise.to(prev.device).float().contiguous()], [1.0, std])
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)


class PNDMScheduler(_SchedulerBase):
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, skip_prk_steps=False, set_alpha_to_one=False, prediction_type="epsilon",
                     timestep_spacing="leading", steps_offset=0)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if self.config["prediction_type"] not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {self.config['prediction_type']} must be one of `epsilon` or `v_prediction`")
        self.pndm_order = 4
        self.cur_model_output = None
        self.counter = 0
        self.cur_sample = None
        self.ets: List[torch.Tensor] = []
        self.prk_timesteps = None
        self.plms_timesteps = None
        self.timesteps = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        c = self.config
        self.num_inference_steps = num_inference_steps
        nt = c["num_train_timesteps"]
        sp = c["timestep_spacing"]
        if sp == "linspace":
            _ts = np.linspace(0, nt - 1, num_inference_steps).round().astype(np.int64)
        elif sp == "leading":
            _ts = (np.arange(0, num_inference_steps) * (nt // num_inference_steps)).round()
            _ts = _ts + c["steps_offset"]
        elif sp == "trailing":
            _ts = np.round(np.arange(nt, 0, -nt / num_inference_steps))[::-1].astype(np.int64) - 1
        else:
            raise ValueError(f"{sp} is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'.")
        if c["skip_prk_steps"]:
            self.prk_timesteps = np.array([])
            self.plms_timesteps = np.concatenate([_ts[:-1], _ts[-2:-1], _ts[-1:]])[::-1].copy()
        else:
            prk = np.array(_ts[-self.pndm_order:]).repeat(2) + np.tile(
                np.array([0, nt // num_inference_steps // 2]), self.pndm_order)
            self.prk_timesteps = (prk[:-1].repeat(2)[1:-1])[::-1].copy()
            self.plms_timesteps = _ts[:-3][::-1].copy()
        self.timesteps = torch.from_numpy(np.concatenate([self.prk_timesteps, self.plms_timesteps]).astype(np.int64))
        self.ets = []
        self.counter = 0
        self.cur_model_output = None
        self.cur_sample = None

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True):
        if self.counter < len(self.prk_timesteps) and not self.config["skip_prk_steps"]:
            return self.step_prk(model_output, timestep, sample, return_dict)
        return self.step_plms(model_output, timestep, sample, return_dict)

    def _check_ready(self):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")

    def step_prk(self, model_output, timestep, sample, return_dict: bool = True):
        self._check_ready()
        timestep = int(timestep)
        ratio = self.config["num_train_timesteps"] // self.num_inference_steps
        diff_to_prev = 0 if self.counter % 2 else ratio // 2
        prev_t = timestep - diff_to_prev
        timestep = int(self.prk_timesteps[self.counter // 4 * 4])
        mo = model_output.float().contiguous()
        acc = self.cur_model_output
        if self.counter % 4 == 0:
            self.cur_model_output = hip.axpby_n([mo], [1 / 6]) if acc is None else hip.axpby_n([acc, mo], [1.0, 1 / 6])
            self.ets.append(mo)
            self.cur_sample = sample
        elif (self.counter - 1) % 4 == 0 or (self.counter - 2) % 4 == 0:
            self.cur_model_output = hip.axpby_n([acc, mo], [1.0, 1 / 3])
        else:
            mo = hip.axpby_n([acc, mo], [1.0, 1 / 6])
            self.cur_model_output = None
        cur_sample = self.cur_sample if self.cur_sample is not None else sample
        prev = self._get_prev_sample(cur_sample, timestep, prev_t, mo)
        self.counter += 1
        return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)

    def step_plms(self, model_output, timestep, sample, return_dict: bool = True):
        self._check_ready()
        if not self.config["skip_prk_steps"] and len(self.ets) < 3:
            raise ValueError(f"{self.__class__} can only be run AFTER scheduler has been run in 'prk' mode for at "
                             "least 12 iterations")
        timestep = int(timestep)
        ratio = self.config["num_train_timesteps"] // self.num_inference_steps
        prev_t = timestep - ratio
        mo = model_output.float().contiguous()
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(mo)
        else:
            prev_t = timestep
            timestep = timestep + ratio
        e = self.ets
        if len(e) == 1 and self.counter == 0:
            self.cur_sample = sample
        elif len(e) == 1 and self.counter == 1:
            mo = hip.axpby_n([mo, e[-1]], [0.5, 0.5])
            sample = self.cur_sample
            self.cur_sample = None
        elif len(e) == 2:
            mo = hip.axpby_n([e[-1], e[-2]], [3 / 2, -1 / 2])
        elif len(e) == 3:
            mo = hip.axpby_n([e[-1], e[-2], e[-3]], [23 / 12, -16 / 12, 5 / 12])
        else:
            mo = hip.axpby_n([e[-1], e[-2], e[-3], e[-4]], [55 / 24, -59 / 24, 37 / 24, -9 / 24])
        prev = self._get_prev_sample(sample, timestep, prev_t, mo)
        self.counter += 1
        return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)

    def _get_prev_sample(self, sample, timestep, prev_timestep, model_output):
        """Formula (9) of PNDM (scheduling_pndm.py:407-448) as one fused linear combination."""
        a_t, a_p = self._alpha(int(timestep)), self._alpha(int(prev_timestep))
        b_t, b_p = 1 - a_t, 1 - a_p
        sample_coeff = (a_p / a_t) ** 0.5
        denom = a_t * b_p ** 0.5 + (a_t * b_t * a_p) ** 0.5
        k = -(a_p - a_t) / denom
        x = sample.float().contiguous()
        if self.config["prediction_type"] == "v_prediction":
            # eps = sqrt(a_t) v + sqrt(b_t) x  ->  prev = (sample_coeff + k sqrt(b_t)) x + k sqrt(a_t) v
            return hip.axpby_n([x, model_output], [float(sample_coeff + k * b_t ** 0.5), float(k * a_t ** 0.5)])
        return hip.axpby_n([x, model_output], [float(sample_coeff), float(k)])


class UniPCMultistepScheduler(_SchedulerBase):
    """schedulers/scheduling_unipc_multistep.py (bh1/bh2, predict_x0, lower_order_final; what the reference's own
    scripts select: examples/brushnet/test_brushnet.py:158, train_brushnet_mirror.py:179).  Predictor (:455-582) and
    corrector (:584-719) are linear in {sample, last_sample, converted model outputs}: the host evaluates the scalar
    coefficients exactly like the reference (fp32 0-dim tensor arithmetic on lambda = log(alpha) - log(sigma), expm1)
    and each update is ONE fused mf_axpby_n launch."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False,
                     dynamic_thresholding_ratio=0.995, sample_max_value=1.0, predict_x0=True, solver_type="bh2",
                     lower_order_final=True, disable_corrector=[], solver_p=None, use_karras_sigmas=False,
                     timestep_spacing="linspace", steps_offset=0, set_alpha_to_one=True)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c["thresholding"] or c["use_karras_sigmas"] or c["solver_p"] is not None or not c["predict_x0"]:
            raise NotImplementedError("thresholding / Karras sigmas / solver_p / noise-prediction UniPC are outside the MirrorFusion path")
        if c["solver_type"] not in ("bh1", "bh2"):
            raise NotImplementedError(f"{c['solver_type']} does is not implemented for {self.__class__}")
        if c["prediction_type"] not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {c['prediction_type']} must be one of `epsilon` or `v_prediction`")
        if c["solver_order"] > 3:
            raise NotImplementedError("solver_order > 3")
        self.sigmas = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        self.model_outputs = [None] * c["solver_order"]
        self.lower_order_nums = 0
        self.last_sample = None
        self._step_index = None
        self.disable_corrector = list(c["disable_corrector"])

    @property
    def step_index(self):
        return self._step_index

    def set_timesteps(self, num_inference_steps: int, device=None):
        c = self.config
        nt = c["num_train_timesteps"]
        if c["timestep_spacing"] == "linspace":
            ts = np.linspace(0, nt - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c["timestep_spacing"] == "leading":
            ts = (np.arange(0, num_inference_steps + 1) * (nt // (num_inference_steps + 1))).round()[::-1][:-1].copy().astype(np.int64)
            ts += c["steps_offset"]
        elif c["timestep_spacing"] == "trailing":
            ts = np.arange(nt, 0, -nt / num_inference_steps).round().copy().astype(np.int64) - 1
        else:
            raise ValueError(f"{c['timestep_spacing']} is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'.")
        sig = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sigmas = np.interp(ts, np.arange(0, len(sig)), sig)
        last = ((1 - self.alphas_cumprod[0]) / self.alphas_cumprod[0]) ** 0.5
        new_sigmas = torch.from_numpy(np.concatenate([sigmas, [last]]).astype(np.float32))
        # the scalar coefficients depend only on (sigma table, step index, order): memoised across calls so that the
        # host arithmetic (0-dim tensor math + a small linear solve, ~0.9 ms per step) leaves the critical path
        if getattr(self, "_coef_cache", None) is None or self.sigmas.shape != new_sigmas.shape \
                or not torch.equal(self.sigmas, new_sigmas):
            self._coef_cache = {}
        self.sigmas = new_sigmas
        self.timesteps = torch.from_numpy(ts)
        self.num_inference_steps = len(ts)
        self.model_outputs = [None] * c["solver_order"]
        self.lower_order_nums = 0
        self.last_sample = None
        self._step_index = None

    @staticmethod
    def _alpha_sigma(sigma):
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
        return alpha_t, sigma * alpha_t

    def _coefs(self, order, idx_t, idx_s0, hist_offset):
        alpha_t, sigma_t = self._alpha_sigma(self.sigmas[idx_t])
        alpha_s0, sigma_s0 = self._alpha_sigma(self.sigmas[idx_s0])
        lambda_s0 = torch.log(alpha_s0) - torch.log(sigma_s0)
        h = (torch.log(alpha_t) - torch.log(sigma_t)) - lambda_s0
        rks = []
        for i in range(1, order):
            a_si, s_si = self._alpha_sigma(self.sigmas[self._step_index - (i + hist_offset)])
            rks.append((torch.log(a_si) - torch.log(s_si) - lambda_s0) / h)
        rks_t = torch.tensor([float(r) for r in rks] + [1.0])
        hh = -h
        h_phi_1 = torch.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1
        B_h = hh if self.config["solver_type"] == "bh1" else torch.expm1(hh)
        R, b, fact = [], [], 1
        for i in range(1, order + 1):
            R.append(torch.pow(rks_t, i - 1))
            b.append(h_phi_k * fact / B_h)
            fact *= i + 1
            h_phi_k = h_phi_k / hh - 1 / fact
        return alpha_t, sigma_t, sigma_s0, h_phi_1, B_h, rks, torch.stack(R), torch.tensor([float(v) for v in b])

    def _index_for_timestep(self, timestep):
        cand = (self.timesteps == int(timestep)).nonzero()
        if len(cand) == 0:
            return len(self.timesteps) - 1
        return int(cand[1]) if len(cand) > 1 else int(cand[0])

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._step_index = self._index_for_timestep(timestep)
        c = self.config
        eps = model_output.float().contiguous()
        x = sample.float().contiguous()
        use_corrector = self._step_index > 0 and self._step_index - 1 not in self.disable_corrector \
            and self.last_sample is not None
        # convert_model_output (:385-453): x0 prediction, linear in (sample, model_output)
        a_c, s_c = self._alpha_sigma(self.sigmas[self._step_index])
        if c["prediction_type"] == "epsilon":
            m_t = hip.axpby_n([x, eps], [float(1 / a_c), float(-s_c / a_c)])
        else:
            m_t = hip.axpby_n([x, eps], [float(a_c), float(-s_c)])
        if use_corrector:                                                       # UniC (:584-719)
            order = self.this_order
            key = ("c", order, self._step_index)
            coefs = self._coef_cache.get(key)
            if coefs is None:
                alpha_t, sigma_t, sigma_s0, h_phi_1, B_h, rks, R, b = self._coefs(order, self._step_index, self._step_index - 1, 1)
                rhos = torch.tensor([0.5]) if order == 1 else torch.linalg.solve(R, b)
                k = -alpha_t * B_h
                coefs, cm0 = [float(sigma_t / sigma_s0), float(k * rhos[-1])], -alpha_t * h_phi_1 - k * rhos[-1]
                for i in range(1, order):
                    w = k * rhos[i - 1] / rks[i - 1]
                    coefs.append(float(w)); cm0 = cm0 - w
                coefs.append(float(cm0))
                self._coef_cache[key] = coefs
            terms = [self.last_sample, m_t] + [self.model_outputs[-(i + 1)] for i in range(1, order)] + [self.model_outputs[-1]]
            x = hip.axpby_n(terms, coefs)
        for i in range(c["solver_order"] - 1):
            self.model_outputs[i] = self.model_outputs[i + 1]
        self.model_outputs[-1] = m_t
        this_order = min(c["solver_order"], len(self.timesteps) - self._step_index) if c["lower_order_final"] else c["solver_order"]
        self.this_order = min(this_order, self.lower_order_nums + 1)
        self.last_sample = x
        order = self.this_order                                                 # UniP (:455-582)
        key = ("p", order, self._step_index)
        coefs = self._coef_cache.get(key)
        if coefs is None:
            alpha_t, sigma_t, sigma_s0, h_phi_1, B_h, rks, R, b = self._coefs(order, self._step_index + 1, self._step_index, 0)
            coefs, cm0 = [float(sigma_t / sigma_s0)], -alpha_t * h_phi_1
            if order > 1:
                rhos_p = torch.tensor([0.5]) if order == 2 else torch.linalg.solve(R[:-1, :-1], b[:-1])
                k = -alpha_t * B_h
                for i in range(1, order):
                    w = k * rhos_p[i - 1] / rks[i - 1]
                    coefs.append(float(w)); cm0 = cm0 - w
            coefs.append(float(cm0))
            self._coef_cache[key] = coefs
        terms = [x] + [self.model_outputs[-(i + 1)] for i in range(1, order)] + [m_t]
        prev = hip.axpby_n(terms, coefs)
        if self.lower_order_nums < c["solver_order"]:
            self.lower_order_nums += 1
        self._step_index += 1
        return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)

    def add_noise(self, original_samples, noise, timesteps):
        raise NotImplementedError("UniPC.add_noise is only used by the training script (SURVEY.md §8 f-2)")


class DPMSolverMultistepScheduler(_SchedulerBase):
    """schedulers/scheduling_dpmsolver_multistep.py: DPM-Solver++ (2M and its orders 1 / 3, midpoint / heun, Karras sigmas) and its SDE
    variant.  The data prediction (convert_model_output :489-555) and every update (:588-863) are linear in {sample, converted model
    outputs, noise}: the host evaluates the scalar coefficients like the reference (fp32 0-dim tensor arithmetic on the sigma table),
    folds the differences D1 / D2 into them, and each update is ONE mf_axpby_n launch.  scale_model_input is the identity and
    init_noise_sigma is 1, so the step body before the update is that of DDIM / PNDM / UniPC."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                     euler_at_final=False, use_karras_sigmas=False, use_lu_lambdas=False, final_sigmas_type="zero",
                     lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace", steps_offset=0,
                     rescale_betas_zero_snr=False)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        for key in ("thresholding", "use_lu_lambdas", "variance_type", "rescale_betas_zero_snr"):
            if c[key]:
                raise NotImplementedError(f"{key} is outside the MirrorFusion path")
        if c["algorithm_type"] not in ("dpmsolver++", "sde-dpmsolver++"):
            raise NotImplementedError(f"algorithm_type {c['algorithm_type']} is not built: 'dpmsolver++' and 'sde-dpmsolver++' are")
        if c["solver_type"] not in ("midpoint", "heun"):
            raise NotImplementedError(f"{c['solver_type']} does is not implemented for {self.__class__}")
        if c["prediction_type"] not in ("epsilon", "v_prediction", "sample"):
            raise ValueError(f"prediction_type given as {c['prediction_type']} must be one of `epsilon`, `sample`, or `v_prediction` "
                             "for the DPMSolverMultistepScheduler.")
        if c["final_sigmas_type"] not in ("zero", "sigma_min"):
            raise ValueError(f"`final_sigmas_type` must be one of 'zero', or 'sigma_min', but got {c['final_sigmas_type']}")
        if not 1 <= c["solver_order"] <= 3 or (c["solver_order"] == 3 and c["algorithm_type"] != "dpmsolver++"):
            raise NotImplementedError("solver_order is 1, 2 or 3, and 3 for algorithm_type 'dpmsolver++' only (the reference has no "
                                      "third-order SDE update)")
        self.alpha_t = torch.sqrt(self.alphas_cumprod)
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self.sigmas = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        self.timesteps = torch.from_numpy(np.linspace(0, c["num_train_timesteps"] - 1, c["num_train_timesteps"], dtype=np.float32)[::-1].copy())
        self.model_outputs = [None] * c["solver_order"]
        self.lower_order_nums = 0
        self._step_index = None
        self._begin_index = None

    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index

    @staticmethod
    def _sigma_to_t(sigma, log_sigmas):
        """:421-442 (Euler's): the fractional training timestep whose log sigma interpolates to log(sigma)."""
        log_sigma = np.log(np.maximum(sigma, 1e-10))
        dists = log_sigma - log_sigmas[:, np.newaxis]
        low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
        high_idx = low_idx + 1
        low, high = log_sigmas[low_idx], log_sigmas[high_idx]
        w = np.clip((low - log_sigma) / (low - high), 0, 1)
        return ((1 - w) * low_idx + w * high_idx).reshape(sigma.shape)

    def set_timesteps(self, num_inference_steps: int = None, device=None):
        c = self.config
        nt = c["num_train_timesteps"]
        clipped_idx = torch.searchsorted(torch.flip(self.lambda_t, [0]), c["lambda_min_clipped"])
        last = int((nt - clipped_idx).item())
        if c["timestep_spacing"] == "linspace":
            ts = np.linspace(0, last - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c["timestep_spacing"] == "leading":
            ts = (np.arange(0, num_inference_steps + 1) * (last // (num_inference_steps + 1))).round()[::-1][:-1].copy().astype(np.int64)
            ts += c["steps_offset"]
        elif c["timestep_spacing"] == "trailing":
            ts = np.arange(last, 0, -nt / num_inference_steps).round().copy().astype(np.int64)
            ts -= 1
        else:
            raise ValueError(f"{c['timestep_spacing']} is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'.")
        sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        if c["use_karras_sigmas"]:                                   # Karras et al. (2022), rho = 7 (:451-474)
            log_sigmas = np.log(sigmas)
            sigma_min, sigma_max = float(sigmas[0]), float(sigmas[-1])
            ramp = np.linspace(0, 1, num_inference_steps)
            min_inv_rho, max_inv_rho = sigma_min ** (1 / 7.0), sigma_max ** (1 / 7.0)
            sigmas = (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** 7.0
            ts = np.array([self._sigma_to_t(s, log_sigmas) for s in sigmas]).round()
        else:
            sigmas = np.interp(ts, np.arange(0, len(sigmas)), sigmas)
        sigma_last = float(((1 - self.alphas_cumprod[0]) / self.alphas_cumprod[0]) ** 0.5) if c["final_sigmas_type"] == "sigma_min" else 0.0
        new_sigmas = torch.from_numpy(np.concatenate([sigmas, [sigma_last]]).astype(np.float32))
        # the coefficients depend only on (sigma table, step index, history length): memoised across calls, like UniPC's
        if getattr(self, "_coef_cache", None) is None or self.sigmas.shape != new_sigmas.shape or not torch.equal(self.sigmas, new_sigmas):
            self._coef_cache = {}
        self.sigmas = new_sigmas
        self.timesteps = torch.from_numpy(np.asarray(ts)).to(torch.int64)       # kept on the host: the loop indexes coefficient tables
        self.num_inference_steps = len(ts)
        self.model_outputs = [None] * c["solver_order"]
        self.lower_order_nums = 0
        self._step_index = None
        self._begin_index = None

    _alpha_sigma = staticmethod(UniPCMultistepScheduler._alpha_sigma)

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        ts = self.timesteps if schedule_timesteps is None else schedule_timesteps
        cand = (ts == int(timestep)).nonzero()
        if len(cand) == 0:
            return len(self.timesteps) - 1
        return int(cand[1]) if len(cand) > 1 else int(cand[0])

    def _lambda(self, idx):
        alpha, sigma = self._alpha_sigma(self.sigmas[idx])
        return alpha, sigma, torch.log(alpha) - torch.log(sigma)

    def _update_coefs(self, order: int) -> List[float]:
        """Coefficients of (sample, m0 [, m1 [, m2]] [, noise]) for the update of this order at the current step index.  The reference's
        own factors (of sample, D0, D1, D2, noise) are fp32 0-dim tensor arithmetic as there; D1 and D2 are differences of the model
        outputs (:717, :843-846), and their weights are folded into the outputs' coefficients in double, rounded once to fp32."""
        i = self._step_index
        sde = self.config["algorithm_type"] == "sde-dpmsolver++"
        heun = self.config["solver_type"] == "heun"
        alpha_t, sigma_t, lambda_t = self._lambda(i + 1)
        _, sigma_s0, lambda_s0 = self._lambda(i)
        h = lambda_t - lambda_s0
        if sde:
            cx = sigma_t / sigma_s0 * torch.exp(-h)
            c0 = alpha_t * (1 - torch.exp(-2.0 * h))
            cn = sigma_t * torch.sqrt(1.0 - torch.exp(-2 * h))
        else:
            cx = sigma_t / sigma_s0
            c0 = -(alpha_t * (torch.exp(-h) - 1.0))
        out = [float(cx), float(c0)]
        if order >= 2:
            _, _, lambda_s1 = self._lambda(i - 1)
            r0 = float((lambda_s0 - lambda_s1) / h)
            if sde:
                c1 = 0.5 * (alpha_t * (1 - torch.exp(-2.0 * h))) if not heun else alpha_t * ((1.0 - torch.exp(-2.0 * h)) / (-2.0 * h) + 1.0)
            elif order == 2 and not heun:
                c1 = -0.5 * (alpha_t * (torch.exp(-h) - 1.0))
            else:
                c1 = alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)
            c1 = float(c1)
            if order == 2:                                           # D1 = (m0 - m1) / r0
                out = [out[0], out[1] + c1 / r0, -c1 / r0]
            else:                                                    # D1 = (1 + k) D1_0 - k D1_1, D2 = (D1_0 - D1_1) / (r0 + r1)
                _, _, lambda_s2 = self._lambda(i - 2)
                r1 = float((lambda_s1 - lambda_s2) / h)
                c2 = float(-(alpha_t * ((torch.exp(-h) - 1.0 + h) / h ** 2 - 0.5)))
                k, q = r0 / (r0 + r1), 1.0 / (r0 + r1)
                a, b = c1 * (1 + k) + c2 * q, -c1 * k - c2 * q       # weights of D1_0 = (m0 - m1) / r0 and D1_1 = (m1 - m2) / r1
                out = [out[0], out[1] + a / r0, -a / r0 + b / r1, -b / r1]
        if sde:
            out.append(float(cn))
        return out

    def _noise(self, shape, generator, device):
        from .rng import PhiloxGenerator, randn_tensor
        if isinstance(generator, PhiloxGenerator):
            generator.device = generator.device or torch.device(device)
            return generator.randn(shape)
        return randn_tensor(shape, generator, device)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None,
             variance_noise: Optional[torch.Tensor] = None, return_dict: bool = True):
        """:896-978.  `variance_noise`: the step's noise for the SDE type (drawn from `generator` when None: one draw per step, the last
        step included, where its coefficient is zero)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._step_index = self.index_for_timestep(timestep) if self._begin_index is None else self._begin_index
        c = self.config
        n = len(self.timesteps)
        final = self._step_index == n - 1 and (c["euler_at_final"] or (c["lower_order_final"] and n < 15) or c["final_sigmas_type"] == "zero")
        second = self._step_index == n - 2 and c["lower_order_final"] and n < 15
        eps = model_output.float().contiguous()
        x = sample.float().contiguous()
        if c["prediction_type"] == "sample":                                    # convert_model_output (:531-555): the x0 prediction
            m_t = eps
        else:
            key = ("m", self._step_index)
            cm = self._coef_cache.get(key)
            if cm is None:
                a_c, s_c = self._alpha_sigma(self.sigmas[self._step_index])
                cm = [float(1 / a_c), float(-s_c / a_c)] if c["prediction_type"] == "epsilon" else [float(a_c), float(-s_c)]
                self._coef_cache[key] = cm
            m_t = hip.axpby_n([x, eps], cm)
        for i in range(c["solver_order"] - 1):
            self.model_outputs[i] = self.model_outputs[i + 1]
        self.model_outputs[-1] = m_t
        sde = c["algorithm_type"] == "sde-dpmsolver++"
        if sde and variance_noise is None:
            variance_noise = self._noise(tuple(x.shape), generator, x.device)
        if c["solver_order"] == 1 or self.lower_order_nums < 1 or final:
            order = 1
        elif c["solver_order"] == 2 or self.lower_order_nums < 2 or second:
            order = 2
        else:
            order = 3
        key = ("u", order, self._step_index)
        coefs = self._coef_cache.get(key)
        if coefs is None:
            coefs = self._coef_cache[key] = self._update_coefs(order)
        terms = [x] + [self.model_outputs[-(i + 1)] for i in range(order)]
        if sde:
            terms.append(variance_noise if isinstance(variance_noise, _Sym) else variance_noise.to(x.device).float().contiguous())
        prev = hip.axpby_n(terms, coefs)
        if self.lower_order_nums < c["solver_order"]:
            self.lower_order_nums += 1
        self._step_index += 1
        return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)

    def add_noise(self, original_samples, noise, timesteps):
        raise NotImplementedError("DPMSolverMultistepScheduler.add_noise is only used by training / image-to-image (SURVEY.md §8 f-2)")


class EulerDiscreteScheduler(_SchedulerBase):
    """schedulers/scheduling_euler_discrete.py (Karras et al. 2022, algorithm 2 without churn).  The sample x lives at the sigma scale
    (init_noise_sigma :242-248), the model reads x / sqrt(sigma_i^2 + 1) (scale_model_input :275-299), and a step (:436-546) is linear
    in {sample, model output}: the host folds the data prediction and the derivative into two coefficients per step, evaluated in double
    on the fp32 sigma table (dt as the reference's fp32 difference) and rounded once, so a step is ONE mf_axpby_n launch.  Timesteps are
    float32, fractional under `linspace` spacing and Karras sigmas.  The reference draws a noise tensor it only uses under s_churn > 0
    (:505); this class draws nothing, so a torch.Generator handed to step() ends in another state than the reference's.

    `model_input_prescaled`: set by the pipeline's captured denoise step, whose static latents buffer already holds the model input
    (the per-step factor travels with the scheduler update, never as a constant of the capture); scale_model_input is then the identity.
    set_timesteps clears it."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     prediction_type="epsilon", interpolation_type="linear", use_karras_sigmas=False, sigma_min=None, sigma_max=None,
                     timestep_spacing="linspace", timestep_type="discrete", steps_offset=0, rescale_betas_zero_snr=False)
    _prediction_types = ("epsilon", "v_prediction", "sample")
    scales_model_input = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.get("rescale_betas_zero_snr"):
            raise NotImplementedError("rescale_betas_zero_snr is outside the MirrorFusion path")
        if c.get("interpolation_type", "linear") != "linear":
            raise NotImplementedError(f"interpolation_type {c['interpolation_type']!r} is not built: 'linear' is")
        if c.get("timestep_type", "discrete") != "discrete":
            raise NotImplementedError(f"timestep_type {c['timestep_type']!r} is not built: 'discrete' is")
        for key in ("sigma_min", "sigma_max"):
            if c.get(key) is not None:
                raise NotImplementedError(f"{key} is not built: Karras sigmas span the schedule's own range")
        if c["prediction_type"] == "original_sample":
            raise NotImplementedError("prediction_type 'original_sample' (the deprecated name of 'sample')")
        if c["prediction_type"] not in self._prediction_types:
            if c["prediction_type"] == "sample":
                raise NotImplementedError("prediction_type not implemented yet: sample")
            raise ValueError(f"prediction_type given as {c['prediction_type']} must be one of `epsilon`, or `v_prediction`")
        self.sigmas = torch.from_numpy(np.concatenate([self._sigma_table()[::-1], np.zeros(1, dtype=np.float32)]))
        self.timesteps = torch.from_numpy(np.linspace(0, c["num_train_timesteps"] - 1, c["num_train_timesteps"], dtype=float)[::-1].copy()
                                          ).to(torch.float32)
        self.init_noise_sigma = self._init_noise_sigma()
        self.model_input_prescaled = False
        self._step_index = None
        self._begin_index = None

    def _sigma_table(self) -> np.ndarray:
        """sqrt((1 - alphas_cumprod) / alphas_cumprod), fp32.  The schedule's scalars (this table, init_noise_sigma, the model-input
        factors, the ancestral sigma_up / sigma_down) are numpy float32 arithmetic with np.sqrt where the reference writes torch's
        `** 0.5`: +, -, *, / and sqrt are correctly rounded on every machine, torch's vectorised float32 math is not on every CPU (where
        it is, the two agree bit for bit), and the ancestral sigma_down is a difference that amplifies a last-bit change a hundredfold."""
        a = self.alphas_cumprod.numpy()
        return np.sqrt((1 - a) / a)

    def _init_noise_sigma(self) -> float:
        """:242-248: the largest sigma, or sqrt(sigma_max^2 + 1) under `leading` spacing (fp32 arithmetic, as there)."""
        m = self.sigmas.numpy().max()
        return float(m if self.config["timestep_spacing"] in ("linspace", "trailing") else np.sqrt(m * m + np.float32(1)))

    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index

    def set_timesteps(self, num_inference_steps: int, device=None):
        c = self.config
        nt = c["num_train_timesteps"]
        self.num_inference_steps = num_inference_steps
        if c["timestep_spacing"] == "linspace":
            ts = np.linspace(0, nt - 1, num_inference_steps, dtype=np.float32)[::-1].copy()
        elif c["timestep_spacing"] == "leading":
            ts = (np.arange(0, num_inference_steps) * (nt // num_inference_steps)).round()[::-1].copy().astype(np.float32)
            ts += c["steps_offset"]
        elif c["timestep_spacing"] == "trailing":
            ts = (np.arange(nt, 0, -nt / num_inference_steps)).round().copy().astype(np.float32)
            ts -= 1
        else:
            raise ValueError(f"{c['timestep_spacing']} is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'.")
        table = self._sigma_table()
        sigmas = np.interp(ts, np.arange(0, len(table)), table)
        if c.get("use_karras_sigmas"):                               # Karras et al. (2022), rho = 7, over the spaced sigmas' range (:389-412)
            log_sigmas = np.log(table)
            min_inv_rho, max_inv_rho = sigmas[-1].item() ** (1 / 7.0), sigmas[0].item() ** (1 / 7.0)
            sigmas = (max_inv_rho + np.linspace(0, 1, num_inference_steps) * (min_inv_rho - max_inv_rho)) ** 7.0
            ts = np.array([DPMSolverMultistepScheduler._sigma_to_t(s, log_sigmas) for s in sigmas])      # (fractional: not rounded)
        self.sigmas = torch.from_numpy(np.concatenate([sigmas.astype(np.float32), np.zeros(1, dtype=np.float32)]))
        self.timesteps = torch.from_numpy(ts.astype(np.float32))     # kept on the host: the loop indexes coefficient tables
        self.init_noise_sigma = self._init_noise_sigma()
        self._coefs = self._step_coefs()
        s = self.sigmas.numpy()
        self._scales = [float(v) for v in np.float32(1) / np.sqrt(s * s + np.float32(1))]     # (fp32, as the reference's divisor; sigma 0: exactly 1)
        self.model_input_prescaled = False
        self._step_index = None
        self._begin_index = None

    def _dt(self):
        """Per step (sigma, dt) as doubles holding the fp32 values the reference computes with (:501, :533)."""
        s = self.sigmas.numpy()
        return s[:-1].astype(np.float64).tolist(), (s[1:] - s[:-1]).astype(np.float64).tolist()

    def _fold(self, sigma: float, dt: float) -> List[float]:
        """x + derivative * dt with derivative = (x - x0) / sigma as coefficients of (sample, model output)."""
        p = self.config["prediction_type"]
        if p == "epsilon":                   # x0 = x - sigma e: the derivative is e
            return [1.0, dt]
        if p == "v_prediction":              # x0 = -sigma / sqrt(sigma^2 + 1) v + x / (sigma^2 + 1)
            return [1.0 + dt * sigma / (sigma * sigma + 1.0), dt / math.sqrt(sigma * sigma + 1.0)]
        return [1.0 + dt / sigma, -dt / sigma]       # x0 is the model output (the last step, dt = -sigma: exactly [0, 1])

    def _step_coefs(self) -> List[List[float]]:
        return [self._fold(s, d) for s, d in zip(*self._dt())]

    def _input_scale(self, index: int) -> float:
        """1 / sqrt(sigma_index^2 + 1): what the model input of step `index` is the sample times."""
        return self._scales[index]

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        ts = self.timesteps if schedule_timesteps is None else schedule_timesteps
        cand = (ts == float(timestep)).nonzero()
        return int(cand[1 if len(cand) > 1 else 0])

    def _ready(self, timestep):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if isinstance(timestep, int) or (torch.is_tensor(timestep) and not torch.is_floating_point(timestep)):
            raise ValueError(f"Passing integer indices (e.g. from `enumerate(timesteps)`) as timesteps to `{type(self).__name__}.step()` is "
                             "not supported. Make sure to pass one of the `scheduler.timesteps` as a timestep.")
        if self._step_index is None:
            self._step_index = self.index_for_timestep(timestep) if self._begin_index is None else self._begin_index

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        if self.model_input_prescaled:
            return sample
        self._ready(timestep)
        return hip.axpby_n([sample.float().contiguous()], [self._input_scale(self._step_index)])

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, s_churn: float = 0.0, s_tmin: float = 0.0,
             s_tmax: float = float("inf"), s_noise: float = 1.0, generator=None, return_dict: bool = True):
        """:436-546 with s_churn == 0 (gamma == 0: sigma_hat is sigma and no noise enters; `generator` is not read)."""
        if s_churn > 0:
            raise NotImplementedError("s_churn > 0 (stochastic churn) is not built")
        self._ready(timestep)
        prev = hip.axpby_n([sample.float().contiguous(), model_output.float().contiguous()], self._coefs[self._step_index])
        self._step_index += 1
        return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)

    def add_noise(self, original_samples, noise, timesteps):
        raise NotImplementedError(f"{type(self).__name__}.add_noise is only used by training / image-to-image (SURVEY.md §8 f-2)")


class EulerAncestralDiscreteScheduler(EulerDiscreteScheduler):
    """schedulers/scheduling_euler_ancestral_discrete.py: the Euler step down to sigma_down, then fresh noise of scale sigma_up (:422-437),
    linear in {sample, model output, noise}: ONE mf_axpby_n launch.  sigma_up / sigma_down are the reference's fp32 arithmetic.  One
    draw per step, the last included, where sigma_up is 0.  The reference has neither Karras sigmas nor the 'sample' prediction here."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0, rescale_betas_zero_snr=False)
    _prediction_types = ("epsilon", "v_prediction")

    def _step_coefs(self) -> List[List[float]]:
        s_from, s_to = self.sigmas.numpy()[:-1], self.sigmas.numpy()[1:]
        up = np.sqrt(s_to * s_to * (s_from * s_from - s_to * s_to) / (s_from * s_from))
        down = np.sqrt(s_to * s_to - up * up)
        dts = (down - s_from).astype(np.float64).tolist()
        return [self._fold(s, d) + [u] for s, d, u in zip(s_from.astype(np.float64).tolist(), dts, up.astype(np.float64).tolist())]

    _noise = DPMSolverMultistepScheduler._noise

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None,
             variance_noise: Optional[torch.Tensor] = None, return_dict: bool = True):
        """:349-450.  `variance_noise`: the step's noise (drawn from `generator` when None)."""
        self._ready(timestep)
        x = sample.float().contiguous()
        if variance_noise is None:
            variance_noise = self._noise(tuple(x.shape), generator, x.device)
        if not isinstance(variance_noise, _Sym):
            variance_noise = variance_noise.to(x.device).float().contiguous()
        prev = hip.axpby_n([x, model_output.float().contiguous(), variance_noise], self._coefs[self._step_index])
        self._step_index += 1
        return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)


class LCMScheduler(_SchedulerBase):
    """schedulers/scheduling_lcm.py: latent-consistency multistep sampling (Luo et al. 2023), 1-8 steps on a distilled UNet or under an
    LCM-LoRA.  set_timesteps (:351-490) picks its steps from the `original_inference_steps`-sized distillation schedule, or takes a custom
    list.  A step (:500-594) is linear in {sample, model output, noise}: the data prediction, the boundary-condition scalings c_skip /
    c_out (:492-498) and sqrt(alpha_prev) / sqrt(1 - alpha_prev) fold into float coefficients, so it is TWO mf_axpby_n launches:
    `denoised` from {sample, model output}, then `prev_sample` from {denoised, noise}.  The last step draws nothing and returns `denoised`
    (:580).  The scalars are numpy float32 arithmetic with np.sqrt on the fp32 alphas_cumprod table (what the reference's 0-dim fp32
    tensors compute; see EulerDiscreteScheduler._sigma_table for why not torch's `** 0.5`), folded in double and rounded once."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None,
                     original_inference_steps=50, clip_sample=False, clip_sample_range=1.0, set_alpha_to_one=True, steps_offset=0,
                     prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                     timestep_spacing="leading", timestep_scaling=10.0, rescale_betas_zero_snr=False)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c["thresholding"]:
            raise NotImplementedError("thresholding is not built: the quantile clamp is not linear in the sample")
        if c["clip_sample"]:
            raise NotImplementedError("clip_sample=True is not built: the clamp is not linear in the sample (LCM checkpoints ship it off)")
        if c["rescale_betas_zero_snr"]:
            raise NotImplementedError("rescale_betas_zero_snr is outside the MirrorFusion path")
        if c["prediction_type"] not in ("epsilon", "sample", "v_prediction"):
            raise ValueError(f"prediction_type given as {c['prediction_type']} must be one of `epsilon`, `sample` or `v_prediction` for "
                             "`LCMScheduler`.")
        self.custom_timesteps = False
        self._step_index = None
        self._begin_index = None

    step_index = EulerDiscreteScheduler.step_index
    begin_index = EulerDiscreteScheduler.begin_index
    set_begin_index = EulerDiscreteScheduler.set_begin_index

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        ts = self.timesteps if schedule_timesteps is None else schedule_timesteps
        cand = (ts == int(timestep)).nonzero()
        return int(cand[1 if len(cand) > 1 else 0])

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, original_inference_steps: Optional[int] = None,
                      timesteps: Optional[List[int]] = None, strength: float = 1.0):
        """:351-490.  The integer schedule and the ValueErrors are the reference's; what it only warns about (a custom schedule off the
        distillation grid, or not starting at the last training step) is accepted silently."""
        c = self.config
        nt = c["num_train_timesteps"]
        if num_inference_steps is None and timesteps is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `custom_timesteps`.")
        if num_inference_steps is not None and timesteps is not None:
            raise ValueError("Can only pass one of `num_inference_steps` or `custom_timesteps`.")
        original_steps = original_inference_steps if original_inference_steps is not None else c["original_inference_steps"]
        if original_steps > nt:
            raise ValueError(f"`original_steps`: {original_steps} cannot be larger than `self.config.train_timesteps`: {nt} as the unet "
                             f"model trained with this scheduler can only handle maximal {nt} timesteps.")
        k = nt // original_steps                                     # the skipping step of the distillation schedule
        origin = np.asarray(list(range(1, int(original_steps * strength) + 1))) * k - 1
        if timesteps is not None:
            timesteps = [int(t) for t in timesteps]
            for i in range(1, len(timesteps)):
                if timesteps[i] >= timesteps[i - 1]:
                    raise ValueError("`custom_timesteps` must be in descending order.")
            if timesteps[0] >= nt:
                raise ValueError(f"`timesteps` must start before `self.config.train_timesteps`: {nt}.")
            ts = np.array(timesteps, dtype=np.int64)
            self.num_inference_steps = len(ts)
            self.custom_timesteps = True
            init_timestep = min(int(self.num_inference_steps * strength), self.num_inference_steps)      # (strength: the img2img cut)
            ts = ts[max(self.num_inference_steps - init_timestep, 0) * self.order:]
        else:
            if num_inference_steps > nt:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than `self.config.train_timesteps`: {nt} "
                                 f"as the unet model trained with this scheduler can only handle maximal {nt} timesteps.")
            if len(origin) // num_inference_steps < 1:
                raise ValueError(f"The combination of `original_steps x strength`: {original_steps} x {strength} is smaller than "
                                 f"`num_inference_steps`: {num_inference_steps}. Make sure to either reduce `num_inference_steps` to a "
                                 f"value smaller than {int(original_steps * strength)} or increase `strength` to a value higher than "
                                 f"{float(num_inference_steps / original_steps)}.")
            self.num_inference_steps = num_inference_steps
            if num_inference_steps > original_steps:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than `original_inference_steps`: "
                                 f"{original_steps} because the final timestep schedule will be a subset of the "
                                 "`original_inference_steps`-sized initial timestep schedule.")
            origin = origin[::-1].copy()
            idx = np.floor(np.linspace(0, len(origin), num=num_inference_steps, endpoint=False)).astype(np.int64)
            ts = origin[idx]
        self.timesteps = torch.from_numpy(ts).to(torch.int64)        # kept on the host: the loop indexes coefficient tables
        self._coef_cache = {}
        self._step_index = None
        self._begin_index = None

    def get_scalings_for_boundary_condition_discrete(self, timestep):
        """:492-498 in fp32, what the reference computes for a timestep taken from `timesteps` (an int64 tensor times a float)."""
        sd = np.float32(0.5)
        st = np.float32(int(timestep)) * np.float32(self.config["timestep_scaling"])
        return float(sd * sd / (st * st + sd * sd)), float(st / np.sqrt(st * st + sd * sd))

    def _step_coefs(self, timestep: int, index: int):
        """((of sample, of model output) for `denoised`, (of denoised, of noise) for `prev_sample` | None on the last step)."""
        n = len(self.timesteps)
        prev_t = int(self.timesteps[index + 1]) if index + 1 < n else timestep
        f32 = np.float32
        a_t, a_p = f32(float(self._alpha(timestep))), f32(float(self._alpha(prev_t)))
        sa, sb = float(np.sqrt(a_t)), float(np.sqrt(f32(1) - a_t))
        c_skip, c_out = self.get_scalings_for_boundary_condition_discrete(timestep)
        p = self.config["prediction_type"]
        if p == "epsilon":                   # x0 = (x - sqrt(b_t) e) / sqrt(a_t)
            den = [c_skip + c_out / sa, -c_out * sb / sa]
        elif p == "sample":
            den = [c_skip, c_out]
        else:                                # x0 = sqrt(a_t) x - sqrt(b_t) v
            den = [c_skip + c_out * sa, -c_out * sb]
        if index == self.num_inference_steps - 1:
            return den, None
        return den, [float(np.sqrt(a_p)), float(np.sqrt(f32(1) - a_p))]

    _noise = DPMSolverMultistepScheduler._noise

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None,
             variance_noise: Optional[torch.Tensor] = None, return_dict: bool = True):
        """:500-594.  Returns (prev_sample, denoised).  `variance_noise`: the step's noise (drawn from `generator` when None; the last
        step of the schedule neither draws nor reads one)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._step_index = self.index_for_timestep(timestep) if self._begin_index is None else self._begin_index
        key = (int(timestep), self._step_index)
        coefs = self._coef_cache.get(key)
        if coefs is None:
            coefs = self._coef_cache[key] = self._step_coefs(*key)
        den, nxt = coefs
        x = sample.float().contiguous()
        denoised = hip.axpby_n([x, model_output.float().contiguous()], den)
        if nxt is not None:
            if variance_noise is None:
                variance_noise = self._noise(tuple(x.shape), generator, x.device)
            if not isinstance(variance_noise, _Sym):
                variance_noise = variance_noise.to(x.device).float().contiguous()
            prev = hip.axpby_n([denoised, variance_noise], nxt)
        else:
            prev = denoised
        self._step_index += 1
        return (prev, denoised) if not return_dict else LCMSchedulerOutput(prev_sample=prev, denoised=denoised)

    def add_noise(self, original_samples, noise, timesteps):
        raise NotImplementedError("LCMScheduler.add_noise is only used by training / image-to-image (SURVEY.md §8 f-2)")


# ---- the multistep schedulers' update on the device (mf_sched_step_dev) ------------------------------------------------------------
# A step of PNDM / UniPC is a short list of mf_axpby_n calls over the guided noise prediction, the latents and the history the
# scheduler keeps.  device_plan() runs the scheduler's OWN step() on stand-in tensors that record those calls (terms, order, float
# coefficients) and maps every value onto the per-element register file of mf_sched_step_dev (include/mfhip.h): 0 = e, 1 = latents,
# 2 .. 2+S-1 = state slots persisted between steps, then temporaries.  The coefficient math stays in step(); the rows only carry it.
REG_EPS, REG_LATENTS = 0, 1
_MAX_OPS, _MAX_TERMS, _MAX_REGS, _Row = hip.SCHED_MAX_OPS, hip.SCHED_MAX_TERMS, hip.SCHED_MAX_REGS, hip.SchedRow


class _Sym:
    """A tensor of a traced step(): which register holds it is decided by the plan."""
    __slots__ = ("name", "slot")

    def __init__(self, name: str):
        self.name, self.slot = name, None

    def float(self):
        return self

    def contiguous(self):
        return self

    def __repr__(self):
        return self.name


class _TraceHip:
    """Stands in for the hip module while step() is traced: every axpby_n call is written down, nothing is launched."""

    def __init__(self):
        self.calls = []

    def axpby_n(self, xs, coefs, out=None):
        if out is not None or not 1 <= len(xs) <= _MAX_TERMS or not all(isinstance(x, _Sym) for x in xs):
            raise NotImplementedError("a traced step may only combine its own values, at most MF_SCHED_MAX_TERMS at a time")
        y = _Sym(f"v{len(self.calls)}")
        self.calls.append((y, list(xs), [float(c) for c in coefs]))
        return y

    def __getattr__(self, name):
        raise NotImplementedError(f"hip.{name} inside a traced scheduler step: only axpby_n has a device form")


def _held(sched) -> List[_Sym]:
    """The traced values the scheduler's attributes keep (its history), in attribute order."""
    out = {}
    for v in vars(sched).values():
        for x in (v if isinstance(v, (list, tuple)) else (v,)):
            if isinstance(x, _Sym):
                out.setdefault(id(x), x)
    return list(out.values())


def _plan_step(calls, e: _Sym, x: _Sym, prev: _Sym, held: List[_Sym], slots: list, noise: Optional[_Sym] = None):
    """Registers for one traced step.  `slots`: the value each state slot holds (carried from step to step, updated here).  Returns
    ops as (dst, [src], coefs | None for a move) with locations ("r", 0 | 1), ("s", slot), ("t", temporary), and the temporaries used.
    `noise`: the step's noise value, which the launch leaves in temporary 0 (free for reuse once the step has read it)."""
    keep = {id(s) for s in held}
    loc = {id(e): ("r", REG_EPS), id(x): ("r", REG_LATENTS)}
    if noise is not None:
        if id(noise) in keep:
            raise NotImplementedError("device_plan: the scheduler keeps a step's noise between steps")
        loc[id(noise)] = ("t", 0)
    for i, s in enumerate(slots):
        if s is not None:
            loc[id(s)] = ("s", i)
    reads = {}
    for _, xs, _ in calls:
        for i in {id(v) for v in xs}:
            reads[i] = reads.get(i, 0) + 1
    temps, ops = ([] if noise is None else [noise]), []

    def free(v):
        return v is None or (id(v) not in keep and reads.get(id(v), 0) == 0)

    def take(pool, v):
        for i, occ in enumerate(pool):
            if free(occ):
                pool[i] = v
                return i
        pool.append(v)
        return len(pool) - 1
    # inputs the history keeps (PNDM: ets.append(model_output), cur_sample = sample; UniPC: last_sample = sample): copied into a slot
    # first, before anything can overwrite register 1; later reads take the copy
    for v in (e, x):
        if id(v) in keep:
            s = take(slots, v)
            ops.append((("s", s), [loc[id(v)]], None))
            loc[id(v)], v.slot = ("s", s), s
    for y, xs, cs in calls:
        srcs = [loc[id(v)] for v in xs]          # (a KeyError here: a value no register holds any more)
        for i in {id(v) for v in xs}:
            reads[i] -= 1
        if id(y) in keep:
            s = take(slots, y)
            d, y.slot = ("s", s), s
        elif y is prev and (reads.get(id(x), 0) == 0 or loc[id(x)] != ("r", REG_LATENTS)):
            d = ("r", REG_LATENTS)
        else:
            d = ("t", take(temps, y))
        ops.append((d, srcs, cs))
        loc[id(y)] = d
    if loc[id(prev)] != ("r", REG_LATENTS):
        ops.append((("r", REG_LATENTS), [loc[id(prev)]], None))
    for v in held:
        if loc[id(v)][0] != "s":
            raise AssertionError(f"{v} is kept by the scheduler but holds no state slot")
    return ops, len(temps)


class SchedPlan:
    """device_plan()'s result: `rows` (int32 [steps, sizeof(mf_sched_row) / 4], one mf_sched_row per step, host memory), `nslots` (S: the
    state buffer is [S, *latents.shape] fp32) and the traced scheduler, whose end state finish() hands to the real one."""

    def __init__(self, rows: torch.Tensor, nslots: int, traced, steps: int, noise_reg: int = -1, x_slot: int = -1, first_scale: float = 1.0,
                 draws: Optional[List[bool]] = None):
        self.rows, self.nslots, self._traced, self.steps = rows, nslots, traced, steps
        # per step: does the row read the step's noise?  (LCM's last step does not: the host's step() draws nothing there)
        self.draws = [noise_reg >= 0] * steps if draws is None else draws
        # the register mf_sched_step_noise_dev fills with the step's standard normals (SDE and ancestral samplers); -1: the plan reads no noise
        self.noise_reg = noise_reg
        # Euler family: the slot that holds the sample x, while the latents (register 1) hold the model input, x / sqrt(sigma^2 + 1) of
        # the step about to run.  A run starts with x0 in the slot and x0 * first_scale in the latents.  -1: the latents are the sample.
        self.x_slot, self.first_scale = x_slot, first_scale

    def finish(self, sched, state: torch.Tensor) -> None:
        """After the last device step: `sched` ends in the state its own step() would have left — the counters of the trace, and the
        history tensors taken from the slots of `state` (copies)."""
        def real(v):
            return state[v.slot].clone() if isinstance(v, _Sym) else v
        for k, v in vars(self._traced).items():
            if isinstance(v, list):
                v = [real(x) for x in v]
            elif isinstance(v, tuple):
                v = tuple(real(x) for x in v)
            else:
                v = real(v)
            setattr(sched, k, v)


def device_plan(sched, steps: Optional[int] = None) -> SchedPlan:
    """The rows of mf_sched_step_dev for the first `steps` (default: all) entries of `sched.timesteps`, for a PNDMScheduler,
    UniPCMultistepScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler, EulerAncestralDiscreteScheduler or LCMScheduler right after set_timesteps.  `sched` itself is not changed (a copy is traced).
    The SDE type of DPM-Solver++, the ancestral Euler class and LCM read a noise value per step (`plan.draws`: which steps do): its register is `noise_reg` of the plan (mf_sched_step_noise_dev)."""
    global hip
    if not isinstance(sched, (PNDMScheduler, UniPCMultistepScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler, LCMScheduler)):
        raise NotImplementedError(f"{type(sched).__name__} has no device plan (DDIM updates through mf_cfg_ddim_step_dev)")
    if sched.num_inference_steps is None:
        raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
    history = [getattr(sched, k, None) for k in ("model_outputs", "last_sample", "ets", "cur_sample", "cur_model_output")]
    if getattr(sched, "_step_index", None) is not None or getattr(sched, "counter", 0) != 0 or any(
            x is not None for v in history for x in (v if isinstance(v, list) else [v])):
        raise ValueError("device_plan: the scheduler has already stepped; call set_timesteps first")
    traced = copy.copy(sched)
    for k, v in list(vars(traced).items()):
        if isinstance(v, list):
            setattr(traced, k, list(v))
    ts = sched.timesteps
    steps = len(ts) if steps is None else int(steps)
    slots, per_step, ntemps, draws = [], [], 0, []
    real, tracer = hip, _TraceHip()
    noisy = isinstance(sched, (EulerAncestralDiscreteScheduler, LCMScheduler)) or (
        isinstance(sched, DPMSolverMultistepScheduler) and sched.config["algorithm_type"] == "sde-dpmsolver++")
    # Euler family: the sample keeps slot 0 from step to step (the host puts x0 there), and every row ends with one more op, the next
    # step's model input into register 1
    euler = isinstance(sched, EulerDiscreteScheduler)
    sample = _Sym("x") if euler else None
    first_scale = 1.0
    if euler:
        slots.append(sample)
        sample.slot = 0
        first_scale = sched._input_scale(sched.index_for_timestep(ts[0]) if sched.begin_index is None else sched.begin_index) if steps else 1.0
    for k in range(steps):
        e, x = _Sym(f"e{k}"), (sample if euler else _Sym(f"x{k}"))
        noise = _Sym(f"n{k}") if noisy else None
        tracer.calls = []
        hip = tracer
        try:
            prev = traced.step(e, ts[k], x, **(dict(variance_noise=noise) if noisy else {}), return_dict=False)[0]
        finally:
            hip = real
        draws.append(noisy and any(v is noise for _, xs, _ in tracer.calls for v in xs))
        held = _held(traced)
        if euler:
            sample = prev
            prev = tracer.axpby_n([sample], [traced._input_scale(traced.step_index)])
            held = held + [sample]
        ops, nt = _plan_step(tracer.calls, e, x, prev, held, slots, noise)
        if euler and sample.slot != 0:
            raise AssertionError("device_plan: the Euler sample left its slot")
        per_step.append(ops)
        ntemps = max(ntemps, nt)
    nslots = len(slots)
    if 2 + nslots + ntemps > _MAX_REGS:
        raise NotImplementedError(f"device_plan: {nslots} state slots + {ntemps} temporaries exceed MF_SCHED_MAX_REGS")
    base = {"r": 0, "s": 2, "t": 2 + nslots}
    rows = []
    for ops in per_step:
        if len(ops) > _MAX_OPS:
            raise NotImplementedError(f"device_plan: {len(ops)} ops in one step exceed MF_SCHED_MAX_OPS")
        row = _Row(nops=len(ops), nslots=nslots)
        written, load, store = set(), 0, 0
        for j, (d, srcs, cs) in enumerate(ops):
            op = row.ops[j]
            for i, (kind, n) in enumerate(srcs):
                r = base[kind] + n
                op.src[i] = r
                if r not in written and kind != "t" and r != REG_EPS:
                    load |= 1 << r
            op.nterms = 0 if cs is None else len(cs)
            for i, c in enumerate(cs or ()):
                op.coef[i] = c
            op.dst = base[d[0]] + d[1]
            written.add(op.dst)
            if d[0] != "t":
                store |= 1 << op.dst
        row.load, row.store = load, store
        rows.append(bytes(row))
    table = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.int32).view(steps, -1).clone() if rows else \
        torch.zeros(0, C.sizeof(_Row) // 4, dtype=torch.int32)
    return SchedPlan(table, nslots, traced, steps, base["t"] if noisy else -1, 0 if euler else -1, first_scale, draws)
