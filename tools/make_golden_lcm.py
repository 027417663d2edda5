"""Golden fixtures for LCMScheduler, the guidance-scale embedding and the UNet's timestep_cond, from the IMPORTED REFERENCE
(schedulers/scheduling_lcm.py, pipelines/brushnet/pipeline_brushnet.py:795-822, models/unets/unet_2d_condition.py).

Runs only where the reference checkout that tools/make_golden.py imports exists; nothing under tests/, bench.py or the package reads it
at run time.  Results only: every input is regenerated from a seed by the tests.

    python tools/make_golden_lcm.py

  tests/golden/lcm.npz            `ts/<num>_<original>_<strength>`: set_timesteps(num, original_inference_steps=, strength=).timesteps
                                  (int64) over SCHEDULES; `ts/custom`, `ts/custom_half`: set_timesteps(timesteps=CUSTOM[, strength=0.5]);
                                  `raises/<name>`: the exception type's name for every entry of RAISES; `trace/<prediction_type>/
                                  {timesteps, ref64, den64, ref32, den32}`: 4 steps on a [2, 4, 8, 8] sample, per step the reference's
                                  prev_sample / denoised on float64 and on fp32 tensors; `emb/<dim>`: get_guidance_scale_embedding(W, dim)
  tests/golden/lcm_envelope.json  "fp32": per prediction type the reference's own fp32 deviation PER STEP, max |ref32 - ref64| /
                                  (1 + |ref64|), for prev_sample (`<type>`) and denoised (`<type>/denoised`); "_about" states the bound
  tests/golden/lcm_tiny.npz       the tiny UNet (keys_tiny.json, synth seed 0) with time_cond_proj_dim = 32: `cond_proj_weight`,
                                  `timestep_cond` (the embedding of w = 0.5, 6.5), `timestep`, `eps` (inputs: the tiny tests' seed-42 draw)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as MG  # noqa: E402  (sets up the reference import path + the FLAX_WEIGHTS_NAME shim)
from make_golden import GOLD, R, StableDiffusionBrushNetPipeline, synth  # noqa: E402
import make_golden_dpmsolver as MD  # noqa: E402
import diffusers.schedulers.scheduling_lcm as ref_lcm  # noqa: E402
from diffusers import LCMScheduler  # noqa: E402

torch.set_grad_enabled(False)
SD = MD.SD
SHAPE = (2, 4, 8, 8)
STEPS = 4
PREDICTIONS = ("epsilon", "v_prediction", "sample")
SCHEDULES = [(n, o, s) for n in (1, 2, 4, 8) for o in (50, 25) for s in (1.0, 0.5)]
CUSTOM = [999, 759, 499, 259]
W = (0.0, 0.5, 6.5)
EMB_DIMS = (32, 33, 256)
# the issue's table of refused inputs; tests/test_lcm_cpu.py feeds the library's class the same keywords
RAISES = {
    "neither": dict(),
    "both": dict(num_inference_steps=4, timesteps=CUSTOM),
    "original_above_train": dict(num_inference_steps=4, original_inference_steps=2000),
    "steps_above_train": dict(num_inference_steps=1001),
    "steps_above_original": dict(num_inference_steps=60),
    "steps_above_original_x_strength": dict(num_inference_steps=30, strength=0.5),
    "custom_ascending": dict(timesteps=[999, 499, 759, 259]),
    "custom_repeated": dict(timesteps=[999, 499, 499]),
    "custom_past_train": dict(timesteps=[1000, 499]),
}


def trace_inputs():
    """{prediction type: (x0, [model outputs], [noises])} from ONE np.random.default_rng(7), in PREDICTIONS order: the start sample, 4
    model outputs, 4 noises (the last step reads none)."""
    rng = np.random.default_rng(7)
    out = {}
    for p in PREDICTIONS:
        x0 = rng.standard_normal(SHAPE, dtype=np.float32)
        mos = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(STEPS)]
        noises = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(STEPS)]
        out[p] = (x0, mos, noises)
    return out


class scheduler_noise(MD.scheduler_noise):
    """make_golden_dpmsolver.scheduler_noise on the LCM module's randn_tensor."""

    def __enter__(self):
        self.orig = ref_lcm.randn_tensor

        def fake(shape, generator=None, device=None, dtype=None, layout=None):
            n = self.noises.pop(0)
            assert tuple(n.shape) == tuple(shape)
            return n.to(dtype)
        ref_lcm.randn_tensor = fake
        return self

    def __exit__(self, *a):
        ref_lcm.randn_tensor = self.orig


def run_trace(p, x0, mos, noises, dtype):
    s = LCMScheduler(**SD, prediction_type=p)
    s.set_timesteps(STEPS)
    x = torch.from_numpy(x0).to(dtype)
    prevs, dens = [], []
    with scheduler_noise(noises):
        for k, t in enumerate(s.timesteps):              # (t: a 0-dim int64 tensor, as the pipeline's loop hands it over)
            x, den = s.step(torch.from_numpy(mos[k]).to(dtype), t, x, return_dict=False)
            prevs.append(x.clone())
            dens.append(den.clone())
    assert torch.equal(prevs[-1], dens[-1])
    return s, torch.stack(prevs), torch.stack(dens)


def _dev(a32, a64):
    return [float(((a32[k].double() - a64[k]).abs() / (1 + a64[k].abs())).max()) for k in range(a64.shape[0])]


def schedules(out):
    for n, o, st in SCHEDULES:
        s = LCMScheduler(**SD)
        s.set_timesteps(n, original_inference_steps=o, strength=st)
        out[f"ts/{n}_{o}_{st}"] = s.timesteps.numpy()
    for name, kw in (("custom", {}), ("custom_half", dict(strength=0.5))):
        s = LCMScheduler(**SD)
        s.set_timesteps(timesteps=list(CUSTOM), **kw)
        out[f"ts/{name}"] = s.timesteps.numpy()
    for name, kw in RAISES.items():
        try:
            LCMScheduler(**SD).set_timesteps(**kw)
        except Exception as e:
            out[f"raises/{name}"] = np.array(type(e).__name__)
        else:
            raise AssertionError(f"the reference accepts {name}: {kw}")


def traces(out, env):
    for p, (x0, mos, noises) in trace_inputs().items():
        s, r64, d64 = run_trace(p, x0, mos, noises, torch.float64)
        _, r32, d32 = run_trace(p, x0, mos, noises, torch.float32)
        assert r64.dtype == d64.dtype == torch.float64 and r32.dtype == d32.dtype == torch.float32
        key = f"trace/{p}"
        out[f"{key}/timesteps"] = s.timesteps.numpy()
        out[f"{key}/ref64"], out[f"{key}/den64"] = r64.numpy(), d64.numpy()
        out[f"{key}/ref32"], out[f"{key}/den32"] = r32.numpy(), d32.numpy()
        env["fp32"][p], env["fp32"][f"{p}/denoised"] = _dev(r32, r64), _dev(d32, d64)
        print(f"{key:24s} reference fp32 deviation per step: prev_sample {env['fp32'][p]}, denoised {env['fp32'][p + '/denoised']}")


def embeddings(out):
    for dim in EMB_DIMS:
        out[f"emb/{dim}"] = StableDiffusionBrushNetPipeline.get_guidance_scale_embedding(None, torch.tensor(W), embedding_dim=dim).numpy()


def tiny_unet():
    cfg = R.TINY_UNET
    with open(os.path.join(GOLD, "keys_tiny.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f)["unet"].items()}
    unet = MG.UNet2DConditionModel(
        sample_size=8, in_channels=cfg["in_channels"], out_channels=cfg["out_channels"], down_block_types=cfg["down_block_types"],
        up_block_types=cfg["up_block_types"], block_out_channels=cfg["block_out_channels"], layers_per_block=cfg["layers_per_block"],
        cross_attention_dim=cfg["cross_attention_dim"], attention_head_dim=cfg["attention_head_dim"],
        norm_num_groups=cfg["norm_num_groups"], time_cond_proj_dim=32).eval()
    sd = synth.state_dict_for(shapes, 0)                  # the tiny fixture's weights, unchanged
    w = torch.randn(cfg["block_out_channels"][0], 32, generator=torch.Generator().manual_seed(2024)) * 0.2
    assert tuple(unet.state_dict()["time_embedding.cond_proj.weight"].shape) == tuple(w.shape)
    unet.load_state_dict(dict(sd, **{"time_embedding.cond_proj.weight": w}), strict=True)
    g = torch.Generator().manual_seed(42)                 # tests/test_models_gpu.py tiny_inputs()
    x = torch.randn(2, 4, 8, 8, generator=g)
    torch.randn(2, 6, 8, 8, generator=g)
    ehs = torch.randn(2, 77, cfg["cross_attention_dim"], generator=g)
    cond = StableDiffusionBrushNetPipeline.get_guidance_scale_embedding(None, torch.tensor([0.5, 6.5]), embedding_dim=32)
    eps = unet(x, 501, ehs, timestep_cond=cond, return_dict=False)[0]
    plain = unet(x, 501, ehs, return_dict=False)[0]
    print(f"tiny UNet: |eps(timestep_cond) - eps(None)| max {float((eps - plain).abs().max()):.3e} (absmax {float(eps.abs().max()):.3e})")
    return dict(cond_proj_weight=w.numpy(), timestep_cond=cond.numpy(), timestep=np.array(501), eps=eps.numpy())


if __name__ == "__main__":
    out, env = {}, dict(fp32={})
    env["_about"] = ("fp32: per step k, max |ref32 - ref64| / (1 + |ref64|) of the imported reference's LCMScheduler.step on the traces of "
                     "lcm.npz (4 steps, [2, 4, 8, 8]) for prev_sample (<prediction type>) and denoised (<prediction type>/denoised): the "
                     "reference's own fp32 deviation (tools/make_golden_lcm.py).  tests/test_lcm_cpu.py holds the host scheduler, per step, "
                     "to ENVELOPE_K = 4 x that figure, the multiple of dpmsolver_envelope.json / euler_envelope.json and for their reason: "
                     "the library's step is a second, independent fp32 evaluation of the same formula with errors of the same size (the "
                     "scalings folded into two coefficients in double and rounded once, a multiply by a folded reciprocal where the "
                     "reference divides, fmaf chaining), not another algorithm; two independent draws of a rounding error of one size "
                     "differ by a small factor in their maxima over 512 elements, a wrong coefficient by orders of magnitude.")
    schedules(out)
    traces(out, env)
    embeddings(out)
    np.savez_compressed(os.path.join(GOLD, "lcm.npz"), **out)
    np.savez_compressed(os.path.join(GOLD, "lcm_tiny.npz"), **tiny_unet())
    with open(os.path.join(GOLD, "lcm_envelope.json"), "w") as f:
        json.dump(env, f, indent=1, sort_keys=True)
