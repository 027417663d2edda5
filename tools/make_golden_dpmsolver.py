"""Golden fixtures for DPMSolverMultistepScheduler, from the IMPORTED REFERENCE (schedulers/scheduling_dpmsolver_multistep.py).

Runs only where the reference checkout that tools/make_golden.py imports exists; nothing under tests/, bench.py or the package reads it
at run time.  Results
only: every input is regenerated from a seed by the tests.

    python tools/make_golden_dpmsolver.py

  tests/golden/dpmsolver.npz            scheduler traces `trace/<case>/<steps>/{timesteps, sigmas, ref64}` (per-step samples of the
                                        reference on float64 tensors; those on fp32 tensors, `.../ref32`, are in
                                        dpmsolver_ref32.npz) and the tiny pipeline's `<case>_{timesteps, cond, vae_noise,
                                        latents_<i>, image}` (keys as in tiny_pipeline.npz) for dpmpp_2m and dpmpp_2m_karras
  tests/golden/dpmsolver_envelope.json  "fp32": per trace, max |ref32 - ref64| / (1 + |ref64|) — the reference's own fp32 deviation;
                                        "bf16" / "fp16": the reference's deviation from its fp32 pipeline results in that dtype, produced
                                        the way tools/make_bf16_envelope.py produces its entries
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
from make_golden import PNDMScheduler, StableDiffusionBrushNetPipeline, R, synth, GOLD  # noqa: E402
from make_bf16_envelope import fixed_noise, stats  # noqa: E402
import diffusers.schedulers.scheduling_dpmsolver_multistep as ref_dpm  # noqa: E402
from diffusers import DPMSolverMultistepScheduler  # noqa: E402

torch.set_grad_enabled(False)
SD = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SHAPE = (2, 4, 8, 8)
STEPS = (5, 20)


def _pndm_config():
    return PNDMScheduler(**SD, steps_offset=1, skip_prk_steps=True, set_alpha_to_one=False).config


# the issue's case table; tests/test_dpmsolver_cpu.py builds the same schedulers from the library's classes
CASES = {
    "from_pndm": lambda: DPMSolverMultistepScheduler.from_config(_pndm_config()),
    "2m_karras": lambda: DPMSolverMultistepScheduler(**SD, use_karras_sigmas=True),
    "2m_heun_v": lambda: DPMSolverMultistepScheduler(**SD, solver_type="heun", prediction_type="v_prediction", timestep_spacing="trailing"),
    "o1": lambda: DPMSolverMultistepScheduler(**SD, solver_order=1),
    "o3": lambda: DPMSolverMultistepScheduler(**SD, solver_order=3),
    "euler_final": lambda: DPMSolverMultistepScheduler(**SD, euler_at_final=True, timestep_spacing="leading", steps_offset=1),
    "sigma_min": lambda: DPMSolverMultistepScheduler(**SD, final_sigmas_type="sigma_min"),
    "sde": lambda: DPMSolverMultistepScheduler(**SD, algorithm_type="sde-dpmsolver++"),
    "sde_karras_o1": lambda: DPMSolverMultistepScheduler(**SD, algorithm_type="sde-dpmsolver++", use_karras_sigmas=True, solver_order=1),
}


def trace_inputs():
    """{(case, steps): (x0, [model outputs], [noises] | None)} from ONE np.random.default_rng(7), cases in table order, then 5 and 20
    steps; per entry: the start sample, the model outputs, then (SDE) the noises."""
    rng = np.random.default_rng(7)
    out = {}
    for name in CASES:
        for n in STEPS:
            x0 = rng.standard_normal(SHAPE, dtype=np.float32)
            mos = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(n)]
            noises = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(n)] if name.startswith("sde") else None
            out[(name, n)] = (x0, mos, noises)
    return out


class scheduler_noise:
    """The SDE type draws its noise with randn_tensor: hand it the recorded arrays instead."""

    def __init__(self, noises):
        self.noises = [torch.from_numpy(n) for n in (noises or [])]

    def __enter__(self):
        self.orig = ref_dpm.randn_tensor

        def fake(shape, generator=None, device=None, dtype=None, layout=None):
            n = self.noises.pop(0)
            assert tuple(n.shape) == tuple(shape)
            return n.to(dtype)
        ref_dpm.randn_tensor = fake
        return self

    def __exit__(self, *a):
        ref_dpm.randn_tensor = self.orig


def run_trace(make, n, x0, mos, noises, dtype):
    s = make()
    s.set_timesteps(n)
    assert len(s.timesteps) == n
    x = torch.from_numpy(x0).to(dtype)
    steps = []
    with scheduler_noise(noises):
        for k, t in enumerate(s.timesteps):
            x = s.step(torch.from_numpy(mos[k]).to(dtype), t, x, return_dict=False)[0]
            steps.append(x.clone())
    return s, torch.stack(steps)


def traces(out, env):
    for (name, n), (x0, mos, noises) in trace_inputs().items():
        s, r64 = run_trace(CASES[name], n, x0, mos, noises, torch.float64)
        _, r32 = run_trace(CASES[name], n, x0, mos, noises, torch.float32)
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32
        key = f"trace/{name}/{n}"
        out[f"{key}/timesteps"] = s.timesteps.numpy()
        out[f"{key}/sigmas"] = s.sigmas.numpy()
        out[f"{key}/ref64"] = r64.numpy()
        out[f"{key}/ref32"] = r32.numpy()
        dev = float(((r32.double() - r64).abs() / (1 + r64.abs())).max())
        env["fp32"][f"{name}/{n}"] = dev
        print(f"{key:32s} reference fp32 deviation {dev:.3e}")


PIPE_CASES = {
    "dpmpp_2m": lambda: DPMSolverMultistepScheduler.from_config(_pndm_config()),
    "dpmpp_2m_karras": lambda: DPMSolverMultistepScheduler.from_config(_pndm_config(), use_karras_sigmas=True),
}


def run_pipe(name, unet, brushnet, vae, dtype, vae_noise=None):
    ucfg = R.TINY_UNET
    pipe = StableDiffusionBrushNetPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, brushnet=brushnet,
                                           scheduler=PIPE_CASES[name](), safety_checker=None, feature_extractor=None,
                                           requires_safety_checker=False, depth_conditioning_mode="concat")
    pipe.set_progress_bar_config(disable=True)
    inp = synth.pipeline_inputs(1, 16, 16, seed=1234, cross_dim=ucfg["cross_attention_dim"], vae_scale=2)
    trace, captured = [], {}
    hook = brushnet.register_forward_pre_hook(
        lambda mod, args, kwargs: captured.update(cond=kwargs["brushnet_cond"].clone()), with_kwargs=True)
    call = lambda: pipe(prompt_embeds=inp["prompt_embeds"].to(dtype), negative_prompt_embeds=inp["negative_prompt_embeds"].to(dtype),
                        image=inp["image"], mask=inp["mask"], depth=inp["depth"], num_inference_steps=4, guidance_scale=7.5,
                        latents=inp["latents"].clone().to(dtype), output_type="pt", brushnet_conditioning_scale=1.0,
                        callback_on_step_end=lambda p, i, t, k: trace.append(k["latents"].clone()) or {}, height=16, width=16)
    if vae_noise is None:
        torch.manual_seed(777)       # the reference draws the VAE posterior noise from the global RNG (:1188)
        res = call()
    else:
        with fixed_noise([vae_noise]):
            res = call()
    hook.remove()
    return pipe, captured["cond"], trace, res.images


def pipelines(out, env):
    ucfg, vcfg = R.TINY_UNET, R.TINY_VAE
    (unet, _, _), (brushnet, _, _), (vae, _, _) = MG.models(ucfg, vcfg, 0)
    for name in PIPE_CASES:
        pipe, cond, trace, image = run_pipe(name, unet, brushnet, vae, torch.float32)
        torch.manual_seed(777)
        out[f"{name}_vae_noise"] = torch.randn(2, 4, 8, 8).numpy()
        out[f"{name}_timesteps"] = pipe.scheduler.timesteps.numpy()
        out[f"{name}_cond"] = cond.numpy()
        for i, l in enumerate(trace):
            out[f"{name}_latents_{i}"] = l.numpy()
        out[f"{name}_image"] = image.numpy()
    for dt_name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        (u, _, _), (b, _, _), (v, _, _) = MG.models(ucfg, vcfg, 0)
        for m in (u, b, v):
            m.to(dt)
        for name in PIPE_CASES:
            _, cond, trace, image = run_pipe(name, u, b, v, dt, torch.from_numpy(out[f"{name}_vae_noise"]))
            e = env[dt_name]
            e[f"dpmsolver/{name}/cond"] = stats(cond, out[f"{name}_cond"])
            for i, l in enumerate(trace):
                e[f"dpmsolver/{name}/latents_{i}"] = stats(l, out[f"{name}_latents_{i}"])
            e[f"dpmsolver/{name}/image"] = stats(image, out[f"{name}_image"])
            print(f"[{dt_name}] {name}: latents linf {[round(e[f'dpmsolver/{name}/latents_{i}']['linf'], 5) for i in range(len(trace))]} "
                  f"image linf {e[f'dpmsolver/{name}/image']['linf']:.3e}")


if __name__ == "__main__":
    out, env = {}, dict(fp32={}, bf16={}, fp16={})
    env["_about"] = ("fp32: max |ref32 - ref64| / (1 + |ref64|) of the imported reference's DPMSolverMultistepScheduler per trace case / steps; "
                     "bf16, fp16: |reference(dtype) - reference(fp32)| on the tiny pipeline cases, as in bf16_envelope.json "
                     "(tools/make_golden_dpmsolver.py)")
    traces(out, env)
    pipelines(out, env)
    # (the fp32 traces go to a file of their own: together the two pass the size limit of a committed file)
    np.savez_compressed(os.path.join(GOLD, "dpmsolver.npz"), **{k: v for k, v in out.items() if not k.endswith("/ref32")})
    np.savez_compressed(os.path.join(GOLD, "dpmsolver_ref32.npz"), **{k: v for k, v in out.items() if k.endswith("/ref32")})
    with open(os.path.join(GOLD, "dpmsolver_envelope.json"), "w") as f:
        json.dump(env, f, indent=1, sort_keys=True)
