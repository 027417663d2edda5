"""Golden fixtures for EulerDiscreteScheduler / EulerAncestralDiscreteScheduler, from the IMPORTED REFERENCE
(schedulers/scheduling_euler_discrete.py, scheduling_euler_ancestral_discrete.py).

Runs only where the reference checkout that tools/make_golden.py imports exists; nothing under tests/, bench.py or the package reads it
at run time.  Results only: every input is regenerated from a seed by the tests.

    python tools/make_golden_euler.py

  tests/golden/euler.npz            scheduler traces `trace/<case>/<steps>/{timesteps, sigmas, init_noise_sigma, ref64, scaled64}`: per step
                                    the reference's sample after step() and what its scale_model_input returned before it, on float64
                                    tensors (`.../scaled64` is in euler_scaled64.npz; those on fp32 tensors, `.../ref32` and
                                    `.../scaled32`, are in euler_ref32.npz: each file stays under the committed-file limit); and the tiny
                                    pipeline's `<case>_{timesteps, cond, vae_noise, latents_<i>, image}` (keys and inputs as in
                                    dpmsolver.npz) for euler and euler_linspace_karras; `machine/log_sigmas`: numpy's float32 log of
                                    the training sigmas on the machine that ran the reference
  tests/golden/euler_envelope.json  "fp32": per trace, max |ref32 - ref64| / (1 + |ref64|) over the samples (`<case>/<steps>`) and over the
                                    scaled model inputs (`<case>/<steps>/scaled`) — the reference's own fp32 deviation; "bf16" / "fp16":
                                    the reference's deviation from its fp32 pipeline results in that dtype, as tools/make_golden_dpmsolver.py

The reference's ancestral class has no Karras option: `a_linspace_karras` is built from the Karras Euler config by from_config, which
drops the key (as the library's class does), so the case is the ancestral sampler on the fractional `linspace` timesteps.
"""
import contextlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as MG  # noqa: E402  (sets up the reference import path + the FLAX_WEIGHTS_NAME shim)
from make_golden import PNDMScheduler, GOLD  # noqa: E402
import make_golden_dpmsolver as MD  # noqa: E402
import diffusers.schedulers.scheduling_euler_ancestral_discrete as ref_anc  # noqa: E402
from diffusers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler  # noqa: E402

torch.set_grad_enabled(False)
SD = MD.SD
SHAPE = (2, 4, 8, 8)
STEPS = (5, 20)


def _pndm_config():
    """The checkpoint's scheduler as its scheduler_config.json states it: the spacing is an explicit key there, so it crosses classes."""
    return PNDMScheduler(**SD, steps_offset=1, skip_prk_steps=True, set_alpha_to_one=False, timestep_spacing="leading").config


# the issue's case table; tests/test_euler_cpu.py builds the same schedulers from the library's classes
CASES = {
    "from_pndm": lambda: EulerDiscreteScheduler.from_config(_pndm_config()),
    "linspace": lambda: EulerDiscreteScheduler(**SD),
    "trailing_karras": lambda: EulerDiscreteScheduler(**SD, timestep_spacing="trailing", use_karras_sigmas=True),
    "v_pred": lambda: EulerDiscreteScheduler(**SD, prediction_type="v_prediction"),
    "sample": lambda: EulerDiscreteScheduler(**SD, prediction_type="sample"),
    "a_from_pndm": lambda: EulerAncestralDiscreteScheduler.from_config(_pndm_config()),
    "a_linspace_karras": lambda: EulerAncestralDiscreteScheduler.from_config(EulerDiscreteScheduler(**SD, use_karras_sigmas=True).config),
    "a_v_trailing": lambda: EulerAncestralDiscreteScheduler(**SD, prediction_type="v_prediction", timestep_spacing="trailing"),
}


def trace_inputs():
    """{(case, steps): (x0, [model outputs], [noises] | None)} from ONE np.random.default_rng(7), cases in table order, then 5 and 20
    steps; per entry: the start sample (a unit normal: the trace multiplies it by init_noise_sigma), the model outputs, then
    (ancestral) the noises."""
    rng = np.random.default_rng(7)
    out = {}
    for name in CASES:
        for n in STEPS:
            x0 = rng.standard_normal(SHAPE, dtype=np.float32)
            mos = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(n)]
            noises = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(n)] if name.startswith("a_") else None
            out[(name, n)] = (x0, mos, noises)
    return out


class scheduler_noise(MD.scheduler_noise):
    """make_golden_dpmsolver.scheduler_noise on the ancestral module's randn_tensor."""

    def __enter__(self):
        self.orig = ref_anc.randn_tensor

        def fake(shape, generator=None, device=None, dtype=None, layout=None):
            n = self.noises.pop(0)
            assert tuple(n.shape) == tuple(shape)
            return n.to(dtype)
        ref_anc.randn_tensor = fake
        return self

    def __exit__(self, *a):
        ref_anc.randn_tensor = self.orig


def run_trace(make, n, x0, mos, noises, dtype):
    s = make()
    s.set_timesteps(n)
    assert len(s.timesteps) == n
    x = torch.from_numpy(x0).to(dtype) * s.init_noise_sigma.to(dtype)
    steps, scaled = [], []
    with scheduler_noise(noises) if noises is not None else contextlib.nullcontext():
        for k, t in enumerate(s.timesteps):
            scaled.append(s.scale_model_input(x, t).clone())
            x = s.step(torch.from_numpy(mos[k]).to(dtype), t, x, return_dict=False)[0]
            steps.append(x.clone())
    return s, torch.stack(steps), torch.stack(scaled)


def _dev(a32, a64):
    return float(((a32.double() - a64).abs() / (1 + a64.abs())).max())


def traces(out, env):
    for (name, n), (x0, mos, noises) in trace_inputs().items():
        s, r64, s64 = run_trace(CASES[name], n, x0, mos, noises, torch.float64)
        _, r32, s32 = run_trace(CASES[name], n, x0, mos, noises, torch.float32)
        assert r64.dtype == s64.dtype == torch.float64 and r32.dtype == s32.dtype == torch.float32
        key = f"trace/{name}/{n}"
        out[f"{key}/timesteps"] = s.timesteps.numpy()
        out[f"{key}/sigmas"] = s.sigmas.numpy()
        out[f"{key}/init_noise_sigma"] = np.asarray(s.init_noise_sigma.numpy())
        out[f"{key}/ref64"], out[f"{key}/scaled64"] = r64.numpy(), s64.numpy()
        out[f"{key}/ref32"], out[f"{key}/scaled32"] = r32.numpy(), s32.numpy()
        env["fp32"][f"{name}/{n}"], env["fp32"][f"{name}/{n}/scaled"] = _dev(r32, r64), _dev(s32, s64)
        print(f"{key:32s} reference fp32 deviation: samples {env['fp32'][f'{name}/{n}']:.3e}, model inputs {env['fp32'][f'{name}/{n}/scaled']:.3e}")


PIPE_CASES = {
    "euler": lambda: EulerDiscreteScheduler.from_config(_pndm_config()),
    "euler_linspace_karras": lambda: EulerDiscreteScheduler.from_config(_pndm_config(), timestep_spacing="linspace", use_karras_sigmas=True),
}


def pipelines(out, env):
    """make_golden_dpmsolver.pipelines over this file's cases (run_pipe reads the case table of its module)."""
    saved, MD.PIPE_CASES = MD.PIPE_CASES, PIPE_CASES
    try:
        sub = dict(fp32={}, bf16={}, fp16={})
        MD.pipelines(out, sub)
    finally:
        MD.PIPE_CASES = saved
    for dt in ("bf16", "fp16"):
        env[dt].update({k.replace("dpmsolver/", "euler/", 1): v for k, v in sub[dt].items()})


if __name__ == "__main__":
    out, env = {}, dict(fp32={}, bf16={}, fp16={})
    env["_about"] = ("fp32: max |ref32 - ref64| / (1 + |ref64|) of the imported reference's Euler / Euler-ancestral schedulers per trace "
                     "case / steps, over the samples and (…/scaled) over scale_model_input's outputs; bf16, fp16: |reference(dtype) - "
                     "reference(fp32)| on the tiny pipeline cases, as in bf16_envelope.json (tools/make_golden_euler.py)")
    traces(out, env)
    pipelines(out, env)
    # numpy's float32 log differs in the last bits between CPU dispatch paths, and _sigma_to_t divides by the table's small differences:
    # Karras timesteps are bit-reproducible only where this table is (tests/test_euler_cpu.py assert_timesteps)
    ac = torch.cumprod(1.0 - torch.linspace(SD["beta_start"] ** 0.5, SD["beta_end"] ** 0.5, SD["num_train_timesteps"], dtype=torch.float32) ** 2, dim=0)
    out["machine/log_sigmas"] = np.log(np.array(((1 - ac) / ac) ** 0.5))
    # (the fp32 traces and the float64 model inputs go to files of their own: together they pass the size limit of a committed file)
    is32 = lambda k: k.endswith("/ref32") or k.endswith("/scaled32")
    is_scaled64 = lambda k: k.endswith("/scaled64")
    np.savez_compressed(os.path.join(GOLD, "euler.npz"), **{k: v for k, v in out.items() if not is32(k) and not is_scaled64(k)})
    np.savez_compressed(os.path.join(GOLD, "euler_scaled64.npz"), **{k: v for k, v in out.items() if is_scaled64(k)})
    np.savez_compressed(os.path.join(GOLD, "euler_ref32.npz"), **{k: v for k, v in out.items() if is32(k)})
    with open(os.path.join(GOLD, "euler_envelope.json"), "w") as f:
        json.dump(env, f, indent=1, sort_keys=True)
