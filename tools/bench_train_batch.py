"""From pixels to train_step inputs: today's composition against the device front end, and the training step fed from pixels.

Shape: the training leg's (bench.py --mode train) — batch 8 x 512 x 512, SD1.5 VAE / UNet / BrushNet with the bench's synthetic weights,
depth 'concat' (6 conditioning channels), snr_gamma 5.  From the SAME uint8 inputs, alternating in one process after warming every shape:
  (a) vae.encode(...).latent_dist.sample() * scaling_factor (x2), F.interpolate (mask, depth), torch.cat, add_noise (timesteps drawn on the
      device, as the script draws them), the compute_snr weights and their upload — what a caller of train_step composes today;
  (b) BatchFrontEnd: the same encodes, then one mf_train_batch_assemble launch.
The encodes and the rest ("staging") are timed separately with device events; the spread of the repeats is reported with the median.
Then GraphedTrainStep.from_pixels (uint8 host arrays -> training_example -> encodes -> captured step) against GraphedTrainStep.__call__
on prepared latents, in samples/s.  Writes profiles/train_batch_bench.txt.

usage: python tools/bench_train_batch.py [--batch 8] [--size 512] [--repeats 9] [--steps 6] [--no-train]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return f"median {statistics.median(xs):8.3f}  min {min(xs):8.3f}  max {max(xs):8.3f}  (n={len(xs)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--steps", type=int, default=6, help="training steps per timed window")
    ap.add_argument("--no-train", action="store_true", help="skip the GraphedTrainStep comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_batch_bench.txt"))
    a = ap.parse_args()
    from reflecting_reality_amd import AutoencoderKL, BrushNetModel, DDPMScheduler, UNet2DConditionModel, frontend, hip, synth
    from reflecting_reality_amd.configs import SD15_SCHED, SD15_UNET, SD15_VAE, brushnet_config
    from reflecting_reality_amd.training import AdamW, BatchFrontEnd, GraphedTrainStep, MirrorFusionModel, compute_snr
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_batch.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    hip.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    b, size, gamma = a.batch, a.size, 5.0
    vae = AutoencoderKL(dict(SD15_VAE), precision="bf16", device=dev)
    vae.load_state_dict(synth.state_dict_for(vae.param_shapes(), 2))
    ns = DDPMScheduler(**{k: v for k, v in SD15_SCHED.items() if k in ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule")})
    fe = BatchFrontEnd(vae, ns, depth_conditioning_mode="concat", snr_gamma=gamma)
    r = np.random.RandomState(7)
    data = dict(image=r.randint(0, 256, (b, size, size, 3)).astype(np.uint8), mask=np.zeros((b, size, size), np.uint8),
                depth=(r.rand(b, size, size) * 4 + 0.5).astype(np.float32))
    data["mask"][:, size // 4: size // 2, size // 3: 2 * size // 3] = 255
    flips = [bool(i % 2) for i in range(b)]
    g = torch.Generator().manual_seed(3)
    ehs = torch.randn(b, 77, 768, generator=g).to(dev)
    sf = vae.config["scaling_factor"]

    def example():
        batch = frontend.training_example(data, resolution=size, flip=flips, depth=True)
        batch["encoder_hidden_states"] = ehs
        return batch

    batch = example()
    hl = size // 8
    pn = [torch.randn(b, 4, hl, hl, generator=g).to(dev) for _ in range(2)]
    noise = torch.randn(b, 4, hl, hl, generator=g).to(dev)

    def encodes():
        return [vae.encode(batch[k]).latent_dist for k in ("pixel_values", "conditioning_pixel_values")]

    def staging_a(dists, ts):
        latents = dists[0].sample(noise=pn[0]) * sf
        cond = dists[1].sample(noise=pn[1]) * sf
        cond = torch.cat([cond, F.interpolate(batch["masks"], size=latents.shape[-2:])], 1)
        cond = torch.cat([cond, F.interpolate(batch["depths"], size=latents.shape[-2:])], 1)
        noisy = ns.add_noise(latents, noise, ts)
        snr = compute_snr(ns, ts)
        w = torch.stack([snr, gamma * torch.ones_like(snr)], dim=1).min(dim=1)[0] / snr
        return noisy, noise, cond, hip.h2d(w.float().contiguous(), dev), hip.h2d(ts.reshape(-1).float().contiguous(), dev)

    def staging_b(dists, ts):
        from reflecting_reality_amd.training import EncodedBatch
        return fe.assemble(EncodedBatch([d.moments_nhwc for d in dists] + [None, None], pn + [None, None], noise, ts, batch["masks"],
                                        batch["depths"], None, None))

    def timed(fn, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn(*args)
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    draw = lambda: torch.randint(0, 1000, (b,), device=dev).long()
    for _ in range(3):                                     # every shape of the timed window, tuned and loaded
        d = encodes()
        ra, rb = staging_a(d, draw()), staging_b(d, draw())
    ts = draw()
    ra, rb = staging_a(d, ts), staging_b(d, ts)
    same = torch.equal(ra[0], rb["noisy_latents"]) and torch.equal(ra[2], rb["conditioning_latents"]) and torch.equal(ra[3], rb["loss_weights"]) \
        and torch.equal(ra[4], rb["timesteps_f32"])
    say(f"# tools/bench_train_batch.py  batch {b} x {size} x {size}, SD1.5 VAE (bf16), depth 'concat', snr_gamma {gamma}; device events, ms")
    say(f"outputs of (a) and (b) on the same draws bit-equal: {same}")
    T = {k: [] for k in ("enc_a", "enc_b", "stage_a", "stage_b", "stage_a_host", "stage_b_host", "example")}
    for _ in range(a.repeats):
        ts = draw()
        d, t, _ = timed(encodes)
        T["enc_a"].append(t)
        _, t, th = timed(staging_a, d, ts)
        T["stage_a"].append(t); T["stage_a_host"].append(th)
        d, t, _ = timed(encodes)
        T["enc_b"].append(t)
        _, t, th = timed(staging_b, d, ts)
        T["stage_b"].append(t); T["stage_b_host"].append(th)
        _, t, _ = timed(example)
        T["example"].append(t)
    say(f"(a) VAE encodes x2                      {spread(T['enc_a'])}")
    say(f"(b) VAE encodes x2 (the same calls)     {spread(T['enc_b'])}")
    say(f"(a) staging: sample, scale, interpolate, cat, add_noise, SNR weights     {spread(T['stage_a'])}")
    say(f"(b) staging: one mf_train_batch_assemble launch                          {spread(T['stage_b'])}")
    say(f"(a) staging, host clock to synchronise  {spread(T['stage_a_host'])}")
    say(f"(b) staging, host clock to synchronise  {spread(T['stage_b_host'])}")
    say(f"dataset side (b only): training_example from host uint8 arrays, upload included   {spread(T['example'])}")
    if not a.no_train:
        prec = "bf16x1"
        unet = UNet2DConditionModel(dict(SD15_UNET), precision=prec, device=dev)
        unet.load_state_dict(synth.state_dict_for(unet.param_shapes(), 0))
        bn = BrushNetModel(dict(brushnet_config(SD15_UNET, 6)), precision=prec, device=dev)
        bn.load_state_dict(synth.state_dict_for(bn.param_shapes(), 1))
        model = MirrorFusionModel(unet, bn).prepare_training()
        opt = AdamW(model.get_trainable_modules(), lr=1e-5)
        step = GraphedTrainStep(model, ns, opt, snr_gamma=gamma, max_grad_norm=1.0, front_end=fe)
        lat, cond = rb["latents"].clone(), rb["conditioning_latents"].clone()
        hg = torch.Generator().manual_seed(5)

        def latent_step():
            return step(lat, noise, torch.randint(0, 1000, (b,), generator=hg), ehs, cond)

        def pixel_step():
            return step.from_pixels(example())

        for _ in range(4):                                 # two eager warm-up calls, the capture, one replay — of each path
            latent_step()
        for _ in range(4):
            pixel_step()
        rates = {"latents": [], "pixels": []}
        for _ in range(3):
            for name, fn in (("latents", latent_step), ("pixels", pixel_step)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loss, norm = fn()
                torch.cuda.synchronize()
                rates[name].append(b * a.steps / (time.perf_counter() - t0))
                assert torch.isfinite(loss).all() and torch.isfinite(norm).all()
        say(f"GraphedTrainStep.__call__ on prepared latents ({prec}), samples/s     {spread(rates['latents'])}")
        say(f"GraphedTrainStep.from_pixels from host uint8 arrays ({prec}), samples/s {spread(rates['pixels'])}")
        step_ms = 1e3 * b / statistics.median(rates["pixels"])
        say(f"share of the from-pixels step the two VAE encodes take: {statistics.median(T['enc_b']) / step_ms * 100:.1f} % "
            f"({statistics.median(T['enc_b']):.1f} of {step_ms:.1f} ms)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
