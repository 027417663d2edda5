"""GraphedTrainStep.from_pixels with its draws from a torch generator (made ahead of every replay by ATen kernels and copied into static
buffers) against the same step drawing from a rng.PhiloxGenerator INSIDE its graph (one mf_train_batch_draw launch and the advance).

Shape: tools/bench_train_batch.py's — batch 8 x 512 x 512, SD1.5 VAE / UNet / BrushNet with the bench's synthetic weights, depth 'concat',
snr_gamma 5, bf16x1.  Both steps live in one process on one model and optimizer and are timed alternately after both are captured:
  draws + staging   what runs ahead of a replay besides the dataset side: (torch) BatchFrontEnd.draw — two posterior noises, the noise,
                    the timesteps — and the copies of draws, pixels and text states into the static inputs; (philox) the copies of
                    pixels and text states alone, plus — timed on its own, it replays inside the graph — the one draw launch and the advance
  samples/s         whole steps from host uint8 arrays
Informational: no threshold.  Writes profiles/philox_bench.txt.

usage: python tools/bench_philox.py [--batch 8] [--size 512] [--repeats 9] [--steps 6]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "philox_bench.txt"))
    a = ap.parse_args()
    from reflecting_reality_amd import AutoencoderKL, BrushNetModel, DDPMScheduler, UNet2DConditionModel, frontend, hip, synth
    from reflecting_reality_amd.configs import SD15_SCHED, SD15_UNET, SD15_VAE, brushnet_config
    from reflecting_reality_amd.rng import PhiloxGenerator
    from reflecting_reality_amd.training import AdamW, BatchFrontEnd, GraphedTrainStep, MirrorFusionModel
    if not torch.cuda.is_available():
        raise SystemExit("bench_philox.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    hip.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    b, size, gamma, prec = a.batch, a.size, 5.0, "bf16x1"
    vae = AutoencoderKL(dict(SD15_VAE), precision="bf16", device=dev)
    vae.load_state_dict(synth.state_dict_for(vae.param_shapes(), 2))
    ns = DDPMScheduler(**{k: v for k, v in SD15_SCHED.items() if k in ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule")})
    fe = BatchFrontEnd(vae, ns, depth_conditioning_mode="concat", snr_gamma=gamma)
    r = np.random.RandomState(7)
    data = dict(image=r.randint(0, 256, (b, size, size, 3)).astype(np.uint8), mask=np.zeros((b, size, size), np.uint8),
                depth=(r.rand(b, size, size) * 4 + 0.5).astype(np.float32))
    data["mask"][:, size // 4: size // 2, size // 3: 2 * size // 3] = 255
    flips = [bool(i % 2) for i in range(b)]
    ehs = torch.randn(b, 77, 768, generator=torch.Generator().manual_seed(3)).to(dev)

    def example():
        batch = frontend.training_example(data, resolution=size, flip=flips, depth=True)
        batch["encoder_hidden_states"] = ehs
        return batch

    unet = UNet2DConditionModel(dict(SD15_UNET), precision=prec, device=dev)
    unet.load_state_dict(synth.state_dict_for(unet.param_shapes(), 0))
    bn = BrushNetModel(dict(brushnet_config(SD15_UNET, 6)), precision=prec, device=dev)
    bn.load_state_dict(synth.state_dict_for(bn.param_shapes(), 1))
    model = MirrorFusionModel(unet, bn).prepare_training()
    opt = AdamW(model.get_trainable_modules(), lr=1e-5)
    steps = {name: GraphedTrainStep(model, ns, opt, snr_gamma=gamma, max_grad_norm=1.0, front_end=fe) for name in ("torch", "philox")}
    gens = {"torch": torch.Generator(dev).manual_seed(5), "philox": PhiloxGenerator(5, dev)}
    run = {name: (lambda name=name: steps[name].from_pixels(example(), generator=gens[name])) for name in steps}
    for name in steps:                                     # two eager warm-up calls, the capture, one replay — of each path
        for _ in range(4):
            run[name]()
    px = {name: steps[name]._px for name in steps}
    assert px["philox"]._philox is not None and px["torch"]._philox is None and all(p.graph is not None for p in px.values())
    shape = px["torch"]._latent_shape
    batch = example()

    def ahead_torch():
        px["torch"]._stage_pixels(batch, fe.draw(batch, shape, generator=gens["torch"]))

    def ahead_philox():
        px["philox"]._stage_pixels(batch, ([None] * 4, None, None, ehs))

    scratch = [torch.empty_like(t) if t is not None else None for t in px["philox"].draws]
    state = PhiloxGenerator(9, dev).device_state()

    def draw_launches():
        fe.philox_draw(scratch, gens["philox"], 0, b, state=state)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    T = {k: [] for k in ("torch", "torch_host", "philox", "philox_host", "launch", "launch_host")}
    for fn in (ahead_torch, ahead_philox, draw_launches):
        fn()
    for _ in range(a.repeats):
        for key, fn in (("torch", ahead_torch), ("philox", ahead_philox), ("launch", draw_launches)):
            t, th = timed(fn)
            T[key].append(t); T[key + "_host"].append(th)
    say(f"# tools/bench_philox.py  batch {b} x {size} x {size}, SD1.5 ({prec}; VAE bf16), depth 'concat', snr_gamma {gamma}; ms unless said otherwise")
    say(f"torch generator: draws (3 randn + randint) + staging copies, device events   {spread(T['torch'])}")
    say(f"torch generator: the same, host clock to synchronise                          {spread(T['torch_host'])}")
    say(f"PhiloxGenerator: staging copies ahead of the replay (no draws), device events {spread(T['philox'])}")
    say(f"PhiloxGenerator: the same, host clock to synchronise                          {spread(T['philox_host'])}")
    say(f"PhiloxGenerator: the draw + advance launches on their own, device events      {spread(T['launch'])}")
    say(f"PhiloxGenerator: the same, host clock to synchronise (in the graph: no host)  {spread(T['launch_host'])}")
    rates = {name: [] for name in steps}
    for _ in range(3):
        for name in steps:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss, norm = run[name]()
            torch.cuda.synchronize()
            rates[name].append(b * a.steps / (time.perf_counter() - t0))
            assert torch.isfinite(loss).all() and torch.isfinite(norm).all()
    say(f"from_pixels, torch-generator draws, samples/s   {spread(rates['torch'])}")
    say(f"from_pixels, PhiloxGenerator draws, samples/s   {spread(rates['philox'])}")
    mt, mp = statistics.median(rates["torch"]), statistics.median(rates["philox"])
    say(f"PhiloxGenerator / torch generator, samples/s: {mp / mt:.4f} (the windows' ranges above say how much of that is noise)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
