"""Golden fixtures of tiled VAE encode / decode, produced by running the IMPORTED REFERENCE (its AutoencoderKL.enable_tiling(),
models/autoencoders/autoencoder_kl.py:311-423), and the reference's own bf16 / fp16 deviation on the same cases.

Runs only where the reference is importable (the same set-up as tools/make_golden.py).  Writes
    tests/golden/vae_tiling.npz             tiled and (as fp16) untiled outputs of the main case, whose inputs the tests regenerate from
                                            their seeds; the batch-3 case; the pipeline case; the shape table
    tests/golden/vae_tiling_envelope.json   |reference(bf16 / fp16) - reference(fp32)| on the tiled cases: linf / mean

    python tools/make_golden_vae_tiling.py
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
from make_golden import AutoencoderKL, DDIMScheduler, StableDiffusionBrushNetPipeline, R, synth, GOLD  # noqa: E402
from make_bf16_envelope import fixed_noise, stats  # noqa: E402

torch.set_grad_enabled(False)
SAMPLE_SIZE = 16            # main case: latent tile 8, overlap 6; decode extent 4 / limit 12; encode extent 2 / limit 6
# (mode, H, W, sample_size): decode sizes are latents, encode sizes are pixels
SHAPE_CASES = [("decode", 13, 11, 16), ("decode", 23, 17, 20), ("decode", 14, 14, 24), ("decode", 8, 8, 16), ("decode", 8, 12, 16),
               ("encode", 27, 23, 16), ("encode", 40, 35, 20), ("encode", 28, 28, 24), ("encode", 16, 16, 16)]


def build_vae(cfg, sample_size):
    """make_golden.build_vae with a sample_size (the tile threshold); weights synth seed 2 like every tiny VAE fixture."""
    n = len(cfg["block_out_channels"])
    vae = AutoencoderKL(in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",) * n,
                        up_block_types=("UpDecoderBlock2D",) * n, block_out_channels=cfg["block_out_channels"],
                        layers_per_block=cfg["layers_per_block"], latent_channels=cfg["latent_channels"],
                        norm_num_groups=cfg["norm_num_groups"], scaling_factor=cfg["scaling_factor"], sample_size=sample_size).eval()
    MG.load_synth(vae, 2)
    return vae


def main_inputs():
    g = torch.Generator().manual_seed(4242)
    z = torch.randn(2, 4, 13, 11, generator=g)
    img = torch.rand(2, 3, 27, 23, generator=g) * 2 - 1
    return z, img


def batch3_input():
    return torch.randn(3, 4, 9, 9, generator=torch.Generator().manual_seed(4243))


def main_case(out):
    vae = build_vae(R.TINY_VAE, SAMPLE_SIZE)
    z, img = main_inputs()
    # the inputs are regenerated from their seeds by the tests (main_inputs / batch3_input); the untiled results only have to show
    # that tiling changes the result by ~1, so they are kept as fp16
    out["decode_untiled"] = vae.decode(z, return_dict=False)[0].numpy().astype(np.float16)
    out["moments_untiled"] = vae.encode(img).latent_dist.parameters.numpy().astype(np.float16)
    vae.enable_tiling()
    out["decode_tiled"] = vae.decode(z, return_dict=False)[0].numpy()
    out["moments_tiled"] = vae.encode(img).latent_dist.parameters.numpy()
    assert out["decode_tiled"].shape == (2, 3, 26, 22) and out["moments_tiled"].shape == (2, 8, 13, 11)
    print("main case: tiled vs untiled  decode", float(np.abs(out["decode_tiled"] - out["decode_untiled"].astype(np.float32)).max()),
          " moments", float(np.abs(out["moments_tiled"] - out["moments_untiled"].astype(np.float32)).max()))
    # batch 3 for the slicing test: sliced == whole batch in the reference (every layer is per sample); tiled decode of 3 latents
    z3 = batch3_input()
    out["decode3_tiled"] = vae.decode(z3, return_dict=False)[0].numpy()
    vae.enable_slicing()
    print("batch 3: sliced vs whole in the reference", float((vae.decode(z3, return_dict=False)[0] - torch.from_numpy(out["decode3_tiled"])).abs().max()))


def shape_table():
    table = []
    for mode, H, W, ss in SHAPE_CASES:
        vae = build_vae(R.TINY_VAE, ss)
        vae.enable_tiling()
        calls = []
        net = vae.decoder if mode == "decode" else vae.encoder
        hook = net.register_forward_pre_hook(lambda mod, args: calls.append(list(args[0].shape[-2:])))
        if mode == "decode":
            res = vae.decode(torch.zeros(1, 4, H, W), return_dict=False)[0]
        else:
            res = vae.encode(torch.zeros(1, 3, H, W)).latent_dist.parameters
        hook.remove()
        table.append(dict(mode=mode, H=H, W=W, sample_size=ss, tile_shapes=calls, out=list(res.shape[-2:])))
        print(f"shape table: {mode} {H} x {W} sample_size {ss}: {len(calls)} tiles -> {list(res.shape[-2:])}")
    return table


def pipeline_case(out, env):
    ucfg, vcfg = R.TINY_UNET, R.TINY_VAE
    (unet, _, _), (brushnet, _, _), _ = MG.models(ucfg, vcfg, 0)
    vae = build_vae(vcfg, SAMPLE_SIZE)
    vae.enable_tiling()
    sc = R.SD15_SCHED
    inp = synth.pipeline_inputs(1, 32, 32, seed=1234, cross_dim=ucfg["cross_attention_dim"], vae_scale=2)

    def run(dtype, noises=None):
        sched = DDIMScheduler(num_train_timesteps=1000, beta_start=sc["beta_start"], beta_end=sc["beta_end"], beta_schedule="scaled_linear",
                              clip_sample=False, set_alpha_to_one=False, steps_offset=1)
        pipe = StableDiffusionBrushNetPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, brushnet=brushnet, scheduler=sched,
                                               safety_checker=None, feature_extractor=None, requires_safety_checker=False,
                                               depth_conditioning_mode="concat")
        pipe.set_progress_bar_config(disable=True)
        captured = {}
        hook = brushnet.register_forward_pre_hook(
            lambda mod, args, kwargs: captured.update(cond=kwargs["brushnet_cond"].clone()), with_kwargs=True)
        kw = dict(prompt_embeds=inp["prompt_embeds"].to(dtype), negative_prompt_embeds=inp["negative_prompt_embeds"].to(dtype),
                  image=inp["image"], mask=inp["mask"], depth=inp["depth"], num_inference_steps=2, guidance_scale=7.5,
                  latents=inp["latents"].clone().to(dtype), output_type="pt", brushnet_conditioning_scale=1.0, height=32, width=32)
        if noises is None:
            torch.manual_seed(777)           # the reference draws the VAE posterior noise from the global RNG
            res = pipe(**kw)
        else:
            with fixed_noise(noises):
                res = pipe(**kw)
        hook.remove()
        return captured["cond"], res.images

    cond, image = run(torch.float32)
    torch.manual_seed(777)
    vae_noise = torch.randn(2, 4, 16, 16)
    cond2, image2 = run(torch.float32, [vae_noise])
    assert torch.equal(cond, cond2) and torch.equal(image, image2), "the recorded posterior noise does not reproduce the run"
    out["pipe_vae_noise"], out["pipe_cond"], out["pipe_image"] = vae_noise.numpy(), cond.numpy(), image.numpy()
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        for m in (unet, brushnet, vae):
            m.to(dt)
        c, im = run(dt, [vae_noise])
        env[name]["pipeline_cond"], env[name]["pipeline_image"] = stats(c, cond), stats(im, image)
    for m in (unet, brushnet, vae):
        m.to(torch.float32)


def envelope(out, env):
    z, img = main_inputs()
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        vae = build_vae(R.TINY_VAE, SAMPLE_SIZE).to(dt)
        vae.enable_tiling()
        env[name]["decode"] = stats(vae.decode(z.to(dt), return_dict=False)[0], out["decode_tiled"])
        env[name]["encode"] = stats(vae.encode(img.to(dt)).latent_dist.parameters, out["moments_tiled"])
        env[name]["decode3"] = stats(vae.decode(batch3_input().to(dt), return_dict=False)[0], out["decode3_tiled"])


if __name__ == "__main__":
    out = {}
    env = {"_about": "|reference(bf16 / fp16) - reference(fp32)| of the imported reference with enable_tiling() on the cases of "
                     "tests/golden/vae_tiling.npz (tools/make_golden_vae_tiling.py): linf / mean abs error, and the fp32 result's abs max / mean",
           "bf16": {}, "fp16": {}}
    main_case(out)
    envelope(out, env)
    pipeline_case(out, env)
    out["shape_table_json"] = np.array(json.dumps(shape_table()))
    np.savez_compressed(os.path.join(GOLD, "vae_tiling.npz"), **out)
    with open(os.path.join(GOLD, "vae_tiling_envelope.json"), "w") as f:
        json.dump(env, f, indent=1, sort_keys=True)
    for name in ("bf16", "fp16"):
        for k, v in sorted(env[name].items()):
            print(f"{name} {k:16s} linf {v['linf']:.3e} mean {v['mean']:.3e}  |ref| max {v['ref_absmax']:.2f} mean {v['ref_absmean']:.3f}")
    print("vae tiling fixtures written")
