"""Tiled and sliced VAE encode / decode on the device against the imported reference with enable_tiling()
(tests/golden/vae_tiling.npz, tools/make_golden_vae_tiling.py).

The two data-movement kernels are checked bit for bit against torch ops on the device: mf_vae_tile_blend against the reference's two
one-line ramps applied in place in its order (autoencoder_kl.py:311-321, 357-369), mf_crop_pack_nhwc against slicing + mf_pack_nhwc.
End to end, fp32 and f16x3 hold atol = rtol = 2e-4 — the TOL of test_models_gpu.test_tiny_vae: the same nets, each tile being a pass
that test already bounds, and a blend is a convex combination of two such results — while bf16 and fp16 stay inside the reference's
own deviation in that dtype on the same case (tests/golden/vae_tiling_envelope.json) times util's ENV_K_* factors.
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mirrorfusion_ref as R  # noqa: E402
from reflecting_reality_amd import DDIMScheduler, StableDiffusionBrushNetPipeline, hip, models as M, synth  # noqa: E402
from test_models_gpu import build  # noqa: E402
import util  # noqa: E402
from util import golden, keys, report  # noqa: E402

DEV = "cuda"
TOL = dict(atol=2e-4, rtol=2e-4)
PRECS = ["fp32", "f16x3", "bf16", "fp16"]
SD_SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                set_alpha_to_one=False)
_vaes = {}
_env = {}


def tiled_vae(prec):
    """The tiny VAE with sample_size 16 (latent tile 8, overlap 6; decode extent 4 / limit 12; encode extent 2 / limit 6), synth seed 2."""
    if prec not in _vaes:
        vae = M.AutoencoderKL(dict(R.TINY_VAE, sample_size=16), precision=prec, device=DEV)
        vae.load_state_dict(synth.state_dict_for(keys("tiny")["vae"], 2))
        _vaes[prec] = vae
    vae = _vaes[prec]
    vae.enable_tiling()
    vae.disable_slicing()
    vae.tile_batch = 16
    return vae


def main_inputs():                      # tools/make_golden_vae_tiling.py: main_inputs / batch3_input
    g = torch.Generator().manual_seed(4242)
    z = torch.randn(2, 4, 13, 11, generator=g)
    img = torch.rand(2, 3, 27, 23, generator=g) * 2 - 1
    return z, img


def batch3_input():
    return torch.randn(3, 4, 9, 9, generator=torch.Generator().manual_seed(4243))


def check(name, got, ref, prec, key):
    """fp32 / f16x3: TOL.  bf16 / fp16: the reference's own deviation on this case, times util.ENV_K_LINF_SMALL or ENV_K_LINF by element
    count, and ENV_K_MEAN."""
    if prec not in ("bf16", "fp16"):
        return report(name, got, ref, **TOL)
    if not _env:
        with open(os.path.join(util.GOLD, "vae_tiling_envelope.json")) as f:
            _env.update(json.load(f))
    env = _env[prec][key]
    got, ref = got.float().cpu(), torch.as_tensor(ref).float()
    err = (got - ref).abs()
    linf, mean = err.max().item(), err.mean().item()
    k_linf = util.ENV_K_LINF if ref.numel() >= util.ENV_SMALL_NUMEL else util.ENV_K_LINF_SMALL
    print(f"{name}: max_abs_err={linf:.3e} (reference {prec}: {env['linf']:.3e}) mean_abs_err={mean:.3e} (reference {prec}: {env['mean']:.3e}) "
          f"ENVRATIO linf {linf / env['linf']:.3f} mean {mean / env['mean']:.3f}")
    assert linf == linf, f"{name}: NaN"
    assert linf <= k_linf * env["linf"], f"{name}: L-inf {linf:.3e} > {k_linf} x the reference's {prec} envelope {env['linf']:.3e}"
    assert mean <= util.ENV_K_MEAN * env["mean"], f"{name}: mean error {mean:.3e} > {util.ENV_K_MEAN} x the reference's {prec} envelope {env['mean']:.3e}"


# ---- mf_vae_tile_blend, bit for bit ---------------------------------------------------------------------------------------------------
def reference_blend(tiles, nrows, ncols, extent, limit):
    """blend_v / blend_h / crop / cat of tiled_decode on NHWC tensors, in place in `tiles` like the reference in its stored tiles."""
    rows = []
    for i in range(nrows):
        row = []
        for j in range(ncols):
            t = tiles[(i, j)]
            if i > 0:
                a = tiles[(i - 1, j)]
                e = min(a.shape[1], t.shape[1], extent)
                for y in range(e):
                    t[:, y, :, :] = a[:, -e + y, :, :] * (1 - y / e) + t[:, y, :, :] * (y / e)
            if j > 0:
                a = tiles[(i, j - 1)]
                e = min(a.shape[2], t.shape[2], extent)
                for x in range(e):
                    t[:, :, x, :] = a[:, :, -e + x, :] * (1 - x / e) + t[:, :, x, :] * (x / e)
            row.append(t[:, :limit, :limit, :])
        rows.append(torch.cat(row, dim=2))
    return torch.cat(rows, dim=1)


# (tile heights, tile widths, blend_extent, row_limit): the main case's 3 x 2 grid with every min() clip and a 1-row tile; the decoded
# sizes of the same grid; a tile narrower than the extent; an extent that is no power of two (weights like 1/7) on one-shape tiles
GRIDS = [((8, 7, 1), (8, 5), 4, 6), ((16, 14, 2), (16, 10), 4, 12), ((8, 5), (8, 3), 4, 6), ((9, 9), (9, 9, 9), 7, 5)]


@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("heights,widths,extent,limit", GRIDS)
def test_tile_blend_is_the_references_arithmetic_bit_for_bit(heights, widths, extent, limit, nhwc):
    g = torch.Generator().manual_seed(7)
    for ld, c in ((4, 3), (8, 3), (8, 8)):
        for b in (1, 2):
            src = {(i, j): torch.randn(b, th, tw, ld, generator=g).to(DEV) for i, th in enumerate(heights) for j, tw in enumerate(widths)}
            want_tiles = {k: v.clone() for k, v in src.items()}
            want = reference_blend(want_tiles, len(heights), len(widths), extent, limit)
            got_tiles = {k: v.clone() for k, v in src.items()}
            oh, ow = want.shape[1], want.shape[2]
            out = torch.full((b, oh, ow, ld) if nhwc else (b, c, oh, ow), float("nan"), device=DEV)
            oy = 0
            for i, th in enumerate(heights):
                ox = 0
                for j, tw in enumerate(widths):
                    hip.vae_tile_blend(got_tiles[(i, j)], got_tiles.get((i - 1, j)), got_tiles.get((i, j - 1)), extent, limit, c, out, oy, ox,
                                       nhwc=nhwc)
                    ox += min(tw, limit)
                oy += min(th, limit)
            for k in src:
                assert torch.equal(got_tiles[k], want_tiles[k]), (k, ld, c, b)
            assert torch.equal(out, want if nhwc else want[..., :c].permute(0, 3, 1, 2).contiguous()), (ld, c, b)
            changed = sum(int(not torch.equal(src[k], want_tiles[k])) for k in src)
            assert changed == len(src) - 1                  # every tile but (0, 0) has a blended strip: the comparison is not vacuous


# ---- mf_crop_pack_nhwc, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_crop_pack_is_slicing_plus_pack_nhwc_bit_for_bit(dtype):
    g = torch.Generator().manual_seed(11)
    src = torch.randn(2, 3, 13, 11, generator=g).to(DEV)
    for c_pad in (8, 4, 6, 3):                               # 16-byte vectors, 8-byte vectors, and the scalar path
        for y0, x0, th, tw in ((0, 0, 8, 8), (6, 6, 7, 5), (12, 6, 1, 5), (5, 10, 8, 1), (0, 0, 13, 11)):
            want = hip.pack_nhwc(src[:, :, y0:y0 + th, x0:x0 + tw].contiguous(), None, c_pad, dtype)
            for slots, slot in ((1, 0), (3, 1), (3, 2)):
                stack = torch.full((slots * 2, th, tw, c_pad), 7.0, dtype=dtype, device=DEV)
                hip.crop_pack_nhwc(src, y0, x0, th, tw, stack, slot * 2)
                assert torch.equal(stack[slot * 2:slot * 2 + 2], want), (c_pad, y0, x0, th, tw, slot)
                rest = torch.cat([stack[:slot * 2], stack[slot * 2 + 2:]])
                assert bool((rest == 7.0).all()), "a launch wrote outside its samples"
    with pytest.raises(hip.MfhipError, match="outside"):
        hip.crop_pack_nhwc(src, 6, 6, 8, 5, torch.empty(2, 8, 5, 8, dtype=dtype, device=DEV))
    with pytest.raises(hip.MfhipError, match="outside the buffer"):
        hip.crop_pack_nhwc(src, 0, 0, 8, 8, torch.empty(2, 8, 8, 8, dtype=dtype, device=DEV), 1)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_tiled_decode_and_encode_against_the_reference(prec):
    vae = tiled_vae(prec)
    G = golden("vae_tiling.npz")
    z, img = main_inputs()
    dec = vae.decode(z.to(DEV), return_dict=False)[0]
    assert tuple(dec.shape) == (2, 3, 26, 22)
    check(f"tiled decode[{prec}]", dec, G["decode_tiled"], prec, "decode")
    mom = vae.encode(img.to(DEV)).latent_dist.parameters
    assert tuple(mom.shape) == (2, 8, 13, 11)
    check(f"tiled moments[{prec}]", mom, G["moments_tiled"], prec, "encode")
    assert torch.equal(vae.tiled_decode(z.to(DEV)).sample, dec)
    assert torch.equal(vae.tiled_encode(img.to(DEV)).latent_dist.parameters, mom)
    if prec == "fp32":                  # the tiled path ran: tiling moves the result by ~1 (the untiled golden is kept as fp16)
        assert (dec.cpu() - torch.from_numpy(G["decode_untiled"]).float()).abs().max().item() > 0.1
        assert (mom.cpu() - torch.from_numpy(G["moments_untiled"]).float()).abs().max().item() > 0.1


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_tiling_at_the_threshold_is_todays_path_bit_for_bit(prec):
    vae = tiled_vae(prec)
    g = torch.Generator().manual_seed(5)
    img, z = (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(DEV), torch.randn(2, 4, 8, 8, generator=g).to(DEV)
    on = vae.encode(img).latent_dist.parameters, vae.decode(z, return_dict=False)[0]
    vae.disable_tiling()
    off = vae.encode(img).latent_dist.parameters, vae.decode(z, return_dict=False)[0]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


@pytest.mark.parametrize("prec", PRECS)
def test_sliced_batch_is_the_concatenation_of_single_calls(prec):
    vae = tiled_vae(prec)
    G = golden("vae_tiling.npz")
    z3 = batch3_input().to(DEV)
    singles = torch.cat([vae.decode(z3[i:i + 1], return_dict=False)[0] for i in range(3)])
    vae.enable_slicing()
    sliced = vae.decode(z3, return_dict=False)[0]
    assert torch.equal(sliced, singles)
    check(f"sliced tiled decode[{prec}]", sliced, G["decode3_tiled"], prec, "decode3")
    # untiled: slicing alone, encode and decode
    vae.disable_tiling()
    g = torch.Generator().manual_seed(6)
    img, z = (torch.rand(3, 3, 16, 16, generator=g) * 2 - 1).to(DEV), torch.randn(3, 4, 8, 8, generator=g).to(DEV)
    dec, mom = vae.decode(z, return_dict=False)[0], vae.encode(img).latent_dist.parameters
    vae.disable_slicing()
    assert torch.equal(dec, torch.cat([vae.decode(z[i:i + 1], return_dict=False)[0] for i in range(3)]))
    assert torch.equal(mom, torch.cat([vae.encode(img[i:i + 1]).latent_dist.parameters for i in range(3)]))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_one_tile_per_pass_and_the_grouped_schedule_agree(prec):
    """tile_batch = 1 is the reference's one-tile-at-a-time loop; the default stacks the tiles of a shape.  Both meet the bound."""
    vae = tiled_vae(prec)
    G = golden("vae_tiling.npz")
    z, img = main_inputs()
    for tb in (1, 2, 16):
        vae.tile_batch = tb
        check(f"tiled decode, tile_batch {tb}[{prec}]", vae.decode(z.to(DEV), return_dict=False)[0], G["decode_tiled"], prec, "decode")
        check(f"tiled moments, tile_batch {tb}[{prec}]", vae.encode(img.to(DEV)).latent_dist.parameters, G["moments_tiled"], prec, "encode")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_pipeline_with_vae_tiling_against_the_reference(prec):
    """2 DDIM steps at 32 x 32 pixels with enable_vae_tiling(): the conditioning image is encoded as 3 x 3 tiles, the result decoded as
    3 x 3 tiles."""
    unet, bn, _ = build("tiny", prec)
    vae = tiled_vae(prec)
    vae.disable_tiling()
    G = golden("vae_tiling.npz")
    pipe = StableDiffusionBrushNetPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, brushnet=bn,
                                           scheduler=DDIMScheduler(**SD_SCHED, clip_sample=False), safety_checker=None,
                                           feature_extractor=None, requires_safety_checker=False, depth_conditioning_mode="concat")
    pipe.set_progress_bar_config(disable=True)
    assert pipe.enable_vae_tiling() is None and vae.use_tiling
    inp = synth.pipeline_inputs(1, 32, 32, seed=1234, cross_dim=32, vae_scale=2)
    noise = torch.from_numpy(G["pipe_vae_noise"])
    cond = pipe.build_conditioning(inp["image"], inp["mask"], inp["depth"], 32, 32, 1, 1, True, noise)
    check(f"conditioning with tiling[{prec}]", cond, G["pipe_cond"], prec, "pipeline_cond")
    res = pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"], mask=inp["mask"],
               depth=inp["depth"], num_inference_steps=2, guidance_scale=7.5, latents=inp["latents"].clone(), output_type="pt",
               brushnet_conditioning_scale=1.0, height=32, width=32, conditioning_noise=noise)
    check(f"image with tiling[{prec}]", res.images, G["pipe_image"], prec, "pipeline_image")
