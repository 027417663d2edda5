"""Tiled / sliced VAE, the part that needs no GPU: the two new entries exist in the cross-compiled library and refuse bad arguments on
the host, vae_tile_plan reproduces the grids the reference ran (tests/golden/vae_tiling.npz, tools/make_golden_vae_tiling.py), the
AutoencoderKL thresholds and switches are the reference's, the pipeline switches forward, and an export with a switch on is refused."""
import json

import numpy as np
import pytest
import torch

import abi_header
from reflecting_reality_amd import (AutoencoderKL, BrushNetModel, DDIMScheduler, StableDiffusionBrushNetPipeline, UNet2DConditionModel, _build,
                                    configs, hip, program)
from reflecting_reality_amd.models import vae_tile_plan
from util import golden

ENTRIES = ("mf_crop_pack_nhwc", "mf_vae_tile_blend")
P = 0x1000          # a non-null, 16-byte aligned address no entry dereferences: every case below is refused on the host, before any launch


def _err(lib):
    return lib.mf_last_error().decode()


def test_new_entries_are_declared_exported_and_the_abi_version_stays():
    lib = hip.load()
    protos = abi_header.prototypes()
    for name in ENTRIES:
        assert name in protos and name in hip.SIGNATURES and name in hip.EXPORTS and hasattr(lib, name), name
    assert lib.mf_abi_version() == hip.ABI_VERSION == 23
    assert "vae_tile.hip" in _build.SOURCES
    for name in ENTRIES:                                   # not part of step programs
        assert name not in program.SIGNATURES and name not in program.SIGNATURES_CALL


def test_vae_tile_plan_reproduces_every_grid_the_reference_ran():
    table = json.loads(str(golden("vae_tiling.npz")["shape_table_json"]))
    assert len(table) >= 6
    seen_untiled = seen_quirk = False
    for row in table:
        mode, H, W, ss = row["mode"], row["H"], row["W"], row["sample_size"]
        vae = AutoencoderKL(dict(configs.TINY_VAE, sample_size=ss), device="cpu")
        vae.enable_tiling()
        tiles_here = vae._tiles_latents(H, W) if mode == "decode" else vae._tiles_pixels(H, W)
        if not tiles_here:                                 # at the threshold: one untiled pass over the whole input
            assert row["tile_shapes"] == [[H, W]] and row["out"] == ([2 * H, 2 * W] if mode == "decode" else [H // 2, W // 2]), row
            seen_untiled = True
            continue
        if mode == "decode":
            plan = vae_tile_plan(H, W, vae.tile_latent_min_size, vae.tile_overlap_factor, 2, 1, vae.tile_sample_min_size)
        else:
            plan = vae_tile_plan(H, W, vae.tile_sample_min_size, vae.tile_overlap_factor, 1, 2, vae.tile_latent_min_size)
        assert [[t["h"], t["w"]] for t in plan["tiles"]] == row["tile_shapes"], row
        assert [plan["out_h"], plan["out_w"]] == row["out"], row
        # the crops tile the output exactly, in raster order
        cover = np.zeros((plan["out_h"], plan["out_w"]), np.int32)
        for t in plan["tiles"]:
            assert t["crop_h"] == min(t["out_h"], plan["row_limit"]) and t["crop_w"] == min(t["out_w"], plan["row_limit"])
            cover[t["oy"]:t["oy"] + t["crop_h"], t["ox"]:t["ox"] + t["crop_w"]] += 1
        assert (cover == 1).all(), row
        if mode == "decode" and (H, W, ss) == (23, 17, 20):
            assert row["out"] == [49, 36] and [2 * H, 2 * W] == [46, 34]        # the sum of the crops, not the scaled input
            seen_quirk = True
    assert seen_untiled and seen_quirk


def test_vae_tile_plan_integers_of_the_main_case():
    d = vae_tile_plan(13, 11, 8, 0.25, 2, 1, 16)
    assert (d["overlap_size"], d["blend_extent"], d["row_limit"]) == (6, 4, 12)
    assert d["rows"] == [(0, 8), (6, 7), (12, 1)] and d["cols"] == [(0, 8), (6, 5)] and (d["out_h"], d["out_w"]) == (26, 22)
    assert [(t["i"], t["j"], t["oy"], t["ox"]) for t in d["tiles"]] == [(0, 0, 0, 0), (0, 1, 0, 12), (1, 0, 12, 0), (1, 1, 12, 12), (2, 0, 24, 0),
                                                                       (2, 1, 24, 12)]
    e = vae_tile_plan(27, 23, 16, 0.25, 1, 2, 8)
    assert (e["overlap_size"], e["blend_extent"], e["row_limit"]) == (12, 2, 6)
    assert e["rows"] == [(0, 16), (12, 15), (24, 3)] and (e["out_h"], e["out_w"]) == (13, 11)
    assert vae_tile_plan(13, 11, 8, 0.25, 2, 1) == d               # out_tile defaults to the scaled tile
    with pytest.raises(ValueError, match="reference fails on such a tile too"):
        vae_tile_plan(25, 23, 16, 0.25, 1, 2, 8)                    # a 1-row encoder tile: not padded, not skipped
    with pytest.raises(ValueError, match="do not advance"):
        vae_tile_plan(8, 8, 1, 0.25, 2, 1)
    with pytest.raises(ValueError, match="positive"):
        vae_tile_plan(0, 8, 8, 0.25, 2, 1)


def test_thresholds_and_switches_are_the_references():
    mk = lambda **kw: AutoencoderKL(dict(configs.TINY_VAE, **kw), device="cpu")
    for kw, sample, latent in ((dict(sample_size=16), 16, 8), (dict(sample_size=20), 20, 10), (dict(sample_size=24), 24, 12),
                               (dict(sample_size=[24, 16]), 24, 12), (dict(sample_size=(16, 24)), 16, 8), (dict(), 32, 16)):
        vae = mk(**kw)
        assert (vae.tile_sample_min_size, vae.tile_latent_min_size, vae.tile_overlap_factor) == (sample, latent, 0.25), kw
        assert vae.use_tiling is False and vae.use_slicing is False
        assert vae.param_shapes() == mk().param_shapes()
    sd = AutoencoderKL(dict(configs.SD15_VAE, sample_size=512), device="cpu")
    assert (sd.tile_sample_min_size, sd.tile_latent_min_size) == (512, 64)
    vae = mk(sample_size=16)
    assert not vae._tiles_pixels(64, 64) and not vae._tiles_latents(64, 64)          # off by default
    vae.enable_tiling()
    assert vae.use_tiling is True
    assert not vae._tiles_pixels(16, 16) and vae._tiles_pixels(16, 17) and vae._tiles_pixels(17, 16)
    assert not vae._tiles_latents(8, 8) and vae._tiles_latents(9, 8) and vae._tiles_latents(8, 9)
    vae.enable_tiling(False)
    assert vae.use_tiling is False and not vae._tiles_pixels(64, 64)
    vae.enable_tiling()
    vae.disable_tiling()
    assert vae.use_tiling is False
    vae.enable_slicing()
    assert vae.use_slicing is True
    vae.disable_slicing()
    assert vae.use_slicing is False
    assert isinstance(vae.tile_batch, int) and vae.tile_batch >= 1
    for name in ("tiled_encode", "tiled_decode"):
        assert callable(getattr(vae, name))


def _crop(lib, **kw):
    g = lambda k, d: kw.get(k, d)
    return lib.mf_crop_pack_nhwc(g("src", P), g("b", 2), g("c", 4), g("h", 13), g("w", 11), g("y0", 6), g("x0", 6), g("th", 7), g("tw", 5),
                                 g("dst", P), g("dtype", hip.MF_BF16), g("c_pad", 8), g("dst_batch", 6), g("offset", 2), None)


def test_crop_pack_refuses_bad_arguments_without_a_gpu():
    lib = hip.load()
    cases = [(dict(src=None), "null"), (dict(dst=None), "null"),
             (dict(b=0), "positive"), (dict(c=0), "positive"), (dict(h=0), "positive"), (dict(w=-1), "positive"), (dict(th=0), "positive"),
             (dict(tw=0), "positive"),
             (dict(y0=-1), "outside"), (dict(x0=-1), "outside"), (dict(y0=7), "outside"), (dict(x0=7), "outside"), (dict(th=8), "outside"),
             (dict(tw=6), "outside"),
             (dict(dtype=hip.MF_FP8), "dst_dtype"), (dict(c_pad=3), "c_pad 3 < c"),
             (dict(dst_batch=0), "outside the buffer"), (dict(offset=-1), "outside the buffer"), (dict(offset=5), "outside the buffer")]
    for kw, word in cases:
        assert _crop(lib, **kw) != 0, kw
        assert word in _err(lib), (kw, _err(lib))


def _blend(lib, **kw):
    g = lambda k, d: kw.get(k, d)
    return lib.mf_vae_tile_blend(g("tile", P), g("above", P), g("left", P), g("b", 2), g("th", 14), g("tw", 10), g("ah", 16), g("aw", 10),
                                 g("lh", 14), g("lw", 16), g("ld", 8), g("c", 3), g("extent", 4), g("limit", 12), g("out", P), g("nhwc", 0),
                                 g("oh", 26), g("ow", 22), g("oy", 12), g("ox", 12), None)


def test_tile_blend_refuses_bad_arguments_without_a_gpu():
    lib = hip.load()
    cases = [(dict(tile=None), "null tile or output"), (dict(out=None), "null tile or output"),
             (dict(b=0), "positive"), (dict(th=0), "positive"), (dict(tw=-3), "positive"), (dict(c=0), "positive"), (dict(oh=0), "positive"),
             (dict(ow=0), "positive"),
             (dict(ld=2, c=3), "ld 2 < c"), (dict(ld=6), "multiple of 4"), (dict(ld=9, c=8), "multiple of 4"),
             (dict(extent=-1), "blend_extent"), (dict(limit=0), "row_limit"), (dict(nhwc=2), "out_nhwc"),
             (dict(aw=9), "widths differ"), (dict(ah=0), "widths differ"), (dict(lh=13), "heights differ"), (dict(lw=0), "heights differ"),
             (dict(oy=-1), "outside"), (dict(ox=-1), "outside"), (dict(oy=15), "outside"), (dict(ox=13), "outside"),
             (dict(oh=23), "outside"), (dict(ow=21), "outside"), (dict(limit=16, oy=13), "outside"),
             (dict(tile=P + 4), "aligned"), (dict(above=P + 8), "aligned"), (dict(left=P + 4), "aligned"), (dict(nhwc=1, out=P + 4), "aligned")]
    for kw, word in cases:
        assert _blend(lib, **kw) != 0, kw
        assert word in _err(lib), (kw, _err(lib))
    # a missing neighbour is the first row / column: its sizes are not looked at (refused only later, for what IS wrong)
    assert _blend(lib, above=None, ah=0, aw=0, tile=None) != 0 and "null tile" in _err(lib)


def test_wrappers_refuse_host_tensors_and_recording():
    z = torch.zeros
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        hip.crop_pack_nhwc(z(1, 4, 8, 8), 0, 0, 4, 4, z(1, 4, 4, 8))
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        hip.vae_tile_blend(z(1, 4, 4, 8), None, None, 2, 3, 3, z(1, 3, 4, 4), 0, 0, nhwc=False)
    hip._RECORDER = object()
    try:
        with pytest.raises(hip.MfhipError, match="not part of step programs"):
            hip.crop_pack_nhwc(z(1, 4, 8, 8), 0, 0, 4, 4, z(1, 4, 4, 8))
        with pytest.raises(hip.MfhipError, match="not part of step programs"):
            hip.vae_tile_blend(z(1, 4, 4, 8), None, None, 2, 3, 3, z(1, 3, 4, 4), 0, 0, nhwc=False)
    finally:
        hip._RECORDER = None


def _pipe(vae):
    mk = lambda cls, cfg: cls(dict(cfg), device="cpu")
    return StableDiffusionBrushNetPipeline(
        vae=vae, text_encoder=None, tokenizer=None, unet=mk(UNet2DConditionModel, configs.TINY_UNET),
        brushnet=mk(BrushNetModel, configs.brushnet_config(configs.TINY_UNET, 6)),
        scheduler=DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False),
        safety_checker=None, feature_extractor=None, requires_safety_checker=False, depth_conditioning_mode="concat")


def test_pipeline_switches_forward_to_the_vae_and_return_none():
    vae = AutoencoderKL(dict(configs.TINY_VAE, sample_size=16), device="cpu")
    pipe = _pipe(vae)
    assert pipe.enable_vae_tiling() is None and vae.use_tiling is True
    assert pipe.disable_vae_tiling() is None and vae.use_tiling is False
    assert pipe.enable_vae_slicing() is None and vae.use_slicing is True
    assert pipe.disable_vae_slicing() is None and vae.use_slicing is False

    class Stub:                                            # a VAE without the switches (host tests build such pipelines)
        config = vae.config
    pipe.vae = Stub()
    for name in ("enable_vae_tiling", "disable_vae_tiling", "enable_vae_slicing", "disable_vae_slicing"):
        assert getattr(pipe, name)() is None


def test_export_with_a_switch_on_is_refused_before_anything_runs(tmp_path):
    vae = AutoencoderKL(dict(configs.TINY_VAE, sample_size=16), device="cpu")
    z, img = torch.zeros(1, 4, 16, 16), torch.zeros(1, 3, 32, 32)
    vae.enable_tiling()
    with pytest.raises(NotImplementedError, match="tiling"):
        program.export_vae_decode(vae, str(tmp_path / "d.mfprog"), z)
    with pytest.raises(NotImplementedError, match="tiling"):
        program.export_vae_decode(vae, str(tmp_path / "d.mfprog"), z, postprocess=True)
    with pytest.raises(NotImplementedError, match="tiling"):
        program.export_vae_encode(vae, str(tmp_path / "e.mfprog"), img)
    pipe = _pipe(vae)
    u8 = torch.zeros(1, 32, 32, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="tiling"):
        pipe.export_call(str(tmp_path / "call"), prompt="a mirror", image=u8, mask=u8, conditioning_noise=torch.zeros(1, 4, 16, 16))
    vae.disable_tiling()
    vae.enable_slicing()
    with pytest.raises(NotImplementedError, match="slicing"):
        program.export_vae_decode(vae, str(tmp_path / "d.mfprog"), torch.zeros(2, 4, 8, 8))
    with pytest.raises(NotImplementedError, match="slicing"):
        program.export_vae_encode(vae, str(tmp_path / "e.mfprog"), torch.zeros(2, 3, 16, 16))
    with pytest.raises(NotImplementedError, match="slicing"):
        pipe.export_call(str(tmp_path / "call"), prompt=["a", "b"], image=torch.zeros(2, 16, 16, 3, dtype=torch.uint8),
                         mask=torch.zeros(2, 16, 16, 3, dtype=torch.uint8), conditioning_noise=torch.zeros(2, 4, 8, 8))
    assert not list(tmp_path.iterdir())                    # no partial export
    # where the switch would not apply, the refusal does not fire (the export then fails later, for want of a device)
    vae.disable_slicing()
    vae.enable_tiling()
    vae.refuse_export("export_vae_decode", 1, 8, 8, latents=True)
    vae.refuse_export("export_vae_encode", 1, 16, 16, latents=False)
    vae.enable_slicing()
    vae.refuse_export("export_vae_decode", 1, 8, 8, latents=True)
