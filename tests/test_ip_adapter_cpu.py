"""Host side of the 'ip_adapter' normals mode, no GPU: the ABI 23 symbols in the cross-compiled library, the mapping of an
ip-adapter.bin's "<i>." keys through the reference's attn_processors order (tests/golden/keys_ip_adapter_tiny.json, recorded from the
reference by tools/make_golden_ip.py), and what set_attn_processor accepts and refuses with IP processor dicts."""
import json
import os

import pytest
import torch

from reflecting_reality_amd import MfhipAttnProcessor, MfhipIPAttnProcessor, configs, hip, synth
from reflecting_reality_amd.models import BrushNetModel, UNet2DConditionModel
from reflecting_reality_amd.pipeline import StableDiffusionBrushNetPipeline, StableDiffusionXLBrushNetPipeline
from util import GOLD, golden, keys

with open(os.path.join(GOLD, "keys_ip_adapter_tiny.json")) as _f:
    KEYS = json.load(_f)


def tiny_unet(cfg=configs.TINY_UNET, size="tiny"):
    unet = UNet2DConditionModel(dict(cfg), precision="fp32", device="cpu")
    unet.load_state_dict(synth.state_dict_for(keys(size)["unet"], 0))
    return unet


def checkpoint():
    G = golden("ip_adapter_tiny.npz")
    return {"image_proj": {k[len("proj/"):]: torch.from_numpy(G[k]) for k in G.files if k.startswith("proj/")},
            "ip_adapter": {k[len("ipw/"):]: torch.from_numpy(G[k]) for k in G.files if k.startswith("ipw/")}}


def ip_dict(unet, **kw):
    cross = unet.config["cross_attention_dim"]
    return {n: MfhipAttnProcessor() if ".attn1." in n else MfhipIPAttnProcessor(unet.P[n[: -len("processor")] + "to_q"].n, cross, **kw)
            for n in unet.attn_processors}


def test_abi_23_symbols():
    lib = hip.load()
    assert hip.ABI_VERSION == 23 and lib.mf_abi_version() == 23
    for name in ("mf_attention_ip_bf16", "mf_attention_ip_f16", "mf_attention_ip_f16x3", "mf_freq_encode", "mf_masked_mean_normal"):
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    assert hip.SIGNATURES["mf_attention_ip_bf16"] == hip.SIGNATURES["mf_attention_ip_f16"] == "i:plplplplplpliiiiiiffp"
    # not replayable: a step program cannot hold them (tests/test_program_cpu.py pins the thunk table)
    from reflecting_reality_amd import program
    assert not any(n.startswith("mf_attention_ip") for n in program._REPLAYABLE)


def test_processor_order_is_the_references():
    unet = tiny_unet()
    assert list(unet.attn_processors) == KEYS["attn_processors"]          # down blocks, then up blocks, then the mid block
    assert [i for i, n in enumerate(unet.attn_processors) if ".attn2." in n] == sorted({int(k.split(".")[0]) for k in KEYS["ip_adapter"]})


def test_load_ip_adapter_maps_indices_and_round_trips(tmp_path):
    unet = tiny_unet()
    ck = checkpoint()
    assert {k: list(v.shape) for k, v in ck["ip_adapter"].items()} == KEYS["ip_adapter"]
    image_proj = unet.load_ip_adapter(ck)
    assert {k: list(v.shape) for k, v in image_proj.items()} == KEYS["image_proj"]
    procs = unet.attn_processors
    for i, n in enumerate(KEYS["attn_processors"]):
        if ".attn2." in n:
            assert isinstance(procs[n], MfhipIPAttnProcessor) and procs[n].num_tokens == 4 and procs[n].scale == 1.0
            assert torch.equal(procs[n].to_k_ip.weight, ck["ip_adapter"][f"{i}.to_k_ip.weight"])
            assert torch.equal(procs[n].to_v_ip.weight, ck["ip_adapter"][f"{i}.to_v_ip.weight"])
        else:
            assert type(procs[n]) is MfhipAttnProcessor
    back = unet.ip_adapter_state_dict()
    assert list(back) == list(ck["ip_adapter"]) and all(torch.equal(back[k], ck["ip_adapter"][k]) for k in back)
    # the reference's file: torch.save({"image_proj": ..., "ip_adapter": ...})
    path = str(tmp_path / "ip-adapter.bin")
    torch.save({"image_proj": image_proj, "ip_adapter": back}, path)
    other = tiny_unet()
    other.load_ip_adapter(path, scale=0.5, num_tokens=1)
    again = other.ip_adapter_state_dict()
    assert all(torch.equal(again[k], back[k]) for k in back)
    assert all(p.scale == 0.5 and p.num_tokens == 1 for p in other.attn_processors.values() if isinstance(p, MfhipIPAttnProcessor))
    # a key of another model's layer table is refused
    bad = dict(ck["ip_adapter"])
    bad["13.to_k_ip.weight"] = bad.pop("1.to_k_ip.weight")
    with pytest.raises(ValueError, match="do not match"):
        tiny_unet().load_ip_adapter({"image_proj": ck["image_proj"], "ip_adapter": bad})


def test_set_attn_processor_with_ip_dicts():
    unet = tiny_unet()
    good = ip_dict(unet)
    unet.set_attn_processor(good)
    assert all(unet.attn_processors[n] is p for n, p in good.items() if isinstance(p, MfhipIPAttnProcessor))
    unet.set_attn_processor(MfhipAttnProcessor())                          # back to the plain processors
    assert not any(isinstance(p, MfhipIPAttnProcessor) for p in unet.attn_processors.values())
    with pytest.raises(NotImplementedError):                               # one IP processor for every layer: attn1 has no ip tokens
        unet.set_attn_processor(MfhipIPAttnProcessor(32, 32))
    mixed = ip_dict(unet)
    first2 = next(n for n in mixed if ".attn2." in n)
    mixed[first2] = MfhipAttnProcessor()
    with pytest.raises(NotImplementedError, match="every attn2"):
        unet.set_attn_processor(mixed)
    on1 = ip_dict(unet)
    first1 = next(n for n in on1 if ".attn1." in n)
    on1[first1] = MfhipIPAttnProcessor(32, 32)
    with pytest.raises(NotImplementedError, match="self-attention"):
        unet.set_attn_processor(on1)
    renamed = ip_dict(unet)
    renamed["x." + first2] = renamed.pop(first2)
    with pytest.raises(ValueError, match="exactly the keys"):
        unet.set_attn_processor(renamed)
    wrong = ip_dict(unet)
    wrong[first2] = MfhipIPAttnProcessor(48, 32)
    with pytest.raises(ValueError, match="to_k_ip"):
        unet.set_attn_processor(wrong)
    with pytest.raises(ValueError, match="num_tokens"):
        MfhipIPAttnProcessor(32, 32, num_tokens=65)
    with pytest.raises(ValueError, match="number of processors"):
        unet.set_attn_processor({first2: MfhipIPAttnProcessor(32, 32)})
    with pytest.raises(NotImplementedError):
        unet.set_attn_processor(object())


def test_ip_processors_are_refused_off_the_sd15_unet():
    xl = tiny_unet(configs.TINY_XL_UNET, "tiny_xl")
    with pytest.raises(NotImplementedError, match="SD1.5"):
        xl.set_attn_processor(ip_dict(xl))
    bn = BrushNetModel(dict(configs.brushnet_config(configs.TINY_UNET, 6)), precision="fp32", device="cpu")
    bn.load_state_dict(synth.state_dict_for(keys("tiny")["brushnet"], 1))
    if bn.attn_processors:
        with pytest.raises(NotImplementedError):
            bn.set_attn_processor({n: MfhipIPAttnProcessor(32, 32) for n in bn.attn_processors})


def test_pipeline_mode_surface():
    kw = dict(vae=type("V", (), {"config": type("C", (), {"block_out_channels": (32, 64)})()})(), text_encoder=None, tokenizer=None,
              unet=None, brushnet=None, scheduler=None, safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe = StableDiffusionBrushNetPipeline(**kw, normals_conditioning_mode="ip_adapter")
    assert pipe.normals_conditioning_mode == "ip_adapter" and pipe.normal_embedder is None
    with pytest.raises(ValueError, match="depth_conditioning_mode"):
        StableDiffusionBrushNetPipeline(**kw, depth_conditioning_mode="ip_adapter")
    with pytest.raises(TypeError):                 # the XL pipeline has no normals modes at all
        StableDiffusionXLBrushNetPipeline(vae=kw["vae"], text_encoder=None, text_encoder_2=None, tokenizer=None, tokenizer_2=None, unet=None,
                                          brushnet=None, scheduler=None, normals_conditioning_mode="ip_adapter")


def test_normal_token_follows_its_prompt_with_several_images_per_prompt():
    """pe is [negative | positive], each half prompt-major (p0, p0, p1, p1): the token of prompt i lands on the rows of prompt i."""
    kw = dict(vae=type("V", (), {"config": type("C", (), {"block_out_channels": (32, 64)})()})(), text_encoder=None, tokenizer=None,
              unet=None, brushnet=None, scheduler=None, safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe = StableDiffusionBrushNetPipeline(**kw, normals_conditioning_mode="ip_adapter")
    pe = torch.randn(8, 77, 4)
    t = torch.arange(2.0).view(2, 1, 1).expand(2, 1, 4).contiguous()
    out = pipe._append_normal_token(pe, 2, 2, True, None, [t])
    assert out.shape == (8, 78, 4) and torch.equal(out[:, :77], pe) and out[:, 77, 0].tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    out = pipe._append_normal_token(pe, 2, 2, True, None, [torch.cat([t, t + 10])])        # get_normal_embeds' [uncond | cond] stack
    assert out[:, 77, 0].tolist() == [0, 0, 1, 1, 10, 10, 11, 11]
    assert pipe._append_normal_token(pe[:4], 2, 2, False, None, t)[:, 77, 0].tolist() == [0, 0, 1, 1]
    for bad in (torch.zeros(3, 1, 4), torch.zeros(8, 1, 4), torch.zeros(2, 2, 4), torch.zeros(2, 1, 5)):
        with pytest.raises(ValueError):
            pipe._append_normal_token(pe, 2, 2, True, None, [bad])
    with pytest.raises(ValueError, match="normal_embedder"):
        pipe._append_normal_token(pe, 2, 2, True, torch.zeros(2, 1, 3), None)
