"""LoRA adapters without a GPU: the three key formats against the names the reference's converters produce
(tests/golden/lora_keys.json), the fixture against the oracle on host-merged weights, and the C entry's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import abi_header
import lora_ref
from oracle import mirrorfusion_ref as R
from reflecting_reality_amd import hip, lora, models as M, synth
from util import GOLD, golden, keys

with open(os.path.join(GOLD, "lora_keys.json")) as f:
    KEYS = json.load(f)
CFG = {"tiny": R.TINY_UNET, "sd15": R.SD15_UNET}


def unet_of(size):
    return M.UNet2DConditionModel(dict(CFG[size]), precision="fp32", device="cpu")


# ---- key readers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["tiny", "sd15"])
def test_every_reference_module_is_capable_and_kohya_names_resolve(size):
    unet, K = unet_of(size), KEYS[size]
    capable = unet.lora_modules()
    assert set(K["modules"]) <= set(capable)
    by_us = {m.replace(".", "_"): m for m in capable}
    assert len(by_us) == len(capable), "two modules collide once their dots are underscores"
    # what the reference's converter made of the kohya names.  Its rewrite rules cut time_embedding_linear_1 / _2 into
    # "time.embedding.linear" (kohya files never target them); matching against the model's own names resolves those too (below)
    emb = ("time_embedding.", "add_embedding.", "time.embedding.", "add.embedding.")
    converted = set()
    for name in K["kohya_converted"]:
        model, style, module, part = lora.parse_key(name)
        assert (model, style) == ("unet", "dotted") and part in ("down", "up"), name
        converted.add(module)
    want = {m for m in K["modules"] if not m.startswith(emb)}
    assert {m for m in converted if not m.startswith(emb)} == want
    assert {m for m in (lora.parse_key(a)[2] for a in K["kohya_alphas"]) if not m.startswith(emb)} == want
    for m, k in K["kohya"].items():
        for tail, part in ((".lora_down.weight", "down"), (".lora_up.weight", "up"), (".alpha", "alpha")):
            model, style, name, got = lora.parse_key(k + tail)
            assert (model, style, got) == ("unet", "kohya", part)
            assert by_us[name] == m


@pytest.mark.parametrize("size", ["tiny", "sd15"])
def test_legacy_attention_processor_names(size):
    K = KEYS[size]
    assert K["legacy"]
    want = set()
    for m, k in K["legacy"].items():
        assert lora.parse_key(k) == ("", "dotted", m, "down")
        assert lora.parse_key("unet." + k.replace(".down.", ".up.")) == ("unet", "dotted", m, "up")
        want.add(m)
    assert {lora.parse_key(k)[2] for k in K["legacy_converted"]} == want


def _one(module, shape, rank=4, fmt="diffusers", alpha=None, prefix="unet."):
    down, up = torch.zeros((rank,) + tuple(shape[1:])), torch.zeros((shape[0], rank) + ((1, 1) if len(shape) == 4 else ()))
    if fmt == "kohya":
        k = ("lora_unet_" if prefix == "unet." else "lora_te_") + module.replace(".", "_")
        sd = {k + ".lora_down.weight": down, k + ".lora_up.weight": up}
        if alpha is not None:
            sd[k + ".alpha"] = torch.tensor(alpha)
        return sd
    sd = {f"{prefix}{module}.lora.down.weight": down, f"{prefix}{module}.lora.up.weight": up}
    if alpha is not None:
        sd[f"{prefix}{module}.alpha"] = alpha
    return sd


def test_alpha_prefix_split_and_shapes():
    unet = unet_of("tiny")
    shapes, capable = unet.param_shapes(), unet.lora_modules()
    q = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q"
    c1 = "down_blocks.0.resnets.0.conv1"
    sd = {**_one(q, shapes[q + ".weight"], rank=4, fmt="kohya", alpha=2.0), **_one(c1, shapes[c1 + ".weight"], rank=3),
          "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_linear_layer.down.weight": torch.zeros(2, 32),
          "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_linear_layer.up.weight": torch.zeros(32, 2)}
    groups = lora.group_keys(sd, {f"unet.{c1}.alpha": 6.0})
    assert len(groups["unet"]) == 2 and len(groups["text_encoder"]) == 1 and not groups[""]
    found = lora.resolve(groups["unet"], shapes, capable)
    assert list(found) == [c1, q]                                 # parameter order
    assert found[q][2] == 2.0 / 4 and found[c1][2] == 6.0 / 3     # alpha / rank
    assert tuple(found[c1][0].shape) == (3, 4 * 0 + shapes[c1 + ".weight"][1] * 9) and tuple(found[c1][1].shape) == (shapes[c1 + ".weight"][0], 3)
    assert lora.resolve(lora.group_keys(_one(q, shapes[q + ".weight"]))["unet"], shapes, capable)[q][2] == 1.0      # no alpha: 1
    assert lora.scale_of(None) is None and lora.scale_of({}) is None and lora.scale_of({"scale": 0.5}) == 0.5
    with pytest.raises(NotImplementedError, match="gligen"):
        lora.scale_of({"scale": 1.0, "gligen": {}})


def test_refusals_name_the_key():
    unet = unet_of("tiny")
    shapes, capable = unet.param_shapes(), unet.lora_modules()
    q = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q"
    res = lambda sd, al=None: lora.resolve(lora.group_keys(sd, al)["unet"], shapes, capable)
    with pytest.raises(ValueError, match="no_such_layer"):
        res(_one("down_blocks.0.no_such_layer", (32, 32)))
    with pytest.raises(ValueError, match="lora_unet_down_blocks_9_x"):
        res({"lora_unet_down_blocks_9_x.lora_down.weight": torch.zeros(4, 32), "lora_unet_down_blocks_9_x.lora_up.weight": torch.zeros(32, 4)})
    bad = _one(q, shapes[q + ".weight"])
    bad[f"unet.{q}.lora.down.weight"] = torch.zeros(4, 31)
    with pytest.raises(ValueError, match="to_q.lora"):
        res(bad)
    bad = _one(q, shapes[q + ".weight"])
    bad[f"unet.{q}.lora.up.weight"] = torch.zeros(32, 5)          # rank 5 against down's 4
    with pytest.raises(ValueError, match="rank 4"):
        res(bad)
    half = _one(q, shapes[q + ".weight"])
    del half[f"unet.{q}.lora.up.weight"]
    with pytest.raises(ValueError, match="both its down and its up"):
        res(half)
    with pytest.raises(ValueError, match="not a LoRA key"):
        lora.parse_key("unet.conv_in.weight")
    with pytest.raises(NotImplementedError, match="SGM"):
        lora.parse_key("lora_unet_input_blocks_4_1_proj_in.lora_down.weight")
    for k in ("lora_te1_text_model_encoder_layers_0_mlp_fc1.alpha", "lora_te2_text_model_encoder_layers_0_mlp_fc1.alpha"):
        with pytest.raises(NotImplementedError, match="lora_te"):
            lora.parse_key(k)


def test_model_refusals_without_a_device():
    bn = M.BrushNetModel(dict(R.brushnet_config(R.TINY_UNET, 6)), precision="fp32", device="cpu")
    with pytest.raises(NotImplementedError, match="BrushNet"):
        bn.load_attn_procs({})
    unet = unet_of("tiny")
    with pytest.raises(RuntimeError, match="master copy"):       # nothing loaded: no base to merge into
        unet.load_attn_procs({})


def test_a_path_is_a_safetensors_file_or_a_directory(tmp_path):
    from safetensors.torch import save_file
    sd = {"unet.a.lora.down.weight": torch.ones(2, 3)}
    save_file(sd, str(tmp_path / lora.WEIGHT_NAME))
    for p in (tmp_path, tmp_path / lora.WEIGHT_NAME):
        assert torch.equal(lora.read_state_dict(p)["unet.a.lora.down.weight"], sd["unet.a.lora.down.weight"])
    with pytest.raises(FileNotFoundError):
        lora.read_state_dict(tmp_path / "missing.safetensors")


# ---- the fixture: alpha / rank, the scale and the conv flattening, pinned without a GPU --------------------------------------------------
def fixture_inputs(G, case):
    x, ehs = torch.from_numpy(G[f"{case}_x"]), torch.from_numpy(G[f"{case}_ehs"])
    added = None
    if f"{case}_text_embeds" in G:
        added = dict(text_embeds=torch.from_numpy(G[f"{case}_text_embeds"]), time_ids=torch.from_numpy(G[f"{case}_time_ids"]))
    return x, ehs, added, int(G[f"{case}_timestep"])


@pytest.mark.parametrize("case,cfg,wseed", [("tiny", R.TINY_UNET, 0), ("tiny_xl", R.TINY_XL_UNET, 20)])
def test_fixture_is_the_oracle_on_host_merged_weights(case, cfg, wseed):
    G = golden("lora_tiny.npz")
    with open(os.path.join(GOLD, "lora_envelope.json")) as f:
        env = json.load(f)
    unet = M.UNet2DConditionModel(dict(cfg), precision="fp32", device="cpu")
    shapes = unet.param_shapes()
    sd = synth.state_dict_for(keys(case)["unet"], wseed)
    asd, alphas = lora_ref.adapter_of(G, case, shapes)
    kinds = {m.split(".")[-1] if not m.endswith("to_out.0") else "to_out.0" for m, _, _ in lora_ref.plan_of(G, case)}
    assert {"to_q", "to_k", "to_v", "to_out.0", "proj", "2", "proj_in", "proj_out", "conv1", "conv2", "conv_shortcut", "time_emb_proj",
            "conv"} <= kinds
    assert {r for _, r, _ in lora_ref.plan_of(G, case)} == {3, 4} and {a is None for _, _, a in lora_ref.plan_of(G, case)} == {True, False}
    x, ehs, added, t = fixture_inputs(G, case)
    base = torch.from_numpy(G[f"{case}_base"])
    delta = float((torch.from_numpy(G[f"{case}_s07"]) - base).abs().max())
    print(f"{case}: max|scale 0.7 - base| = {delta:.4f}, bf16 envelope L-inf {env[f'bf16/{case}/s07']['linf']:.4f}")
    assert delta >= 0.05 and delta >= 20 * env[f"bf16/{case}/s07"]["linf"]            # a no-op merge cannot pass
    for scale, names in ((0.7, ("s07", "fused07")), (1.0, ("s10",))):
        merged = lora_ref.host_merged(sd, shapes, unet.lora_modules(), [(asd, alphas, 1.0)], scale)
        got = R.unet_forward(merged, cfg, x, t, ehs, added=added)
        for n in names:
            ref = torch.from_numpy(G[f"{case}_{n}"])
            err = float((got - ref).abs().max())
            print(f"{case}/{n}: oracle on merged weights vs reference {err:.3e}")
            assert torch.allclose(got, ref, atol=2e-4, rtol=2e-4), (n, err)
        assert float((got - base).abs().max()) >= 0.05
    assert torch.allclose(R.unet_forward(sd, cfg, x, t, ehs, added=added), base, atol=2e-4, rtol=2e-4)


# ---- the C entry --------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_lora_entries():
    protos = abi_header.prototypes()
    for name in ("mf_lora_merge", "mf_lora_tiles", "mf_sizeof_lora_target", "mf_sizeof_lora_term"):
        ret, _, params = hip.SIGNATURES[name].partition(":")
        assert protos[name] == (ret, list(params)), name
    lib = hip.load()
    assert lib.mf_abi_version() == 23
    assert lib.mf_sizeof_lora_target() == ctypes.sizeof(hip.LoraTarget) == 40
    assert lib.mf_sizeof_lora_term() == ctypes.sizeof(hip.LoraTerm) == 24
    assert lib.mf_lora_tiles(32, 256) == 1 and lib.mf_lora_tiles(33, 257) == 4 and lib.mf_lora_tiles(1280, 1280) == 200
    assert lib.mf_lora_tiles(0, 4) == -1 and b"at least 1" in lib.mf_last_error()


def test_argument_errors_return_einval_with_their_text():
    lib = hip.load()
    A, B, U, D, T, C = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000      # never dereferenced: every call below is refused first

    def call(tg, tm, dev=(T, T + 0x1000, C), nt=None):
        tga, tma = (hip.LoraTarget * len(tg))(*tg), (hip.LoraTerm * len(tm))(*tm)
        rc = lib.mf_lora_merge(ctypes.cast(tga, ctypes.c_void_p), ctypes.cast(tma, ctypes.c_void_p), dev[0], dev[1], dev[2], len(tg),
                               len(tm) if nt is None else nt, None)
        return rc, lib.mf_last_error().decode()

    ok_t, ok_m = hip.LoraTarget(A, B, 4, 8, 0, 1, 0), hip.LoraTerm(U, D, 2, 0)
    assert lib.mf_lora_merge(None, None, T, T, C, 1, 1, None) == -1 and b"null host table" in lib.mf_last_error()
    for dev in ((None, T, C), (T, None, C), (T, T, None)):
        rc, msg = call([ok_t], [ok_m], dev)
        assert rc == -1 and "null device table" in msg
    cases = [
        ([hip.LoraTarget(A, A, 4, 8, 0, 1, 0)], [ok_m], "must not alias"),
        ([hip.LoraTarget(A, A + 64, 4, 8, 0, 1, 0)], [ok_m], "must not alias"),          # overlapping ranges
        ([hip.LoraTarget(None, B, 4, 8, 0, 1, 0)], [ok_m], "null base or out"),
        ([hip.LoraTarget(A, None, 4, 8, 0, 1, 0)], [ok_m], "null base or out"),
        ([hip.LoraTarget(A, B, 0, 8, 0, 1, 0)], [ok_m], "must be at least 1"),
        ([hip.LoraTarget(A, B, 4, 0, 0, 1, 0)], [ok_m], "must be at least 1"),
        ([ok_t], [hip.LoraTerm(U, D, 0, 0)], "rank 0"),
        ([ok_t], [hip.LoraTerm(None, D, 2, 0)], "null up or down"),
        ([ok_t], [hip.LoraTerm(U, None, 2, 0)], "null up or down"),
        ([hip.LoraTarget(A, B, 4, 8, 0, 2, 0)], [ok_m], "terms"),                         # runs past the term table
        ([hip.LoraTarget(A, B, 4, 8, 0, 1, 3)], [ok_m], "first_tile"),
        ([ok_t], [ok_m, ok_m], "use 1 of the 2 terms"),
    ]
    for tg, tm, text in cases:
        rc, msg = call(tg, tm)
        assert rc == -1 and text in msg, (text, rc, msg)
    rc, msg = call([], [ok_m])
    assert rc == -1 and "at least 1" in msg
