"""Host-side logic of the CLIP text encoders and of both pipelines' encode_prompt (no GPU): parameter tables, the on-disk format,
the pooling rules, the SDXL encode_prompt's structure against the reference's recorded outputs (tools/make_golden_clip.py ->
tests/golden/clip_pipelines.npz), and the argument checks of the new C entry points."""
import ctypes as C
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from reflecting_reality_amd import StableDiffusionXLBrushNetPipeline, hip, synth
from reflecting_reality_amd.configs import CLIP_FIXTURES
from reflecting_reality_amd.text_encoder import CLIPTextModel, CLIPTextModelWithProjection, CLIPTextOutput
from util import GOLD, golden

CONFIGS = {name: ((CLIPTextModelWithProjection if proj else CLIPTextModel), cfg) for name, (cfg, proj) in CLIP_FIXTURES.items()}


def clip_keys(name):
    with open(os.path.join(GOLD, f"keys_clip_{name}.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_parameter_tables_match_transformers(name):
    klass, cfg = CONFIGS[name]
    assert dict(klass(dict(cfg), precision="fp32", device="cpu").param_shapes()) == clip_keys(name)


def test_synth_norm_rule_leaves_existing_keys_alone():
    """synth.fill now treats CLIP's layer_norm* as norms; no key of the existing fixtures carries that name."""
    for fn in os.listdir(GOLD):
        if fn.startswith("keys_") and not fn.startswith("keys_clip_"):
            with open(os.path.join(GOLD, fn)) as f:
                assert "layer_norm" not in f.read(), fn


@pytest.mark.parametrize("name", ["tiny_l", "tiny_g"])
def test_round_trip_on_cpu_and_loud_forward(name, tmp_path):
    from safetensors.torch import load_file, save_file
    klass, cfg = CONFIGS[name]
    m = klass(dict(cfg), precision="fp32", device="cpu")
    sd = synth.state_dict_for(m.param_shapes(), 3)
    m.load_state_dict(sd)
    m.save_pretrained(str(tmp_path / "te"))
    with open(tmp_path / "te" / "config.json") as f:
        saved = json.load(f)
    assert saved["architectures"] == [klass.__name__] and saved["hidden_act"] == cfg["hidden_act"]
    on_disk = load_file(str(tmp_path / "te" / "model.safetensors"))
    assert set(on_disk) == set(sd) and all(torch.equal(on_disk[k], sd[k]) for k in sd)
    m2 = klass.from_pretrained(str(tmp_path), subfolder="te", torch_dtype=torch.float32, device="cpu")
    assert m2.prec.name == "fp32" and m2.dtype == torch.float32 and m2.device == torch.device("cpu")
    assert m2.config.projection_dim == cfg["projection_dim"]
    assert all(torch.equal(m2.state_dict()[k], sd[k]) for k in sd)
    assert next(m2.parameters()).device == torch.device("cpu")
    assert klass.from_pretrained(str(tmp_path / "te"), torch_dtype=torch.float16, device="cpu").prec.name == "fp16"
    # older checkpoints carry the position_ids buffer: tolerated on load, never written; anything else is refused
    save_file({**on_disk, "text_model.embeddings.position_ids": torch.arange(77)[None]}, str(tmp_path / "te" / "model.safetensors"))
    m3 = klass.from_pretrained(str(tmp_path / "te"), torch_dtype=torch.float32, device="cpu")
    assert "text_model.embeddings.position_ids" not in m3.state_dict()
    with pytest.raises(RuntimeError, match="unexpected"):
        m.load_state_dict({**sd, "text_model.extra.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="missing"):
        m.load_state_dict({k: v for k, v in sd.items() if "final_layer_norm" not in k})
    # no CPU path: the forward fails loudly
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        m2(torch.from_numpy(golden(f"clip_{name}.npz")["ids"]))
    with pytest.raises(NotImplementedError):
        m2(torch.zeros(1, 77, dtype=torch.long), attention_mask=torch.ones(1, 77))
    with pytest.raises(ValueError):
        klass(dict(cfg), precision="fp8", device="cpu")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_pooling_rules_on_the_stored_ids(name):
    """eos_token_id == 2: argmax of the ids (legacy rule); else the first position holding eos_token_id — both against the index
    transformers' own pooled row was taken from (recorded by the tool, which asserts it against pooler_output)."""
    klass, cfg = CONFIGS[name]
    G = golden(f"clip_{name}.npz")
    m = klass(dict(cfg), precision="fp32", device="cpu")
    ids = torch.from_numpy(G["ids"])
    assert m._pool_index(ids).tolist() == G["pool_index"].tolist()
    assert len(set(G["pool_index"].tolist())) == 2                       # prompts of different length
    tok = synth.HashTokenizer(cfg["vocab_size"], 77, pad_token_id=None if cfg["eos_token_id"] == 2 else 0)
    if cfg["eos_token_id"] != 2:       # padded with 0 and eos is not the row maximum's first occurrence under the other rule
        assert int(ids[0, -1]) == 0 and int(ids.max()) == tok.eos_token_id == cfg["eos_token_id"]
    else:
        assert int(ids[0, -1]) == tok.eos_token_id


def test_hash_tokenizer_surface():
    tok = synth.HashTokenizer(1000, 77)
    a = tok(["a red chair", "a"], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert a.shape == (2, 77) and a.dtype == torch.int64 and int(a[0, 0]) == 998 and int(a[0, 4]) == 999 and int(a.max()) == 999
    assert torch.equal(a, tok(["a red chair", "a"], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids)
    long = tok(" ".join(["w%d" % i for i in range(100)]), padding="longest", return_tensors="pt").input_ids
    assert long.shape == (1, 102)
    cut = tok(" ".join(["w%d" % i for i in range(100)]), padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert cut.shape == (1, 77) and int(cut[0, -1]) == 999
    assert len(tok.batch_decode(long[:, 76:-1])) == 1
    assert int(synth.HashTokenizer(1000, 77, pad_token_id=0)("a", padding="max_length", return_tensors="pt").input_ids[0, -1]) == 0


# ---- SDXL encode_prompt against the reference's recorded calls ------------------------------------------------------------------
class StubEncoder:
    """Answers with what transformers' module returned for the same ids when the reference pipeline called it."""

    def __init__(self, name, P, projection):
        self.table = {}
        for n in range(int(P["ncalls"])):
            if str(P[f"call{n}/enc"]) == name:
                self.table[tuple(P[f"call{n}/ids"].flatten().tolist())] = n
        self.P, self.projection, self.dtype, self.seen = P, projection, torch.float32, []

    def __call__(self, ids, output_hidden_states=False, **kw):
        assert output_hidden_states and not kw
        n = self.table[tuple(ids.flatten().tolist())]
        self.seen.append(n)
        f = OrderedDict()
        f["text_embeds" if self.projection else "last_hidden_state"] = torch.from_numpy(self.P[f"call{n}/first"])
        if self.projection:
            f["last_hidden_state"] = torch.from_numpy(self.P[f"call{n}/last"])
        else:
            f["pooler_output"] = torch.zeros(ids.shape[0], 32)
        f["hidden_states"] = tuple(torch.from_numpy(self.P[f"call{n}/hs"]))
        return CLIPTextOutput(f)


def stub_xl(P, first=True):
    pipe = StableDiffusionXLBrushNetPipeline.__new__(StableDiffusionXLBrushNetPipeline)
    pipe.config = dict(force_zeros_for_empty_prompt=True)
    pipe.unet = type("U", (), {"device": torch.device("cpu")})()
    pipe.text_encoder = StubEncoder("tiny_l", P, False) if first else None
    pipe.tokenizer = synth.HashTokenizer(1000, 77) if first else None
    pipe.text_encoder_2 = StubEncoder("tiny_g", P, True)
    pipe.tokenizer_2 = synth.HashTokenizer(1000, 77, pad_token_id=0)
    return pipe


NAMES = ("prompt_embeds", "negative_prompt_embeds", "pooled_prompt_embeds", "negative_pooled_prompt_embeds")


@pytest.mark.parametrize("case,kw", [
    ("xl_zeros", dict(prompt=["a mirror reflecting a chair"], prompt_2=["a photo of a room"], negative_prompt=None)),
    ("xl_neg", dict(prompt=["a mirror reflecting a chair"], prompt_2=None, negative_prompt=["blurry"], negative_prompt_2=["low quality"],
                    num_images_per_prompt=2)),
    ("xl_skip1", dict(prompt=["a mirror reflecting a chair"], prompt_2=["a photo of a room"], negative_prompt=None, clip_skip=1)),
    ("xl_only2", dict(prompt=["a mirror reflecting a chair"])),
])
def test_xl_encode_prompt_reproduces_the_reference(case, kw):
    """Which hidden state, the concat order, the pooled vector of encoder 2, the zeros, the per-image repeats: bit for bit the
    reference's outputs when the encoders answer what the reference's encoders answered."""
    P = golden("clip_pipelines.npz")
    pipe = stub_xl(P, first=case != "xl_only2")
    got = pipe.encode_prompt(device=torch.device("cpu"), do_classifier_free_guidance=True, **kw)
    for nm, t in zip(NAMES, got):
        ref = torch.from_numpy(P[f"{case}/{nm}"])
        assert t.dtype == torch.float32 and t.shape == ref.shape, (nm, t.shape, ref.shape)
        assert torch.equal(t, ref), f"{case}/{nm}: max diff {float((t - ref).abs().max()):.3e}"
    if case == "xl_zeros":
        assert float(got[1].abs().max()) == 0.0 and float(got[3].abs().max()) == 0.0
        assert got[0].shape[-1] == 64 and got[2].shape[-1] == 16
    if case == "xl_neg":
        assert got[0].shape[0] == 2 and float(got[1].abs().max()) > 0


def test_xl_encode_prompt_error_texts():
    pipe = stub_xl(golden("clip_pipelines.npz"))
    with pytest.raises(TypeError, match="`negative_prompt` should be the same type to `prompt`"):
        pipe.encode_prompt(["a mirror reflecting a chair"], device=torch.device("cpu"), negative_prompt=("blurry",))
    with pytest.raises(ValueError, match="has batch size 2, but `prompt`"):
        pipe.encode_prompt(["a mirror reflecting a chair"], device=torch.device("cpu"), negative_prompt=["blurry", "low quality"])
    bare = stub_xl(golden("clip_pipelines.npz"))
    bare.text_encoder_2 = bare.tokenizer_2 = None
    bare.text_encoder = None
    with pytest.raises(ValueError, match="text encoders"):
        bare.encode_prompt(["a"], device=torch.device("cpu"))


def test_sd15_recorded_outputs_follow_the_stored_calls():
    """The SD1.5 reference outputs in the fixture are what its encoder returned: [0] for clip_skip None, the final LayerNorm of
    hidden_states[-2] for clip_skip 1 (not recomputable without the GPU, so only the first is checked here)."""
    P = golden("clip_pipelines.npz")
    tok = synth.HashTokenizer(1000, 77)
    ids = tok(["a mirror reflecting a chair"], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    stub = StubEncoder("tiny_l", P, False)
    n = stub.table[tuple(ids.flatten().tolist())]
    assert np.array_equal(P["sd_none/prompt_embeds"], P[f"call{n}/first"])
    assert not np.array_equal(P["sd_skip1/prompt_embeds"], P["sd_none/prompt_embeds"])


# ---- C entry points report argument errors without a GPU -----------------------------------------------------------------------
def test_new_entry_points_report_argument_errors():
    lib = hip.load()
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    p16 = C.c_void_p((p.value + 15) // 16 * 16)
    args16 = lambda sq, skv, d: (p16, C.c_int64(64), p16, C.c_int64(64), p16, C.c_int64(80), p16, C.c_int64(64), 1, 1, sq, skv, d,
                                 C.c_float(0.125), None)
    for fn in (lib.mf_attention_causal_bf16, lib.mf_attention_causal_f16):
        assert fn(*args16(64, 80, 64)) == -1
        assert b"sq == skv" in lib.mf_last_error()
        assert fn(None, *args16(64, 64, 64)[1:]) == -1
        assert b"null pointer" in lib.mf_last_error()
        assert fn(*args16(64, 64, 40)) == -1
        assert b"unsupported head_dim 40" in lib.mf_last_error()
    x3 = lambda sq, skv: (p16, p16, C.c_int64(64), p16, p16, C.c_int64(64), p16, p16, C.c_int64(80), p16, C.c_int64(64), 1, 1, sq, skv, 64,
                          C.c_float(0.125), None)
    assert lib.mf_attention_causal_f16x3(*x3(64, 80)) == -1
    assert b"sq == skv" in lib.mf_last_error()
    assert lib.mf_attention_causal_f16x3(None, *x3(64, 64)[1:]) == -1
    assert b"null pointer" in lib.mf_last_error()
    assert lib.mf_embed_tokens(None, p16, p16, hip.MF_F32, p16, hip.MF_F32, 1, 77, 32, 100, None) == -1
    assert b"null pointer" in lib.mf_last_error()
    assert lib.mf_embed_tokens(p16, p16, p16, hip.MF_F32, p16, hip.MF_F32, 1, 77, 30, 100, None) == -1
    assert b"hidden" in lib.mf_last_error()
    assert lib.mf_embed_tokens(p16, p16, p16, hip.MF_BF16, p16, hip.MF_F16, 1, 77, 32, 100, None) == -1
    assert lib.mf_embed_tokens(p16, C.c_void_p(p16.value + 4), p16, hip.MF_F32, p16, hip.MF_F32, 1, 77, 32, 100, None) == -3
    assert lib.mf_softmax_rows_causal(p16, p16, hip.MF_F32, C.c_int64(77), 77, 80, 64, None) == -1
    assert b"sq == cols" in lib.mf_last_error()
    assert lib.mf_act(p16, p16, hip.MF_F32, hip.ACT_SILU, C.c_int64(64), None) == -1
    assert b"kind" in lib.mf_last_error()
    assert lib.mf_act(p16, p16, hip.MF_F32, hip.ACT_GELU_ERF, C.c_int64(63), None) == -1
    with pytest.raises(ValueError, match="token ids"):
        hip.embed_tokens(torch.tensor([[0, 100]]), torch.zeros(100, 8), torch.zeros(77, 8), torch.float32)
    with pytest.raises(hip.MfhipError):
        hip.act(torch.zeros(8), hip.ACT_QUICK_GELU)


def test_bad_ids_are_rejected_wherever_the_tensor_lives():
    """The model checks its host copy of the ids before any launch, so ids that a pipeline already moved to the device are rejected
    like host ids (mf_embed_tokens alone would clamp them)."""
    klass, cfg = CONFIGS["tiny_l"]
    m = klass(dict(cfg), precision="fp32", device="cpu")
    m.load_state_dict(synth.state_dict_for(m.param_shapes(), 3))
    for bad in (-1, cfg["vocab_size"]):
        ids = torch.zeros(1, 77, dtype=torch.long)
        ids[0, 5] = bad
        with pytest.raises(ValueError, match="token ids"):
            m(ids)
