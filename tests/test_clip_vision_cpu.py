"""Host-side logic of the CLIP vision tower, the image preprocessing and CLIP_Similarity (no GPU): parameter tables, the on-disk format,
the integer resize tables of frontend.clip_preprocess against PIL's stored outputs (tools/make_golden_clip_vision.py ->
tests/golden/clip_preprocess.npz), the argument checks of the new C entry points, MetricsCalculator's dispatch and the score's finishing rule."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import clip_score_ref as S
from reflecting_reality_amd import frontend, hip, metrics, synth
from reflecting_reality_amd.configs import CLIP_VISION_FIXTURES, TINY_CLIP
from reflecting_reality_amd.image_encoder import CLIPModel, CLIPVisionModel, CLIPVisionModelWithProjection
from util import GOLD, golden


def clip_keys(name):
    with open(os.path.join(GOLD, f"keys_clip_{name}.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


@pytest.mark.parametrize("name", list(CLIP_VISION_FIXTURES))
def test_parameter_tables_match_transformers(name):
    m = CLIPVisionModelWithProjection(dict(CLIP_VISION_FIXTURES[name]), precision="fp32", device="cpu")
    assert dict(m.param_shapes()) == clip_keys(name)
    plain = dict(CLIPVisionModel(dict(CLIP_VISION_FIXTURES[name]), precision="fp32", device="cpu").param_shapes())
    assert plain == {k: v for k, v in clip_keys(name).items() if k != "visual_projection.weight"}


def test_clip_model_parameter_table():
    m = CLIPModel(dict(TINY_CLIP), precision="fp32", device="cpu")
    assert dict(m.param_shapes()) == clip_keys("tiny_clip")
    assert m.param_shapes()["logit_scale"] == () and m.param_shapes()["text_projection.weight"] == (16, 32)


def test_synth_treats_the_vision_norms_as_norms():
    for key in ("vision_model.pre_layrnorm.weight", "vision_model.post_layernorm.weight"):
        assert abs(float(synth.fill(key, (64,), 1).mean()) - 1.0) < 0.1
    assert abs(float(synth.fill("vision_model.embeddings.class_embedding", (64,), 1).mean())) < 0.05


@pytest.mark.parametrize("klass,cfg", [(CLIPVisionModel, CLIP_VISION_FIXTURES["tiny_vit_a"]), (CLIPVisionModelWithProjection, CLIP_VISION_FIXTURES["tiny_vit_b"]),
                                       (CLIPModel, TINY_CLIP)])
def test_round_trip_on_cpu_and_loud_forward(klass, cfg, tmp_path):
    from safetensors.torch import load_file, save_file
    m = klass(dict(cfg), precision="fp32", device="cpu")
    sd = synth.state_dict_for(m.param_shapes(), 3)
    m.load_state_dict(sd)
    m.save_pretrained(str(tmp_path / "clip"))
    with open(tmp_path / "clip" / "config.json") as f:
        saved = json.load(f)
    assert saved["architectures"] == [klass.__name__]
    on_disk = load_file(str(tmp_path / "clip" / "model.safetensors"))
    assert set(on_disk) == set(sd) and all(torch.equal(on_disk[k], sd[k]) for k in sd)
    m2 = klass.from_pretrained(str(tmp_path), subfolder="clip", torch_dtype=torch.float32, device="cpu")
    assert m2.prec.name == "fp32" and m2.device == torch.device("cpu") and dict(m2.param_shapes()) == dict(m.param_shapes())
    assert all(torch.equal(m2.state_dict()[k], sd[k]) for k in sd)
    assert next(m2.parameters()).device == torch.device("cpu")
    assert klass.from_pretrained(str(tmp_path / "clip"), torch_dtype=torch.float16, device="cpu").prec.name == "fp16"
    save_file({**on_disk, "vision_model.embeddings.position_ids": torch.arange(17)[None]}, str(tmp_path / "clip" / "model.safetensors"))
    m3 = klass.from_pretrained(str(tmp_path / "clip"), torch_dtype=torch.float32, device="cpu")
    assert "vision_model.embeddings.position_ids" not in m3.state_dict()
    with pytest.raises(RuntimeError, match="unexpected"):
        m.load_state_dict({**sd, "vision_model.extra.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="missing"):
        m.load_state_dict({k: v for k, v in sd.items() if "pre_layrnorm" not in k})
    with pytest.raises(hip.MfhipError):
        m2.train()
    with pytest.raises(ValueError):
        klass(dict(cfg), precision="fp8", device="cpu")
    vis = m2.vision if klass is CLIPModel else m2
    r = vis.config["image_size"]
    with pytest.raises(hip.MfhipError, match="no CPU path"):          # no CPU path: the forward fails loudly
        vis(torch.zeros(1, 3, r, r))
    with pytest.raises(NotImplementedError, match="interpolate_pos_encoding"):
        vis(torch.zeros(1, 3, r + 8, r + 8))
    with pytest.raises(NotImplementedError, match="interpolate_pos_encoding"):
        vis(torch.zeros(1, 3, r, r), interpolate_pos_encoding=True)
    with pytest.raises(NotImplementedError, match="attention_mask"):
        vis(torch.zeros(1, 3, r, r), attention_mask=torch.ones(1, 17))


def test_refused_configurations():
    base = CLIP_VISION_FIXTURES["tiny_vit_a"]
    with pytest.raises(NotImplementedError, match="head dims"):
        CLIPVisionModel(dict(base, hidden_size=48, num_attention_heads=4), device="cpu")          # head dim 12
    with pytest.raises(NotImplementedError, match="hidden_act"):
        CLIPVisionModel(dict(base, hidden_act="relu"), device="cpu")
    with pytest.raises(NotImplementedError, match="whole patches"):
        CLIPVisionModel(dict(base, image_size=30), device="cpu")


# ---- the host tables of the integer resize ------------------------------------------------------------------------------------------------
def resize_pass(a, table, axis):
    """One pass of PIL's 8-bit resize along `axis`, in numpy integers, driven by a (bounds, coefficients) table."""
    if table is None:
        return a
    bounds, k = table
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.uint8)
    for i, (x0, n) in enumerate(bounds):
        acc = (1 << 21) + np.tensordot(k[i, :n].astype(np.int64), a[x0:x0 + n], 1)
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def test_host_tables_reproduce_pil_bit_for_bit():
    G = golden("clip_preprocess.npz")
    cases = G["cases"].tolist()
    assert cases == [[80, 56, 32], [40, 100, 32], [20, 24, 32], [32, 32, 32], [64, 64, 28], [57, 91, 56]]
    for n, (h, w, size) in enumerate(cases):
        img = G[f"case{n}_in"]
        assert img.shape == (h, w, 3) and img.dtype == np.uint8
        (h1, w1), (top, left) = frontend.clip_resize_geometry(h, w, size, size)
        assert (h1, w1) == G[f"case{n}_resized"].shape[:2] and [top, left] == G[f"case{n}_offsets"].tolist()
        tabs = [None if a == b else frontend.clip_resize_table(a, b) for a, b in ((w, w1), (h, h1))]
        for t in tabs:
            if t is not None:
                assert t[0].dtype == np.int32 and t[1].dtype == np.int32 and int((t[0][:, 0] + t[0][:, 1]).max()) <= max(h, w)
        got = resize_pass(resize_pass(img, tabs[0], 1), tabs[1], 0)          # horizontal first, then vertical, uint8 in between
        assert np.array_equal(got, G[f"case{n}_resized"]), f"case {n}"
        assert np.array_equal(got[top:top + size, left:left + size], G[f"case{n}_crop"])
    assert frontend.clip_resize_geometry(80, 56, 32, 32) == ((45, 32), (6, 0))               # the odd offset: (45 - 32) // 2
    assert frontend.clip_resize_geometry(32, 32, 32, 32) == ((32, 32), (0, 0))
    b, k = frontend.clip_resize_table(20, 32)                                                 # upscale: the filter scale stays 1, 5 taps
    assert k.shape == (32, 5)


# ---- the C entries without a device -------------------------------------------------------------------------------------------------------
NEW = ("mf_clip_preprocess", "mf_clip_preprocess_ws_bytes", "mf_clip_vision_embed", "mf_clip_score")


def test_new_entries_exist_and_the_abi_version_stays():
    lib = hip.load()
    for name in NEW:
        assert name in hip.SIGNATURES and hasattr(lib, name)
    assert "clip_vision.hip" in __import__("reflecting_reality_amd._build", fromlist=["SOURCES"]).SOURCES
    assert lib.mf_abi_version() == hip.ABI_VERSION           # additive entries only


def test_new_entry_points_report_argument_errors():
    lib = hip.load()
    buf = (C.c_char * 8192)()
    p16 = (C.cast(buf, C.c_void_p).value + 15) // 16 * 16
    f = C.c_float
    ok = dict(img=p16, batch=1, h=80, w=56, c=3, size=32, crop=32, patch=8, htab=p16 + 64, hk=11, vtab=p16 + 128, vk=11, out=p16 + 256, dt=hip.MF_F32,
              k8=192, u8=None, ws=p16 + 512)

    def pre(**kw):
        v = {**ok, **kw}
        return lib.mf_clip_preprocess(v["img"], v["batch"], v["h"], v["w"], v["c"], v["size"], v["crop"], v["patch"], v["htab"], v["hk"], v["vtab"],
                                      v["vk"], f(0.5), f(0.5), f(0.5), f(0.25), f(0.25), f(0.25), v["out"], v["dt"], v["k8"], v["u8"], v["ws"], None)
    for kw, what in ((dict(img=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                     (dict(patch=7), b"not a multiple of the patch size 7"), (dict(c=4), b"4 channels"), (dict(c=1), b"1 channels"),
                     (dict(k8=188), b"K8 = 188"), (dict(k8=200), b"K8 = 200"), (dict(crop=40), b"crop <= size"), (dict(batch=0), b"batch 0"),
                     (dict(htab=None), b"horizontal"), (dict(h=32, w=32), b"is skipped"), (dict(dt=7), b"fp32, bf16 or fp16")):
        assert pre(**kw) == -1, kw
        assert what in lib.mf_last_error(), (kw, lib.mf_last_error())
    assert pre(out=p16 + 260) == -3 and b"16-byte aligned" in lib.mf_last_error()             # a misaligned output
    assert pre(ws=p16 + 520) == -3
    assert lib.mf_clip_preprocess_ws_bytes(1, 80, 56, 32, 40) == -1 and lib.mf_clip_preprocess_ws_bytes(0, 80, 56, 32, 32) == -1
    one, three = lib.mf_clip_preprocess_ws_bytes(1, 80, 56, 32, 32), lib.mf_clip_preprocess_ws_bytes(3, 80, 56, 32, 32)
    assert one >= 80 * 32 * 3 and three >= 3 * 80 * 32 * 3 and one % 16 == 0 and three % 16 == 0
    assert 0 < lib.mf_clip_preprocess_ws_bytes(1, 32, 32, 32, 32) <= 32                        # both passes skipped: nothing in between
    with pytest.raises(C.ArgumentError):          # the mean is a float, the height an int32_t
        lib.mf_clip_preprocess(p16, 1, 80.0, 56, 3, 32, 32, 8, p16, 11, p16, 11, f(0), f(0), f(0), f(1), f(1), f(1), p16, 0, 192, None, p16, None)

    emb = lambda **kw: lib.mf_clip_vision_embed(*[{**dict(p=p16, cls=p16, pos=p16, idt=hip.MF_F32, out=p16, odt=hip.MF_F32, b=1, s=17, h=32), **kw}[k]
                                                  for k in ("p", "cls", "pos", "idt", "out", "odt", "b", "s", "h")], None)
    for kw, what in ((dict(p=None), b"null pointer"), (dict(cls=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(h=30), b"hidden"),
                     (dict(s=1), b"tokens"), (dict(idt=hip.MF_BF16, odt=hip.MF_F16), b"fp16 and bf16")):
        assert emb(**kw) == -1, kw
        assert what in lib.mf_last_error(), (kw, lib.mf_last_error())
    assert emb(pos=p16 + 4) == -3 and emb(out=p16 + 8) == -3

    assert lib.mf_clip_score(None, p16, 1, 16, p16, p16, None) == -1 and b"null pointer" in lib.mf_last_error()
    assert lib.mf_clip_score(p16, p16, 1, 16, p16, None, None) == -1 and b"norms_out" in lib.mf_last_error()
    assert lib.mf_clip_score(p16, p16, 0, 16, p16, p16, None) == -1 and lib.mf_clip_score(p16, p16, 1, 0, p16, p16, None) == -1
    assert lib.mf_clip_score(p16 + 2, p16, 1, 16, p16, p16, None) == -3
    with pytest.raises(hip.MfhipError):
        hip.clip_score(torch.zeros(2, 16), torch.zeros(2, 16))                                 # host tensors
    with pytest.raises(ValueError, match="RGB"):
        frontend.clip_preprocess(np.zeros((16, 16, 4), np.uint8), 32, 32, patch=8, device="cpu")
    with pytest.raises(ValueError, match="multiple of the patch"):
        frontend.clip_preprocess(np.zeros((16, 16, 3), np.uint8), 32, 30, patch=8, device="cpu")


# ---- MetricsCalculator and the finishing rule -------------------------------------------------------------------------------------------
def tiny_clip_cpu():
    m = CLIPModel(dict(TINY_CLIP), precision="fp32", device="cpu")
    m.load_state_dict(synth.state_dict_for(m.param_shapes(), int(golden("clip_tiny_clip.npz")["seed"])))
    return m, synth.HashTokenizer(1000, 77)


def test_metrics_calculator_takes_clip_similarity_with_a_model():
    model, tok = tiny_clip_cpu()
    calc = metrics.MetricsCalculator(["PSNR", "CLIP_Similarity"], "cpu", clip_model=model, clip_tokenizer=tok)
    assert calc.metrics_to_compute == ["PSNR", "CLIP_Similarity"] and calc.clip_model is model
    for name in ("Aesthetic_Score", "LPIPS", "Image_Reward", "HPS_V2.1", "IoU"):          # still refused, model or not
        with pytest.raises(NotImplementedError, match=r"metrics\.py:\d+"):
            metrics.MetricsCalculator(["PSNR", name], "cpu", clip_model=model, clip_tokenizer=tok)
        with pytest.raises(NotImplementedError):
            calc.compute_metric(name, None, {}, "a cat")
    with pytest.raises(NotImplementedError, match=r"metrics\.py:156-157"):                 # without a model the refusal is the old one
        metrics.MetricsCalculator(["CLIP_Similarity"], "cpu")
    with pytest.raises(ValueError, match="clip_tokenizer"):
        metrics.MetricsCalculator(["CLIP_Similarity"], "cpu", clip_model=model)
    img = np.zeros((40, 48, 3), np.uint8)
    for caption in (None, ""):
        with pytest.raises(ValueError, match="caption"):
            calc.compute_metric("CLIP_Similarity", img, {}, caption)
    with pytest.raises(hip.MfhipError):                                                     # no CPU path behind it
        calc.compute_metric("CLIP_Similarity", img, {}, "a cat")
    with pytest.raises(ValueError, match="2 images but 1 captions"):
        metrics.clip_score(np.zeros((2, 40, 48, 3), np.uint8), ["a cat"], model, tok, device="cpu")


def test_reference_restatement_reproduces_the_stored_scores():
    G = golden("clip_tiny_clip.npz")
    pairs = S.pair_scores(G["image_embeds"], G["text_embeds"])
    assert np.abs(pairs - G["scores"]).max() <= 1e-12
    neg = int(G["negative_pair"])
    assert pairs[neg] < 0 and all(pairs[i] > 0 for i in range(3) if i != neg)
    assert abs(S.clip_score(G["image_embeds"], G["text_embeds"]) - float(G["score_all"])) <= 1e-12
    assert S.clip_score(G["image_embeds"][neg:neg + 1], G["text_embeds"][neg:neg + 1]) == 0.0


def test_finishing_rule_is_the_float64_mean_clamped_at_zero():
    G = golden("clip_tiny_clip.npz")
    assert metrics.clip_finish(G["scores"]) == max(float(np.mean(G["scores"])), 0.0) == float(G["score_all"])
    assert metrics.clip_finish(np.array([-9.4, 3.0], np.float32)) == 0.0 and metrics.clip_finish([-1.0]) == 0.0
    assert metrics.clip_finish(np.array([25.0, 35.0], np.float32)) == 30.0
    assert np.isnan(metrics.clip_finish([float("nan"), 1.0]))          # torch.max(mean, 0) keeps a NaN, and so does this
