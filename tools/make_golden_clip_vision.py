"""Golden fixtures of the CLIP vision tower, CLIPModel scoring and the image preprocessing (reflecting_reality_amd/image_encoder.py,
frontend.clip_preprocess, metrics.clip_score).

Runs on the CPU in the build container: needs transformers and PIL.  Nothing under tests/, bench.py or the package reads either at
run time.  Weights come from `synth.state_dict_for` (key-seeded, keyed on the checkpoint names), input images from a seeded numpy
generator and token ids from `synth.HashTokenizer`, so the tests regenerate all three; only OUTPUTS of transformers' and PIL's own code
are stored, the networks' from their float64 run:

    tests/golden/clip_<model>.npz          (tiny_vit_a, tiny_vit_b, vit_d64, vit_l4: CLIPVisionModelWithProjection) last_hidden_state,
                                           hidden_states (tiny models: every one; vit_l4: entry 0), pooler_output, image_embeds =
                                           visual_projection(pooler_output), NOT normalised; vit_l4 keeps the token rows listed in `rows`
    tests/golden/clip_tiny_clip.npz        a CLIPModel of tiny_l's text tower + tiny_vit_a: images, captions' ids, both unnormalised
                                           projections, the per-pair scores 100 cos, which pair is negative
    tests/golden/clip_vision_envelope.json transformers' fp32 run against its float64 run (`fp32_vs_f64`), its bf16 / fp16 runs against
                                           its fp32 run: L-inf and mean per stored tensor
    tests/golden/clip_preprocess.npz       uint8 inputs, PIL's resized and cropped uint8 outputs, CLIPImageProcessor's pixel_values
    tests/golden/keys_clip_<model>.json    state-dict key / shape tables
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reflecting_reality_amd import synth  # noqa: E402
from reflecting_reality_amd.configs import CLIP_VISION_FIXTURES, TINY_CLIP  # noqa: E402
from reflecting_reality_amd.frontend import CLIP_MEAN, CLIP_STD  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)

SEEDS = {"tiny_vit_a": 90, "tiny_vit_b": 91, "vit_d64": 92, "vit_l4": 93, "tiny_clip": 94}
ROW_STRIDE = 16           # vit_l4: every 16th token row plus rows 0 and 256
BATCH = 2
# (height, width, size): portrait with an odd crop offset (the long edge becomes 45), landscape, upscale (the filter scale stays 1),
# both passes skipped, two square reductions
PREPROCESS_CASES = ((80, 56, 32), (40, 100, 32), (20, 24, 32), (32, 32, 32), (64, 64, 28), (57, 91, 56))
# tiny_clip: candidate captions; three pairs are chosen from the float64 run so that exactly the last one has a negative cosine
CAPTIONS = ["a mirror on the wall reflecting a red chair", "a cat", "a perfect plane mirror reflection of a wooden chair",
            "a mug on a table", "a dog on a sofa", "blurry", "a photo of a room", "low quality", "a green plant in front of a mirror",
            "two chairs", "a lamp", "a bathroom sink below a mirror"]
CLIP_IMAGE_HW = (40, 48)


def pixel_values_of(u8: np.ndarray) -> np.ndarray:
    """CLIPImageProcessor's rescale + normalise on images that already have the model's size, restated in numpy: [B, 3, R, R] fp32."""
    x = (u8.astype(np.float64) * (1 / 255)).astype(np.float32)
    x = (x - np.array(CLIP_MEAN, dtype=np.float32)) / np.array(CLIP_STD, dtype=np.float32)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def processor(size: int):
    from transformers import CLIPImageProcessor
    return CLIPImageProcessor(do_resize=True, size={"shortest_edge": size}, resample=3, do_center_crop=True, crop_size={"height": size, "width": size},
                              do_rescale=True, rescale_factor=1 / 255, do_normalize=True, image_mean=list(CLIP_MEAN), image_std=list(CLIP_STD),
                              do_convert_rgb=True)


def process(u8: np.ndarray, size: int) -> np.ndarray:
    from PIL import Image
    return processor(size)(images=[Image.fromarray(im) for im in u8], return_tensors="np")["pixel_values"].astype(np.float32)


def stats(a, b):
    e = (a.double() - b.double()).abs()
    return dict(linf=float(e.max()), mean=float(e.mean()), absmax=float(b.abs().max()))


def canon(k: str) -> str:
    """The on-disk name of a key of transformers' module (newer versions build CLIPVisionModel without the `vision_model.` level)."""
    return k if k.startswith(("vision_model.", "visual_projection.", "text_model.", "text_projection.", "logit_scale")) else "vision_model." + k


def load_synth(model, seed):
    own = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("position_ids")}
    shapes = {canon(k): v for k, v in own.items()}
    sd = synth.state_dict_for(shapes, seed)
    model.load_state_dict({k: sd[canon(k)] for k in own}, strict=False)
    return shapes


def build_vision(name, dtype):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    cfg = CLIPVisionConfig(**CLIP_VISION_FIXTURES[name])
    cfg._attn_implementation = "eager"
    model = CLIPVisionModelWithProjection(cfg).eval()
    shapes = load_synth(model, SEEDS[name])
    return model.to(dtype), shapes


def run_vision(model, pv):
    out = model.vision_model(pixel_values=pv, output_hidden_states=True)
    return dict(last_hidden_state=out.last_hidden_state.double(), hidden_states=[h.double() for h in out.hidden_states],
                pooler_output=out.pooler_output.double(), image_embeds=model.visual_projection(out.pooler_output).double())


def make_vision(env):
    for name, cfg in CLIP_VISION_FIXTURES.items():
        r = cfg["image_size"]
        u8 = synth.images_u8(SEEDS[name], BATCH, r, r)
        pv = pixel_values_of(u8)
        assert np.array_equal(pv, process(u8, r)), f"{name}: the numpy restatement of rescale + normalise differs from CLIPImageProcessor"
        tokens = (r // cfg["patch_size"]) ** 2 + 1
        tiny = name != "vit_l4"
        rows = np.arange(tokens) if tiny else np.array(sorted(set(range(0, tokens, ROW_STRIDE)) | {0, tokens - 1}))
        runs = {}
        for dname, dt in (("f64", torch.float64), ("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)):
            model, shapes = build_vision(name, dt)
            runs[dname] = run_vision(model, torch.from_numpy(pv).to(dt))
            del model
            print(f"[{name}] {dname} done", flush=True)
        with open(os.path.join(GOLD, f"keys_clip_{name}.json"), "w") as f:
            json.dump({k: list(v) for k, v in shapes.items()}, f, indent=0)

        def tensors(r_):
            t = dict(last_hidden_state=r_["last_hidden_state"][:, rows], pooler_output=r_["pooler_output"], image_embeds=r_["image_embeds"])
            for i, h in enumerate(r_["hidden_states"]):
                if tiny or i == 0:
                    t[f"hidden_states_{i}"] = h[:, rows]
            return t

        ref = tensors(runs["f64"])
        np.savez(os.path.join(GOLD, f"clip_{name}.npz"), rows=rows, seed=np.int64(SEEDS[name]), batch=np.int64(BATCH),
                 **{k: v.numpy() for k, v in ref.items()})
        f32 = tensors(runs["fp32"])
        env[name] = dict(fp32_vs_f64={k: stats(f32[k], ref[k]) for k in ref},
                         bf16={k: stats(v, f32[k]) for k, v in tensors(runs["bf16"]).items()},
                         fp16={k: stats(v, f32[k]) for k, v in tensors(runs["fp16"]).items()})
        for mode in ("fp32_vs_f64", "bf16", "fp16"):
            worst = max(env[name][mode].values(), key=lambda s: s["linf"])
            print(f"[{name}] {mode}: worst L-inf {worst['linf']:.3e} (mean {worst['mean']:.3e}, |ref| max {worst['absmax']:.2f})")


def build_clip(dtype):
    from transformers import CLIPConfig, CLIPModel
    t = dict(TINY_CLIP["text_config"])
    cfg = CLIPConfig(text_config=dict(t, bos_token_id=t["vocab_size"] - 2, pad_token_id=1), vision_config=dict(TINY_CLIP["vision_config"]),
                     projection_dim=TINY_CLIP["projection_dim"], logit_scale_init_value=TINY_CLIP["logit_scale_init_value"])
    cfg._attn_implementation = cfg.text_config._attn_implementation = cfg.vision_config._attn_implementation = "eager"
    model = CLIPModel(cfg).eval()
    shapes = load_synth(model, SEEDS["tiny_clip"])
    return model.to(dtype), shapes


def run_clip(model, ids, pv):
    vis = model.vision_model(pixel_values=pv)
    txt = model.text_model(input_ids=ids)
    return dict(image_embeds=model.visual_projection(vis.pooler_output).double(), text_embeds=model.text_projection(txt.pooler_output).double())


def make_clip(env):
    t = TINY_CLIP["text_config"]
    r = TINY_CLIP["vision_config"]["image_size"]
    tok = synth.HashTokenizer(t["vocab_size"], t["max_position_embeddings"])
    u8 = synth.images_u8(SEEDS["tiny_clip"], 3, *CLIP_IMAGE_HW)
    pv = process(u8, r)
    model, shapes = build_clip(torch.float64)
    all_ids = tok(CAPTIONS, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
    full = run_clip(model, all_ids, torch.from_numpy(pv).double())
    i_n = full["image_embeds"] / full["image_embeds"].norm(dim=-1, keepdim=True)
    t_n = full["text_embeds"] / full["text_embeds"].norm(dim=-1, keepdim=True)
    cos = 100 * i_n @ t_n.T                                                   # [3 images, all captions]
    pick = [int(torch.argmax(cos[0])), int(torch.argmax(cos[1])), int(torch.argmin(cos[2]))]
    assert cos[0, pick[0]] > 0 and cos[1, pick[1]] > 0 and cos[2, pick[2]] < 0, f"no caption gives the wanted signs: {cos}"
    captions = [CAPTIONS[i] for i in pick]
    ids = all_ids[pick]
    runs = {"f64": run_clip(model, ids, torch.from_numpy(pv).double())}
    for dname, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)):
        m, _ = build_clip(dt)
        runs[dname] = run_clip(m, ids, torch.from_numpy(pv).to(dt))
    ref = runs["f64"]
    scores = torch.stack([cos[i, pick[i]] for i in range(3)])
    with open(os.path.join(GOLD, "keys_clip_tiny_clip.json"), "w") as f:
        json.dump({k: list(v) for k, v in shapes.items()}, f, indent=0)
    np.savez(os.path.join(GOLD, "clip_tiny_clip.npz"), seed=np.int64(SEEDS["tiny_clip"]), images=u8, ids=ids.numpy(), captions=np.array(captions),
             image_embeds=ref["image_embeds"].numpy(), text_embeds=ref["text_embeds"].numpy(), scores=scores.numpy(), negative_pair=np.int64(2),
             score_all=np.float64(max(float(scores.mean()), 0.0)))
    env["tiny_clip"] = dict(fp32_vs_f64={k: stats(runs["fp32"][k], ref[k]) for k in ref},
                            bf16={k: stats(runs["bf16"][k], runs["fp32"][k]) for k in ref},
                            fp16={k: stats(runs["fp16"][k], runs["fp32"][k]) for k in ref})
    print(f"[tiny_clip] captions {captions}, scores {scores.tolist()}")


def make_preprocess():
    from PIL import Image
    out = {"cases": np.array(PREPROCESS_CASES, dtype=np.int64)}
    for n, (h, w, size) in enumerate(PREPROCESS_CASES):
        u8 = synth.images_u8(200 + n, 1, h, w)[0]
        if h <= w:
            h1, w1 = size, int(size * w / h)
        else:
            h1, w1 = int(size * h / w), size
        resized = np.array(Image.fromarray(u8).resize((w1, h1), Image.BICUBIC))
        top, left = (h1 - size) // 2, (w1 - size) // 2
        pv = process(u8[None], size)[0]
        crop = resized[top:top + size, left:left + size]
        # the processor's own resize + crop is PIL's: its pixel_values are the stored crop, rescaled and normalised
        assert np.array_equal(pv, pixel_values_of(crop[None])[0]), f"case {n}: CLIPImageProcessor does not resize / crop like PIL here"
        out[f"case{n}_in"], out[f"case{n}_resized"], out[f"case{n}_crop"], out[f"case{n}_pixel_values"] = u8, resized, crop, pv
        out[f"case{n}_offsets"] = np.array([top, left], dtype=np.int64)
    np.savez(os.path.join(GOLD, "clip_preprocess.npz"), **out)
    print(f"[preprocess] {len(PREPROCESS_CASES)} cases")


if __name__ == "__main__":
    env = {}
    make_preprocess()
    make_clip(env)
    make_vision(env)
    with open(os.path.join(GOLD, "clip_vision_envelope.json"), "w") as f:
        json.dump(env, f, indent=1, sort_keys=True)
