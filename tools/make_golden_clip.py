"""Golden fixtures of the CLIP text encoders (reflecting_reality_amd/text_encoder.py) and of both pipelines' encode_prompt.

Runs on the CPU in the build container: needs transformers, and for the pipeline part the reference tree
(`--reference PATH/MirrorFusion/src`, or $MIRRORFUSION_SRC).  Nothing under tests/, bench.py or the package reads either at
run time.  Weights come from `synth.state_dict_for` (key-seeded), token ids from `synth.HashTokenizer`, so the tests
regenerate both; only OUTPUTS of transformers' own modules are stored, from their float64 run:

    tests/golden/clip_<model>.npz     ids, last_hidden_state, hidden_states[-2] (tiny models: every hidden state), pooled,
                                      text_embeds; full-size models keep the rows listed in `rows` of each sequence
    tests/golden/clip_envelope.json   transformers' fp32 run against its float64 run (`fp32_vs_f64`), and its bf16 / fp16 runs
                                      against its fp32 run (`bf16`, `fp16`): L-inf and mean per stored tensor
    tests/golden/clip_pipelines.npz   the reference pipelines' encode_prompt on the tiny models: every text-encoder call they made
                                      (ids + outputs) and the tensors they returned
    tests/golden/keys_clip_<model>.json   state-dict key / shape tables
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reflecting_reality_amd import synth  # noqa: E402
from reflecting_reality_amd.configs import CLIP_FIXTURES  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)

# name -> (config and projection flag from configs.CLIP_FIXTURES, weight seed, pad token id (None: <eos>), prompts)
_LONG = ["a perfect plane mirror reflection of a wooden chair standing on a tiled floor", "a mug"]
_SHORT = ["a mirror on the wall reflecting a red chair", "a cat"]
MODELS = {name: (dict(cfg), proj, seed, (0 if proj else None), (_SHORT if name.startswith("tiny") else _LONG))
          for (name, (cfg, proj)), seed in zip(CLIP_FIXTURES.items(), (70, 71, 72, 73))}
FULL_ROW_STRIDE = 4       # full-size models: every 4th position of each sequence plus the pooled positions


def build(name, dtype=torch.float64):
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    cfg, proj, seed, pad, prompts = MODELS[name]
    tcfg = CLIPTextConfig(**cfg, bos_token_id=cfg["vocab_size"] - 2, pad_token_id=1)
    tcfg._attn_implementation = "eager"
    model = (CLIPTextModelWithProjection if proj else CLIPTextModel)(tcfg).eval()
    # the on-disk names of the SD1.5 / SDXL checkpoints (`text_model.` prefix): newer transformers builds CLIPTextModel without that
    # level and renames on load, so the synth weights are keyed on the checkpoint names either way
    own = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    canon = {k: (k if k.startswith(("text_model.", "text_projection.")) else "text_model." + k) for k in own}
    shapes = {canon[k]: v for k, v in own.items()}
    sd = synth.state_dict_for(shapes, seed)
    model.load_state_dict({k: sd[canon[k]] for k in own}, strict=True)
    return model.to(dtype), shapes


def tokenizer_for(name):
    cfg, _, _, pad, _ = MODELS[name]
    return synth.HashTokenizer(cfg["vocab_size"], cfg["max_position_embeddings"], pad_token_id=pad)


def run(model, ids, proj):
    out = model(ids, output_hidden_states=True)
    hs = [h.double() for h in out.hidden_states]
    res = dict(last_hidden_state=out.last_hidden_state.double(), hidden_states=hs)
    if proj:
        res["text_embeds"] = out.text_embeds.double()
    return res


def pool_index(ids, eos):
    return ids.argmax(-1) if eos == 2 else (ids == eos).int().argmax(-1)


def stats(a, b):
    e = (a.double() - b.double()).abs()
    return dict(linf=float(e.max()), mean=float(e.mean()), absmax=float(b.abs().max()))


def make_models(only=None):
    env = {}
    env_path = os.path.join(GOLD, "clip_envelope.json")
    if only and os.path.exists(env_path):
        with open(env_path) as f:
            env = json.load(f)
    for name, (cfg, proj, seed, pad, prompts) in MODELS.items():
        if only and name not in only:
            continue
        tok = tokenizer_for(name)
        ids = tok(prompts, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
        pidx = pool_index(ids, cfg["eos_token_id"])
        tiny = name.startswith("tiny")
        rows = np.arange(ids.shape[1]) if tiny else np.array(sorted(set(range(0, ids.shape[1], FULL_ROW_STRIDE)) | set(pidx.tolist())))
        runs = {}
        for dname, dt in (("f64", torch.float64), ("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)):
            model, shapes = build(name, dt)
            runs[dname] = run(model, ids, proj)
            runs[dname]["pooled"] = runs[dname]["last_hidden_state"][torch.arange(ids.shape[0]), pidx]
            if not proj:     # transformers' own pooled row must be the rule the HIP model restates
                got = model(ids).pooler_output.double()
                assert torch.equal(got, runs[dname]["pooled"]), f"{name}: pooling rule differs from transformers'"
            del model
            print(f"[{name}] {dname} done", flush=True)
        with open(os.path.join(GOLD, f"keys_clip_{name}.json"), "w") as f:
            json.dump({k: list(v) for k, v in shapes.items()}, f, indent=0)

        def tensors(r):
            t = dict(last_hidden_state=r["last_hidden_state"][:, rows], pooled=r["pooled"])
            if tiny:
                for i, h in enumerate(r["hidden_states"]):
                    t[f"hidden_states_{i}"] = h
            else:
                t["hidden_states_m2"] = r["hidden_states"][-2][:, rows]
            if proj:
                t["text_embeds"] = r["text_embeds"]
            return t

        ref = tensors(runs["f64"])
        np.savez(os.path.join(GOLD, f"clip_{name}.npz"), ids=ids.numpy(), rows=rows, pool_index=pidx.numpy(), seed=np.int64(seed),
                 **{k: v.numpy() for k, v in ref.items()})
        f32 = tensors(runs["fp32"])
        env[name] = dict(fp32_vs_f64={k: stats(f32[k], ref[k]) for k in ref},
                         bf16={k: stats(v, f32[k]) for k, v in tensors(runs["bf16"]).items()},
                         fp16={k: stats(v, f32[k]) for k, v in tensors(runs["fp16"]).items()})
        for mode in ("fp32_vs_f64", "bf16", "fp16"):
            worst = max(env[name][mode].values(), key=lambda s: s["linf"])
            print(f"[{name}] {mode}: worst L-inf {worst['linf']:.3e} (mean {worst['mean']:.3e}, |ref| max {worst['absmax']:.2f})")
    with open(env_path, "w") as f:
        json.dump(env, f, indent=1, sort_keys=True)


class Recorder:
    """Wraps a transformers text encoder: every call's ids and outputs are kept for the fixture."""

    def __init__(self, name, model, calls):
        self.name, self.model, self.calls = name, model, calls
        self.config, self.dtype = model.config, model.dtype
        self.text_model = getattr(model, "text_model", model)       # (final_layer_norm: pipeline_brushnet.py:370)

    def __call__(self, ids, **kw):
        out = self.model(ids, **kw)
        full = self.model(ids, output_hidden_states=True)
        self.calls.append(dict(enc=self.name, ids=ids.clone(), first=full[0].clone(), last=full.last_hidden_state.clone(),
                               hs=torch.stack(list(full.hidden_states))))
        return out


def make_pipelines(reference_src):
    sys.path.insert(0, reference_src)
    import transformers.utils as _tu
    if not hasattr(_tu, "FLAX_WEIGHTS_NAME"):          # removed in transformers 5; the reference imports it
        _tu.FLAX_WEIGHTS_NAME = "flax_model.msgpack"
    from diffusers.pipelines.brushnet.pipeline_brushnet import StableDiffusionBrushNetPipeline as RefSD
    from diffusers.pipelines.brushnet.pipeline_brushnet_sd_xl import StableDiffusionXLBrushNetPipeline as RefXL
    calls = []
    enc_l = Recorder("tiny_l", build("tiny_l", torch.float32)[0], calls)
    enc_g = Recorder("tiny_g", build("tiny_g", torch.float32)[0], calls)
    tok_l, tok_g = tokenizer_for("tiny_l"), tokenizer_for("tiny_g")
    dev = torch.device("cpu")
    out = {}
    xl = types.SimpleNamespace(tokenizer=tok_l, tokenizer_2=tok_g, text_encoder=enc_l, text_encoder_2=enc_g, unet=None,
                               _execution_device=dev, config=types.SimpleNamespace(force_zeros_for_empty_prompt=True))
    cases = {
        # prompt_2 differs from prompt; negative_prompt None -> zeros
        "xl_zeros": dict(prompt=["a mirror reflecting a chair"], prompt_2=["a photo of a room"], negative_prompt=None),
        # explicit negatives through both encoders, two images per prompt
        "xl_neg": dict(prompt=["a mirror reflecting a chair"], prompt_2=None, negative_prompt=["blurry"], negative_prompt_2=["low quality"],
                       num_images_per_prompt=2),
        "xl_skip1": dict(prompt=["a mirror reflecting a chair"], prompt_2=["a photo of a room"], negative_prompt=None, clip_skip=1),
    }
    for cname, kw in cases.items():
        res = RefXL.encode_prompt(xl, device=dev, do_classifier_free_guidance=True, **kw)
        for nm, t in zip(("prompt_embeds", "negative_prompt_embeds", "pooled_prompt_embeds", "negative_pooled_prompt_embeds"), res):
            out[f"{cname}/{nm}"] = t.float().numpy()
    xl2 = types.SimpleNamespace(**{**vars(xl), "tokenizer": None, "text_encoder": None})      # only the second encoder (:299-302)
    res = RefXL.encode_prompt(xl2, prompt=["a mirror reflecting a chair"], device=dev, do_classifier_free_guidance=True)
    for nm, t in zip(("prompt_embeds", "negative_prompt_embeds", "pooled_prompt_embeds", "negative_pooled_prompt_embeds"), res):
        out[f"xl_only2/{nm}"] = t.float().numpy()
    sd = types.SimpleNamespace(tokenizer=tok_l, text_encoder=enc_l, unet=None)
    for cname, skip in (("sd_none", None), ("sd_skip1", 1)):
        pe, npe = RefSD.encode_prompt(sd, ["a mirror reflecting a chair"], dev, 1, True, negative_prompt=["blurry"], clip_skip=skip)
        out[f"{cname}/prompt_embeds"], out[f"{cname}/negative_prompt_embeds"] = pe.float().numpy(), npe.float().numpy()
    seen = {}
    for c in calls:
        seen.setdefault((c["enc"], tuple(c["ids"].flatten().tolist())), c)
    for n, c in enumerate(seen.values()):
        out[f"call{n}/enc"] = np.array(c["enc"])
        out[f"call{n}/ids"] = c["ids"].numpy()
        out[f"call{n}/first"], out[f"call{n}/last"], out[f"call{n}/hs"] = c["first"].numpy(), c["last"].numpy(), c["hs"].numpy()
    out["ncalls"] = np.int64(len(seen))
    np.savez(os.path.join(GOLD, "clip_pipelines.npz"), **out)
    print(f"[pipelines] {len(cases) + 3} encode_prompt cases, {len(seen)} distinct text-encoder calls")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("MIRRORFUSION_SRC"), help="the reference's src directory (pipelines part)")
    ap.add_argument("--models", nargs="*", default=None, help="only these models (default: all)")
    ap.add_argument("--skip-models", action="store_true")
    a = ap.parse_args()
    if not a.skip_models:
        make_models(a.models)
    if a.reference:
        make_pipelines(a.reference)
    else:
        print("no --reference: clip_pipelines.npz not regenerated")
