"""Generate the LoRA fixtures under tests/golden/ by running the IMPORTED REFERENCE's no-PEFT route (loaders/unet.py:74
load_attn_procs, cross_attention_kwargs={"scale": s}, fuse_lora / unfuse_lora).  Runs where tools/make_golden.py runs.

    python tools/make_golden_lora.py

  lora_tiny.npz       TINY_UNET and TINY_XL_UNET with synth weights and a synth adapter on EVERY LoRA-capable module of the reference
                      (ranks 4 and 3, alphas on two targets of three: synth.lora_plan / synth.lora_adapter): inputs, the base output,
                      scale 0.7 unfused, fuse_lora(0.7), scale 1.0
  lora_keys.json      names only: the LoRA-capable modules of TINY_UNET and SD15_UNET, their kohya and legacy attention-processor key
                      names, and the names the reference's converters map those to
  lora_envelope.json  the reference's own bf16 / fp16 deviation from its fp32 result on each recorded tensor
The tool refuses to write unless max|scale 0.7 - base| >= 0.05 and >= 20 x the bf16 envelope's L-inf: a no-op merge cannot pass.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as MG  # noqa: E402  (puts the reference on sys.path)

from diffusers.loaders.lora_conversion_utils import _convert_kohya_lora_to_diffusers  # noqa: E402
from diffusers.models.lora import LoRACompatibleConv, LoRACompatibleLinear  # noqa: E402

from oracle import mirrorfusion_ref as R  # noqa: E402
from reflecting_reality_amd import synth  # noqa: E402

GOLD = MG.GOLD
# config, weight seed, timestep, input seed, (adapter gain, adapter seed).  Gain and seed are what makes the adapter's effect stand
# clear of the bf16 envelope (the refusal below).  The tiny XL net's own bf16 deviation is 0.13 on outputs of magnitude 1.5, four
# times the tiny SD1.5 net's, so its ratio scatters between 12 and 22 over gains and seeds: this pair gives 22.
CASES = {"tiny": (R.TINY_UNET, 0, 501, 42, (0.6, 7)), "tiny_xl": (R.TINY_XL_UNET, 20, 401, 43, (0.58, 9))}
torch.set_grad_enabled(False)


def capable(unet):
    return [n for n, m in unet.named_modules() if isinstance(m, (LoRACompatibleConv, LoRACompatibleLinear))]


def targets(unet):
    """The fixture's targets: every capable module the reference's forward hands the call's `scale` to.  TimestepEmbedding calls its
    two Linears without it (embeddings.py), so an adapter there runs at 1.0 unfused and at lora_scale fused: left out."""
    return [m for m in capable(unet) if not m.startswith(("time_embedding.", "add_embedding."))]


def inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 4, 8, 8, generator=g)
    ehs = torch.randn(2, 77, cfg["cross_attention_dim"], generator=g)
    added = None
    if cfg.get("addition_embed_type") == "text_time":
        added = dict(text_embeds=torch.randn(2, 24, generator=g),
                     time_ids=torch.tensor([[16., 16., 0., 0., 16., 16.], [32., 24., 4., 2., 16., 16.]]))
    return x, ehs, added


def run_case(cfg, wseed, t, iseed, gain, dtype=torch.float32):
    """{name: output} of the reference for one configuration, in `dtype`."""
    unet = MG.build_unet(cfg)
    _, shapes = MG.load_synth(unet, wseed)
    mods = targets(unet)
    plan = synth.lora_plan(mods)
    sd, alphas = synth.lora_adapter(plan, shapes, gain[1], gain[0], prefix="")
    x, ehs, added = inputs(cfg, iseed)
    unet.to(dtype)
    cast = lambda v: None if v is None else {k: a.to(dtype) for k, a in v.items()}
    call = lambda **kw: unet(x.to(dtype), t, encoder_hidden_states=ehs.to(dtype), added_cond_kwargs=cast(added), return_dict=False, **kw)[0].float()
    out = {"base": call()}
    unet.load_attn_procs({k: v.clone() for k, v in sd.items()}, network_alphas=dict(alphas))
    unet.to(dtype)
    out["s07"] = call(cross_attention_kwargs={"scale": 0.7})
    out["s10"] = call()
    unet.fuse_lora(0.7)
    out["fused07"] = call()
    return out, mods, (x, ehs, added)


def key_names(cfg):
    unet = MG.build_unet(cfg)
    mods = capable(unet)
    kohya = {m: "lora_unet_" + m.replace(".", "_") for m in mods}
    fake = {}
    for m, k in kohya.items():
        fake[k + ".lora_down.weight"] = torch.zeros(2, 1)
        fake[k + ".lora_up.weight"] = torch.zeros(1, 2)
        fake[k + ".alpha"] = torch.tensor(1.0)
    conv, alphas = _convert_kohya_lora_to_diffusers(dict(fake))
    legacy_in = {}
    for m in mods:
        head, _, leaf = m.rpartition(".")
        if ".attn" in m and (leaf in ("to_q", "to_k", "to_v") or m.endswith(".to_out.0")):
            base = head if leaf != "0" else head.rpartition(".")[0]
            name = "to_out" if leaf == "0" else leaf
            legacy_in[m] = f"{base}.processor.{name}_lora.down.weight"
    legacy_out, _ = unet.convert_state_dict_legacy_attn_format({k: torch.zeros(1) for k in legacy_in.values()}, None)
    return dict(modules=mods, kohya=kohya, kohya_converted=sorted(conv), kohya_alphas=sorted(alphas), legacy=legacy_in,
                legacy_converted=sorted(legacy_out))


def stats(got, ref):
    e = (got.float() - ref.float()).abs()
    return dict(linf=float(e.max()), mean=float(e.mean()), ref_absmax=float(ref.abs().max()), ref_absmean=float(ref.abs().mean()))


def main():
    arrays, env = {}, {"_about": "|reference(bf16 / fp16) - reference(fp32)| on the tensors of lora_tiny.npz (tools/make_golden_lora.py)"}
    for name, (cfg, wseed, t, iseed, gain) in CASES.items():
        ref, mods, (x, ehs, added) = run_case(cfg, wseed, t, iseed, gain)
        print(f"{name}: {len(mods)} LoRA-capable modules; fused vs unfused {float((ref['s07'] - ref['fused07']).abs().max()):.2e}; "
              f"|s07 - base| {float((ref['s07'] - ref['base']).abs().max()):.3f}; |s10 - base| {float((ref['s10'] - ref['base']).abs().max()):.3f}")
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
            low, _, _ = run_case(cfg, wseed, t, iseed, gain, dt)
            for k in ref:
                env[f"{tag}/{name}/{k}"] = stats(low[k], ref[k])
        delta = float((ref["s07"] - ref["base"]).abs().max())
        floor = 20 * env[f"bf16/{name}/s07"]["linf"]
        if delta < 0.05 or delta < floor:
            raise SystemExit(f"{name}: max|scale 0.7 - base| = {delta:.4f} is below 0.05 or 20 x the bf16 envelope ({floor:.4f}): "
                             "the fixture would not tell a merge from a no-op; change the case's gain")
        for k, v in ref.items():
            arrays[f"{name}_{k}"] = v.numpy()
        arrays[f"{name}_x"], arrays[f"{name}_ehs"] = x.numpy(), ehs.numpy()
        if added:
            arrays[f"{name}_text_embeds"], arrays[f"{name}_time_ids"] = added["text_embeds"].numpy(), added["time_ids"].numpy()
        arrays[f"{name}_plan"] = np.array(json.dumps(synth.lora_plan(mods)))
        arrays[f"{name}_timestep"], arrays[f"{name}_gain"], arrays[f"{name}_seed"] = np.array(t), np.array(gain[0]), np.array(gain[1])
    np.savez(os.path.join(GOLD, "lora_tiny.npz"), **arrays)
    with open(os.path.join(GOLD, "lora_envelope.json"), "w") as f:
        json.dump(env, f, indent=1, sort_keys=True)
    with open(os.path.join(GOLD, "lora_keys.json"), "w") as f:
        json.dump({"tiny": key_names(R.TINY_UNET), "sd15": key_names(R.SD15_UNET)}, f, indent=0, sort_keys=True)
    for k, v in sorted(env.items()):
        if k != "_about":
            print(f"{k:30s} linf {v['linf']:.3e} mean {v['mean']:.3e}")


if __name__ == "__main__":
    main()
