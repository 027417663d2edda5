"""Build-owned deterministic weights and inputs.

No pretrained checkpoint exists offline, so every run (golden generation against the imported
reference, parity tests on the GPU box, bench.py) draws parameters from this key-seeded CPU generator:
the value of a tensor depends only on (base seed, state-dict key, shape), never on creation order, so
the reference modules here and the HIP models on the GPU box see bit-identical fp32 parameters.
"""
from __future__ import annotations

import math
import zlib
from typing import Dict, Iterable, Tuple

import torch


def _gen(key: str, seed: int) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed((zlib.crc32(key.encode()) ^ (seed * 0x9E3779B1)) & 0x7FFFFFFF)


def fill(key: str, shape: Iterable[int], seed: int = 0) -> torch.Tensor:
    """Deterministic fp32 tensor for state-dict entry `key`."""
    shape = tuple(int(s) for s in shape)
    g = _gen(key, seed)
    parts = key.split(".")
    leaf = parts[-1]
    parent = parts[-2] if len(parts) >= 2 else ""
    is_norm = (parent.startswith("norm") or parent in ("conv_norm_out", "group_norm") or "layer_norm" in parent   # (CLIP: layer_norm1, final_layer_norm)
               or parent in ("pre_layrnorm", "post_layernorm"))                                                  # (CLIP vision; `layrnorm` is transformers' spelling)
    if leaf == "weight" and is_norm and len(shape) == 1:
        return 1.0 + 0.1 * torch.randn(shape, generator=g)
    if leaf == "bias":
        return (0.1 if is_norm else 0.02) * torch.randn(shape, generator=g)
    if leaf == "weight" and len(shape) >= 2:
        fan_in = 1
        for s in shape[1:]:
            fan_in *= s
        std = 1.0 / math.sqrt(fan_in)
        if key.startswith("brushnet_"):          # the reference zero-inits these; make the injection path live
            std *= 0.5
        return std * torch.randn(shape, generator=g)
    return 0.05 * torch.randn(shape, generator=g)


def state_dict_for(shapes: Dict[str, Tuple[int, ...]], seed: int = 0) -> Dict[str, torch.Tensor]:
    return {k: fill(k, s, seed) for k, s in shapes.items()}


def pipeline_inputs(batch: int, height: int, width: int, seed: int = 1234, cross_dim: int = 768, seq: int = 77,
                    latent_channels: int = 4, vae_scale: int = 8) -> Dict[str, torch.Tensor]:
    """Synthetic pipeline inputs of SURVEY.md §8(d): all drawn on the CPU so they are device-independent."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    hl, wl = height // vae_scale, width // vae_scale
    prompt_embeds = torch.randn(batch, seq, cross_dim, generator=g)
    negative_prompt_embeds = torch.randn(batch, seq, cross_dim, generator=g)
    image = torch.rand(batch, 3, height, width, generator=g)
    mask = torch.zeros(batch, 3, height, width)
    mask[:, :, height // 4: height // 4 + height // 2, width // 4: width // 4 + width // 2] = 1.0   # 25 % hole
    image = image * (1.0 - mask)                                  # hole zeroed
    depth = torch.rand(batch, 1, height, width, generator=g) * 2.0 - 1.0
    latents = torch.randn(batch, latent_channels, hl, wl, generator=g)
    vae_noise = torch.randn(2 * batch, latent_channels, hl, wl, generator=g)   # uncond half, then cond half
    return dict(prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, image=image, mask=mask,
                depth=depth, latents=latents, vae_noise=vae_noise)


def images_u8(seed: int, batch: int, height: int, width: int):
    """Seeded uint8 [batch, height, width, 3] images with some structure (a gradient under noise) as a numpy array: the inputs of the
    CLIP vision fixtures, the same on every machine (numpy's PCG64 stream is stable across versions)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    base = (yy[None, :, :, None] * 3 + xx[None, :, :, None] * 2 + np.arange(3)[None, None, None, :] * 40
            + np.arange(batch)[:, None, None, None] * 25) % 256
    return ((base + rng.integers(0, 96, (batch, height, width, 3))) % 256).astype(np.uint8)


class HashTokenizer:
    """Deterministic stand-in for CLIPTokenizer (no vocabulary file exists offline): lower-cased whitespace words hash to ids in
    [1, vocab_size - 3], wrapped in <bos> = vocab_size - 2 and <eos> = vocab_size - 1 (the highest id, as in CLIP's 49406 / 49407).
    `pad_token_id` None pads with <eos> (CLIP-L's tokenizer), 0 pads with "!" like SDXL's second tokenizer.  Provides what both
    pipelines' encode_prompt touch: model_max_length, __call__ with padding / max_length / truncation / return_tensors, batch_decode."""

    class _Encoding:
        def __init__(self, input_ids):
            self.input_ids = input_ids

    def __init__(self, vocab_size: int = 49408, model_max_length: int = 77, pad_token_id=None):
        self.vocab_size, self.model_max_length = int(vocab_size), int(model_max_length)
        self.bos_token_id, self.eos_token_id = self.vocab_size - 2, self.vocab_size - 1
        self.pad_token_id = self.eos_token_id if pad_token_id is None else int(pad_token_id)

    def _ids(self, text: str):
        return [self.bos_token_id] + [1 + zlib.crc32(w.encode()) % (self.vocab_size - 3) for w in text.lower().split()] + [self.eos_token_id]

    def __call__(self, text, padding=False, max_length=None, truncation=False, return_tensors=None):
        rows = [self._ids(t) for t in ([text] if isinstance(text, str) else list(text))]
        limit = max_length if max_length is not None else self.model_max_length
        if truncation:
            rows = [r if len(r) <= limit else r[:limit - 1] + [self.eos_token_id] for r in rows]
        if padding == "max_length":
            width = limit
        elif padding in ("longest", True):
            width = max(len(r) for r in rows)
        else:
            width = None
        if width is not None:
            rows = [r + [self.pad_token_id] * (width - len(r)) for r in rows]
        if return_tensors == "pt":
            return self._Encoding(torch.tensor(rows, dtype=torch.int64))
        return self._Encoding(rows if not isinstance(text, str) else rows[0])

    def batch_decode(self, ids):
        return [" ".join(f"<{int(i)}>" for i in row) for row in ids]


def lora_plan(modules: Iterable[str]):
    """The fixture adapters' (module, rank, alpha) per LoRA-capable module (tools/make_golden_lora.py and the LoRA tests): ranks 4 and 3
    alternate, every third target has no alpha."""
    return [(m, 4 if i % 2 == 0 else 3, (None, 2.0, 6.0)[i % 3]) for i, m in enumerate(modules)]


def lora_adapter(plan, shapes: Dict[str, Tuple[int, ...]], seed: int, gain: float, prefix: str = "unet."):
    """A diffusers-format LoRA state dict and its network_alphas for plan = [(module, rank, alpha or None)]: every tensor is
    gain * fill(its key without the prefix, its shape, seed).  down is [r, Cin(, kh, kw)], up [N, r(, 1, 1)]."""
    sd, alphas = {}, {}
    for module, rank, alpha in plan:
        shp = tuple(shapes[module + ".weight"])
        kd, ku = f"{module}.lora.down.weight", f"{module}.lora.up.weight"          # (the values do not depend on the prefix)
        sd[prefix + kd] = gain * fill(kd, (rank,) + shp[1:], seed)
        sd[prefix + ku] = gain * fill(ku, (shp[0], rank) + ((1, 1) if len(shp) == 4 else ()), seed)
        if alpha is not None:
            alphas[f"{prefix}{module}.alpha"] = float(alpha)
    return sd, alphas
