"""CLIPTextModel and CLIPTextModelWithProjection on the libmfhip kernels: the prompt encoders of both pipelines.

Reference: `encode_prompt` of pipelines/brushnet/pipeline_brushnet.py:271-450 and pipeline_brushnet_sd_xl.py:213-420 call
transformers' CLIPTextModel (SD1.5: CLIP ViT-L/14, `quick_gelu`; SDXL adds OpenCLIP bigG/14 with a text projection, `gelu`), and
the training loop runs the frozen encoder every step (examples/brushnet/train_brushnet_mirror.py:1419-1420).  The on-disk format
(`config.json` + `model.safetensors`), the state-dict keys and the call surface are transformers'; the arithmetic is not ATen:
embedding gather, LayerNorm, the bias / residual GEMMs, causal flash attention and the activation are HIP kernels behind
include/mfhip.h, and nothing falls back to PyTorch math.  PyTorch moves the token ids to the device, picks the pooled row and
converts the returned tensors to fp32.

Inference only (the text encoder is frozen in the reference): no tape, no fp8.  The tokenizer stays the caller's object.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from typing import Any, Dict, Optional, Tuple

import torch

from . import hip, ops
from .models import F32, HipModel
from .ops import ConvWeight

_DEFAULTS = dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, projection_dim=512, num_hidden_layers=12,
                 num_attention_heads=8, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2)
_ACTS = {"quick_gelu": hip.ACT_QUICK_GELU, "gelu": hip.ACT_GELU_ERF}
_POSITION_IDS = "text_model.embeddings.position_ids"     # integer buffer of older checkpoints: dropped on load, never written


def layer_param_shapes(out, prefix: str, cfg) -> None:
    """The state-dict keys of CLIPEncoder's layers under `prefix` ("text_model.encoder.layers." / "vision_model.encoder.layers."), in
    transformers' order."""
    c, inner = cfg["hidden_size"], cfg["intermediate_size"]
    for i in range(cfg["num_hidden_layers"]):
        p = f"{prefix}{i}."
        for nm, shp in (("self_attn.k_proj", (c, c)), ("self_attn.v_proj", (c, c)), ("self_attn.q_proj", (c, c)),
                        ("self_attn.out_proj", (c, c)), ("layer_norm1", None), ("mlp.fc1", (inner, c)), ("mlp.fc2", (c, inner)),
                        ("layer_norm2", None)):
            out[p + nm + ".weight"] = shp or (c,)
            out[p + nm + ".bias"] = (shp[0],) if shp else (c,)


def norm_pair(sd, name: str, device):
    return (sd[name + ".weight"].to(device, F32).contiguous(), sd[name + ".bias"].to(device, F32).contiguous())


def prepare_layers(P: Dict[str, Any], sd, prefix: str, layers: int, prec, dev, only=None) -> None:
    """The device weights of the layers under `prefix`, as encoder_layer() reads them from P.  `only`: the module names whose weights
    changed (a selective rebuild, lora.py) — the entries that derive from none of them stay the objects they are."""
    def put(key, deps, make):
        if only is None or any(d in only for d in deps):
            P[key] = make()

    def rows(*ws):                                   # a merged adapter weight lives on the device, its untargeted neighbour on the host
        return torch.cat([w.to(dev) for w in ws] if any(w.is_cuda for w in ws) else list(ws))

    for i in range(layers):
        p = f"{prefix}{i}."
        a = p + "self_attn."
        put(f"{i}.ln1", (), lambda: norm_pair(sd, p + "layer_norm1", dev))
        put(f"{i}.ln2", (), lambda: norm_pair(sd, p + "layer_norm2", dev))
        put(f"{i}.to_qk", (a + "q_proj", a + "k_proj"),
            lambda: ConvWeight(rows(sd[a + "q_proj.weight"], sd[a + "k_proj.weight"]),
                               torch.cat([sd[a + "q_proj.bias"], sd[a + "k_proj.bias"]]), prec, dev))
        # V^T leaves ops.linear_t with the weight as the A operand: never pre-split
        put(f"{i}.to_v", (a + "v_proj",), lambda: ConvWeight(sd[a + "v_proj.weight"], sd[a + "v_proj.bias"], prec, dev, raw=True))
        put(f"{i}.out", (a + "out_proj",), lambda: ConvWeight(sd[a + "out_proj.weight"], sd[a + "out_proj.bias"], prec, dev))
        put(f"{i}.fc1", (p + "mlp.fc1",), lambda: ConvWeight(sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], prec, dev))
        put(f"{i}.fc2", (p + "mlp.fc2",), lambda: ConvWeight(sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"], prec, dev))


def encoder_layer(P: Dict[str, Any], i: int, x: torch.Tensor, cfg, prec, eps: float, causal: bool) -> torch.Tensor:
    """One pre-LN CLIPEncoderLayer (modeling_clip.py) on x [B, S, C]: the text towers run it under the causal mask, the vision tower
    (image_encoder.py) without one."""
    b, s, c = x.shape
    heads = cfg["num_attention_heads"]
    d = c // heads
    h = ops.layernorm(x, P[f"{i}.ln1"], eps, prec.act)
    qk = ops.linear(h, P[f"{i}.to_qk"])
    vt = ops.linear_t(h, P[f"{i}.to_v"], (s + 7) // 8 * 8)            # 77 keys -> ld 80, pad columns zero
    o = ops.attention(qk[..., :c], qk[..., c:], vt, heads, s, d ** -0.5, prec, c=c, causal=causal)
    x = ops.linear(o, P[f"{i}.out"], res0=x)
    h = ops.layernorm(x, P[f"{i}.ln2"], eps, prec.act)
    m = ops.linear(h, P[f"{i}.fc1"])
    hip.act(m, _ACTS[cfg["hidden_act"]], out=m)
    return ops.linear(m, P[f"{i}.fc2"], res0=x)


class CLIPTextOutput:
    """transformers' BaseModelOutputWithPooling / CLIPTextModelOutput as far as the pipelines index them: integer indices walk the
    non-None fields in order (`out[0]`, `out[1]`, `out[-1]`), the names are attributes."""

    def __init__(self, fields: "OrderedDict[str, Any]"):
        self._fields = fields
        for k, v in fields.items():
            setattr(self, k, v)

    def to_tuple(self) -> tuple:
        return tuple(v for v in self._fields.values() if v is not None)

    def __getitem__(self, i):
        return self._fields[i] if isinstance(i, str) else self.to_tuple()[i]

    def __len__(self):
        return len(self.to_tuple())

    def __iter__(self):
        return iter(self.to_tuple())


class _TextTransformer:
    """`model.text_model`: what encode_prompt's clip_skip branch touches (pipeline_brushnet.py:362-370)."""

    def __init__(self, owner: "CLIPTextModel"):
        self._owner = owner

    def final_layer_norm(self, hidden: torch.Tensor) -> torch.Tensor:
        o = self._owner
        return hip.layernorm(hidden.contiguous(), *o.P["final_layer_norm"], o.eps, F32)


class CLIPTextModel(HipModel):
    """transformers.CLIPTextModel (modeling_clip.py): token + position embedding, pre-LN transformer layers under a causal mask,
    final LayerNorm; `pooler_output` is the final hidden state at the end-of-text position."""

    config_name = "config.json"
    weights_name = "model.safetensors"
    _class_name = "CLIPTextModel"
    _projection = False
    _lora_model = "text_encoder"
    _lora_refusal = None
    _lora_layers_prefix = "text_model.encoder.layers."      # the layers' Linears (the embeddings and the projection are no adapter targets)

    def __init__(self, config=None, precision="bf16", device="cuda", **kwargs):
        cfg = dict(_DEFAULTS)
        cfg.update(config or {})
        cfg.update(kwargs)
        super().__init__(cfg, precision, device)
        if self.prec.name not in ("fp32", "f16x3", "bf16", "fp16"):
            raise ValueError(f"{type(self).__name__}: precision {self.prec.name!r} is not built for the text encoders "
                             "(use 'fp32', 'f16x3', 'bf16' or 'fp16')")
        if cfg["hidden_act"] not in _ACTS:
            raise NotImplementedError(f"hidden_act {cfg['hidden_act']!r} (have {sorted(_ACTS)})")
        c, heads = cfg["hidden_size"], cfg["num_attention_heads"]
        if c % heads or c // heads not in ops.FLASH_CAUSAL_HEAD_DIMS or c % 8 or cfg["intermediate_size"] % 8:
            raise NotImplementedError(f"hidden_size {c} / {heads} heads: head dims {ops.FLASH_CAUSAL_HEAD_DIMS} and widths % 8 == 0")
        self.eps = float(cfg["layer_norm_eps"])
        self.text_model = _TextTransformer(self)
        self.P: Dict[str, Any] = {}

    # -- parameters ---------------------------------------------------------------------------------
    def param_shapes(self) -> "OrderedDict[str, Tuple[int, ...]]":
        cfg = self.config
        c = cfg["hidden_size"]
        out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
        out["text_model.embeddings.token_embedding.weight"] = (cfg["vocab_size"], c)
        out["text_model.embeddings.position_embedding.weight"] = (cfg["max_position_embeddings"], c)
        layer_param_shapes(out, "text_model.encoder.layers.", cfg)
        out["text_model.final_layer_norm.weight"] = (c,)
        out["text_model.final_layer_norm.bias"] = (c,)
        if self._projection:
            out["text_projection.weight"] = (cfg["projection_dim"], c)
        return out

    def _convert_deprecated_keys(self, sd):
        sd.pop(_POSITION_IDS, None)
        return sd

    def prepare_training(self, requires_grad=None):
        raise hip.MfhipError("the text encoders are inference only (frozen in the reference: train_brushnet_mirror.py:1076)")

    def parameters(self):
        """Device tensors of the model (callers ask `next(model.parameters()).device`)."""
        if not self._ready:
            raise RuntimeError("no parameters loaded")
        yield self.P["token_embedding"]
        yield self.P["position_embedding"]
        for v in self.P.values():
            if isinstance(v, ConvWeight):
                yield v.w

    def _norm_pair(self, sd, name):
        return (sd[name + ".weight"].to(self.device, F32).contiguous(), sd[name + ".bias"].to(self.device, F32).contiguous())

    def _prepare(self, sd: Dict[str, torch.Tensor]) -> None:
        prec, dev = self.prec, self.device
        tdt = prec.compute if prec.half else F32
        if self._only is not None:         # a selective rebuild (lora.py): only the layers' Linears are adapter targets
            prepare_layers(self.P, sd, "text_model.encoder.layers.", self.config["num_hidden_layers"], prec, dev, only=self._only)
            return
        P: Dict[str, Any] = {}
        P["token_embedding"] = sd["text_model.embeddings.token_embedding.weight"].to(dev, tdt).contiguous()
        P["position_embedding"] = sd["text_model.embeddings.position_embedding.weight"].to(dev, tdt).contiguous()
        prepare_layers(P, sd, "text_model.encoder.layers.", self.config["num_hidden_layers"], prec, dev)
        P["final_layer_norm"] = self._norm_pair(sd, "text_model.final_layer_norm")
        if self._projection:
            P["text_projection"] = ConvWeight(sd["text_projection.weight"], None, prec, dev)
        self.P = P

    # -- loading / saving: transformers' layout -----------------------------------------------------------
    def save_pretrained(self, path: str, **unused):
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        cfg = dict(self.config)
        cfg.update(architectures=[self._class_name], model_type="clip_text_model")
        with open(os.path.join(path, self.config_name), "w") as f:
            json.dump(cfg, f, indent=2, sort_keys=True)
        save_file({k: v.contiguous() for k, v in self.state_dict().items()}, os.path.join(path, self.weights_name))

    # -- forward ------------------------------------------------------------------------------------
    def _layer(self, i: int, x: torch.Tensor) -> torch.Tensor:
        return encoder_layer(self.P, i, x, self.config, self.prec, self.eps, causal=True)

    def _pool_index(self, ids: torch.Tensor) -> torch.Tensor:
        """modeling_clip.py: eos_token_id == 2 is the legacy rule (the SD1.5 / SDXL checkpoints): the highest id of the row is the
        end-of-text token; otherwise the first position that holds eos_token_id."""
        eos = self.config["eos_token_id"]
        if eos == 2:
            return ids.argmax(dim=-1)
        return (ids == eos).to(torch.int32).argmax(dim=-1)

    def _stack(self, ids: torch.Tensor, output_hidden_states: bool = False):
        """Embedding, the layers and the final LayerNorm: launches only (capturable into a hipGraph when `ids` is on the device)."""
        P = self.P
        x = hip.embed_tokens(ids, P["token_embedding"], P["position_embedding"], self.prec.act)
        hidden = [x] if output_hidden_states else None
        for i in range(self.config["num_hidden_layers"]):
            x = self._layer(i, x)
            if hidden is not None:
                hidden.append(x)
        return hip.layernorm(x, *P["final_layer_norm"], self.eps, self.prec.act), hidden

    def _encode(self, input_ids: torch.Tensor, output_hidden_states: bool):
        if not self._ready:
            raise RuntimeError("no parameters loaded")
        if ops.TAPE is not None:
            raise hip.MfhipError("the text encoders are inference only: run them outside the training tape")
        if input_ids.dim() != 2:
            raise ValueError("input_ids is a [batch, seq] tensor of token ids")
        self._lora_sync()
        if input_ids.shape[1] > self.config["max_position_embeddings"]:
            raise ValueError(f"sequence length {input_ids.shape[1]} exceeds max_position_embeddings "
                             f"{self.config['max_position_embeddings']}")
        ids_host = input_ids.detach().to("cpu", torch.int64)
        # checked on the host copy whichever side the caller's tensor lives on (both pipelines move the ids to the device first);
        # mf_embed_tokens clamps on its own, so a bad id could otherwise pass silently as vocab_size - 1
        vocab = self.config["vocab_size"]
        if ids_host.numel() and (int(ids_host.min()) < 0 or int(ids_host.max()) >= vocab):
            raise ValueError(f"token ids must lie in [0, {vocab}), got [{int(ids_host.min())}, {int(ids_host.max())}]")
        last, hidden = self._stack(input_ids if input_ids.is_cuda else ids_host, output_hidden_states)
        rows = torch.arange(ids_host.shape[0], device=last.device)
        pooled = last[rows, self._pool_index(ids_host).to(last.device)].contiguous()
        hs = tuple(h.float() for h in hidden) if hidden is not None else None
        return last, pooled, hs

    def forward(self, input_ids, attention_mask=None, output_hidden_states: bool = False, return_dict: bool = True, **unused):
        if attention_mask is not None:
            raise NotImplementedError("attention_mask: neither pipeline passes one for these checkpoints (the causal mask is built in)")
        last, pooled, hs = self._encode(input_ids, output_hidden_states)
        if self._projection:          # CLIPTextModelOutput: text_embeds = pooled @ text_projection^T comes first
            head = OrderedDict(text_embeds=ops.linear(pooled, self.P["text_projection"], out_dtype=F32), last_hidden_state=last.float())
        else:                         # BaseModelOutputWithPooling
            head = OrderedDict(last_hidden_state=last.float(), pooler_output=pooled.float())
        head["hidden_states"] = hs
        out = CLIPTextOutput(head)
        return out if return_dict else out.to_tuple()

    __call__ = forward


class CLIPTextModelWithProjection(CLIPTextModel):
    """transformers.CLIPTextModelWithProjection: `text_embeds` = pooled @ text_projection^T comes first in the output."""

    _class_name = "CLIPTextModelWithProjection"
    _projection = True
