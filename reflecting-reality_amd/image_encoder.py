"""CLIPVisionModel, CLIPVisionModelWithProjection and CLIPModel on the libmfhip kernels: the image half of the reference's
`CLIP_Similarity` metric (metrics/metrics.py:156-157: torchmetrics' clip_score on openai/clip-vit-large-patch14) and the tower
examples/brushnet/ip_adapter/ loads for image prompts.

The on-disk format (`config.json` + `model.safetensors`), the state-dict keys (`vision_model.pre_layrnorm` is transformers' spelling) and
the call surface are transformers'; the arithmetic is not ATen.  An image goes through mf_clip_preprocess (CLIPImageProcessor's integer
bicubic resize, crop, normalisation and the unfold of the stride-p patch convolution, written as the A operand of a GEMM: the fp32
`pixel_values` tensor never exists), the patch-embedding GEMM, mf_clip_vision_embed (class token + positions), LayerNorm, the text
towers' encoder layer without its causal mask (text_encoder.encoder_layer: plain flash attention), LayerNorm of token 0 and the
projection GEMM.  PyTorch allocates, slices token 0 and converts the returned tensors to fp32.

Inference only.  Not built, and refused by name: another image size than the config's (`interpolate_pos_encoding`), `attention_mask`,
training.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from typing import Any, Dict, Optional, Tuple

import torch

from . import frontend, hip, ops
from .models import F32, HipModel
from .ops import ConvWeight
from .text_encoder import (_ACTS, CLIPTextModelWithProjection, CLIPTextOutput, encoder_layer, layer_param_shapes, norm_pair,
                           prepare_layers)

_VISION_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, projection_dim=512, num_hidden_layers=12, num_attention_heads=12,
                        num_channels=3, image_size=224, patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5)
HEAD_DIMS = tuple(d for d in ops.FLASH_HEAD_DIMS if d in ops.FLASH_SPLIT_HEAD_DIMS)       # the plain flash kernel in every precision


class CLIPVisionOutput(CLIPTextOutput):
    """transformers' BaseModelOutputWithPooling / CLIPVisionModelOutput: the same indexing rules as the text towers' output."""


class CLIPVisionModel(HipModel):
    """transformers.CLIPVisionModel (modeling_clip.py CLIPVisionTransformer): patch + class + position embedding, `pre_layrnorm`, pre-LN
    layers without a mask; `last_hidden_state` is the encoder's output, `pooler_output` the `post_layernorm` of its token 0, and
    `hidden_states[0]` the encoder's INPUT, i.e. the embeddings after `pre_layrnorm`."""

    config_name = "config.json"
    weights_name = "model.safetensors"
    _class_name = "CLIPVisionModel"
    _projection = False
    image_mean, image_std = frontend.CLIP_MEAN, frontend.CLIP_STD         # preprocessor_config.json of every OpenAI CLIP checkpoint

    def __init__(self, config=None, precision="bf16", device="cuda", **kwargs):
        cfg = dict(_VISION_DEFAULTS)
        cfg.update(config or {})
        cfg.update(kwargs)
        super().__init__(cfg, precision, device)
        if self.prec.name not in ("fp32", "f16x3", "bf16", "fp16"):
            raise ValueError(f"{type(self).__name__}: precision {self.prec.name!r} is not built for the CLIP towers "
                             "(use 'fp32', 'f16x3', 'bf16' or 'fp16')")
        if cfg["hidden_act"] not in _ACTS:
            raise NotImplementedError(f"hidden_act {cfg['hidden_act']!r} (have {sorted(_ACTS)})")
        c, heads = cfg["hidden_size"], cfg["num_attention_heads"]
        if c % heads or c // heads not in HEAD_DIMS or c % 8 or cfg["intermediate_size"] % 8:
            raise NotImplementedError(f"hidden_size {c} / {heads} heads: head dims {HEAD_DIMS} and widths % 8 == 0")
        if cfg["num_channels"] != 3 or cfg["image_size"] % cfg["patch_size"]:
            raise NotImplementedError(f"{cfg['num_channels']} channels, image {cfg['image_size']} / patch {cfg['patch_size']}: RGB images "
                                      "and whole patches")
        self.eps = float(cfg["layer_norm_eps"])
        self.P: Dict[str, Any] = {}

    # -- geometry -----------------------------------------------------------------------------------
    @property
    def num_patches(self) -> int:
        return (self.config["image_size"] // self.config["patch_size"]) ** 2

    @property
    def patch_k(self) -> int:
        return 3 * self.config["patch_size"] ** 2

    @property
    def patch_k8(self) -> int:
        return (self.patch_k + 7) // 8 * 8

    # -- parameters ---------------------------------------------------------------------------------
    def param_shapes(self) -> "OrderedDict[str, Tuple[int, ...]]":
        cfg = self.config
        c, p = cfg["hidden_size"], cfg["patch_size"]
        out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
        out["vision_model.embeddings.class_embedding"] = (c,)
        out["vision_model.embeddings.patch_embedding.weight"] = (c, 3, p, p)
        out["vision_model.embeddings.position_embedding.weight"] = (self.num_patches + 1, c)
        out["vision_model.pre_layrnorm.weight"] = (c,)
        out["vision_model.pre_layrnorm.bias"] = (c,)
        layer_param_shapes(out, "vision_model.encoder.layers.", cfg)
        out["vision_model.post_layernorm.weight"] = (c,)
        out["vision_model.post_layernorm.bias"] = (c,)
        if self._projection:
            out["visual_projection.weight"] = (cfg["projection_dim"], c)
        return out

    def _convert_deprecated_keys(self, sd):
        sd.pop("vision_model.embeddings.position_ids", None)          # integer buffer of older checkpoints
        return sd

    def prepare_training(self, requires_grad=None):
        raise hip.MfhipError("the CLIP vision tower is inference only (the reference scores with it, it never trains it)")

    def train(self, mode: bool = True):
        if mode:
            self.prepare_training()
        return self

    def parameters(self):
        if not self._ready:
            raise RuntimeError("no parameters loaded")
        yield self.P["position_embedding"]
        for v in self.P.values():
            if isinstance(v, ConvWeight):
                yield v.w

    def _prepare(self, sd: Dict[str, torch.Tensor]) -> None:
        prec, dev, cfg = self.prec, self.device, self.config
        tdt = prec.compute if prec.half else F32
        e = "vision_model.embeddings."
        P: Dict[str, Any] = {}
        P["class_embedding"] = sd[e + "class_embedding"].to(dev, tdt).contiguous()
        P["position_embedding"] = sd[e + "position_embedding.weight"].to(dev, tdt).contiguous()
        # the stride-p convolution as a GEMM: weight.reshape(C, 3 p p), K zero-padded to K8 (mf_clip_preprocess writes zero pad columns)
        P["patch"] = ConvWeight(sd[e + "patch_embedding.weight"].reshape(cfg["hidden_size"], -1), None, prec, dev, cin_pad=self.patch_k8)
        P["pre_ln"] = norm_pair(sd, "vision_model.pre_layrnorm", dev)
        prepare_layers(P, sd, "vision_model.encoder.layers.", cfg["num_hidden_layers"], prec, dev)
        P["post_ln"] = norm_pair(sd, "vision_model.post_layernorm", dev)
        if self._projection:
            P["visual_projection"] = ConvWeight(sd["visual_projection.weight"], None, prec, dev)
        self.P = P

    def save_pretrained(self, path: str, **unused):
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        cfg = dict(self.config)
        cfg.update(architectures=[self._class_name], model_type="clip_vision_model")
        with open(os.path.join(path, self.config_name), "w") as f:
            json.dump(cfg, f, indent=2, sort_keys=True)
        save_file({k: v.contiguous() for k, v in self.state_dict().items()}, os.path.join(path, self.weights_name))

    # -- forward ------------------------------------------------------------------------------------
    def preprocess(self, images, return_u8: bool = False):
        """CLIPImageProcessor for this tower's image and patch size: images (metrics.to_u8_nhwc's rules) -> the patch matrix
        [B, num_patches, K8] in the activation dtype, on the device."""
        size = self.config["image_size"]
        return frontend.clip_preprocess(images, size, size, self.image_mean, self.image_std, self.prec.act, patch=self.config["patch_size"],
                                        return_u8=return_u8, device=self.device)

    def patches_of(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """A caller's own fp32 `pixel_values` [B, 3, R, R] as the patch matrix (a layout copy: no arithmetic).  The product path never
        builds pixel_values: preprocess() writes the patch matrix from the uint8 image."""
        cfg = self.config
        r, p = cfg["image_size"], cfg["patch_size"]
        if pixel_values.dim() != 4 or pixel_values.shape[1] != 3:
            raise ValueError(f"pixel_values is [batch, 3, {r}, {r}], got {tuple(pixel_values.shape)}")
        if tuple(pixel_values.shape[2:]) != (r, r):
            raise NotImplementedError(f"pixel_values {tuple(pixel_values.shape[2:])} differ from the config's image_size {r}: "
                                      "interpolate_pos_encoding is not built")
        b, n = pixel_values.shape[0], r // p
        x = pixel_values.to(self.device, F32).reshape(b, 3, n, p, n, p).permute(0, 2, 4, 1, 3, 5).reshape(b, n * n, self.patch_k)
        out = torch.zeros(b, n * n, self.patch_k8, dtype=self.prec.act, device=self.device)
        out[..., :self.patch_k] = x
        return out

    def _stack(self, patches: torch.Tensor, output_hidden_states: bool = False):
        """Patch GEMM, embedding, pre_layrnorm and the layers: launches only."""
        P, prec = self.P, self.prec
        pe = ops.linear(patches, P["patch"])
        x = hip.clip_vision_embed(pe, P["class_embedding"], P["position_embedding"], prec.act)
        x = hip.layernorm(x, *P["pre_ln"], self.eps, prec.act)
        hidden = [x] if output_hidden_states else None
        for i in range(self.config["num_hidden_layers"]):
            x = encoder_layer(P, i, x, self.config, prec, self.eps, causal=False)
            if hidden is not None:
                hidden.append(x)
        pooled = hip.layernorm(x[:, 0].contiguous(), *P["post_ln"], self.eps, prec.act)
        return x, pooled, hidden

    def _encode(self, pixel_values, patches, images, output_hidden_states: bool):
        if not self._ready:
            raise RuntimeError("no parameters loaded")
        if ops.TAPE is not None:
            raise hip.MfhipError("the CLIP vision tower is inference only: run it outside the training tape")
        if sum(v is not None for v in (pixel_values, patches, images)) != 1:
            raise ValueError("give exactly one of pixel_values, patches (preprocess()'s output) and images")
        if images is not None:
            patches = self.preprocess(images)
        elif pixel_values is not None:
            patches = self.patches_of(pixel_values)
        want = (self.num_patches, self.patch_k8)
        if patches.dim() != 3 or tuple(patches.shape[1:]) != want or patches.dtype != self.prec.act or not patches.is_contiguous():
            raise ValueError(f"patches is a contiguous [batch, {want[0]}, {want[1]}] {self.prec.act} tensor, got {tuple(patches.shape)} {patches.dtype}")
        last, pooled, hidden = self._stack(patches, output_hidden_states)
        hs = tuple(h.float() for h in hidden) if hidden is not None else None
        return last, pooled, hs

    def forward(self, pixel_values=None, attention_mask=None, output_hidden_states: bool = False, return_dict: bool = True,
                interpolate_pos_encoding: bool = False, patches=None, images=None, **unused):
        if attention_mask is not None:
            raise NotImplementedError("attention_mask: the vision tower attends every token (transformers passes none either)")
        if interpolate_pos_encoding:
            raise NotImplementedError("interpolate_pos_encoding: only the config's image_size is built")
        last, pooled, hs = self._encode(pixel_values, patches, images, output_hidden_states)
        if self._projection:          # CLIPVisionModelOutput: image_embeds = pooler_output @ visual_projection^T comes first
            head = OrderedDict(image_embeds=ops.linear(pooled, self.P["visual_projection"], out_dtype=F32), last_hidden_state=last.float())
        else:                         # BaseModelOutputWithPooling
            head = OrderedDict(last_hidden_state=last.float(), pooler_output=pooled.float())
        head["hidden_states"] = hs
        out = CLIPVisionOutput(head)
        if self._projection:
            out.pooler_output = pooled.float()    # (an attribute only: transformers' CLIPVisionModelOutput has no such field)
        return out if return_dict else out.to_tuple()

    __call__ = forward


class CLIPVisionModelWithProjection(CLIPVisionModel):
    """transformers.CLIPVisionModelWithProjection: `image_embeds` = pooler_output @ visual_projection^T (not normalised) comes first."""

    _class_name = "CLIPVisionModelWithProjection"
    _projection = True


class CLIPModel(HipModel):
    """transformers.CLIPModel as far as scoring needs it: a CLIPTextModelWithProjection and a CLIPVisionModelWithProjection from ONE
    checkpoint (`text_model.*`, `text_projection.weight`, `vision_model.*`, `visual_projection.weight`, `logit_scale`).
    get_text_features / get_image_features return the projected, NOT normalised features as fp32 device tensors."""

    config_name = "config.json"
    weights_name = "model.safetensors"
    _class_name = "CLIPModel"

    def __init__(self, config=None, precision="bf16", device="cuda", **kwargs):
        cfg = dict(projection_dim=512, logit_scale_init_value=2.6592, text_config={}, vision_config={})
        cfg.update(config or {})
        cfg.update(kwargs)
        cfg["text_config"] = dict(cfg["text_config"] or {})
        cfg["vision_config"] = dict(cfg["vision_config"] or {})
        super().__init__(cfg, precision, device)
        proj = cfg["projection_dim"]
        self.text = CLIPTextModelWithProjection(dict(cfg["text_config"], projection_dim=proj), precision=self.prec, device=device)
        self.vision = CLIPVisionModelWithProjection(dict(cfg["vision_config"], projection_dim=proj), precision=self.prec, device=device)
        self.logit_scale: Optional[float] = None

    def param_shapes(self) -> "OrderedDict[str, Tuple[int, ...]]":
        out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
        out["logit_scale"] = ()
        out.update(self.text.param_shapes())
        out.update(self.vision.param_shapes())
        return out

    def _convert_deprecated_keys(self, sd):
        for k in ("text_model.embeddings.position_ids", "vision_model.embeddings.position_ids"):
            sd.pop(k, None)
        return sd

    def prepare_training(self, requires_grad=None):
        raise hip.MfhipError("CLIPModel is inference only (the reference scores with it, it never trains it)")

    def train(self, mode: bool = True):
        if mode:
            self.prepare_training()
        return self

    def to(self, *args, **kwargs):
        super().to(*args, **kwargs)
        self.text.device = self.vision.device = self.device
        return self

    def parameters(self):
        yield from self.text.parameters()
        yield from self.vision.parameters()

    def _prepare(self, sd: Dict[str, torch.Tensor]) -> None:
        self.text.device = self.vision.device = self.device
        self.text.load_state_dict({k: sd[k] for k in self.text.param_shapes()})
        self.vision.load_state_dict({k: sd[k] for k in self.vision.param_shapes()})
        self.logit_scale = float(sd["logit_scale"])

    def save_pretrained(self, path: str, **unused):
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        cfg = dict(self.config)
        cfg.update(architectures=[self._class_name], model_type="clip", text_config=dict(cfg["text_config"]),
                   vision_config=dict(cfg["vision_config"]))
        with open(os.path.join(path, self.config_name), "w") as f:
            json.dump(cfg, f, indent=2, sort_keys=True)
        save_file({k: v.contiguous() for k, v in self.state_dict().items()}, os.path.join(path, self.weights_name))

    def get_text_features(self, input_ids, attention_mask=None) -> torch.Tensor:
        return self.text(input_ids, attention_mask=attention_mask).text_embeds

    def get_image_features(self, pixel_values=None, patches=None, images=None) -> torch.Tensor:
        return self.vision(pixel_values, patches=patches, images=images).image_embeds

    def forward(self, *args, **kwargs):
        raise NotImplementedError("CLIPModel.forward (the logits of every image against every text) is not built: scoring pairs "
                                  "get_image_features / get_text_features through metrics.clip_score")

    __call__ = forward
