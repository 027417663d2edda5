"""`MfhipAttnProcessor`: the HIP attention kernels behind the reference's own operator ABI.

The one operator plug-in point the reference has is `Attention.set_processor` / `model.set_attn_processor(proc)`
(models/attention_processor.py:216; brushnet.py:558-590; unets/unet_2d_condition.py:716-748): any callable
`proc(attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, scale=1.0) -> Tensor` replaces
`AttnProcessor2_0` (attention_processor.py:1213-1286).  A maintainer who keeps the reference's torch modules on a ROCm
device installs this class to run the `softmax(q k^T / sqrt(d)) v` core on `mf_attention_bf16` (bf16 inputs, head dims
8 / 40 / 64 / 80 / 160) or on the strided-batched `mf_gemm_conv` + `mf_softmax_rows` path (fp32, other head dims); the
projections, norms and the residual stay the module's own torch layers, exactly as in the reference processor.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .ops import Precision


class MfhipAttnProcessor:
    def __call__(self, attn, hidden_states: torch.Tensor, encoder_hidden_states: Optional[torch.Tensor] = None,
                 attention_mask: Optional[torch.Tensor] = None, temb: Optional[torch.Tensor] = None, scale: float = 1.0
                 ) -> torch.Tensor:
        if attention_mask is not None:
            raise NotImplementedError("attention_mask is never passed on the MirrorFusion path (SURVEY.md §8 a-9)")
        if not hidden_states.is_cuda:
            raise RuntimeError("MfhipAttnProcessor needs tensors on a ROCm device: there is no CPU fallback")
        residual = hidden_states
        if getattr(attn, "spatial_norm", None) is not None:
            hidden_states = attn.spatial_norm(hidden_states, temb)
        input_ndim = hidden_states.ndim
        if input_ndim == 4:                                                  # the VAE's spatial attention (:1228-1230)
            b, c, hh, ww = hidden_states.shape
            hidden_states = hidden_states.view(b, c, hh * ww).transpose(1, 2)
        if getattr(attn, "group_norm", None) is not None:
            hidden_states = attn.group_norm(hidden_states.transpose(1, 2)).transpose(1, 2)
        q = attn.to_q(hidden_states)
        if encoder_hidden_states is None:
            encoder_hidden_states = hidden_states
        elif getattr(attn, "norm_cross", None):
            encoder_hidden_states = attn.norm_encoder_hidden_states(encoder_hidden_states)
        k = attn.to_k(encoder_hidden_states)
        v = attn.to_v(encoder_hidden_states)
        heads = attn.heads
        inner = k.shape[-1]
        d = inner // heads
        skv = k.shape[1]
        prec = Precision.get("bf16" if q.dtype == torch.bfloat16 else "fp16" if q.dtype == torch.float16 else "fp32")
        ld = (skv + 7) // 8 * 8
        vt = torch.zeros(v.shape[0], inner, ld, dtype=prec.act, device=v.device)      # V^T, keys contiguous
        vt[:, :, :skv] = v.to(prec.act).transpose(1, 2)
        o = ops.attention(q.to(prec.act).contiguous(), k.to(prec.act).contiguous(), vt, heads, skv, 1.0 / (d ** 0.5), prec)
        o = o.to(q.dtype)
        o = attn.to_out[0](o)
        o = attn.to_out[1](o)
        if input_ndim == 4:
            o = o.transpose(-1, -2).reshape(b, c, hh, ww)
        if getattr(attn, "residual_connection", False):
            o = o + residual
        return o / getattr(attn, "rescale_output_factor", 1.0)


class MfhipIPAttnProcessor(torch.nn.Module):
    """The reference's `IPAttnProcessor2_0(hidden_size, cross_attention_dim, scale, num_tokens)` (ip_adapter/attention_processor.py:282-410,
    installed on every attn2 by train_brushnet_mirror.py's 'ip_adapter' normals mode) on the HIP decoupled cross-attention
    (`ops.attention(ip=...)`: mf_attention_ip_* — both softmaxes in one launch).  The last `num_tokens` rows of `encoder_hidden_states`
    are the image-prompt tokens: they go through `to_k_ip` / `to_v_ip` (no bias; the checkpoint keys "<i>.to_k_ip.weight" /
    "<i>.to_v_ip.weight") and get a softmax of their own, scaled by `scale`; the rows before them are the text.

    Two uses.  Called with a reference `Attention` module it follows that processor line by line with the module's own torch layers
    for the projections, like `MfhipAttnProcessor`.  Installed on this library's `UNet2DConditionModel` through
    `set_attn_processor({... "attn2.processor": MfhipIPAttnProcessor(...)})` it is the holder of the layer's `to_k_ip` / `to_v_ip`
    weights, `scale` and `num_tokens`; the model runs the fused path itself (models._UNetCore._attention)."""

    def __init__(self, hidden_size: int, cross_attention_dim: Optional[int] = None, scale: float = 1.0, num_tokens: int = 4):
        super().__init__()
        if not 1 <= num_tokens <= 64:
            raise ValueError(f"num_tokens = {num_tokens}: the ip segment is one key tile of the attention kernel (1 .. 64)")
        self.hidden_size, self.cross_attention_dim, self.scale, self.num_tokens = hidden_size, cross_attention_dim, scale, num_tokens
        self.to_k_ip = torch.nn.Linear(cross_attention_dim or hidden_size, hidden_size, bias=False)
        self.to_v_ip = torch.nn.Linear(cross_attention_dim or hidden_size, hidden_size, bias=False)

    def __call__(self, attn, hidden_states: torch.Tensor, encoder_hidden_states: Optional[torch.Tensor] = None,
                 attention_mask: Optional[torch.Tensor] = None, temb: Optional[torch.Tensor] = None, *args, **kwargs) -> torch.Tensor:
        if attention_mask is not None:
            raise NotImplementedError("attention_mask is never passed on the MirrorFusion path (SURVEY.md §8 a-9)")
        if encoder_hidden_states is None:
            raise ValueError("MfhipIPAttnProcessor is a cross-attention processor: encoder_hidden_states carries the ip tokens in its last rows")
        if not hidden_states.is_cuda:
            raise RuntimeError("MfhipIPAttnProcessor needs tensors on a ROCm device: there is no CPU fallback")
        residual = hidden_states
        if getattr(attn, "spatial_norm", None) is not None:
            hidden_states = attn.spatial_norm(hidden_states, temb)
        input_ndim = hidden_states.ndim
        if input_ndim == 4:
            b, c, hh, ww = hidden_states.shape
            hidden_states = hidden_states.view(b, c, hh * ww).transpose(1, 2)
        if getattr(attn, "group_norm", None) is not None:
            hidden_states = attn.group_norm(hidden_states.transpose(1, 2)).transpose(1, 2)
        q = attn.to_q(hidden_states)
        end_pos = encoder_hidden_states.shape[1] - self.num_tokens
        if end_pos < 1:
            raise ValueError(f"encoder_hidden_states has {encoder_hidden_states.shape[1]} rows: fewer than num_tokens + 1 = {self.num_tokens + 1}")
        encoder_hidden_states, ip_hidden_states = encoder_hidden_states[:, :end_pos, :], encoder_hidden_states[:, end_pos:, :]
        if getattr(attn, "norm_cross", None):
            encoder_hidden_states = attn.norm_encoder_hidden_states(encoder_hidden_states)
        k = attn.to_k(encoder_hidden_states)
        v = attn.to_v(encoder_hidden_states)
        k_ip = self.to_k_ip(ip_hidden_states)
        v_ip = self.to_v_ip(ip_hidden_states)
        heads = attn.heads
        inner = k.shape[-1]
        d = inner // heads
        prec = Precision.get("bf16" if q.dtype == torch.bfloat16 else "fp16" if q.dtype == torch.float16 else "fp32")

        def transposed(t):          # V^T, keys contiguous, zero pad columns
            n = t.shape[1]
            vt = torch.zeros(t.shape[0], inner, (n + 7) // 8 * 8, dtype=prec.act, device=t.device)
            vt[:, :, :n] = t.to(prec.act).transpose(1, 2)
            return vt
        o = ops.attention(q.to(prec.act).contiguous(), k.to(prec.act).contiguous(), transposed(v), heads, end_pos, 1.0 / (d ** 0.5), prec,
                          ip=(k_ip.to(prec.act).contiguous(), transposed(v_ip), self.num_tokens, float(self.scale)))
        o = o.to(q.dtype)
        o = attn.to_out[0](o)
        o = attn.to_out[1](o)
        if input_ndim == 4:
            o = o.transpose(-1, -2).reshape(b, c, hh, ww)
        if getattr(attn, "residual_connection", False):
            o = o + residual
        return o / getattr(attn, "rescale_output_factor", 1.0)
