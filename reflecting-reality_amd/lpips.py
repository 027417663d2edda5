"""LPIPS on the libmfhip kernels: the third image-quality number of the reference's `compute_metrics` (metrics/metrics.py:51-67; the
network is chosen at :202-204: torchmetrics' LearnedPerceptualImagePatchSimilarity(net_type="squeeze"), scored with normalize=False).

The network is torchvision's `squeezenet1_1.features` plus one non-negative 1 x 1 weight per tapped layer.  The state-dict keys are
torchvision's (`features.0.weight`, `features.3.squeeze.weight`, ...) and the `lpips` package's (`lin0.model.1.weight` ...), so the two
published files load as they are; `classifier.*` of the torchvision file is ignored.

The uint8 images go through mf_lpips_prepare (normalisation, region blackening and the scaling layer, written as the first conv's
8-channel A operand: the fp32 [B, 3, H, W] tensors never exist), both images of every pair in ONE batch of 2 B through the convolutions
(mf_gemm_conv: stride 2 / no padding, 1 x 1, 3 x 3 / padding 1; a Fire's two expands write the two channel halves of one buffer), mf_relu in
place, mf_maxpool3s2_ceil, and the seven tapped features through mf_lpips_layer; mf_lpips_finish leaves one fp32 [B, 7] row of per-layer
sums on the device.  The division by the pixel counts, the sum over the layers and the mean over the pairs are float64 on the host
(metrics.lpips_finish).  Inference only.
"""
from __future__ import annotations

import contextlib
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import hip, ops
from .models import F32, HipModel
from .ops import ConvWeight

# squeezenet1_1.features: index -> (squeeze, expand) of its Fire modules; MaxPool2d(3, 2, ceil_mode=True) sits at 2, 5 and 8
FIRES = OrderedDict([(3, (64, 16, 64)), (4, (128, 16, 64)), (6, (128, 32, 128)), (7, (256, 32, 128)), (9, (256, 48, 192)), (10, (384, 48, 192)),
                     (11, (384, 64, 256)), (12, (512, 64, 256))])
POOLS = (2, 5, 8)
TAPS = (1, 4, 7, 9, 10, 11, 12)                      # the features LPIPS compares are the outputs of these indices
TAP_CHANNELS = (64, 128, 256, 384, 384, 512, 512)
MIN_SIDE = 31                                        # from here upward every pool still has one whole window


def conv1_extent(n: int) -> int:
    return (n - 3) // 2 + 1


def pool_extent(n: int) -> int:
    return -(-(n - 3) // 2) + 1                      # ceil((n - 3) / 2) + 1; the last window starts inside the image for every n >= 3


def stage_shapes(h: int, w: int) -> List[Tuple[int, int]]:
    """The (height, width) of the seven tapped features for an h x w image."""
    if h < MIN_SIDE or w < MIN_SIDE:
        raise ValueError(f"LPIPS (squeeze) needs at least {MIN_SIDE} pixels per edge (three 3 x 3 / stride 2 pools behind a stride 2 conv), got {h} x {w}")
    s1 = (conv1_extent(h), conv1_extent(w))
    s2 = tuple(pool_extent(n) for n in s1)
    s3 = tuple(pool_extent(n) for n in s2)
    s4 = tuple(pool_extent(n) for n in s3)
    return [s1, s2, s3, s4, s4, s4, s4]


@contextlib.contextmanager
def tiles_by_rule(on: bool):
    """The library's own tile rule instead of the timing tuner: the tile, and with it the summation order of every convolution, is then a
    function of the shapes alone, so a score has the same bits in every process, and nothing is measured on the first call."""
    prev = hip.AUTOTUNE
    if on:
        hip.AUTOTUNE = False
    try:
        yield
    finally:
        hip.AUTOTUNE = prev


class LPIPS(HipModel):
    """torchmetrics' LPIPS with net_type="squeeze" (the `lpips` package's `LPIPS(net="squeeze")`, version 0.1, eval mode)."""

    _class_name = "LPIPS"

    def __init__(self, config=None, precision="fp32", device="cuda", autotune: bool = False, **kwargs):
        cfg = dict(net_type="squeeze")
        cfg.update(config or {})
        cfg.update(kwargs)
        super().__init__(cfg, precision, device)
        if cfg["net_type"] != "squeeze":
            raise NotImplementedError(f"net_type {cfg['net_type']!r}: only 'squeeze' is built (what the reference scores with, metrics.py:202-204)")
        if self.prec.name not in ("fp32", "f16x3", "bf16", "fp16"):
            raise ValueError(f"LPIPS: precision {self.prec.name!r} is not built (use 'fp32', 'f16x3', 'bf16' or 'fp16')")
        self.autotune = bool(autotune)
        self.P: Dict[str, Any] = {}

    # -- parameters ---------------------------------------------------------------------------------
    @staticmethod
    def param_shapes() -> "OrderedDict[str, Tuple[int, ...]]":
        out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
        out["features.0.weight"], out["features.0.bias"] = (64, 3, 3, 3), (64,)
        for i, (cin, s, e) in FIRES.items():
            for name, shape in (("squeeze", (s, cin, 1, 1)), ("expand1x1", (e, s, 1, 1)), ("expand3x3", (e, s, 3, 3))):
                out[f"features.{i}.{name}.weight"], out[f"features.{i}.{name}.bias"] = shape, shape[:1]
        for l, c in enumerate(TAP_CHANNELS):
            out[f"lin{l}.model.1.weight"] = (1, c, 1, 1)
        return out

    def _convert_deprecated_keys(self, sd):
        for k in [k for k in sd if k.startswith("classifier.")]:          # the rest of torchvision's squeezenet1_1 file
            sd.pop(k)
        return sd

    def prepare_training(self, requires_grad=None):
        raise hip.MfhipError("LPIPS is inference only (the reference scores with it, it never trains it)")

    def train(self, mode: bool = True):
        if mode:
            self.prepare_training()
        return self

    def parameters(self):
        if not self._ready:
            raise RuntimeError("no parameters loaded")
        for v in self.P.values():
            yield v.w if isinstance(v, ConvWeight) else v

    def _prepare(self, sd: Dict[str, torch.Tensor]) -> None:
        prec, dev = self.prec, self.device
        P: Dict[str, Any] = {}
        # the first conv reads mf_lpips_prepare's 8-channel pixels: [64][(ky * 3 + kx) * 8 + c], zero pad columns, K = 72
        P["conv1"] = ConvWeight(sd["features.0.weight"], sd["features.0.bias"], prec, dev, cin_pad=8)
        for i in FIRES:
            for name in ("squeeze", "expand1x1", "expand3x3"):
                P[f"{i}.{name}"] = ConvWeight(sd[f"features.{i}.{name}.weight"], sd[f"features.{i}.{name}.bias"], prec, dev)
        for l in range(len(TAPS)):
            P[f"lin{l}"] = sd[f"lin{l}.model.1.weight"].reshape(-1).to(dev, F32).contiguous()
        self.P = P

    @classmethod
    def from_pretrained(cls, backbone, linear=None, precision="fp32", device="cuda", **kw):
        """backbone: torchvision's squeezenet1_1 state dict (a dict, or the path of its .pth / a .safetensors file); linear: the `lpips`
        package's squeeze.pth likewise.  One dict or file that holds both may be given alone."""
        sd: Dict[str, torch.Tensor] = {}
        for src in (backbone, linear):
            if src is None:
                continue
            if not isinstance(src, dict):
                path = str(src)
                if path.endswith(".safetensors"):
                    from safetensors.torch import load_file
                    src = load_file(path)
                else:
                    src = torch.load(path, map_location="cpu", weights_only=True)
            sd.update(src)
        model = cls(precision=precision, device=device, **kw)
        model.load_state_dict(sd)
        return model

    def save_pretrained(self, path: str, **unused):
        import os
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        save_file({k: v.contiguous() for k, v in self.state_dict().items()}, os.path.join(path, "lpips_squeeze.safetensors"))

    # -- forward ------------------------------------------------------------------------------------
    stage_shapes = staticmethod(stage_shapes)

    def _fire(self, i: int, x: torch.Tensor) -> torch.Tensor:
        P = self.P
        _, s, e = FIRES[i]
        b, h, w, _ = x.shape
        sq = hip.relu_(ops.conv2d(x, P[f"{i}.squeeze"], padding=0))
        out = torch.empty(b, h, w, 2 * e, dtype=self.prec.act, device=x.device)
        ops.conv2d(sq, P[f"{i}.expand1x1"], padding=0, out=out[..., :e], ldc=2 * e)          # cat([expand1x1, expand3x3], C) without a copy
        ops.conv2d(sq, P[f"{i}.expand3x3"], padding=1, out=out[..., e:], ldc=2 * e)
        return hip.relu_(out)

    def features(self, x8: torch.Tensor) -> List[torch.Tensor]:
        """mf_lpips_prepare's [N, H, W, 8] tensor -> the seven tapped NHWC features (launches only)."""
        if not self._ready:
            raise RuntimeError("no parameters loaded")
        if ops.TAPE is not None:
            raise hip.MfhipError("LPIPS is inference only: run it outside the training tape")
        taps = []
        with tiles_by_rule(not self.autotune):
            x = hip.relu_(ops.conv2d(x8, self.P["conv1"], stride=2, padding=0))
            taps.append(x)
            for i in range(2, 13):
                if i in POOLS:
                    x = hip.maxpool3s2_ceil(x)
                else:
                    x = self._fire(i, x)
                if i in TAPS:
                    taps.append(x)
        return taps

    def forward(self, pred_u8: torch.Tensor, gt_u8: torch.Tensor, mask: Optional[torch.Tensor] = None, region=None,
                norm_range=[-1, 1]) -> torch.Tensor:
        """uint8 NHWC device tensors [B, H, W, 3] (mask: uint8 [B, H, W], region None / "mask" / "mirror") -> the fp32 [B, 7] DEVICE row of
        per-layer sums over the pixels (metrics.lpips_finish divides by stage_shapes' pixel counts).  Nothing is read back."""
        if list(norm_range) not in ([-1, 1], [0, 1]):
            raise ValueError("Unsupported normalization range. Use [-1, 1] or [0, 1].")
        if pred_u8.dim() != 4 or pred_u8.shape[-1] != 3 or pred_u8.shape != gt_u8.shape:
            raise ValueError(f"LPIPS scores two uint8 [batch, height, width, 3] images of one shape, got {tuple(pred_u8.shape)} and {tuple(gt_u8.shape)}")
        stage_shapes(pred_u8.shape[1], pred_u8.shape[2])                                      # (refuses small sides before any launch)
        x8 = hip.lpips_prepare(pred_u8, gt_u8, mask, region, list(norm_range) == [0, 1], self.prec.act)
        b = pred_u8.shape[0]
        ws = hip.lpips_ws(b, x8.device)
        for l, f in enumerate(self.features(x8)):
            hip.lpips_layer(f, self.P[f"lin{l}"], l, ws)
        return hip.lpips_finish(ws, b)

    __call__ = forward
