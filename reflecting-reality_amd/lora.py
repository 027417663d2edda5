"""LoRA adapters, always merged: W + sum coef * up @ down is computed on the device in fp32 (mf_lora_merge, csrc/lora.hip) and only
the device layouts that derive from a targeted weight are derived again.  A denoise step reads the same layouts as without an adapter,
so an adapter costs nothing per step; the reference's per-call `scale` (models/lora.py LoRACompatibleConv / LoRACompatibleLinear
.forward(scale)) becomes "merge again when the scale on the device differs".

Reference surface kept (its no-PEFT route): loaders/unet.py:74 `load_attn_procs(state_dict_or_path, network_alphas=...)`,
`cross_attention_kwargs={"scale": s}`, `fuse_lora(lora_scale, safe_fusing)`, `unfuse_lora()`.  The base weight is KEPT on the device
(a stash of the targeted weights only), never subtracted back: un-merging is exact, where the reference's `_unfuse_lora` is lossy.

Formats, read from their specifications (module names are checked against the model's own param_shapes()):
  diffusers   [unet. | text_encoder.]<module>.lora.down.weight / .lora.up.weight  (also .lora_linear_layer. for the text encoder),
              alphas in `network_alphas` as [unet.]<module>.alpha or in the dict itself as <module>.alpha
  legacy      ...attn1.processor.to_q_lora.down.weight (to_q / to_k / to_v / to_out -> to_out.0)
  kohya       lora_unet_<module with _ for .>.lora_down.weight / .lora_up.weight / .alpha, lora_te_... for the text encoder; the
              underscore ambiguity is resolved by matching against {name.replace(".", "_"): name} of the model, not by rewrite rules
SDXL's SGM block numbering (lora_unet_input_blocks_...) and lora_te1_ / lora_te2_ keys raise NotImplementedError.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import hip

F32 = torch.float32
WEIGHT_NAME = "pytorch_lora_weights.safetensors"
_SGM = ("input_blocks_", "middle_block_", "output_blocks_", "out_", "time_embed_", "label_emb_")
_LEGACY = {"to_q_lora": "to_q", "to_k_lora": "to_k", "to_v_lora": "to_v", "to_out_lora": "to_out.0"}


# ---- format readers -------------------------------------------------------------------------------------------------------------
def read_state_dict(state_or_path, weight_name: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """A dict as it is; a .safetensors file; or a directory holding `weight_name` (default pytorch_lora_weights.safetensors)."""
    if isinstance(state_or_path, dict):
        return dict(state_or_path)
    path = os.fspath(state_or_path)
    if os.path.isdir(path):
        path = os.path.join(path, weight_name or WEIGHT_NAME)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no LoRA weights at {path}")
    if not path.endswith(".safetensors"):
        raise ValueError(f"{path}: LoRA weights are read from .safetensors files")
    from safetensors.torch import load_file
    return load_file(path)


def parse_key(key: str) -> Tuple[str, str, str, str]:
    """One key of a LoRA state dict -> (model, style, module, part): model "unet" / "text_encoder" / "" (no prefix: the model that
    loads it), style "dotted" (module is the model's own name) or "kohya" (module is the name with _ for .), part "down" / "up" /
    "alpha".  ValueError names a key of no known format."""
    for pre in ("lora_te1_", "lora_te2_"):
        if key.startswith(pre):
            raise NotImplementedError(f"{key}: {pre}* keys are SDXL's two text encoders in kohya's layout, which is not built")
    for pre, model in (("lora_unet_", "unet"), ("lora_te_", "text_encoder")):
        if key.startswith(pre):
            name, dot, part = key[len(pre):].partition(".")
            parts = {"lora_down.weight": "down", "lora_up.weight": "up", "alpha": "alpha"}
            if not dot or part not in parts:
                raise ValueError(f"{key}: a kohya key ends in .lora_down.weight, .lora_up.weight or .alpha")
            if model == "unet" and name.startswith(_SGM):
                raise NotImplementedError(f"{key}: SDXL's SGM block numbering (input_blocks / middle_block / output_blocks) is not built; "
                                          "convert the file to diffusers names first")
            return model, "kohya", name, parts[part]
    model, rest = "", key
    for pre in ("unet.", "text_encoder."):
        if key.startswith(pre):
            model, rest = pre[:-1], key[len(pre):]
    if key.startswith("text_encoder_2."):
        raise NotImplementedError(f"{key}: SDXL's second text encoder is not an adapter target here")
    if rest.endswith(".alpha"):
        module = rest[: -len(".alpha")]
        try:                                         # the reference's converters name an alpha <the down weight's key>.alpha
            return model, "dotted", parse_key(module)[2], "alpha"
        except ValueError:
            pass
        head, _, leaf = module.rpartition(".")
        if leaf in _LEGACY and head.endswith(".processor"):
            module = head[: -len(".processor")] + "." + _LEGACY[leaf]
        return model, "dotted", module, "alpha"
    for mid in (".lora.", ".lora_linear_layer."):
        for part in ("down", "up"):
            tail = f"{mid}{part}.weight"
            if rest.endswith(tail):
                return model, "dotted", rest[: -len(tail)], part
    for part in ("down", "up"):                       # the legacy attention-processor form
        tail = f".{part}.weight"
        if rest.endswith(tail):
            head, _, leaf = rest[: -len(tail)].rpartition(".")
            if leaf in _LEGACY and head.endswith(".processor"):
                return model, "dotted", head[: -len(".processor")] + "." + _LEGACY[leaf], part
    raise ValueError(f"{key}: not a LoRA key of the diffusers, legacy attention-processor or kohya format")


def group_keys(sd: Dict[str, torch.Tensor], network_alphas: Optional[Dict[str, Any]] = None) -> Dict[str, "OrderedDict"]:
    """{model: {(style, module): {"down", "up", "alpha", "key"}}} of a LoRA state dict (+ the reference's separate alpha dict)."""
    out: Dict[str, OrderedDict] = {"unet": OrderedDict(), "text_encoder": OrderedDict(), "": OrderedDict()}
    items = list(sd.items())
    for k, v in (network_alphas or {}).items():
        if v is None:
            continue
        if parse_key(k)[3] != "alpha":
            raise ValueError(f"network_alphas[{k!r}]: an alpha key ends in .alpha")
        items.append((k, v))
    for key, val in items:
        model, style, module, part = parse_key(key)
        ent = out[model].setdefault((style, module), {"key": key})
        if part in ent:
            raise ValueError(f"{key}: the {part} part of {module} is given twice")
        ent[part] = float(val) if part == "alpha" else val
    return out


def resolve(entries: "OrderedDict", shapes: Dict[str, Tuple[int, ...]], capable: Sequence[str]) -> "OrderedDict[str, tuple]":
    """Entries of group_keys for ONE model -> {module: (down [r, K], up [N, r], coef)} in the order of the model's parameters, every
    shape checked against param_shapes(): down [r, Cin, kh, kw] or [r, Cin], up [N, r, 1, 1] or [N, r]; coef = alpha / r, 1 without
    an alpha.  ValueError names the offending key; nothing is returned half-checked."""
    by_us = {m.replace(".", "_"): m for m in capable}
    cap = set(capable)
    found = {}
    for (style, name), ent in entries.items():
        key = ent["key"]
        module = by_us.get(name) if style == "kohya" else (name if name in cap else None)
        if module is None:
            raise ValueError(f"{key}: {name!r} is no LoRA-capable module of this model")
        if module in found:
            raise ValueError(f"{key}: {module} is targeted twice in one adapter")
        if "down" not in ent or "up" not in ent:
            raise ValueError(f"{key}: {module} needs both its down and its up weight")
        down, up = ent["down"], ent["up"]
        shp = tuple(shapes[module + ".weight"])
        n, tail = shp[0], shp[1:]
        r = down.shape[0] if down.dim() >= 1 else 0
        if r < 1 or tuple(down.shape[1:]) != tail:
            raise ValueError(f"{key}: down weight {tuple(down.shape)} does not fit {module} {shp} (expected [r, {', '.join(map(str, tail))}])")
        if tuple(up.shape) not in ((n, r), (n, r, 1, 1)):
            raise ValueError(f"{key}: up weight {tuple(up.shape)} does not fit {module} {shp} at rank {r} (expected [{n}, {r}] or [{n}, {r}, 1, 1])")
        alpha = ent.get("alpha")
        found[module] = (down.detach().to("cpu", F32).reshape(r, -1).contiguous(), up.detach().to("cpu", F32).reshape(n, r).contiguous(),
                         (alpha / r) if alpha is not None else 1.0)
    order = {m: i for i, m in enumerate(capable)}
    return OrderedDict((m, found[m]) for m in sorted(found, key=order.__getitem__))


def scale_of(cross_attention_kwargs) -> Optional[float]:
    """The reference's cross_attention_kwargs as far as they are built: {"scale": s} (None / {} -> None).  Any other key is refused."""
    if not cross_attention_kwargs:
        return None
    other = [k for k in cross_attention_kwargs if k != "scale"]
    if other:
        raise NotImplementedError(f"cross_attention_kwargs {other}: only 'scale' (the LoRA scale) is built")
    return float(cross_attention_kwargs["scale"])


def merge_host(sd: Dict[str, torch.Tensor], terms: Dict[str, List[tuple]], dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """The host route, for comparison and tests: {name: W + sum coef * up @ down} in `dtype`, returned as fp32, for
    terms = {module: [(down [r, K], up [N, r], coef), ...]}.  coef is taken at its fp32 value, as the device reads it."""
    out = dict(sd)
    for module, ts in terms.items():
        w = sd[module + ".weight"]
        acc = w.detach().to(dtype).reshape(w.shape[0], -1).clone()
        for down, up, coef in ts:
            c = float(torch.tensor(coef, dtype=F32))
            acc += c * (up.to(dtype) @ down.to(dtype))
        out[module + ".weight"] = acc.to(F32).reshape(w.shape)
    return out


# ---- the model side -----------------------------------------------------------------------------------------------------------------
class _State:
    def __init__(self):
        self.adapters: "OrderedDict[str, OrderedDict]" = OrderedDict()   # name -> {module: (down_dev, up_dev, coef)}
        self.active: List[Tuple[str, float]] = []
        self.scale = 1.0                  # the scale a call runs at when it names none
        self.pinned: Optional[float] = None
        self.stash: Dict[str, torch.Tensor] = {}                          # module -> fp32 base [N, K] on the device
        self.tables: Optional[hip.LoraTables] = None
        self.merged: Dict[str, torch.Tensor] = {}                         # module -> the tables' out buffer [N, K]
        self.term_coef: List[float] = []                                  # per term: adapter weight * alpha / r
        self.on_device = None             # (tables, coefs) the device layouts were derived from; None: the base
        self.device_modules: set = set()
        self.host_cache: Dict[str, torch.Tensor] = {}


class LoraMixin:
    """What HipModel gains (models.UNet2DConditionModel, text_encoder.CLIPTextModel).  A class refuses by setting _lora_refusal."""

    _lora_refusal: Optional[str] = None
    _lora_model = "unet"                  # which prefix of a combined file is this model's
    _lora_layers_prefix = ""              # adapter targets are the conv / linear weights under this prefix

    # -- names ------------------------------------------------------------------------------------------------------------------
    def lora_modules(self) -> List[str]:
        """The LoRA-capable modules in parameter order: the reference's LoRACompatibleConv / LoRACompatibleLinear layers."""
        return [k[: -len(".weight")] for k, s in self.param_shapes().items()
                if k.endswith(".weight") and len(s) in (2, 4) and k.startswith(self._lora_layers_prefix)]

    def _lora_state(self) -> Optional[_State]:
        return self.__dict__.get("_lora")

    def _lora_guard(self) -> None:
        if self._lora_refusal:
            raise NotImplementedError(self._lora_refusal)
        if self.training:
            raise NotImplementedError(f"{type(self).__name__}: LoRA adapters are merged into the inference layouts; a model in the training "
                                      "layout takes none (training LoRA layers is not built)")
        if self._src is None:
            raise RuntimeError(f"{type(self).__name__}: the fp32 master copy was dropped, so there is no base weight to merge an adapter into")

    # -- loading ----------------------------------------------------------------------------------------------------------------
    def load_lora(self, state_dict_or_path, network_alphas=None, adapter_name: Optional[str] = None, weight_name: Optional[str] = None,
                  _entries=None) -> str:
        """Parse, check every shape against param_shapes(), then upload up / down and the fp32 base of each targeted weight and build
        the device tables.  Nothing is changed when a check fails.  The adapter is active at weight 1.0; returns its name."""
        self._lora_guard()
        if _entries is None:
            groups = group_keys(read_state_dict(state_dict_or_path, weight_name), network_alphas)
            other = "text_encoder" if self._lora_model == "unet" else "unet"
            if groups[other] and not (groups[self._lora_model] or groups[""]):
                raise ValueError(f"the state dict holds only {other} keys ({next(iter(groups[other].values()))['key']}, ...): "
                                 f"this is the {self._lora_model}")
            _entries = OrderedDict(list(groups[self._lora_model].items()) + list(groups[""].items()))
        if not _entries:
            raise ValueError("the state dict holds no LoRA weights for this model")
        found = resolve(_entries, self.param_shapes(), self.lora_modules())
        st = self._lora_state()
        name = adapter_name or f"default_{len(st.adapters) if st else 0}"
        if st is not None and name in st.adapters:
            raise ValueError(f"adapter_name {name!r} is already loaded: unload_lora() it or pick another name")
        if st is None:
            st = self.__dict__["_lora"] = _State()
        dev = self.device
        st.adapters[name] = OrderedDict((m, (d.to(dev), u.to(dev), c)) for m, (d, u, c) in found.items())
        for m in found:
            if m not in st.stash:
                w = self._src[m + ".weight"]
                st.stash[m] = w.reshape(w.shape[0], -1).to(dev, F32).contiguous()
        st.active.append((name, 1.0))
        self._lora_tables()
        return name

    def load_attn_procs(self, pretrained_model_name_or_path_or_dict, network_alphas=None, adapter_name=None, **kwargs):
        """loaders/unet.py:74, the no-PEFT route: LoRA files only (custom diffusion is not built)."""
        weight_name = kwargs.pop("weight_name", None)
        if kwargs:
            raise NotImplementedError(f"load_attn_procs: {sorted(kwargs)} are not built")
        self.load_lora(pretrained_model_name_or_path_or_dict, network_alphas=network_alphas, adapter_name=adapter_name, weight_name=weight_name)

    def _lora_tables(self) -> None:
        """The device tables of the ACTIVE adapters: one target per touched weight (parameter order), one term per adapter (the order
        of set_adapters).  New output buffers every time: layouts derived from the old ones stay valid until they are rebuilt."""
        st = self._lora_state()
        order = {m: i for i, m in enumerate(self.lora_modules())}
        mods = sorted({m for n, _ in st.active for m in st.adapters[n]}, key=order.__getitem__)
        st.tables, st.merged, st.term_coef = None, {}, []
        if not mods:
            return
        targets = []
        for m in mods:
            out = torch.empty_like(st.stash[m])
            pairs = []
            for n, w in st.active:
                if m in st.adapters[n]:
                    d, u, c = st.adapters[n][m]
                    pairs.append((u, d))
                    st.term_coef.append(float(w) * c)
            targets.append((st.stash[m], out, pairs))
            st.merged[m] = out
        st.tables = hip.LoraTables(targets, self.device)

    # -- adapters and scales ------------------------------------------------------------------------------------------------------
    def set_adapters(self, adapter_names: Union[str, Sequence[str]], weights: Union[None, float, Sequence[float]] = None) -> None:
        """One term per named adapter per target, coef = weight * scale * alpha / r (the reference offers this through PEFT only)."""
        st = self._lora_state()
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        if weights is None or isinstance(weights, (int, float)):
            weights = [1.0 if weights is None else float(weights)] * len(names)
        weights = list(weights)
        if len(weights) != len(names) or len(set(names)) != len(names):
            raise ValueError(f"set_adapters: {len(names)} distinct names need {len(names)} weights, got {names} / {weights}")
        for n in names:
            if st is None or n not in st.adapters:
                raise ValueError(f"set_adapters: adapter {n!r} is not loaded (have {list(st.adapters) if st else []})")
        st.active = [(n, float(w)) for n, w in zip(names, weights)]
        self._lora_tables()

    def active_adapters(self) -> List[str]:
        st = self._lora_state()
        return [n for n, _ in st.active] if st else []

    def set_lora_scale(self, scale: float) -> None:
        """The scale the adapters run at when a call names none (1.0 after loading).  The pipeline sets it per call."""
        st = self._lora_state()
        if st is not None:
            st.scale = float(scale)

    def fuse_lora(self, lora_scale: float = 1.0, safe_fusing: bool = False) -> None:
        """Merge at lora_scale and pin it: later `scale` arguments have no effect (the reference's _fuse_lora drops the layer).
        safe_fusing: a non-finite merged weight raises ValueError and the device weights stay what they were."""
        st = self._lora_state()
        if st is None:
            return
        self._lora_guard()
        self._lora_apply(float(lora_scale), check=bool(safe_fusing))
        st.pinned = float(lora_scale)

    def unfuse_lora(self) -> None:
        """Back to the loaded, unpinned state.  The device weights are the base again (bit for bit: it was kept) until the next forward
        merges the active adapters at its scale, as the reference's unfused layers would apply them."""
        st = self._lora_state()
        if st is None:
            return
        st.pinned = None
        self._lora_apply(None)

    def unload_lora(self) -> None:
        """Drop every adapter, table and stash; the device weights are the base again, bit for bit."""
        st = self._lora_state()
        if st is None:
            return
        st.pinned = None
        self._lora_apply(None)
        del self.__dict__["_lora"]

    # -- merging ------------------------------------------------------------------------------------------------------------------
    def _lora_sync(self, scale: Optional[float] = None) -> None:
        """Before a forward: make the device weights those of the active adapters at the pinned scale, else `scale`, else the model's
        call scale.  Merges only when that differs from what is on the device."""
        st = self._lora_state()
        if st is None:
            return
        self._lora_apply(st.pinned if st.pinned is not None else (st.scale if scale is None else float(scale)))

    def _lora_apply(self, scale: Optional[float], check: bool = False) -> None:
        """scale None: the base.  Runs mf_lora_merge into the tables' fp32 buffers (reference layout) and re-derives the entries of
        self.P that derive from a weight that changed, and only those, by the derivation _prepare runs (HipModel._put)."""
        st = self._lora_state()
        want = None
        if scale is not None and st.tables is not None:
            coefs = torch.tensor([c * scale for c in st.term_coef], dtype=torch.float64).to(F32)
            want = (st.tables, tuple(coefs.tolist()))
        if want == st.on_device and not check:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the LoRA scale or adapter set changed inside a graph capture: merge before capturing")
        if self.training:
            raise NotImplementedError("LoRA adapters and the training layout do not mix: unload_lora() first")
        new = set()
        if want is not None:
            if want != st.on_device:
                hip.lora_merge(st.tables, coefs)
            if check and not all(bool(torch.isfinite(t).all()) for t in st.merged.values()):
                if st.on_device is not None and st.on_device[0] is st.tables:       # layouts may alias these buffers: put their values back
                    hip.lora_merge(st.tables, torch.tensor(st.on_device[1], dtype=F32))
                raise ValueError(f"fuse_lora(safe_fusing=True): the weights merged at scale {scale} are not finite; nothing was changed")
            if want == st.on_device:
                return
            new = set(st.merged)
        rebuild = new | st.device_modules
        sd = dict(self._src)
        for m in new:
            sd[m + ".weight"] = st.merged[m].view(self._src[m + ".weight"].shape)
        self._only = rebuild
        try:
            self._prepare(sd)
        finally:
            self._only = None
        st.on_device, st.device_modules, st.host_cache = want, new, {}
        self._weights_gen += 1

    def _current_weight(self, name: str) -> torch.Tensor:
        """The fp32 host value of parameter `name` as the device holds it NOW: the merged weight for a module an adapter is merged into
        (downloaded once per merge), the master copy otherwise."""
        st = self._lora_state()
        m = name[: -len(".weight")] if name.endswith(".weight") else None
        if st is None or m not in st.device_modules:
            return self._src[name]
        if m not in st.host_cache:
            st.host_cache[m] = st.merged[m].cpu().view(self._src[name].shape)
        return st.host_cache[m]

    def _lora_state_dict(self) -> Optional[Dict[str, torch.Tensor]]:
        """What state_dict() returns when fused: the merged fp32 weights (what the reference saves after fuse_lora); None otherwise."""
        st = self._lora_state()
        if st is None or st.pinned is None:
            return None
        self._lora_sync()
        return {k: (self._current_weight(k).clone() if k.endswith(".weight") else v) for k, v in self._src.items()}
