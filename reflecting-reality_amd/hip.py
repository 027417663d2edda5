"""ctypes binding of libmfhip.so (C ABI in include/mfhip.h) on top of torch-ROCm tensors.

PyTorch is used only to own device memory and the HIP stream; every arithmetic op below is a
hand-written gfx950 kernel.  There is NO fallback: if the library is missing or a call fails this
module raises, it never computes on the host or through ATen.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple, Union

import torch

from . import _build

MF_F32, MF_BF16, MF_F16X3, MF_BF16X3, MF_FP8, MF_BF16X1, MF_F16 = 0, 1, 2, 3, 4, 5, 6
FP8 = torch.float8_e4m3fn          # OCP e4m3 (gfx950's fp8), 1 byte per element
ACT_NONE, ACT_SILU, ACT_GEGLU4 = 0, 1, 2
ACT_QUICK_GELU, ACT_GELU_ERF = 3, 4      # mf_act only (the CLIP text encoders' MLP): mf_gemm_conv has no such epilogue
ABI_VERSION = 23


class MfhipError(RuntimeError):
    pass


class GemmDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int32),
        ("a0", C.c_void_p), ("a1", C.c_void_p),
        ("c0", C.c_int32), ("c1", C.c_int32),
        ("lda0", C.c_int64), ("lda1", C.c_int64),
        ("a_dtype", C.c_int32),
        ("batch", C.c_int32), ("h_in", C.c_int32), ("w_in", C.c_int32),
        ("h_out", C.c_int32), ("w_out", C.c_int32),
        ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad_t", C.c_int32), ("pad_l", C.c_int32),
        ("upsample", C.c_int32),
        ("w", C.c_void_p), ("ldw", C.c_int64), ("w_split", C.c_int32),
        ("n", C.c_int32),
        ("nz", C.c_int32), ("zdiv", C.c_int32),
        ("a_zs_o", C.c_int64), ("a_zs_i", C.c_int64), ("w_zs_o", C.c_int64), ("w_zs_i", C.c_int64),
        ("o_zs_o", C.c_int64), ("o_zs_i", C.c_int64),
        ("bias", C.c_void_p), ("bias_mode", C.c_int32),
        ("temb", C.c_void_p), ("ld_temb", C.c_int64),
        ("a_scale", C.c_void_p), ("w_scale", C.c_void_p), ("a_scale_zs", C.c_int64), ("w_scale_zs", C.c_int64),
        ("res0", C.c_void_p), ("res0_dtype", C.c_int32), ("ld_res0", C.c_int64),
        ("res1", C.c_void_p), ("res1_dtype", C.c_int32), ("ld_res1", C.c_int64), ("res1_rows", C.c_int32),
        ("alpha", C.c_float), ("act", C.c_int32),
        ("out", C.c_void_p), ("out_dtype", C.c_int32), ("ldc", C.c_int64),
        ("splitk", C.c_int32), ("ws", C.c_void_p), ("ws_floats", C.c_int64),
        ("tile", C.c_int32),
        ("ln_colsum", C.c_void_p), ("ln_eps", C.c_float),
        ("vt_out", C.c_void_p), ("vt_n0", C.c_int32), ("vt_tokens", C.c_int32), ("vt_ld", C.c_int64),
        ("sk_tickets", C.c_void_p), ("sk_ticket_cap", C.c_int32),
        ("gn_part", C.c_void_p), ("gn_part_floats", C.c_int64), ("gn_part_rows", C.c_void_p),
        ("gn_groups", C.c_int32), ("gn_grouped", C.c_void_p),
        ("defer_reduce", C.c_int32), ("deferred_splits", C.c_void_p),
    ]


class GemmPlan(C.Structure):
    """mf_gemm_plan: what mf_gemm_conv would do with a descriptor (mf_gemm_conv_plan; decided on the host, nothing is launched)."""
    _fields_ = [(f, C.c_int32) for f in "tile splitk tiles_per_block blocks reduce_launch deferred_splits gn_part_rows gn_grouped".split()]


class WgradDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int32),
        ("a0", C.c_void_p), ("a1", C.c_void_p),
        ("c0", C.c_int32), ("c1", C.c_int32),
        ("lda0", C.c_int64), ("lda1", C.c_int64),
        ("batch", C.c_int32), ("h_in", C.c_int32), ("w_in", C.c_int32), ("h_out", C.c_int32), ("w_out", C.c_int32),
        ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad_t", C.c_int32), ("pad_l", C.c_int32),
        ("upsample", C.c_int32),
        ("dy", C.c_void_p), ("lddy", C.c_int64),
        ("n", C.c_int32),
        ("dw", C.c_void_p), ("lddw", C.c_int64),
        ("accumulate", C.c_int32), ("splitm", C.c_int32),
        ("ws", C.c_void_p), ("ws_floats", C.c_int64),
    ]


class WgradPlan(C.Structure):
    """mf_wgrad_plan: what mf_conv_wgrad would do with a descriptor (mf_conv_wgrad_plan; decided on the host, nothing is launched).
    form: 0 fp32, 1 128-wide register-staged, 2 160-wide, 3 128-wide LDS-DMA."""
    _fields_ = [(f, C.c_int32) for f in "form tile_w tiles splitm m_per_split reduce_launch slabs_xcd blocks threads lds_bytes".split()]


class GroupNormBwdDesc(C.Structure):
    _fields_ = [
        ("x0", C.c_void_p), ("x1", C.c_void_p), ("c0", C.c_int32), ("c1", C.c_int32),
        ("dy", C.c_void_p),
        ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("dx0", C.c_void_p), ("dx1", C.c_void_p),
        ("dgamma_part", C.c_void_p), ("dbeta_part", C.c_void_p),
        ("batch", C.c_int32), ("hw", C.c_int32), ("groups", C.c_int32), ("silu", C.c_int32),
        ("eps", C.c_float),
        ("ws", C.c_void_p),
        ("dgamma_acc", C.c_void_p), ("dbeta_acc", C.c_void_p),
        ("add0", C.c_void_p), ("add1", C.c_void_p),
        ("stats_in", C.c_void_p),
    ]


class AttnBwdDesc(C.Structure):
    _fields_ = [
        ("q_hi", C.c_void_p), ("q_lo", C.c_void_p), ("ldq", C.c_int64),
        ("k_hi", C.c_void_p), ("k_lo", C.c_void_p), ("ldk", C.c_int64),
        ("v_hi", C.c_void_p), ("v_lo", C.c_void_p), ("ldv", C.c_int64),
        ("do_hi", C.c_void_p), ("do_lo", C.c_void_p), ("lddo", C.c_int64),
        ("qt_hi", C.c_void_p), ("qt_lo", C.c_void_p), ("ldqt", C.c_int64),
        ("kt_hi", C.c_void_p), ("kt_lo", C.c_void_p), ("ldkt", C.c_int64),
        ("dot_hi", C.c_void_p), ("dot_lo", C.c_void_p), ("lddot", C.c_int64),
        ("lse", C.c_void_p), ("dd", C.c_void_p),
        ("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p), ("ldo", C.c_int64),
        ("batch", C.c_int32), ("heads", C.c_int32), ("sq", C.c_int32), ("skv", C.c_int32), ("head_dim", C.c_int32),
        ("scale", C.c_float), ("out_dtype", C.c_int32),
    ]


class GroupNormDesc(C.Structure):
    _fields_ = [
        ("x0", C.c_void_p), ("x1", C.c_void_p),
        ("c0", C.c_int32), ("c1", C.c_int32),
        ("in_dtype", C.c_int32),
        ("batch", C.c_int32), ("hw", C.c_int32),
        ("groups", C.c_int32),
        ("eps", C.c_float),
        ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("silu", C.c_int32),
        ("out", C.c_void_p), ("out_dtype", C.c_int32),
        ("ws", C.c_void_p), ("stats_out", C.c_void_p),
        ("part0", C.c_void_p), ("part0_rows", C.c_int32), ("part1", C.c_void_p), ("part1_rows", C.c_int32),
        ("grp0", C.c_void_p), ("grp0_rows", C.c_int32),
        ("sk_ws", C.c_void_p), ("sk_splits", C.c_int32),
        ("sk_bias", C.c_void_p), ("sk_temb", C.c_void_p), ("sk_ld_temb", C.c_int64), ("sk_alpha", C.c_float),
    ]


class GnPlan(C.Structure):
    """mf_gn_plan: what mf_groupnorm would do with a descriptor (mf_groupnorm_plan; decided on the host, nothing is launched).
    form: 0 one-launch slab, 1 own statistics pass, 2 the producers' per-channel sums, 3 the producer's per-group sums."""
    _fields_ = [(f, C.c_int32) for f in ("form launches vec finalize centered chunks rows_per_chunk rows_per_block blocks threads lds_bytes "
                                         "finalize_parts").split()]


SCHED_MAX_OPS, SCHED_MAX_TERMS, SCHED_MAX_REGS = 8, 6, 16       # include/mfhip.h MF_SCHED_MAX_*


class SchedOp(C.Structure):
    _fields_ = [("dst", C.c_int32), ("nterms", C.c_int32), ("src", C.c_int32 * SCHED_MAX_TERMS), ("coef", C.c_float * SCHED_MAX_TERMS)]


class MetricsRow(C.Structure):
    """mf_metrics_row: what mf_image_metrics writes per image (device memory; metrics.py finishes PSNR / SSIM from it in float64)."""
    _fields_ = [("sq_err", C.c_int64), ("count", C.c_int64), ("ssim_sum", C.c_double),
                ("pred_min", C.c_int32), ("pred_max", C.c_int32), ("target_min", C.c_int32), ("target_max", C.c_int32)]


class SchedRow(C.Structure):
    """mf_sched_row: one denoise step of a multistep scheduler for mf_sched_step_dev (built by schedulers.device_plan)."""
    _fields_ = [("nops", C.c_int32), ("nslots", C.c_int32), ("load", C.c_uint32), ("store", C.c_uint32),
                ("ops", SchedOp * SCHED_MAX_OPS)]


class LoraTarget(C.Structure):
    """mf_lora_target: one weight of mf_lora_merge's target table (a host copy for the entry's checks, a device copy for the kernel)."""
    _fields_ = [("base", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32),
                ("first_term", C.c_int32), ("nterms", C.c_int32), ("first_tile", C.c_int64)]


class LoraTerm(C.Structure):
    """mf_lora_term: one up / down pair of mf_lora_merge's term table."""
    _fields_ = [("up", C.c_void_p), ("down", C.c_void_p), ("rank", C.c_int32), ("reserved", C.c_int32)]


# The C ABI, once: every function include/mfhip.h declares, as "<return kind>:<one kind per parameter>" (the stream included).
# p pointer (device or host memory, an opaque handle, a C string), i int / int32_t, l int64_t, f float; returns also s (const char*) and
# v (void); one letter per host descriptor struct (DESC_KINDS), so that a descriptor parameter takes a pointer to ITS struct only.
# load() turns the table into argtypes / restype, so ctypes converts plain Python values and refuses the wrong ones before the library
# is entered; program.py derives the recorder's signatures from it; tests/test_abi.py checks it against the header's prototypes in full.
# A new entry is its prototype in mfhip.h and its line here.
DESC_KINDS = {"G": GemmDesc, "P": GemmPlan, "N": GroupNormDesc, "A": AttnBwdDesc, "W": WgradDesc, "Q": WgradPlan, "B": GroupNormBwdDesc,
              "R": GnPlan}
SIGNATURES = {
    "mf_abi_version": "i:", "mf_last_error": "s:", "mf_sizeof_gemm_desc": "i:", "mf_sizeof_groupnorm_desc": "i:",
    "mf_gemm_conv": "i:Gp", "mf_gemm_conv_plan": "i:GP", "mf_sizeof_gemm_plan": "i:", "mf_gemm_num_tiles": "i:", "mf_gemm_tile_shape": "i:ipp",
    "mf_gemm_tile_table_version": "i:", "mf_groupnorm": "i:Np", "mf_groupnorm_ws_floats": "l:iii", "mf_groupnorm_slab_applies": "i:iii",
    "mf_groupnorm_plan": "i:NR", "mf_sizeof_gn_plan": "i:",
    "mf_layernorm": "i:pipipplifp", "mf_softmax_rows": "i:ppiliip",
    "mf_attention_bf16": "i:plplplpliiiiifp", "mf_attention_f16": "i:plplplpliiiiifp",
    "mf_attention_f16x3": "i:pplpplpplpliiiiifp", "mf_attention_f16x3_lse": "i:pplpplpplplpiiiiifp", "mf_attention_causal_bf16": "i:plplplpliiiiifp",
    "mf_attention_causal_f16": "i:plplplpliiiiifp", "mf_attention_causal_f16x3": "i:pplpplpplpliiiiifp",
    "mf_softmax_rows_causal": "i:ppiliiip", "mf_embed_tokens": "i:pppipiiiiip", "mf_act": "i:ppiilp", "mf_sizeof_attn_bwd_desc": "i:",
    "mf_attention_bwd_f16x3": "i:Ap", "mf_rowdot_heads": "i:pppiiiilp",
    "mf_attention_bwd_bf16": "i:Ap", "mf_attention_bf16_lse": "i:plplplplpiiiiifp", "mf_rowdot_heads_bf16": "i:pppiiiilp",
    "mf_cast_bf16_colsum": "i:ppiliplipipp", "mf_cast_bf16_colsum_ws_floats": "l:ili",
    "mf_transpose_bf16_bf16": "i:ppiiillllp", "mf_geglu_bwd_bf16": "i:ppplippp", "mf_geglu_bwd_bf16_ws_floats": "l:li",
    "mf_rowdot_heads_cast": "i:ppppiiiip", "mf_debug_set_wgrad_dma": "v:i", "mf_zero_ranges": "i:pppip",
    "mf_split_halves": "i:ppplp", "mf_split_overflow": "i:ipp", "mf_quantize_rows_fp8": "i:pipplippfp",
    "mf_pack_nhwc": "i:pipipiiiip", "mf_unpack_nchw": "i:pilpiiip", "mf_add": "i:pipipilp", "mf_cast_bf16": "i:pplp", "mf_geglu": "i:pipilip",
    "mf_timestep_embedding": "i:ppiiifp", "mf_silu_f32": "i:pplp",
    "mf_cfg_ddim_step": "i:ppfppffffifplp", "mf_cfg_ddim_step_dev": "i:ppfpppiflp", "mf_cfg_combine": "i:ppfplp", "mf_axpby_n": "i:ppiplp",
    "mf_sizeof_sched_row": "i:", "mf_sched_step_dev": "i:ppfppplp", "mf_mse_loss": "i:pppppilp", "mf_vae_sample": "i:pilppiiifp",
    "mf_nearest_resize": "i:ppiiiiip",
    # decoupled cross-attention (ABI 23)
    "mf_attention_ip_bf16": "i:plplplplplpliiiiiiffp", "mf_attention_ip_f16": "i:plplplplplpliiiiiiffp",
    "mf_attention_ip_f16x3": "i:pplpplpplpplpplpliiiiiiffp", "mf_freq_encode": "i:ppiiifp",
    "mf_masked_mean_normal": "i:ppplp",
    # image front-end (csrc/frontend.hip)
    "mf_minmax_ws_floats": "l:", "mf_minmax": "i:pplppp", "mf_image_normalize": "i:pplpp", "mf_mask_keep": "i:ppiilp",
    "mf_concat_channels": "i:pppipilp", "mf_postprocess": "i:pppiilip",
    "mf_depth_normalize": "i:ppplffipp", "mf_select_ws_bytes": "l:", "mf_select_ranks": "i:plpippp", "mf_depth_percentile_normalize": "i:pplpffippp",
    "mf_bicubic_resize_crop": "i:ppiiiiiiiiiffp", "mf_bicubic_aa_resize_crop": "i:ppiiiiiiiiiffp", "mf_hwc_to_chw_affine": "i:ppliffp",
    "mf_u8_to_planes": "i:ppiiilp",
    # the training batch (csrc/train_batch.hip)
    "mf_train_example_u8": "i:ppppppiiiip", "mf_masked_image_u8": "i:pppliip", "mf_fliplr": "i:ppliip",
    "mf_train_batch_assemble": "i:ppiiliiiifpppppipppiiippppppp",
    # tiled VAE encode / decode (csrc/vae_tile.hip)
    "mf_crop_pack_nhwc": "i:piiiiiiiipiiiip", "mf_vae_tile_blend": "i:pppiiiiiiiliiipiiiiip",
    # image scoring (csrc/metrics.hip)
    "mf_sizeof_metrics_row": "i:", "mf_image_metrics_ws_bytes": "l:iiii", "mf_image_metrics": "i:pppiiiiifppp",
    # CLIP image side and score (csrc/clip_vision.hip)
    "mf_clip_preprocess_ws_bytes": "l:iiiii", "mf_clip_preprocess": "i:piiiiiiipipiffffffpiippp", "mf_clip_vision_embed": "i:pppipiiiip",
    "mf_clip_score": "i:ppiippp",
    # LPIPS (csrc/lpips.hip)
    "mf_lpips_ws_bytes": "l:i", "mf_lpips_prepare": "i:pppiiiiiipip", "mf_relu": "i:pililp", "mf_maxpool3s2_ceil": "i:ppiiiiip",
    "mf_lpips_layer": "i:pipiliipp", "mf_lpips_finish": "i:pipp",
    # training (csrc/train.hip)
    "mf_sizeof_wgrad_desc": "i:", "mf_conv_wgrad_ws_floats": "l:W", "mf_conv_wgrad": "i:Wp", "mf_conv_wgrad_plan": "i:WQ",
    "mf_sizeof_wgrad_plan": "i:", "mf_split_pack": "i:plpliip",
    "mf_transpose": "i:ppiiillllp", "mf_transpose_bf16": "i:ppiiillllp", "mf_colsum_ws_floats": "l:ili", "mf_colsum": "i:plpliliipp",
    "mf_sizeof_groupnorm_bwd_desc": "i:", "mf_groupnorm_bwd": "i:Bp", "mf_groupnorm_bwd_ws_floats": "l:iiii", "mf_groupnorm_bwd_streams": "i:iiii",
    "mf_layernorm_bwd": "i:pppppplifpp", "mf_layernorm_bwd_parts": "l:l", "mf_softmax_bwd": "i:pppliifp", "mf_silu_bwd": "i:ppplp",
    "mf_geglu_bwd": "i:ppplip", "mf_zero_insert2x": "i:ppiiiip", "mf_sumpool2x2": "i:ppiiiip", "mf_mse_grad": "i:ppppilp",
    "mf_sumsq_ws_doubles": "l:", "mf_sumsq": "i:plpipp", "mf_clip_coef": "i:pffppp", "mf_adamw": "i:pppplfffffipp",
    # step programs (csrc/program.hip; program.py records them)
    "mf_memcpy2d": "i:plplllp", "mf_memset": "i:pilp", "mf_program_load": "i:plp", "mf_program_destroy": "v:p", "mf_program_num_buffers": "i:p",
    "mf_program_buffer_info": "i:pipppp", "mf_program_find_buffer": "i:pp", "mf_program_bind": "i:pip", "mf_program_num_calls": "i:p",
    "mf_program_meta": "s:p", "mf_program_run": "i:pp", "mf_denoise_step_fused": "i:pppppp", "mf_unet_forward": "i:ppppipp",
    "mf_brushnet_forward": "i:pppppip", "mf_vae_decode": "i:pppp", "mf_vae_encode_moments": "i:pppp",
    # the two ends of a call as step programs (program.export_encode_prompt / pipeline.export_conditioning / export_vae_decode(postprocess=True))
    "mf_encode_prompt": "i:pppp", "mf_build_conditioning": "i:ppppppp", "mf_decode_image": "i:pppp",
    # random numbers (csrc/rng.hip)
    "mf_philox_normal_blocks": "l:ll", "mf_philox_int_blocks": "l:l", "mf_philox_bits_host": "i:plll", "mf_philox_bits": "i:plllpp",
    "mf_philox_normal": "i:pllfllllpp", "mf_philox_randint": "i:pllllllpp", "mf_philox_advance": "i:plp",
    "mf_train_batch_draw": "i:pipplllllllpp",
    # the multistep update with per-step noise drawn in the kernel (csrc/elementwise.hip; DPM-Solver++ SDE)
    "mf_sched_step_noise_dev": "i:ppfppplilllllpp",
    # LoRA adapters merged on the device (csrc/lora.hip)
    "mf_sizeof_lora_target": "i:", "mf_sizeof_lora_term": "i:", "mf_lora_tiles": "l:ii", "mf_lora_merge": "i:pppppiip",
    # the upsampled 3x3 conv as four 2x2 phase convs in one launch (csrc/gemm_conv.hip)
    "mf_conv_up2x": "i:Gp", "mf_conv_up2x_plan": "i:GP",
}
EXPORTS = list(SIGNATURES)
# (struct, the entry that reports its sizeof in the library) — load() refuses a binding whose layout differs
_LAYOUTS = ((GemmDesc, "mf_sizeof_gemm_desc"), (GroupNormDesc, "mf_sizeof_groupnorm_desc"), (AttnBwdDesc, "mf_sizeof_attn_bwd_desc"),
            (WgradDesc, "mf_sizeof_wgrad_desc"), (GroupNormBwdDesc, "mf_sizeof_groupnorm_bwd_desc"), (SchedRow, "mf_sizeof_sched_row"),
            (MetricsRow, "mf_sizeof_metrics_row"), (GemmPlan, "mf_sizeof_gemm_plan"), (WgradPlan, "mf_sizeof_wgrad_plan"),
            (GnPlan, "mf_sizeof_gn_plan"), (LoraTarget, "mf_sizeof_lora_target"), (LoraTerm, "mf_sizeof_lora_term"))
_CTYPES = {"p": C.c_void_p, "i": C.c_int32, "l": C.c_int64, "f": C.c_float, "s": C.c_char_p, "v": None,
           **{kind: C.POINTER(struct) for kind, struct in DESC_KINDS.items()}}

_lib: Optional[C.CDLL] = None
_RECORDER = None        # program.Recorder's proxy while a step program is being recorded: every launch goes through it


def lib_path() -> str:
    # MFHIP_LIB: a developer build of the same sources (e.g. the stamped one of tools/stamps.py); never set in production
    return os.environ.get("MFHIP_LIB") or _build.LIB_PATH


def load() -> C.CDLL:
    """Load libmfhip.so (after torch, so that its libamdhip64.so.7 is the one HIP runtime in-process)."""
    global _lib
    if _RECORDER is not None:
        return _RECORDER
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise MfhipError(
            f"{path} not found: the HIP extension has not been built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (needs hipcc). There is no CPU fallback for the MirrorFusion hot path.")
    lib = C.CDLL(path)
    for name, sig in SIGNATURES.items():      # (symbols beyond the table — a developer build's — stay untyped)
        fn = getattr(lib, name, None)
        if fn is None:
            raise MfhipError(f"{path} does not export {name}, which include/mfhip.h declares: rebuild the library")
        ret, _, params = sig.partition(":")
        fn.restype, fn.argtypes = _CTYPES[ret], [_CTYPES[kind] for kind in params]
    if lib.mf_abi_version() != ABI_VERSION:
        raise MfhipError(f"libmfhip ABI {lib.mf_abi_version()} != binding ABI {ABI_VERSION}: rebuild the library")
    for struct, sizeof in _LAYOUTS:
        if getattr(lib, sizeof)() != C.sizeof(struct):
            raise MfhipError(f"{struct.__name__} layout mismatch between mfhip.h ({sizeof}) and the ctypes binding")
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise MfhipError(f"{what} failed (rc={rc}): {load().mf_last_error().decode()}")


def dt_code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return MF_F32
    if dtype == torch.bfloat16:
        return MF_BF16
    if dtype == torch.float16:
        return MF_F16
    if dtype == FP8:
        return MF_FP8
    raise MfhipError(f"unsupported dtype {dtype}")


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _launch(entry: str, *args) -> None:
    """lib.<entry>(*args, current stream), raising on a non-zero return.  A tensor stands for its address (None: a null pointer); it is
    resolved HERE, so the library object — or the Recorder's proxy in its place — only ever sees addresses, ints, floats and ctypes objects."""
    fn = getattr(load(), entry)
    kinds = SIGNATURES[entry][2:]         # (only a pointer parameter takes a tensor: elsewhere ctypes converts or refuses it, as it always did)
    _check(fn(*[a.data_ptr() if k == "p" and isinstance(a, torch.Tensor) else a for a, k in zip(args, kinds)], _stream()), entry)


def _req_cuda(*ts: Optional[torch.Tensor]) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise MfhipError("libmfhip ops need device tensors (there is no CPU path)")
        if t is not None and getattr(t, "_sk_pending", None) is not None:
            raise MfhipError("a tensor whose split-K reduce was deferred (gemm_conv(defer_reduce=True)) reached an op other than the "
                             "groupnorm() it was promised to: its memory has not been written")


# ---- scratch buffers (split-K slabs, GroupNorm statistics) -------------------------------------
_scratch: dict = {}


def scratch(name: str, nfloats: int, device) -> torch.Tensor:
    # one buffer per (purpose, device, stream): launches on different streams may run concurrently
    key = (name, torch.device(device).index, torch.cuda.current_stream(device).cuda_stream)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nfloats:
        buf = torch.empty(max(nfloats, 1), dtype=torch.float32, device=device)
        _scratch[key] = buf
    return buf


# tiles whose kernels carry the in-launch combine (csrc/gemm_conv.hip: tile_has_skf), per compute code
SK_FUSED_TILES = {MF_BF16: (1, 2, 3, 6, 41, 43, 44, 48), MF_F16X3: (1, 2, 3, 6, 41, 44)}
SK_TICKETS = 8192          # arrival counters of the in-launch split-K combine (mf_gemm_desc.sk_tickets), per stream
SK_STREAMS = 64
_tickets: dict = {}        # device index -> ([SK_STREAMS, SK_TICKETS] zeroed int32, {stream id: row})


def sk_tickets(device) -> torch.Tensor:
    """The zeroed ticket row of the current stream.  Launches on different streams may run concurrently, so every stream owns
    a row of one per-device table; the kernels leave their tickets zeroed, so the table is cleared once, when it is allocated —
    outside any graph capture (a capture stream only picks a row: no allocation, no memset node)."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    ent = _tickets.get(idx)
    if ent is None:
        if torch.cuda.is_current_stream_capturing():
            raise MfhipError("the split-K ticket table must exist before a graph capture (run the step eagerly once)")
        ent = _tickets[idx] = (torch.zeros(SK_STREAMS, SK_TICKETS, dtype=torch.int32, device=dev), {})
    table, rows = ent
    sid = torch.cuda.current_stream(dev).cuda_stream
    row = rows.get(sid)
    if row is None:
        if len(rows) >= SK_STREAMS:
            raise MfhipError(f"more than {SK_STREAMS} streams issued split-K GEMMs on device {idx}")
        row = rows[sid] = len(rows)
    return table[row]


_staging: dict = {}


def h2d(t: torch.Tensor, device) -> torch.Tensor:
    """Host tensor -> device through a persistent pinned staging buffer.  A freshly allocated pageable tensor
    (every preprocessing result is one) pays page faults + driver pinning on a direct .to(device): 12.6 MB took
    31 ms on the MI355X host, 10x the rest of the conditioning build.  Device tensors pass through."""
    if t.device.type != "cpu":
        return t.to(device)
    t = t.contiguous()
    nbytes = t.numel() * t.element_size()
    if nbytes < (1 << 16):
        return t.to(device)
    key = torch.device(device).index
    buf = _staging.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 24), dtype=torch.uint8, pin_memory=True)
        _staging[key] = buf
    stage = buf[:nbytes].view(t.dtype).view(t.shape)
    stage.copy_(t)
    out = stage.to(device, non_blocking=True)
    torch.cuda.current_stream(device).synchronize()      # the staging buffer is reused by the next call
    return out


SPLITK_WS_FLOATS = 16 * 1024 * 1024  # 64 MiB of fp32 slabs

# Optional live profiler used by bench.py: when PROFILE is a list, every mf_gemm_conv launch is bracketed by
# HIP events on the launch stream and appended as (start_event, end_event, algorithmic_flops).
PROFILE = None


PROFILE_ATTN_FLOPS = 0.0      # 4 * batch * heads * Sq * Skv * d of every flash-attention launch between profile_begin / profile_end


def profile_begin():
    global PROFILE, PROFILE_ATTN_FLOPS
    PROFILE = []
    PROFILE_ATTN_FLOPS = 0.0


def profile_end():
    """Returns (n_launches, total_seconds, total_flops) for the bracketed mf_gemm_conv launches."""
    global PROFILE
    rec, PROFILE = PROFILE, None
    torch.cuda.synchronize()
    global LAST_PROFILE
    LAST_PROFILE = [(a.elapsed_time(b) * 1e-3, f, k) for a, b, f, k in rec]
    secs = sum(t for t, _, _ in LAST_PROFILE)
    return len(rec), secs, float(sum(f for _, f, _ in LAST_PROFILE))


LAST_PROFILE = []


# ---- per-shape autotuning of (tile, split-K) ---------------------------------------------------------
# The library's heuristic is only a prior; the host times every instantiated tile (and a few split-K factors
# for grids that cannot fill 256 CUs) the first time a GEMM shape is seen and remembers the winner.  Winners
# are persisted in tune_cache.json next to this file so later processes (and graph capture) start tuned.
AUTOTUNE = os.environ.get("MFHIP_AUTOTUNE", "1") != "0"
# Offer the in-launch split-K combine (mf_gemm_desc.sk_tickets) to the tuner.  OFF by default: measured on MI355X (tools/bench_skf.py,
# profiles/r04_splitk_in_launch.txt) the last-arriver form with an agent-scope release per block is 8-15 us SLOWER than the reduce
# launch it replaces on every small-M shape of the step (each block's release writes back its XCD's L2: ~45 ns per block, serialised).
SK_FUSED = os.environ.get("MFHIP_SK_FUSED", "0") == "1"
# Route the 1x1 GEMMs whose blocks would walk >= 2 output tiles to the persistent tile 70 instead of the cached tile.  A/B switch.
PREFER_PERS = os.environ.get("MFHIP_PREFER_PERS", "1") != "0"
PERS_TILE = 70
PERS_MIN_NLOOP = int(os.environ.get("MFHIP_PERS_MIN_NLOOP", "2"))


def gn_slab_applies(hw: int, c: int, groups: int) -> bool:
    """Whether mf_groupnorm runs its one-launch form on [*, hw, c] in `groups` groups, one segment (csrc/norm.hip, the dispatch of
    gn_slab_kernel) — the form a deferred split-K reduce needs (mf_groupnorm_desc.sk_ws).  The library's own predicate."""
    return bool(load().mf_groupnorm_slab_applies(hw, c, groups))


def _route_pers(d: GemmDesc) -> bool:
    """Sends the call to the persistent tile 70 when the library's plan accepts it there (mf_gemm_conv_plan: nothing is launched) AND
    its grid gives every block at least PERS_MIN_NLOOP output tiles; otherwise the descriptor's tile / split-K stay as they were."""
    tile, splitk = d.tile, d.splitk
    d.tile, d.splitk = PERS_TILE, 1
    plan = GemmPlan()
    if load().mf_gemm_conv_plan(C.byref(d), C.byref(plan)) == 0 and plan.tiles_per_block >= PERS_MIN_NLOOP:
        return True
    d.tile, d.splitk = tile, splitk
    return False


def pers_linear(m: int, n: int, k: int, dtype: torch.dtype) -> bool:
    """Would a plain Linear of this shape (16-bit, no time embedding, at most one residual) go to the persistent tile 70?  models.py asks
    before it picks a form only that tile serves well (a LayerNorm folded into the GEGLU projection)."""
    if not PREFER_PERS or dtype not in (torch.bfloat16, torch.float16):
        return False
    addr = 1 << 20        # a 16-byte aligned stand-in for a0 / w / out: a plan never reads through them
    d = GemmDesc(a0=addr, w=addr, out=addr, c0=k, lda0=k, ldw=k, batch=m, h_in=1, w_in=1, h_out=1, w_out=1, kh=1, kw=1,
                 stride=1, n=n, ldc=n, nz=1, zdiv=1, alpha=1.0)
    d.dtype = d.a_dtype = d.out_dtype = dt_code(dtype)
    return _route_pers(d)


# GroupNorm statistics from the producing GEMM's epilogue (mf_gemm_desc.gn_part -> mf_groupnorm_desc.part0 / part1).  A/B switch.
DEFER_REDUCE = os.environ.get("MFHIP_DEFER_REDUCE", "1") != "0"     # A/B switch: a resnet's conv1 leaves its split-K reduce to norm2
GN_FROM_PARTS = os.environ.get("MFHIP_GN_FROM_PARTS", "1") != "0"
GN_FROM_GROUPS = os.environ.get("MFHIP_GN_FROM_GROUPS", "1") != "0"     # ... per-group sums: no finalize launch either.  A/B switch.
RETUNE = os.environ.get("MFHIP_RETUNE", "0") == "1"      # developer switch: re-measure every shape once (new tiles were added)
TUNE_GRAPH = os.environ.get("MFHIP_TUNE_GRAPH", "0") == "1"   # developer switch: time candidates from a hipGraph (see _tuned_config)
TUNE_LOG: Optional[dict] = None     # developer hook (tools/tune_step.py): every candidate's time of every key tuned while it is a dict
KEY_LOG: Optional[list] = None      # developer hook: the tune key of every autotuned mf_gemm_conv call while it is a list
# Where in the denoise step a call sits ("b": BrushNet, on the side stream under the UNet's encoder; "e": UNet encoder + mid block;
# "d": UNet decoder, alone on the chip once BrushNet has finished).  The best tile for one shape differs between them — a tile that
# leaves room for the other stream's blocks wins under overlap, a whole-CU ring tile wins alone (tools/tune_step.py) — so the tune
# cache may hold "<key>@<ctx>" entries beside the plain one; a missing tagged entry falls back to the plain key.
TUNE_CTX: Optional[str] = None
_NO_TUNE_CTX = os.environ.get("MFHIP_NO_TUNE_CTX", "0") == "1"     # A/B switch: ignore the position-tagged entries
# The package ships a cache tuned on MI355X (read-only); new winners go to a per-user file (MFHIP_TUNE_CACHE, default
# ~/.cache/mfhip/tune_cache.json) that is overlaid on it.  Both carry the library's tile-table version: when tiles are
# renumbered (mf_gemm_tile_table_version changes) stale indices are dropped instead of being trusted.
_TUNE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tune_cache.json")
_tune: Optional[dict] = None
_tune_new: dict = {}
_tune_misses = 0


def tune_user_path() -> str:
    return os.environ.get("MFHIP_TUNE_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "mfhip", "tune_cache.json")


def _tune_read(path: str, version: int) -> dict:
    import json
    try:
        with open(path) as f:
            raw = json.load(f)
        if not isinstance(raw, dict) or raw.get("_meta", {}).get("tile_table") != version:
            return {}
        return {k: tuple(v) for k, v in raw.get("entries", {}).items()}
    except (OSError, ValueError, TypeError, AttributeError):
        return {}


def _tune_load() -> dict:
    global _tune
    if _tune is None:
        version = load().mf_gemm_tile_table_version()
        _tune = _tune_read(_TUNE_PATH, version)
        _tune.update(_tune_read(tune_user_path(), version))
    return _tune


def tune_save(path: Optional[str] = None) -> None:
    """Persist the winners found by this process (merged over what the user file already holds): written to a temporary
    file and renamed, so a concurrent reader never sees half a file."""
    if not _tune_new:
        return
    import json
    import tempfile
    path = path or tune_user_path()
    version = load().mf_gemm_tile_table_version()
    merged = _tune_read(path, version)
    merged.update(_tune_new)
    try:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        fd, tmp = tempfile.mkstemp(dir=os.path.dirname(path) or ".", suffix=".tmp")
        with os.fdopen(fd, "w") as f:
            json.dump({"_meta": {"tile_table": version}, "entries": {k: list(v) for k, v in sorted(merged.items())}}, f, indent=0)
        os.replace(tmp, path)
    except OSError:
        pass


def tune_reload() -> None:
    """Drop the in-memory cache: the next lookup re-reads the shipped file and the per-user file (another rank of this node may
    just have written its winners there: distributed.tuned_once)."""
    global _tune
    _tune = None


def _tune_forget(ks: str) -> None:
    _tune_load().pop(ks, None)
    _tune_new.pop(ks, None)


def _tune_key(key: tuple) -> str:
    return ",".join(x if isinstance(x, str) else str(int(x)) for x in key)


def _tuned_config(d: "GemmDesc", key: tuple):
    cache = _tune_load()
    ks = _tune_key(key)
    hit = cache.get(ks)
    if hit is not None and not (RETUNE and ks not in _tune_new):
        return hit
    if torch.cuda.is_current_stream_capturing() or _RECORDER is not None:
        return (0, 0)           # (a recorded pass, like a capture, must not contain the tuner's trial launches: warm up first)
    lib = load()
    global _tune_misses
    _tune_misses += 1
    if _tune_misses == 1 and os.environ.get("RANK") is not None:
        # multi-rank cold start: every rank measures its own misses (the shipped tune_cache.json covers the benchmark's shapes,
        # so this only shows for new shapes); harmless for results — tiles differ in speed, not in arithmetic order per tile
        import sys
        print(f"[mfhip] rank {os.environ['RANK']}: GEMM shape {ks} is not in the tune cache; autotuning on this rank "
              f"(further misses are tuned silently; winners go to {tune_user_path()})", file=sys.stderr, flush=True)
    m, n, k = key[2], key[3], key[4]
    es = 2 if key[0] in (MF_BF16, MF_F16) else 1 if key[0] == MF_FP8 else 4
    nkt = (k * es + 127) // 128
    cands = []
    ntiles = lib.mf_gemm_num_tiles()
    bm, bn = C.c_int(), C.c_int()
    for t in range(1, ntiles + 1):
        lib.mf_gemm_tile_shape(t, C.byref(bm), C.byref(bn))
        blocks = -(-m // bm.value) * -(-n // bn.value) * key[9]
        sks = [1]
        if blocks < 512 and nkt >= 8 and not key[10]:
            sks += [s for s in (2, 3, 4, 6, 8, 12, 16, 24) if s <= nkt // 4 and blocks * s <= 2048
                    and s * key[9] * m * n <= d.ws_floats]
        cands += [(t, s, 0) for s in sks]
        # the in-launch combine (mode 1: the last-arriving K slice reduces; no second launch) makes a split of 2-4 cheap
        # enough for grids of up to 512 tiles and K of 4+ tiles
        if SK_FUSED and not key[10] and t in SK_FUSED_TILES.get(key[0], ()):
            cands += [(t, s, 1) for s in (2, 3, 4, 6, 8, 12, 16) if s <= max(nkt // 2, 1) and blocks <= SK_TICKETS and blocks * s <= 2048
                      and nkt >= 4 and s * key[9] * m * n <= d.ws_floats]
    best, best_t = (0, 0, 0), float("inf")
    st = _stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tk = sk_tickets(torch.device("cuda", torch.cuda.current_device()))
    for t, s, mode in cands:
        d.tile, d.splitk = t, s
        d.sk_tickets, d.sk_ticket_cap = (tk.data_ptr(), tk.numel()) if mode else (None, 0)
        if lib.mf_gemm_conv(C.byref(d), st) != 0:
            continue
        dt = float("inf")
        if TUNE_GRAPH:
            # developer re-tune: 8 launches replayed from a hipGraph, so that launches shorter than a ctypes call
            # (~16 us) are ranked by their kernel time, not by the host's launch rate (slow: a capture per candidate)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                cs = _stream()
                for _ in range(8):
                    lib.mf_gemm_conv(C.byref(d), cs)
            g.replay()
            for _trial in range(2):
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                dt = min(dt, e0.elapsed_time(e1))
            del g
        else:
            for _trial in range(2):      # best of two bursts: one burst alone mis-ranks candidates that are within a few %
                e0.record()
                for _ in range(4):
                    lib.mf_gemm_conv(C.byref(d), st)
                e1.record()
                e1.synchronize()
                dt = min(dt, e0.elapsed_time(e1))
        if TUNE_LOG is not None:
            TUNE_LOG.setdefault(ks, []).append((dt, t, s, mode))
        if dt < best_t:
            best, best_t = (t, s, mode), dt
    cache[ks] = best
    _tune_new[ks] = best
    return best


def gemm_conv(a0: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, dtype, w_split: int = 0,
              c0: int, lda0: int, batch: int, h_in: int, w_in: int, h_out: int, w_out: int,
              kh: int = 1, kw: int = 1, stride: int = 1, pad_t: int = 0, pad_l: int = 0, upsample: bool = False,
              a1: Optional[torch.Tensor] = None, c1: int = 0, lda1: int = 0,
              ldw: Optional[int] = None, n: int, ldc: Optional[int] = None,
              bias: Optional[torch.Tensor] = None, bias_mode: int = 0,
              temb: Optional[torch.Tensor] = None, ld_temb: int = 0,
              res0: Optional[torch.Tensor] = None, ld_res0: Optional[int] = None,
              res1: Optional[torch.Tensor] = None, ld_res1: Optional[int] = None, res1_rows: int = 0,
              alpha: float = 1.0, act: int = ACT_NONE,
              nz: int = 1, zdiv: int = 1, a_zs=(0, 0), w_zs=(0, 0), o_zs=(0, 0),
              a_scale: Optional[torch.Tensor] = None, w_scale: Optional[torch.Tensor] = None, a_scale_zs: int = 0,
              w_scale_zs: int = 0, splitk: int = 0, tile: int = 0, ln_colsum: Optional[torch.Tensor] = None, ln_eps: float = 1e-5,
              vt_out: Optional[torch.Tensor] = None, vt_n0: int = 0, vt_tokens: int = 0, sk_fused: bool = False,
              gn_part: Union[bool, int] = False, defer_reduce: bool = False) -> torch.Tensor:
    """Raw descriptor-level call of mf_gemm_conv (see include/mfhip.h). All strides in elements.  `dtype`: a torch
    dtype (bf16 / fp32 compute) or an MF_* compute code (the split codes take fp32 a0 and, with w_split=1, a weight
    from ops.split_pack).  `defer_reduce`: the caller hands `out` to groupnorm() next and to nothing else — a split-K launch may
    then leave its reduce to that GroupNorm (mf_gemm_desc.defer_reduce): `out` comes back UNWRITTEN with out._sk_pending set."""
    _req_cuda(a0, a1, w, out, bias, temb, res0, res1)
    d = GemmDesc()
    code = dtype if isinstance(dtype, int) else dt_code(dtype)
    d.dtype = code
    d.a0, d.a1 = _ptr(a0), _ptr(a1)
    d.c0, d.c1, d.lda0, d.lda1 = c0, c1, lda0, lda1
    d.a_dtype = dt_code(a0.dtype)
    d.batch, d.h_in, d.w_in, d.h_out, d.w_out = batch, h_in, w_in, h_out, w_out
    d.kh, d.kw, d.stride, d.pad_t, d.pad_l, d.upsample = kh, kw, stride, pad_t, pad_l, int(upsample)
    want_w = ({MF_F16X3: torch.float16, MF_BF16X3: torch.bfloat16}[code] if w_split else
              torch.bfloat16 if code == MF_BF16 else torch.float16 if code == MF_F16 else FP8 if code == MF_FP8 else torch.float32)
    if w.dtype != want_w:
        raise MfhipError(f"weight dtype {w.dtype} != {want_w} expected by compute code {code} (w_split={w_split})")
    d.w = _ptr(w)
    d.w_split = w_split
    d.ldw = ldw if ldw is not None else kh * kw * (c0 + c1)
    d.n = n
    d.nz, d.zdiv = nz, zdiv
    d.a_zs_o, d.a_zs_i = a_zs
    d.w_zs_o, d.w_zs_i = w_zs
    d.o_zs_o, d.o_zs_i = o_zs
    for t in (bias, temb):
        if t is not None and t.dtype != torch.float32:
            raise MfhipError("bias / temb must be fp32")
    d.bias, d.bias_mode = _ptr(bias), bias_mode
    d.temb, d.ld_temb = _ptr(temb), ld_temb
    for t in (a_scale, w_scale):
        if t is not None and (t.dtype != torch.float32 or not t.is_cuda):
            raise MfhipError("a_scale / w_scale must be fp32 device tensors")
    d.a_scale, d.w_scale, d.a_scale_zs, d.w_scale_zs = _ptr(a_scale), _ptr(w_scale), a_scale_zs, w_scale_zs
    d.res0, d.res0_dtype = _ptr(res0), (dt_code(res0.dtype) if res0 is not None else 0)
    d.ld_res0 = ld_res0 if ld_res0 is not None else n
    d.res1, d.res1_dtype = _ptr(res1), (dt_code(res1.dtype) if res1 is not None else 0)
    d.ld_res1 = ld_res1 if ld_res1 is not None else n
    d.res1_rows = int(res1_rows)
    d.alpha, d.act = alpha, act
    d.out, d.out_dtype = _ptr(out), dt_code(out.dtype)
    d.ldc = ldc if ldc is not None else n
    ws = scratch("splitk", SPLITK_WS_FLOATS, out.device)
    d.splitk, d.ws, d.ws_floats = splitk, ws.data_ptr(), ws.numel()
    d.tile = tile
    fused = 0
    if ln_colsum is not None:
        _req_cuda(ln_colsum)
        if ln_colsum.dtype != torch.float32 or ln_colsum.numel() != n:
            raise MfhipError("ln_colsum must be n fp32 values")
        d.ln_colsum, d.ln_eps = _ptr(ln_colsum), ln_eps
        fused |= 1
    if vt_out is not None:
        _req_cuda(vt_out)
        if vt_out.dtype not in (torch.bfloat16, torch.float16) or vt_out.dim() != 3 or not vt_out.is_contiguous():
            raise MfhipError("vt_out must be a contiguous bf16 / fp16 [images][n - vt_n0][ld] tensor")
        d.vt_out, d.vt_n0, d.vt_tokens, d.vt_ld = _ptr(vt_out), vt_n0, vt_tokens, vt_out.shape[-1]
        fused |= 2
    tkey = None
    # the persistent 128-row GEMM (tile 70) where a block walks two or more output tiles: the epilogue of every tile but the
    # last runs under the next main loop (csrc/gemm_pers.hip; tools/bench_ff1.py for the per-shape table).  Not a tuner candidate
    # for these calls: it wins them by 5-35 % in isolation and the step agrees (same-box A/B, profiles/r06_ab_switches.txt).
    # A cheap gate here; whether tile 70 serves the call is the library's answer (_route_pers)
    use_pers = (PREFER_PERS and tile == 0 and splitk in (0, 1) and code in (MF_BF16, MF_F16) and not gn_part and kh == 1 and kw == 1
                and _route_pers(d))
    if tile == 0 and splitk in (0, 1) and AUTOTUNE and not use_pers:
        tkey = (code, d.a_dtype, batch * h_out * w_out, n, kh * kw * (c0 + c1), kh, stride, int(upsample), int(c1 > 0),
                nz, int(splitk == 1) if not fused else 1, act, h_out, w_out) + ((w_split,) if code in (MF_F16X3, MF_BF16X3) else ()) \
            + ((("ln", "vt", "lnvt")[fused - 1],) if fused else ())
        cfg = None
        if TUNE_CTX is not None and not _NO_TUNE_CTX:
            ks_ctx = _tune_key(tkey) + "@" + TUNE_CTX
            cfg = _tune_load().get(ks_ctx)
            if KEY_LOG is not None:
                KEY_LOG.append(ks_ctx)
        elif KEY_LOG is not None:
            KEY_LOG.append(_tune_key(tkey))
        if cfg is None:
            cfg = _tuned_config(d, tkey)
        d.tile, d.splitk = cfg[0], cfg[1]
        if len(cfg) > 2 and cfg[2]:
            tk = sk_tickets(out.device)
            d.sk_tickets, d.sk_ticket_cap = tk.data_ptr(), tk.numel()
        else:
            d.sk_tickets, d.sk_ticket_cap = None, 0
    elif sk_fused and splitk > 1:
        tk = sk_tickets(out.device)
        d.sk_tickets, d.sk_ticket_cap = tk.data_ptr(), tk.numel()
    part = part_rows = None
    if gn_part:
        # GroupNorm statistics from this launch (mf_gemm_desc.gn_part): per-channel partial sums of the output, attached to `out`
        # as out._gn_part = (fp32 buffer, rows per block) for groupnorm() to pick up.  Set after the tuner ran (it times plain launches).
        m_rows = batch * h_out * w_out
        part = torch.empty(2 * n * (m_rows // 32), dtype=torch.float32, device=out.device)
        part_rows, grouped = C.c_int32(0), C.c_int32(0)
        d.gn_part, d.gn_part_floats, d.gn_part_rows = part.data_ptr(), part.numel(), C.addressof(part_rows)
        # gn_part = the consumer GroupNorm's group count (an int > 1): per-group sums too where the tile allows (no finalize launch then)
        d.gn_groups, d.gn_grouped = (int(gn_part) if (gn_part is not True and int(gn_part) > 1) else 0), C.addressof(grouped)
    deferred = C.c_int32(0)
    if defer_reduce and DEFER_REDUCE and not gn_part:
        d.defer_reduce, d.deferred_splits = 1, C.addressof(deferred)

    def pending():
        if deferred.value > 0:      # (the slabs stay in this stream's split-K scratch until the GroupNorm that follows has read them)
            out._sk_pending = (ws, int(deferred.value), bias, temb, ld_temb, float(alpha))
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _check(load().mf_gemm_conv(C.byref(d), _stream()), "mf_gemm_conv")
        e1.record()
        pending()
        PROFILE.append((e0, e1, 2.0 * batch * h_out * w_out * n * kh * kw * (c0 + c1) * nz,
                        (batch * h_out * w_out, n, kh * kw * (c0 + c1), kh, stride, int(upsample), nz, d.tile, d.splitk, int(code))))
        if part is not None:
            out._gn_part = (part, int(part_rows.value), int(d.gn_groups) if grouped.value else 0)
        return out
    rc = load().mf_gemm_conv(C.byref(d), _stream())
    if rc != 0 and tkey is not None and d.tile != 0:
        # a cached (tile, split-K) the library no longer accepts for this call: forget it and let the heuristic choose
        _tune_forget(_tune_key(tkey))
        d.tile, d.splitk, d.sk_tickets, d.sk_ticket_cap = 0, splitk, None, 0
        rc = load().mf_gemm_conv(C.byref(d), _stream())
    _check(rc, "mf_gemm_conv")
    pending()
    if part is not None:
        # (buffer, rows per block, G): G > 0 = per-group sums of G groups follow the per-channel ones at float 2 * n * (M / rows)
        out._gn_part = (part, int(part_rows.value), int(d.gn_groups) if grouped.value else 0)
    return out


UP2X_TILES = (42, 43, 48)       # tiles with a phase form (csrc/gemm_conv.hip: tile_up2x)


def _up2x_desc(a0: torch.Tensor, w4: torch.Tensor, out: torch.Tensor, *, c0: int, batch: int, h_in: int, w_in: int, n: int,
               lda0: Optional[int] = None, ldw: Optional[int] = None, w_zs: Optional[int] = None, ldc: Optional[int] = None,
               bias: Optional[torch.Tensor] = None, res0: Optional[torch.Tensor] = None, ld_res0: Optional[int] = None,
               res1: Optional[torch.Tensor] = None, ld_res1: Optional[int] = None, res1_rows: int = 0, alpha: float = 1.0,
               act: int = ACT_NONE, splitk: int = 0, tile: int = 0) -> GemmDesc:
    """The mf_gemm_desc of one mf_conv_up2x call (include/mfhip.h): the low-resolution geometry, four [n][4 c0] phase weights."""
    _req_cuda(a0, w4, out, bias, res0, res1)
    if a0.dtype not in (torch.bfloat16, torch.float16) or w4.dtype != a0.dtype:
        raise MfhipError(f"conv_up2x: bf16 / fp16 activations and phase weights of one dtype (got {a0.dtype}, {w4.dtype})")
    if bias is not None and bias.dtype != torch.float32:
        raise MfhipError("bias must be fp32")
    d = GemmDesc()
    d.dtype = d.a_dtype = dt_code(a0.dtype)
    d.a0, d.c0, d.lda0 = _ptr(a0), c0, (lda0 if lda0 is not None else c0)
    d.batch, d.h_in, d.w_in, d.h_out, d.w_out = batch, h_in, w_in, 2 * h_in, 2 * w_in
    d.kh, d.kw, d.stride, d.pad_t, d.pad_l, d.upsample = 2, 2, 1, 1, 1, 1
    d.w, d.ldw = _ptr(w4), (ldw if ldw is not None else 4 * c0)
    d.w_zs_o = w_zs if w_zs is not None else n * d.ldw
    d.n, d.nz, d.zdiv = n, 1, 1
    d.bias = _ptr(bias)
    d.res0, d.res0_dtype, d.ld_res0 = _ptr(res0), (dt_code(res0.dtype) if res0 is not None else 0), (ld_res0 if ld_res0 is not None else n)
    d.res1, d.res1_dtype, d.ld_res1 = _ptr(res1), (dt_code(res1.dtype) if res1 is not None else 0), (ld_res1 if ld_res1 is not None else n)
    d.res1_rows = int(res1_rows)
    d.alpha, d.act = alpha, act
    d.out, d.out_dtype, d.ldc = _ptr(out), dt_code(out.dtype), (ldc if ldc is not None else n)
    ws = scratch("splitk", SPLITK_WS_FLOATS, out.device)
    d.splitk, d.ws, d.ws_floats, d.tile = splitk, ws.data_ptr(), ws.numel(), tile
    return d


def conv_up2x(a0: torch.Tensor, w4: torch.Tensor, out: torch.Tensor, *, gn_part: Union[bool, int] = False, **kw) -> torch.Tensor:
    """Raw descriptor-level call of mf_conv_up2x: the 3x3 conv over the nearest-2x upsampled a0 [batch, h_in, w_in, c0] as four 2x2 phase
    convs in one launch, with the phase weights w4 [4][n][4 c0] of ops.phase_weights.  (tile, split-K): the caller's, else the tune
    cache's entry "up2x,<code>,<M>,<n>,<K>" (M = batch * h_in * w_in rows per phase, K = 4 c0), else the library's own choice.
    gn_part as in gemm_conv: the partial sums are attached to `out` for groupnorm()."""
    d = _up2x_desc(a0, w4, out, **kw)
    n, m_out = d.n, 4 * d.batch * d.h_in * d.w_in
    if d.tile == 0 and d.splitk in (0, 1) and AUTOTUNE:
        cfg = _tune_load().get(_tune_key(("up2x", d.dtype, m_out // 4, n, 4 * d.c0)))
        if cfg is not None:
            d.tile, d.splitk = cfg[0], cfg[1]
    part = part_rows = None
    if gn_part:
        part = torch.empty(2 * n * (m_out // 32), dtype=torch.float32, device=out.device)
        part_rows, grouped = C.c_int32(0), C.c_int32(0)
        d.gn_part, d.gn_part_floats, d.gn_part_rows = part.data_ptr(), part.numel(), C.addressof(part_rows)
        d.gn_groups, d.gn_grouped = (int(gn_part) if (gn_part is not True and int(gn_part) > 1) else 0), C.addressof(grouped)
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _check(load().mf_conv_up2x(C.byref(d), _stream()), "mf_conv_up2x")
    if PROFILE is not None:
        e1.record()
        # as four batched 2x2 convs of M = m_out / 4 rows (nz = 4): bench.py's byte model then counts every phase's weight matrix and
        # output once (and the low-resolution input once per phase, which is what the launch reads)
        PROFILE.append((e0, e1, 2.0 * m_out * n * 4 * d.c0, (m_out // 4, n, 4 * d.c0, 2, 1, 0, 4, d.tile, d.splitk, int(d.dtype))))
    if part is not None:
        out._gn_part = (part, int(part_rows.value), int(d.gn_groups) if grouped.value else 0)
    return out


def conv_up2x_plan(a0: torch.Tensor, w4: torch.Tensor, out: torch.Tensor, **kw) -> GemmPlan:
    """What the library would do with the call conv_up2x(a0, w4, out, **kw) makes (mf_conv_up2x_plan: nothing is launched)."""
    plan = GemmPlan()
    _check(load().mf_conv_up2x_plan(C.byref(_up2x_desc(a0, w4, out, **kw)), C.byref(plan)), "mf_conv_up2x_plan")
    return plan


def _groupnorm_desc(x0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, pend, *, groups: int, eps: float, silu: bool,
                    out_dtype: torch.dtype, x1: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    stats_out: Optional[torch.Tensor] = None):
    """(descriptor, out) of groupnorm()'s one mf_groupnorm call; `pend`: the deferred split-K input taken off x0, or None."""
    _req_cuda(x0, x1, gamma, beta)
    b = x0.shape[0]
    c0 = x0.shape[-1]
    c1 = x1.shape[-1] if x1 is not None else 0
    hw = x0.numel() // (b * c0)
    if not x0.is_contiguous() or (x1 is not None and not x1.is_contiguous()):
        raise MfhipError("groupnorm inputs must be contiguous NHWC")
    if out is None:
        out = torch.empty(*x0.shape[:-1], c0 + c1, dtype=out_dtype, device=x0.device)
    d = GroupNormDesc()
    d.x0, d.x1, d.c0, d.c1 = _ptr(x0), _ptr(x1), c0, c1
    d.in_dtype = dt_code(x0.dtype)
    d.batch, d.hw, d.groups, d.eps = b, hw, groups, eps
    d.gamma, d.beta, d.silu = _ptr(gamma), _ptr(beta), int(silu)
    d.out, d.out_dtype = _ptr(out), dt_code(out.dtype)
    lib = load()
    ws = scratch("gn", lib.mf_groupnorm_ws_floats(b, groups, c0 + c1), x0.device)
    d.ws = ws.data_ptr()
    if stats_out is not None:
        _f32(stats_out)
        if stats_out.numel() != b * groups * 2 or not stats_out.is_contiguous():
            raise MfhipError("groupnorm: stats_out is a contiguous [batch, groups, 2] tensor")
        d.stats_out = stats_out.data_ptr()
    if pend is not None:
        if x1 is not None or stats_out is not None:
            raise MfhipError("groupnorm: a deferred split-K input is a single segment without stats_out")
        ws_t, splits, sk_bias, sk_temb, sk_ld, sk_alpha = pend
        d.sk_ws, d.sk_splits, d.sk_bias, d.sk_temb, d.sk_ld_temb, d.sk_alpha = ws_t.data_ptr(), splits, _ptr(sk_bias), _ptr(sk_temb), sk_ld, sk_alpha
    if GN_FROM_PARTS and hw > 256:
        # statistics handed over by the producing GEMMs (gemm_conv(..., gn_part=True) attached them to its output tensor)
        p0, p1 = getattr(x0, "_gn_part", None), (getattr(x1, "_gn_part", None) if x1 is not None else None)
        if p0 is not None and (x1 is None or p1 is not None):
            d.part0, d.part0_rows = p0[0].data_ptr(), p0[1]
            if p1 is not None:
                d.part1, d.part1_rows = p1[0].data_ptr(), p1[1]
            if x1 is None and len(p0) > 2 and p0[2] == groups and GN_FROM_GROUPS:
                d.grp0, d.grp0_rows = p0[0].data_ptr() + 4 * 2 * c0 * (b * hw // p0[1]), p0[1]
    return d, out


def groupnorm(x0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, groups: int, eps: float, silu: bool,
              out_dtype: torch.dtype, x1: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              stats_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x0/x1: NHWC [B, H, W, C] (or [B, HW, C]); returns the normalised tensor over cat([x0, x1], -1).  stats_out (fp32
    [B, groups, 2], written): every group's (mean, rstd), which groupnorm_bwd takes as `stats`."""
    pend = getattr(x0, "_sk_pending", None)
    if pend is not None:
        x0._sk_pending = None              # consumed here (x0 itself stays unwritten: nothing else may read it)
    d, out = _groupnorm_desc(x0, gamma, beta, pend, groups=groups, eps=eps, silu=silu, out_dtype=out_dtype, x1=x1, out=out, stats_out=stats_out)
    _launch("mf_groupnorm", C.byref(d))
    return out


def groupnorm_plan(x0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, **kw) -> GnPlan:
    """What the library would do with exactly the call groupnorm(x0, gamma, beta, **kw) makes (mf_groupnorm_plan: nothing is launched) —
    the producer's sums and a deferred split-K input attached to x0 / x1 included, and left attached."""
    pend, x0._sk_pending = getattr(x0, "_sk_pending", None), None
    try:
        d, _ = _groupnorm_desc(x0, gamma, beta, pend, **kw)
    finally:
        x0._sk_pending = pend
    plan = GnPlan()
    _check(load().mf_groupnorm_plan(C.byref(d), C.byref(plan)), "mf_groupnorm_plan")
    return plan


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out_dtype: torch.dtype
              ) -> torch.Tensor:
    _req_cuda(x, gamma, beta)
    c = x.shape[-1]
    rows = x.numel() // c
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    _launch("mf_layernorm", x, dt_code(x.dtype), out, dt_code(out_dtype), gamma, beta, rows, c, eps)
    return out


def softmax_rows(scores: torch.Tensor, cols: int, out_dtype: torch.dtype) -> torch.Tensor:
    """scores: [..., ld] fp32; softmax over the first `cols` entries of each row, pad written as 0."""
    _req_cuda(scores)
    ld = scores.shape[-1]
    rows = scores.numel() // ld
    out = torch.empty(scores.shape, dtype=out_dtype, device=scores.device)
    _launch("mf_softmax_rows", scores, out, dt_code(out_dtype), rows, cols, ld)
    return out


def softmax_rows_causal(scores: torch.Tensor, cols: int, sq: int, out_dtype: torch.dtype) -> torch.Tensor:
    """softmax_rows under a causal mask: scores [batch * heads, sq, ld]; query i keeps columns 0 .. i, the rest is written as 0."""
    _req_cuda(scores)
    ld = scores.shape[-1]
    rows = scores.numel() // ld
    out = torch.empty(scores.shape, dtype=out_dtype, device=scores.device)
    _launch("mf_softmax_rows_causal", scores, out, dt_code(out_dtype), rows, cols, ld, sq)
    return out


def embed_tokens(ids: torch.Tensor, token_table: torch.Tensor, pos_table: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """out[b][s] = token_table[ids[b][s]] + pos_table[s] (mf_embed_tokens).  `ids`: [B, S] integers.  A HOST tensor is checked against
    the vocabulary here (ValueError) before it is copied; on the device the kernel clamps, so no id ever reads out of range."""
    if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64):
        raise MfhipError("embed_tokens: ids is a [batch, seq] int32 / int64 tensor")
    vocab, hidden = token_table.shape
    b, s = ids.shape
    if not ids.is_cuda:
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= vocab):
            raise ValueError(f"embed_tokens: token ids must lie in [0, {vocab}), got [{int(ids.min())}, {int(ids.max())}]")
        ids = ids.to(torch.int32).to(token_table.device)
    _req_cuda(ids, token_table, pos_table)
    ids = ids.to(torch.int32).contiguous()
    if (token_table.dtype != pos_table.dtype or pos_table.shape[0] < s or pos_table.shape[1] != hidden
            or not token_table.is_contiguous() or not pos_table.is_contiguous()):
        raise MfhipError("embed_tokens: contiguous tables of one dtype, [vocab, hidden] and [>= seq, hidden]")
    out = torch.empty(b, s, hidden, dtype=out_dtype, device=token_table.device)
    _launch("mf_embed_tokens", ids, token_table, pos_table, dt_code(token_table.dtype), out, dt_code(out_dtype), b, s, hidden, vocab)
    return out


def act(x: torch.Tensor, kind: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ACT_QUICK_GELU (x * sigmoid(1.702 x)) or ACT_GELU_ERF over a contiguous fp32 / bf16 / fp16 tensor; `out=x` runs in place."""
    _req_cuda(x, out)
    if not x.is_contiguous():
        raise MfhipError("act: contiguous input")
    if out is None:
        out = torch.empty_like(x)
    elif out.dtype != x.dtype or out.shape != x.shape or not out.is_contiguous():
        raise MfhipError("act: out has x's dtype and shape")
    _launch("mf_act", x, out, dt_code(x.dtype), kind, x.numel())
    return out


def attention_bf16(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, *, ldq: int, ldk: int,
                   ldvt: int, ldo: int, batch: int, heads: int, sq: int, skv: int, head_dim: int, scale: float,
                   lse: Optional[torch.Tensor] = None, causal: bool = False) -> torch.Tensor:
    """`lse` (fp32 [batch, heads, sq], written): the row statistic of the flash backward (mf_attention_bf16_lse).
    `causal`: query i attends keys 0 .. i (mf_attention_causal_bf16 / _f16; sq == skv, inference: no lse)."""
    _req_cuda(q, k, vt, out, lse)
    if causal:
        if lse is not None or not (q.dtype == k.dtype == vt.dtype == out.dtype) or q.dtype not in (torch.bfloat16, torch.float16):
            raise MfhipError("attention_bf16(causal=True): bf16 or fp16 q / k / vt / out of one dtype and no lse")
        fn = "mf_attention_causal_f16" if q.dtype == torch.float16 else "mf_attention_causal_bf16"
        _launch(fn, q, ldq, k, ldk, vt, ldvt, out, ldo, batch, heads, sq, skv, head_dim, scale)
        return out
    if PROFILE is not None:               # bench.py's FLOP census (no timing here: the GEMM family is the timed one)
        global PROFILE_ATTN_FLOPS
        PROFILE_ATTN_FLOPS += 4.0 * batch * heads * sq * skv * head_dim
    if q.dtype == torch.float16:          # the fp16 storage mode: the same kernel on the f16 MFMA forms (inference: no row statistics)
        if lse is not None or not (k.dtype == vt.dtype == out.dtype == torch.float16):
            raise MfhipError("attention_bf16: fp16 operands take fp16 k / vt / out and no lse")
        _launch("mf_attention_f16", q, ldq, k, ldk, vt, ldvt, out, ldo, batch, heads, sq, skv, head_dim, scale)
        return out
    if lse is None:
        _launch("mf_attention_bf16", q, ldq, k, ldk, vt, ldvt, out, ldo, batch, heads, sq, skv, head_dim, scale)
        return out
    _f32(lse)
    if lse.numel() != batch * heads * sq or not lse.is_contiguous():
        raise MfhipError("attention_bf16: lse is a contiguous [batch, heads, sq] tensor")
    _launch("mf_attention_bf16_lse", q, ldq, k, ldk, vt, ldvt, out, ldo, lse, batch, heads, sq, skv, head_dim, scale)
    return out


def attention_ip_bf16(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, k_ip: torch.Tensor, vt_ip: torch.Tensor, out: torch.Tensor, *,
                      ldq: int, ldk: int, ldvt: int, ldk_ip: int, ldvt_ip: int, ldo: int, batch: int, heads: int, sq: int, skv: int,
                      skv_ip: int, head_dim: int, scale: float, ip_scale: float) -> torch.Tensor:
    """Decoupled cross-attention in one launch (mf_attention_ip_bf16 / _f16 by q.dtype):
    out = softmax(q k^T scale) v + ip_scale softmax(q k_ip^T scale) v_ip, 1 <= skv_ip <= 64.  Inference only."""
    _req_cuda(q, k, vt, k_ip, vt_ip, out)
    if q.dtype not in (torch.bfloat16, torch.float16) or not (q.dtype == k.dtype == vt.dtype == k_ip.dtype == vt_ip.dtype == out.dtype):
        raise MfhipError("attention_ip_bf16: bf16 or fp16 q / k / vt / k_ip / vt_ip / out of one dtype")
    if PROFILE is not None:
        global PROFILE_ATTN_FLOPS
        PROFILE_ATTN_FLOPS += 4.0 * batch * heads * sq * (skv + skv_ip) * head_dim
    _launch("mf_attention_ip_f16" if q.dtype == torch.float16 else "mf_attention_ip_bf16", q, ldq, k, ldk, vt, ldvt, k_ip, ldk_ip, vt_ip,
            ldvt_ip, out, ldo, batch, heads, sq, skv, skv_ip, head_dim, scale, ip_scale)
    return out


def attention_ip_f16x3(q, k, vt, k_ip, vt_ip, out: torch.Tensor, *, ldq: int, ldk: int, ldvt: int, ldk_ip: int, ldvt_ip: int, ldo: int,
                       batch: int, heads: int, sq: int, skv: int, skv_ip: int, head_dim: int, scale: float, ip_scale: float) -> torch.Tensor:
    """attention_ip_bf16 in split precision: q / k / vt / k_ip / vt_ip are (hi, lo) pairs from split_halves; out fp32."""
    _req_cuda(*q, *k, *vt, *k_ip, *vt_ip, out)
    _f32(out)
    if PROFILE is not None:
        global PROFILE_ATTN_FLOPS
        PROFILE_ATTN_FLOPS += 4.0 * batch * heads * sq * (skv + skv_ip) * head_dim
    _launch("mf_attention_ip_f16x3", q[0], q[1], ldq, k[0], k[1], ldk, vt[0], vt[1], ldvt, k_ip[0], k_ip[1], ldk_ip, vt_ip[0], vt_ip[1],
            ldvt_ip, out, ldo, batch, heads, sq, skv, skv_ip, head_dim, scale, ip_scale)
    return out


def freq_encode(x: torch.Tensor, n_freqs: int, max_freq_log2: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [..., in_dim] -> fp32 [..., 2 * n_freqs * in_dim]: cat([sin(x f_0), cos(x f_0), sin(x f_1), ...], -1) with
    f_i = 2^(i max_freq_log2 / (n_freqs - 1)) (mf_freq_encode: the reference's FreqEncoder, log sampling, no input copy)."""
    _req_cuda(x, out)
    _f32(x)
    if not x.is_contiguous():
        raise MfhipError("freq_encode: contiguous input")
    in_dim = x.shape[-1]
    rows = x.numel() // in_dim
    if out is None:
        out = torch.empty(*x.shape[:-1], 2 * n_freqs * in_dim, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.numel() != rows * 2 * n_freqs * in_dim or not out.is_contiguous():
        raise MfhipError("freq_encode: out is a contiguous fp32 [..., 2 * n_freqs * in_dim] tensor")
    _launch("mf_freq_encode", x, out, rows, in_dim, n_freqs, float(max_freq_log2))
    return out


def quantize_rows_fp8(x: torch.Tensor, norm=None, eps: float = 1e-5):
    """Per-row dynamic fp8 quantisation of [..., C] (optionally LayerNorm(x; gamma, beta) first): returns
    (q fp8 [..., C], scale fp32 [rows]) with x ~ q * scale[row]."""
    _req_cuda(x)
    if not x.is_contiguous():
        raise MfhipError("quantize_rows_fp8: contiguous input")
    c = x.shape[-1]
    rows = x.numel() // c
    q = torch.empty(x.shape, dtype=FP8, device=x.device)
    sc = torch.empty(rows, dtype=torch.float32, device=x.device)
    g, b = norm if norm is not None else (None, None)
    _launch("mf_quantize_rows_fp8", x, dt_code(x.dtype), q, sc, rows, c, g, b, eps)
    return q, sc


def split_overflow(reset: bool = True) -> int:
    """Bit mask of the fp16 split precision's range-guard flags (0 = every f16x3 operand since the last reset was inside
    |x| <= 65504; bit 0 GEMM / conv, bit 1 attention operands, bit 2 weight gradients).  Synchronises the current stream."""
    raised = C.c_int32(0)
    _launch("mf_split_overflow", int(reset), C.byref(raised))
    return int(raised.value)


class SplitRangeError(MfhipError):
    """An f16x3 operand left the fp16 range: the products computed from it are wrong (saturated, not inf)."""


def split_pack_check(w: torch.Tensor, code: int) -> None:
    """Weights are split once on the host: refuse an fp16 split of a weight outside the fp16 range."""
    if code == MF_F16X3 and w.numel() and float(w.abs().max()) > 65504.0:
        raise SplitRangeError("f16x3: a weight exceeds the fp16 range (|w| > 65504); use precision 'bf16x3' or 'fp32'")


def split_pack(w: torch.Tensor, code: int, out: Optional[torch.Tensor] = None):
    """fp32 [rows, k] (row stride w.stride(0)) -> (16-bit [rows, 2 * kp] in mf_gemm_desc's w_split layout, kp) on the device
    (mf_split_pack; ops.split_pack is the host-side twin the inference weights go through once)."""
    _req_cuda(w, out)
    if w.dtype != torch.float32 or w.dim() != 2 or w.stride(1) != 1:
        raise MfhipError("split_pack: fp32 [rows, k] with unit column stride")
    rows, k = w.shape
    kp = (k + 31) // 32 * 32
    half = torch.float16 if code == MF_F16X3 else torch.bfloat16
    if out is None:
        out = torch.empty(rows, 2 * kp, dtype=half, device=w.device)
    elif out.dtype != half or out.numel() != rows * 2 * kp or not out.is_contiguous():
        raise MfhipError("split_pack: out must be a contiguous 16-bit [rows, 2 * kp] tensor")
    _launch("mf_split_pack", w, w.stride(0), out, rows, k, code)
    return out, kp


def split_halves(x: torch.Tensor):
    """fp32 tensor -> (hi, lo) fp16 tensors of the same shape with hi + lo = x to 22 bits."""
    _req_cuda(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise MfhipError("split_halves: contiguous fp32 input")
    hi = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    lo = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    _launch("mf_split_halves", x, hi, lo, x.numel())
    return hi, lo


def attention_f16x3(q, k, vt, out: torch.Tensor, *, ldq: int, ldk: int, ldvt: int, ldo: int, batch: int, heads: int,
                    sq: int, skv: int, head_dim: int, scale: float, lse: Optional[torch.Tensor] = None, causal: bool = False) -> torch.Tensor:
    """q / k / vt: (hi, lo) pairs from split_halves; out fp32.  lse (optional, fp32 [batch, heads, sq]): the row statistics the
    flash backward needs.  causal: mf_attention_causal_f16x3 (sq == skv, no lse)."""
    _req_cuda(*q, *k, *vt, out, lse)
    if causal:
        if lse is not None:
            raise MfhipError("attention_f16x3(causal=True): inference only, no lse")
        _launch("mf_attention_causal_f16x3", q[0], q[1], ldq, k[0], k[1], ldk, vt[0], vt[1], ldvt, out, ldo, batch, heads, sq, skv, head_dim, scale)
        return out
    _launch("mf_attention_f16x3_lse", q[0], q[1], ldq, k[0], k[1], ldk, vt[0], vt[1], ldvt, out, ldo, lse, batch, heads, sq, skv, head_dim, scale)
    return out


def rowdot_heads(a: torch.Tensor, b: torch.Tensor, heads: int) -> torch.Tensor:
    """[B, S, C] x [B, S, C] -> [B, heads, S]: per-head dot products of the rows (the D term of the attention backward).
    `b` may be bf16 (the bf16 forward's output)."""
    _f32(a)
    bsz, s, c = a.shape
    out = torch.empty(bsz, heads, s, dtype=torch.float32, device=a.device)
    if b.dtype == torch.bfloat16:
        _req_cuda(b)
        if b.shape != a.shape or not (a.is_contiguous() and b.is_contiguous()):
            raise MfhipError("rowdot_heads: contiguous operands of one shape")
        _launch("mf_rowdot_heads_bf16", a, b, out, bsz, s, heads, c // heads, c)
        return out
    _f32(b)
    _launch("mf_rowdot_heads", a, b, out, bsz, s, heads, c // heads, c)
    return out


def rowdot_heads_cast(a: torch.Tensor, b16: torch.Tensor, heads: int):
    """(D [B, heads, S] = per-head row dots of a (fp32) with b16 (bf16), a16 = bf16(a)) from one read of a (mf_rowdot_heads_cast)."""
    _f32(a)
    _req_cuda(b16)
    bsz, s, c = a.shape
    if b16.dtype != torch.bfloat16 or b16.shape != a.shape or not (a.is_contiguous() and b16.is_contiguous()):
        raise MfhipError("rowdot_heads_cast: contiguous fp32 / bf16 operands of one shape")
    out = torch.empty(bsz, heads, s, dtype=torch.float32, device=a.device)
    a16 = torch.empty_like(b16)
    _launch("mf_rowdot_heads_cast", a, b16, a16, out, bsz, s, heads, c // heads)
    return out, a16


def attention_bwd_f16x3(q, k, v, do, qt, kt, dot, lse: torch.Tensor, dd: torch.Tensor, dq: torch.Tensor, dk: torch.Tensor, dv: torch.Tensor, *,
                        heads: int, scale: float, _entry: str = "mf_attention_bwd_f16x3") -> None:
    """Flash attention backward (mf_attention_bwd_f16x3).  q / k / v / do: (hi, lo) planes [B, S, C]; qt / kt / dot: (hi, lo) planes of
    the transposed tensors [B, C, ld]; lse / dd fp32 [B, heads, Sq]; dq / dk / dv fp32 [B, S, C] (written)."""
    b, sq, c = q[0].shape
    skv = k[0].shape[1]
    d = AttnBwdDesc()
    d.q_hi, d.q_lo, d.ldq = q[0].data_ptr(), q[1].data_ptr(), c
    d.k_hi, d.k_lo, d.ldk = k[0].data_ptr(), k[1].data_ptr(), c
    d.v_hi, d.v_lo, d.ldv = v[0].data_ptr(), v[1].data_ptr(), c
    d.do_hi, d.do_lo, d.lddo = do[0].data_ptr(), do[1].data_ptr(), c
    d.qt_hi, d.qt_lo, d.ldqt = qt[0].data_ptr(), qt[1].data_ptr(), qt[0].shape[-1]
    d.kt_hi, d.kt_lo, d.ldkt = kt[0].data_ptr(), kt[1].data_ptr(), kt[0].shape[-1]
    d.dot_hi, d.dot_lo, d.lddot = dot[0].data_ptr(), dot[1].data_ptr(), dot[0].shape[-1]
    d.lse, d.dd = lse.data_ptr(), dd.data_ptr()
    d.dq, d.dk, d.dv, d.ldo = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), c
    d.batch, d.heads, d.sq, d.skv, d.head_dim, d.scale = b, heads, sq, skv, c // heads, scale
    d.out_dtype = dt_code(dq.dtype)
    _launch(_entry, C.byref(d))


def attention_bwd_bf16(q, k, v, do, qt, kt, dot, lse: torch.Tensor, dd: torch.Tensor, dq: torch.Tensor, dk: torch.Tensor, dv: torch.Tensor, *,
                       heads: int, scale: float) -> None:
    """mf_attention_bwd_bf16: the flash backward on single bf16 planes.  q / k / v / do bf16 [B, S, C]; qt / kt / dot bf16 [B, C, ld]."""
    for t in (q, k, v, do, qt, kt, dot):
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise MfhipError("attention_bwd_bf16: contiguous bf16 operands")
    _f32(lse, dd)
    if not (dq.dtype == dk.dtype == dv.dtype and dq.dtype in (torch.float32, torch.bfloat16)):
        raise MfhipError("attention_bwd_bf16: dq / dk / dv are all fp32 or all bf16")
    attention_bwd_f16x3((q, q), (k, k), (v, v), (do, do), (qt, qt), (kt, kt), (dot, dot), lse, dd, dq, dk, dv, heads=heads, scale=scale,
                        _entry="mf_attention_bwd_bf16")


def pack_nhwc(src0: torch.Tensor, src1: Optional[torch.Tensor], c_pad: int, out_dtype: torch.dtype) -> torch.Tensor:
    """NCHW fp32 (optionally two tensors concatenated on C) -> NHWC out_dtype with channels zero-padded."""
    _req_cuda(src0, src1)
    b, c0, h, w = src0.shape
    c1 = src1.shape[1] if src1 is not None else 0
    src0 = src0.contiguous().float()
    if src1 is not None:
        src1 = src1.contiguous().float()
    out = torch.empty(b, h, w, c_pad, dtype=out_dtype, device=src0.device)
    _launch("mf_pack_nhwc", src0, c0, src1, c1, out, dt_code(out_dtype), c_pad, b, h * w)
    return out


def unpack_nchw(src: torch.Tensor, c: int) -> torch.Tensor:
    """NHWC [B, H, W, ld] -> NCHW fp32 [B, c, H, W] (first c channels)."""
    _req_cuda(src)
    b, h, w, ld = src.shape
    out = torch.empty(b, c, h, w, dtype=torch.float32, device=src.device)
    _launch("mf_unpack_nchw", src, dt_code(src.dtype), ld, out, c, b, h * w)
    return out


def _not_replayable(entry: str) -> None:
    if _RECORDER is not None:
        raise MfhipError(f"{entry} is not part of step programs: a tiled VAE pass cannot be recorded")


def crop_pack_nhwc(src: torch.Tensor, y0: int, x0: int, th: int, tw: int, out: torch.Tensor, batch_offset: int = 0) -> torch.Tensor:
    """src[:, :, y0 : y0 + th, x0 : x0 + tw] of an NCHW fp32 tensor -> NHWC with zero pad channels, written at sample `batch_offset` of
    out = [n * B, th, tw, c_pad] (a stacked group buffer of the tiled VAE; its dtype is the destination dtype)."""
    _not_replayable("mf_crop_pack_nhwc")
    _req_cuda(src, out)
    if src.dtype != torch.float32 or src.dim() != 4 or not src.is_contiguous():
        raise MfhipError(f"crop_pack_nhwc: src is a contiguous NCHW fp32 tensor, got {src.dtype} {tuple(src.shape)}")
    if out.dim() != 4 or not out.is_contiguous() or tuple(out.shape[1:3]) != (th, tw):
        raise MfhipError(f"crop_pack_nhwc: out is a contiguous [n, {th}, {tw}, c_pad] buffer, got {tuple(out.shape)}")
    b, c, h, w = src.shape
    _launch("mf_crop_pack_nhwc", src, b, c, h, w, y0, x0, th, tw, out, dt_code(out.dtype), out.shape[3], out.shape[0], batch_offset)
    return out


def vae_tile_blend(tile: torch.Tensor, above: Optional[torch.Tensor], left: Optional[torch.Tensor], blend_extent: int, row_limit: int,
                   c: int, out: torch.Tensor, out_y: int, out_x: int, nhwc: bool) -> None:
    """blend_v / blend_h / crop / cat of tiled_decode and tiled_encode for one tile (mf_vae_tile_blend): `tile` [B, th, tw, ld] fp32 is
    blended in place against the finished tiles `above` and `left` (None at the first row / column) and its crop is written into `out`
    at (out_y, out_x) — NCHW [B, c, H, W] or, with `nhwc`, NHWC [B, H, W, ld].  Call per tile in raster order."""
    _not_replayable("mf_vae_tile_blend")
    _req_cuda(tile, above, left, out)
    for name, t in (("tile", tile), ("above", above), ("left", left), ("out", out)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous()):
            raise MfhipError(f"vae_tile_blend: {name} is a contiguous 4-d fp32 tensor, got {t.dtype} {tuple(t.shape)}")
    b, th, tw, ld = tile.shape
    for name, t in (("above", above), ("left", left)):
        if t is not None and (t.shape[0] != b or t.shape[3] != ld):
            raise MfhipError(f"vae_tile_blend: {name} {tuple(t.shape)} does not go with the tile {tuple(tile.shape)}")
    want = (b, out.shape[1], out.shape[2], ld) if nhwc else (b, c, out.shape[2], out.shape[3])
    if tuple(out.shape) != want:
        raise MfhipError(f"vae_tile_blend: out {tuple(out.shape)} is not {'NHWC' if nhwc else 'NCHW'} {want}")
    ah, aw = (above.shape[1], above.shape[2]) if above is not None else (0, 0)
    lh, lw = (left.shape[1], left.shape[2]) if left is not None else (0, 0)
    oh, ow = (out.shape[1], out.shape[2]) if nhwc else (out.shape[2], out.shape[3])
    _launch("mf_vae_tile_blend", tile, above, left, b, th, tw, ah, aw, lh, lw, ld, c, blend_extent, row_limit, out, int(bool(nhwc)), oh, ow,
            out_y, out_x)


def add(a: torch.Tensor, b: torch.Tensor, out_dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req_cuda(a, b, out)
    if a.shape != b.shape:
        raise MfhipError(f"mf_add shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    if out is None:
        out = torch.empty(a.shape, dtype=out_dtype, device=a.device)
    elif out.shape != a.shape or out.dtype != out_dtype or not out.is_contiguous():
        raise MfhipError("mf_add: `out` must be a contiguous tensor of the operands' shape and the output dtype")
    _launch("mf_add", a, dt_code(a.dtype), b, dt_code(b.dtype), out, dt_code(out_dtype), a.numel())
    return out


def cast_bf16(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 -> bf16 (nearest-even) copy of a contiguous tensor (mf_cast_bf16)."""
    _req_cuda(x, out)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise MfhipError("cast_bf16: contiguous fp32 input")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    elif out.dtype != torch.bfloat16 or out.numel() != x.numel() or not out.is_contiguous():
        raise MfhipError("cast_bf16: `out` must be a contiguous bf16 tensor of the same size")
    _launch("mf_cast_bf16", x, out, x.numel())
    return out


def cast_bf16_colsum(x: torch.Tensor, n: int, *, segs: int = 1, seg_out: Optional[torch.Tensor] = None, ldo: Optional[int] = None,
                     tot_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 copy of the contiguous fp32 [rows, n] gradient `x` plus, from the same read, its column sums ADDED into
    seg_out[s][:n] (row stride ldo; one row per segment of rows / segs rows) and / or tot_out[:n] (mf_cast_bf16_colsum)."""
    _f32(x, seg_out, tot_out)
    if not x.is_contiguous() or x.numel() % n or (x.numel() // n) % segs:
        raise MfhipError("cast_bf16_colsum: contiguous [segs * rows_per_seg, n] input")
    rps = x.numel() // n // segs
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    lib = load()
    ws = scratch("cast_colsum", lib.mf_cast_bf16_colsum_ws_floats(segs, rps, n), x.device)
    _launch("mf_cast_bf16_colsum", x, out, segs, rps, n, seg_out, n if ldo is None else ldo, 1, tot_out, 1, ws)
    return out


def geglu(h: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    _req_cuda(h)
    c = h.shape[-1] // 2
    rows = h.numel() // (2 * c)
    out = torch.empty(*h.shape[:-1], c, dtype=out_dtype, device=h.device)
    _launch("mf_geglu", h, dt_code(h.dtype), out, dt_code(out_dtype), rows, c)
    return out


def timestep_embedding(t: torch.Tensor, dim: int, flip_sin_to_cos: bool, freq_shift: float) -> torch.Tensor:
    _req_cuda(t)
    t = t.float().contiguous()
    out = torch.empty(t.numel(), dim, dtype=torch.float32, device=t.device)
    _launch("mf_timestep_embedding", t, out, t.numel(), dim, int(flip_sin_to_cos), freq_shift)
    return out


def silu_f32(x: torch.Tensor) -> torch.Tensor:
    _req_cuda(x)
    out = torch.empty_like(x)
    _launch("mf_silu_f32", x, out, x.numel())
    return out


def cfg_ddim_step(eps_u: torch.Tensor, eps_c: Optional[torch.Tensor], g: float, x: torch.Tensor, sqrt_at: float,
                  sqrt_1m_at: float, sqrt_ap: float, dir_coef: float, eps_out: Optional[torch.Tensor] = None,
                  pred_type: int = 0, clip: float = 0.0) -> torch.Tensor:
    _req_cuda(eps_u, eps_c, x, eps_out)
    xp = torch.empty_like(x)
    _launch("mf_cfg_ddim_step", eps_u, eps_c, g, x, xp, sqrt_at, sqrt_1m_at, sqrt_ap, dir_coef, pred_type, clip, eps_out, x.numel())
    return xp


def cfg_ddim_step_dev(eps_u: torch.Tensor, eps_c: Optional[torch.Tensor], g: float, x: torch.Tensor, coef4: torch.Tensor,
                      pred_type: int = 0, clip: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """DDIM update with device-resident coefficients (graph replay); `out` may be `x` itself (in place)."""
    _req_cuda(eps_u, eps_c, x, coef4, out)
    xp = out if out is not None else torch.empty_like(x)
    _launch("mf_cfg_ddim_step_dev", eps_u, eps_c, g, x, xp, coef4, pred_type, clip, x.numel())
    return xp


def cfg_combine(eps_u: torch.Tensor, eps_c: torch.Tensor, g: float) -> torch.Tensor:
    _req_cuda(eps_u, eps_c)
    out = torch.empty_like(eps_u)
    _launch("mf_cfg_combine", eps_u, eps_c, g, out, eps_u.numel())
    return out


def axpby_n(xs, coefs, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = sum_i coefs[i] * xs[i] over fp32 tensors of equal shape (at most 6); `out` may be one of the inputs."""
    _req_cuda(*xs)
    n = len(xs)
    arr = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    cf = (C.c_float * n)(*[float(c) for c in coefs])
    if out is None:
        out = torch.empty_like(xs[0])
    _launch("mf_axpby_n", arr, cf, n, out, out.numel())
    return out


def sched_step_dev(eps_u: torch.Tensor, eps_c: Optional[torch.Tensor], g: float, latents: torch.Tensor, state: Optional[torch.Tensor],
                   row: torch.Tensor) -> torch.Tensor:
    """One multistep-scheduler step on the device (mf_sched_step_dev): the guided noise prediction, then the ops of `row` (the
    step's mf_sched_row in device memory, schedulers.device_plan) on `latents` (updated in place) and `state` ([nslots, *latents.shape]
    fp32, the history kept between steps).  `g < 0`: no guidance, register 0 is `eps_u` as loaded and `eps_c` may be None (the
    convention of cfg_ddim_step_dev); `eps_c=None` with `g >= 0` is the library's argument error."""
    _req_cuda(eps_u, eps_c, latents, state, row)
    n = latents.numel()
    if eps_u.numel() != n or (eps_c is not None and eps_c.numel() != n) or (state is not None and state.numel() % n) or row.numel() * row.element_size() < C.sizeof(SchedRow):
        raise MfhipError("sched_step_dev: mismatched sizes")
    for t in (eps_u, eps_c, latents, state, row):
        if t is not None and (not t.is_contiguous() or (t.dtype != torch.float32 and t is not row)):
            raise MfhipError("sched_step_dev: contiguous fp32 tensors needed")
    _launch("mf_sched_step_dev", eps_u, eps_c, g, latents, state, row, n)
    return latents


def sched_step_noise_dev(eps_u: torch.Tensor, eps_c: Optional[torch.Tensor], g: float, latents: torch.Tensor, state: Optional[torch.Tensor],
                         row: torch.Tensor, noise_reg: int, seed: int = 0, offset: int = 0, first_sample: int = 0,
                         global_batch: Optional[int] = None, rng_state: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sched_step_dev for a row that reads a step's noise (mf_sched_step_noise_dev): register `noise_reg` (plan.noise_reg of
    schedulers.device_plan) holds standard normals drawn in the kernel, bit for bit philox_normal(latents.shape, seed, offset, ...,
    first_sample, global_batch); `rng_state` (PhiloxGenerator.device_state()) overrides (seed, offset) and is not written: follow the
    launch with philox_advance(rng_state, philox_normal_blocks(global_batch, per_sample)).  `g < 0` / `eps_c=None`: as sched_step_dev."""
    _req_cuda(eps_u, eps_c, latents, state, row, rng_state)
    n = latents.numel()
    if latents.dim() < 1 or eps_u.numel() != n or (eps_c is not None and eps_c.numel() != n) or (state is not None and state.numel() % n) \
            or row.numel() * row.element_size() < C.sizeof(SchedRow):
        raise MfhipError("sched_step_noise_dev: mismatched sizes")
    for t in (eps_u, eps_c, latents, state, row):
        if t is not None and (not t.is_contiguous() or (t.dtype != torch.float32 and t is not row)):
            raise MfhipError("sched_step_noise_dev: contiguous fp32 tensors needed")
    b = latents.shape[0]
    gb = b + first_sample if global_batch is None else int(global_batch)
    _launch("mf_sched_step_noise_dev", eps_u, eps_c, g, latents, state, row, n, int(noise_reg), n // b, int(first_sample), gb,
            _s64(seed), _s64(offset), _philox_state(rng_state))
    return latents


def mse_loss(pred: torch.Tensor, target: torch.Tensor, weights: Optional[torch.Tensor] = None):
    """(loss[1], per_sample[B]) with per_sample[b] = mean((pred[b] - target[b])**2) * weights[b]; fp32 tensors."""
    _req_cuda(pred, target)
    if pred.shape != target.shape or pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError("mse_loss: pred and target must be fp32 tensors of the same shape")
    pred, target = pred.contiguous(), target.contiguous()
    rows = pred.shape[0]
    per = torch.empty(rows, dtype=torch.float32, device=pred.device)
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    w = None
    if weights is not None:
        w = weights.to(pred.device, torch.float32).contiguous()
        if w.numel() != rows:
            raise ValueError("mse_loss: one weight per sample")
    _launch("mf_mse_loss", pred, target, w, per, loss, rows, pred.numel() // rows)
    return loss, per


def vae_sample(moments: torch.Tensor, noise: torch.Tensor, c: int, scaling: float) -> torch.Tensor:
    """moments NHWC [B, H, W, ld >= 2c]; noise NCHW fp32 [B, c, H, W] -> z NCHW fp32."""
    _req_cuda(moments, noise)
    b, h, w, ld = moments.shape
    z = torch.empty(b, c, h, w, dtype=torch.float32, device=moments.device)
    noise = noise.float().contiguous()
    _launch("mf_vae_sample", moments, dt_code(moments.dtype), ld, noise, z, c, b, h * w, scaling)
    return z


def nearest_resize(src: torch.Tensor, h_out: int, w_out: int) -> torch.Tensor:
    """F.interpolate(src, size=(h_out, w_out)) (default mode='nearest') for NCHW fp32."""
    _req_cuda(src)
    b, c, h, w = src.shape
    src = src.float().contiguous()
    out = torch.empty(b, c, h_out, w_out, dtype=torch.float32, device=src.device)
    _launch("mf_nearest_resize", src, out, b * c, h, w, h_out, w_out)
    return out


# ---- training (csrc/train.hip): fp32 tensors ---------------------------------------------------------------------
def _f32(*ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_cuda):
            raise MfhipError("training kernels take fp32 device tensors")


def conv_wgrad(x: torch.Tensor, dy: torch.Tensor, dw: torch.Tensor, *, code: int, c0: int, batch: int, h_in: int, w_in: int,
               h_out: int, w_out: int, kh: int = 1, kw: int = 1, stride: int = 1, pad_t: int = 0, pad_l: int = 0,
               upsample: bool = False, x1: Optional[torch.Tensor] = None, c1: int = 0, n: int, accumulate: bool = True) -> None:
    """dw[n][kh*kw*(c0+c1)] (+)= sum_m dy[m][n] * im2col(x | x1)[m][:] (mf_conv_wgrad).  code MF_BF16: x / x1 / dy are bf16 tensors."""
    if code == MF_BF16:
        _req_cuda(x, x1, dy, dw)
        if any(t is not None and t.dtype != torch.bfloat16 for t in (x, x1, dy)) or dw.dtype != torch.float32:
            raise MfhipError("conv_wgrad(MF_BF16): bf16 x / dy, fp32 dw")
    else:
        _f32(x, x1, dy, dw)
    d = WgradDesc()
    d.dtype = code if code in (MF_F16X3, MF_BF16X1, MF_BF16) else MF_F32
    d.a0, d.a1, d.c0, d.c1, d.lda0, d.lda1 = _ptr(x), _ptr(x1), c0, c1, c0, c1
    d.batch, d.h_in, d.w_in, d.h_out, d.w_out = batch, h_in, w_in, h_out, w_out
    d.kh, d.kw, d.stride, d.pad_t, d.pad_l, d.upsample = kh, kw, stride, pad_t, pad_l, int(upsample)
    d.dy, d.lddy, d.n = _ptr(dy), n, n
    d.dw, d.lddw = _ptr(dw), kh * kw * (c0 + c1)
    d.accumulate, d.splitm = int(accumulate), 0
    ws = scratch("wgrad", WGRAD_WS_FLOATS, x.device)
    d.ws, d.ws_floats = ws.data_ptr(), ws.numel()
    _launch("mf_conv_wgrad", C.byref(d))


def zero_ranges(base: torch.Tensor, offs: torch.Tensor, lens: torch.Tensor) -> None:
    """base[offs[i] : offs[i] + lens[i]] = 0 in one launch (mf_zero_ranges; offs / lens: int64 device tensors)."""
    _f32(base)
    _req_cuda(offs, lens)
    if offs.dtype != torch.int64 or lens.dtype != torch.int64 or offs.numel() != lens.numel() or not (offs.is_contiguous() and lens.is_contiguous()):
        raise MfhipError("zero_ranges: two contiguous int64 device tensors of one length")
    _launch("mf_zero_ranges", base, offs, lens, offs.numel())


def set_wgrad_dma(on: bool) -> None:
    """Developer / test switch (mf_debug_set_wgrad_dma): bf16-input weight gradients on the LDS-DMA kernel (default) or the
    register-staged one; bit-identical."""
    load().mf_debug_set_wgrad_dma(int(bool(on)))


WGRAD_WS_FLOATS = 64 * 1024 * 1024      # 256 MiB of split-M slabs


def transpose(x: torch.Tensor, rows: int, cols: int, *, nz: int = 1, ldx: Optional[int] = None, ldy: Optional[int] = None,
              zsx: int = 0, zsy: int = 0, out: Optional[torch.Tensor] = None, y_offset: int = 0) -> torch.Tensor:
    """out[z][c][r] = x[z][r][c] (element strides; see mf_transpose).  A bf16 `out` takes the rounding variant (mf_transpose_bf16)."""
    ldx = cols if ldx is None else ldx
    ldy = rows if ldy is None else ldy
    if x.dtype == torch.bfloat16:
        _req_cuda(x, out)
        if out is None or out.dtype != torch.bfloat16 or y_offset:
            raise MfhipError("transpose: a bf16 input takes a bf16 `out`")
        _launch("mf_transpose_bf16_bf16", x, out, nz, rows, cols, ldx, ldy, zsx, zsy)
        return out
    if out is not None and out.dtype == torch.bfloat16:
        _f32(x)
        _req_cuda(out)
        _launch("mf_transpose_bf16", x, out.data_ptr() + 2 * y_offset, nz, rows, cols, ldx, ldy, zsx, zsy)
        return out
    _f32(x, out)
    if out is None:
        out = torch.empty(nz, cols, ldy, dtype=torch.float32, device=x.device)
    _launch("mf_transpose", x, out.data_ptr() + 4 * y_offset, nz, rows, cols, ldx, ldy, zsx, zsy)
    return out


def colsum(x: torch.Tensor, n: int, *, segs: int = 1, rows_per_seg: Optional[int] = None, ldx: Optional[int] = None,
           out: Optional[torch.Tensor] = None, ldo: Optional[int] = None, accumulate: bool = False) -> torch.Tensor:
    _f32(x, out)
    ldx = n if ldx is None else ldx
    rows_per_seg = x.numel() // ldx // segs if rows_per_seg is None else rows_per_seg
    if out is None:
        out = torch.empty(segs, n, dtype=torch.float32, device=x.device)
    lib = load()
    ws = scratch("colsum", lib.mf_colsum_ws_floats(segs, rows_per_seg, n), x.device)
    _launch("mf_colsum", x, ldx, out, n if ldo is None else ldo, segs, rows_per_seg, n, int(accumulate), ws)
    return out


def groupnorm_bwd(x0: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, groups: int, eps: float, silu: bool,
                  x1: Optional[torch.Tensor] = None, want_param_grads: bool = True, streaming: bool = True,
                  grad_acc: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, add0: Optional[torch.Tensor] = None,
                  add1: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None):
    """`stats`: the [B, groups, 2] (mean, rstd) hip.groupnorm(..., stats_out=) kept for this input (the streaming form skips its
    statistics pass).  Returns (dx0, dx1 or None, dgamma_part [B, C] or None, dbeta_part).  streaming=False withholds the workspace, which keeps
    the one-block-per-(image, group) kernel at every size (tests compare the two).  grad_acc = (dgamma, dbeta) fp32 [C]: where
    the shape runs the streaming form the parameter gradients are ADDED there by the kernel itself and the partials come back
    None; elsewhere it is ignored (sum the partials with colsum)."""
    _f32(x0, x1, dy, gamma, beta)
    b, c0 = x0.shape[0], x0.shape[-1]
    c1 = x1.shape[-1] if x1 is not None else 0
    hw = x0.numel() // (b * c0)
    dx0 = torch.empty_like(x0)
    dx1 = torch.empty_like(x1) if x1 is not None else None
    fused = bool(grad_acc is not None and want_param_grads and streaming and load().mf_groupnorm_bwd_streams(b, hw, c0, c1))
    dg = torch.empty(b, c0 + c1, dtype=torch.float32, device=x0.device) if (want_param_grads and not fused) else None
    db = torch.empty_like(dg) if dg is not None else None
    d = GroupNormBwdDesc()
    if fused:
        _f32(*grad_acc)
        d.dgamma_acc, d.dbeta_acc = _ptr(grad_acc[0]), _ptr(grad_acc[1])
    for t, ref in ((add0, x0), (add1, x1)):       # dx = gradient + add: add is laid out like the matching input
        if t is not None and (ref is None or t.numel() != ref.numel() or not t.is_contiguous()):
            raise MfhipError("groupnorm_bwd: add0 / add1 must be contiguous and sized like x0 / x1")
    _f32(add0, add1)
    d.add0, d.add1 = _ptr(add0), _ptr(add1)
    d.x0, d.x1, d.c0, d.c1, d.dy = _ptr(x0), _ptr(x1), c0, c1, _ptr(dy)
    d.gamma, d.beta, d.dx0, d.dx1, d.dgamma_part, d.dbeta_part = _ptr(gamma), _ptr(beta), _ptr(dx0), _ptr(dx1), _ptr(dg), _ptr(db)
    d.batch, d.hw, d.groups, d.silu, d.eps = b, hw, groups, int(silu), eps
    if stats is not None:
        _f32(stats)
        if stats.numel() != b * groups * 2 or not stats.is_contiguous():
            raise MfhipError("groupnorm_bwd: stats is a contiguous [batch, groups, 2] tensor")
        d.stats_in = stats.data_ptr()
    if streaming:
        d.ws = _ptr(scratch("gn_bwd", load().mf_groupnorm_bwd_ws_floats(b, hw, c0 + c1, groups), x0.device))
    _launch("mf_groupnorm_bwd", C.byref(d))
    return dx0, dx1, dg, db


def layernorm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, eps: float, want_param_grads: bool = True,
                  add: Optional[torch.Tensor] = None):
    """add (optional, sized like x): dx = gradient + add."""
    _f32(x, dy, gamma, add)
    if add is not None and (add.numel() != x.numel() or not add.is_contiguous()):
        raise MfhipError("layernorm_bwd: add must be contiguous and sized like x")
    c = x.shape[-1]
    rows = x.numel() // c
    dx = torch.empty_like(x)
    nb = load().mf_layernorm_bwd_parts(rows)
    dg = torch.empty(nb, c, dtype=torch.float32, device=x.device) if want_param_grads else None
    db = torch.empty_like(dg) if want_param_grads else None
    _launch("mf_layernorm_bwd", x, dy, gamma, dx, dg, db, rows, c, eps, add)
    return dx, dg, db


def softmax_bwd(p: torch.Tensor, dp: torch.Tensor, cols: int, scale: float) -> torch.Tensor:
    _f32(p, dp)
    ld = p.shape[-1]
    ds = torch.empty_like(p)
    _launch("mf_softmax_bwd", p, dp, ds, p.numel() // ld, cols, ld, scale)
    return ds


def silu_bwd(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    _f32(x, dy)
    dx = torch.empty_like(x)
    _launch("mf_silu_bwd", x, dy, dx, x.numel())
    return dx


def geglu_bwd(h: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
    _f32(h, dout)
    c = h.shape[-1] // 2
    dh = torch.empty_like(h)
    _launch("mf_geglu_bwd", h, dout, dh, h.numel() // (2 * c), c)
    return dh


def geglu_bwd_bf16(h16: torch.Tensor, dout: torch.Tensor, bias_grad: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mf_geglu_bwd_bf16: h16 bf16 [..., 2c], dout fp32 [..., c] -> dh bf16 [..., 2c]; the column sums of dh are ADDED into bias_grad."""
    _req_cuda(h16)
    _f32(dout, bias_grad)
    c = h16.shape[-1] // 2
    rows = h16.numel() // (2 * c)
    if h16.dtype != torch.bfloat16 or not h16.is_contiguous() or not dout.is_contiguous() or dout.numel() != rows * c:
        raise MfhipError("geglu_bwd_bf16: contiguous bf16 [rows, 2c] pre-activation and fp32 [rows, c] gradient")
    dh = torch.empty_like(h16)
    lib = load()
    ws = scratch("geglu_bwd", lib.mf_geglu_bwd_bf16_ws_floats(rows, c), h16.device) if bias_grad is not None else None
    _launch("mf_geglu_bwd_bf16", h16, dout, dh, rows, c, bias_grad, ws)
    return dh


def zero_insert2x(x: torch.Tensor) -> torch.Tensor:
    _f32(x)
    b, h, w, c = x.shape
    y = torch.empty(b, 2 * h, 2 * w, c, dtype=torch.float32, device=x.device)
    _launch("mf_zero_insert2x", x, y, b, h, w, c)
    return y


def sumpool2x2(x: torch.Tensor) -> torch.Tensor:
    _f32(x)
    b, h2, w2, c = x.shape
    y = torch.empty(b, h2 // 2, w2 // 2, c, dtype=torch.float32, device=x.device)
    _launch("mf_sumpool2x2", x, y, b, h2 // 2, w2 // 2, c)
    return y


def mse_grad(pred: torch.Tensor, target: torch.Tensor, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    _f32(pred, target, weights)
    rows = pred.shape[0]
    d = torch.empty_like(pred)
    _launch("mf_mse_grad", pred, target, weights, d, rows, pred.numel() // rows)
    return d


def sumsq(x: torch.Tensor, out: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    """out[0] (float64, device) (+)= sum x^2."""
    _f32(x)
    lib = load()
    key = ("sumsq", torch.device(x.device).index, torch.cuda.current_stream(x.device).cuda_stream)
    ws = _scratch.get(key)
    if ws is None:
        ws = torch.empty(lib.mf_sumsq_ws_doubles(), dtype=torch.float64, device=x.device)
        _scratch[key] = ws
    _launch("mf_sumsq", x, x.numel(), out, int(accumulate), ws)
    return out


def clip_coef(sumsq_t: torch.Tensor, max_norm: float, coef: torch.Tensor, norm_out: Optional[torch.Tensor] = None,
              unscale: float = 1.0) -> None:
    _launch("mf_clip_coef", sumsq_t, max_norm, unscale, coef, norm_out)


def adamw(w: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
          weight_decay: float = 1e-2, step: int, grad_scale: Optional[torch.Tensor] = None) -> None:
    _f32(w, g, m, v, grad_scale)
    _launch("mf_adamw", w, g, m, v, w.numel(), lr, betas[0], betas[1], eps, weight_decay, step, grad_scale)


# ---- image front-end (csrc/frontend.hip) ------------------------------------------------------------------------------
def _mm_ws(device) -> torch.Tensor:
    return scratch("minmax", load().mf_minmax_ws_floats() + 2, device)


def minmax(x: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[min, max] of x (where mask > 0) as a 2-element DEVICE tensor."""
    _f32(x, mask)
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    _launch("mf_minmax", x, mask, x.numel(), out, _mm_ws(x.device))
    return out


def image_normalize(x: torch.Tensor) -> torch.Tensor:
    """VaeImageProcessor.preprocess for a device tensor: 2x - 1 unless the tensor already holds negatives."""
    _f32(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    _launch("mf_image_normalize", x, y, x.numel(), minmax(x))
    return y


def mask_keep(m: torch.Tensor) -> torch.Tensor:
    _f32(m)
    b, c, h, w = m.shape
    out = torch.empty(b, 1, h, w, dtype=torch.float32, device=m.device)
    _launch("mf_mask_keep", m.contiguous(), out, b, c, h * w)
    return out


def masked_mean_normal(normals: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """[H, W, 3] fp32 normals, [H, W] fp32 mask -> [1, 3]: the mean normal over mask > 0, L2-normalised (mf_masked_mean_normal)."""
    _f32(normals, mask)
    if normals.dim() != 3 or normals.shape[-1] != 3 or tuple(mask.shape) != tuple(normals.shape[:2]):
        raise MfhipError("masked_mean_normal: [H, W, 3] normals and an [H, W] mask")
    out = torch.empty(1, 3, dtype=torch.float32, device=normals.device)
    _launch("mf_masked_mean_normal", normals.contiguous(), mask.contiguous(), out, mask.numel())
    return out


def concat_channels(srcs, batch: int) -> torch.Tensor:
    """torch.cat(srcs, 1) for NCHW fp32 tensors whose batch divides `batch` (smaller ones are repeated)."""
    _f32(*srcs)
    srcs = [s.contiguous() for s in srcs]
    if _RECORDER is not None and all(s.shape[0] == batch for s in srcs):
        # a step program cannot hold this entry's host arrays: while one is recorded the concatenation is the copies it amounts to
        # (torch.cat: program.Recorder writes them down as mf_memcpy2d), bit for bit the same tensor
        return torch.cat(srcs, 1)
    h, w = srcs[0].shape[-2:]
    n = len(srcs)
    out = torch.empty(batch, sum(s.shape[1] for s in srcs), h, w, dtype=torch.float32, device=srcs[0].device)
    arr = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
    ch = (C.c_int32 * n)(*[s.shape[1] for s in srcs])
    bs = (C.c_int32 * n)(*[s.shape[0] for s in srcs])
    _launch("mf_concat_channels", arr, ch, bs, n, out, batch, h * w)
    return out


def u8_to_planes(src: torch.Tensor, channels_out: Optional[int] = None) -> torch.Tensor:
    """uint8 NHWC pixels [B, H, W, C] (what a host holds after decoding an image file) -> fp32 NCHW planes in [0, 1], bit for bit
    numpy's `arr.astype(np.float32) / 255.0` transposed (mf_u8_to_planes).  `channels_out` > 1 with C == 1 replicates the grey plane
    (a mask the reference converts with .convert("RGB"))."""
    _req_cuda(src)
    if src.dtype != torch.uint8 or src.dim() != 4:
        raise MfhipError("u8_to_planes: a uint8 [batch, height, width, channels] tensor")
    src = src.contiguous()
    b, h, w, ci = src.shape
    co = ci if channels_out is None else int(channels_out)
    out = torch.empty(b, co, h, w, dtype=torch.float32, device=src.device)
    _launch("mf_u8_to_planes", src, out, b, ci, co, h * w)
    return out


# ---- the training batch (csrc/train_batch.hip) ---------------------------------------------------------------------------------
def train_example_u8(image: torch.Tensor, mask: torch.Tensor, flips: Optional[torch.Tensor] = None, normalize: bool = True):
    """uint8 image [B, H, W, 3] and mask [B, H, W] -> (pixel_values [B, 3, H, W], conditioning_pixel_values [B, 3, H, W], masks
    [B, 1, H, W]) fp32 from ONE read of the bytes (mf_train_example_u8): x / 255 (a true division), the image blackened where the
    mask is 255 for the conditioning, (v - 0.5) / 0.5 on both images when `normalize`.  `flips`: int32 [B] on the device (non-zero:
    that sample is read right to left, np.fliplr) or None."""
    _req_cuda(image, mask, flips)
    if image.dtype != torch.uint8 or image.dim() != 4 or image.shape[-1] != 3:
        raise MfhipError("train_example_u8: a uint8 [batch, height, width, 3] image")
    if mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(image.shape[:3]):
        raise MfhipError(f"train_example_u8: a uint8 mask of shape {tuple(image.shape[:3])}, got {mask.dtype} {tuple(mask.shape)}")
    b, h, w, _ = image.shape
    if flips is not None and (flips.dtype != torch.int32 or flips.numel() != b):
        raise MfhipError("train_example_u8: flips is an int32 tensor with one flag per image")
    f32 = dict(dtype=torch.float32, device=image.device)
    pix, cond, m = torch.empty(b, 3, h, w, **f32), torch.empty(b, 3, h, w, **f32), torch.empty(b, 1, h, w, **f32)
    _launch("mf_train_example_u8", image.contiguous(), mask.contiguous(), None if flips is None else flips.contiguous(), pix, cond, m,
            b, h, w, int(bool(normalize)))
    return pix, cond, m


def masked_image_u8(image: torch.Tensor, mask: torch.Tensor, invert: bool = True) -> torch.Tensor:
    """HDF5Dataset.get_masked_image on the device: uint8 image [.., H, W, C] with the pixels zeroed where the uint8 mask [.., H, W] is 255
    (invert, the dataset's default) or 0 (mf_masked_image_u8)."""
    _req_cuda(image, mask)
    if image.dtype != torch.uint8 or mask.dtype != torch.uint8 or image.dim() < 3 or tuple(mask.shape) != tuple(image.shape[:-1]):
        raise MfhipError("masked_image_u8: a uint8 [.., H, W, C] image and a uint8 [.., H, W] mask")
    image, mask = image.contiguous(), mask.contiguous()
    out = torch.empty_like(image)
    _launch("mf_masked_image_u8", image, mask, out, mask.numel(), image.shape[-1], int(bool(invert)))
    return out


def fliplr(x: torch.Tensor, channels: Optional[int] = None) -> torch.Tensor:
    """np.fliplr of an fp32 map (mf_fliplr): [H, W, 3] (channels = 3, the default for a last dimension of 3 behind two others) or
    [H, W] / planes [.., H, W] (channels = 1): the width axis is reversed, leading dimensions count as rows."""
    _req_cuda(x)
    if x.dtype != torch.float32 or x.dim() < 2:
        raise MfhipError("fliplr: an fp32 [H, W] or [H, W, 3] map")
    c = (3 if x.dim() >= 3 and x.shape[-1] == 3 else 1) if channels is None else int(channels)
    if c not in (1, 3) or (c == 3 and (x.dim() < 3 or x.shape[-1] != 3)):
        raise MfhipError("fliplr: channels is 1, or 3 for an [.., W, 3] tensor")
    x = x.contiguous()
    w = x.shape[-2] if c == 3 else x.shape[-1]
    out = torch.empty_like(x)
    _launch("mf_fliplr", x, out, x.numel() // (w * c), w, c)
    return out


ASSEMBLE_OUTPUTS = ("latents", "noisy_latents", "target", "conditioning_latents", "timesteps_f32", "loss_weights")


def train_batch_assemble(moments, posterior_noise, c: int, scaling: float, noise: torch.Tensor, timesteps: torch.Tensor,
                         sqrt_alpha: torch.Tensor, sqrt_one_minus_alpha: torch.Tensor, masks: torch.Tensor,
                         depths: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None,
                         loss_weight: Optional[torch.Tensor] = None, v_prediction: bool = False, out: Optional[dict] = None) -> dict:
    """train_brushnet_mirror.py:1351-1449 minus the networks in one launch (mf_train_batch_assemble; include/mfhip.h has the contract).
    moments: 2 .. 4 NHWC [B, h, w, ld] tensors (image, conditioning image, depth, normals; the last two may be None), posterior_noise
    their fp32 [B, c, h, w] draws.  timesteps: int64 [B]; a DEVICE tensor is trusted (the kernel clamps it to the tables, it cannot be
    range-checked without a synchronise), a host tensor is range-checked here and uploaded.  sqrt_alpha / sqrt_one_minus_alpha /
    loss_weight: fp32 device tables.  masks / depths / normals: full-resolution fp32 planes [B, 1 | 1 | 3, R, R'].  `out`: tensors to
    write into, by name (ASSEMBLE_OUTPUTS); the rest are allocated.  Returns the dict of outputs ('loss_weights' only with a table)."""
    moments, posterior_noise = list(moments), list(posterior_noise)
    n = len(moments)
    if not 2 <= n <= 4 or len(posterior_noise) != n:
        raise MfhipError(f"train_batch_assemble: 2 .. 4 moment tensors with one posterior noise each, got {n} and {len(posterior_noise)}")
    _req_cuda(*moments, *posterior_noise, noise, sqrt_alpha, sqrt_one_minus_alpha, loss_weight, masks, depths, normals)
    if moments[0] is None or moments[1] is None:
        raise MfhipError("train_batch_assemble: the image's and the conditioning image's moments are required")
    b, h, w, ld = moments[0].shape
    dev, dt = moments[0].device, moments[0].dtype
    for m, pn in zip(moments, posterior_noise):
        if (m is None) != (pn is None):
            raise MfhipError("train_batch_assemble: a source is its moments and its posterior noise")
        if m is None:
            continue
        if tuple(m.shape) != (b, h, w, ld) or m.dtype != dt or not m.is_contiguous():
            raise MfhipError(f"train_batch_assemble: every moment tensor must be contiguous {dt} [{b}, {h}, {w}, {ld}], got {m.dtype} {tuple(m.shape)}")
        if tuple(pn.shape) != (b, c, h, w) or pn.dtype != torch.float32 or not pn.is_contiguous():
            raise MfhipError(f"train_batch_assemble: posterior noise must be contiguous fp32 [{b}, {c}, {h}, {w}], got {pn.dtype} {tuple(pn.shape)}")
    if tuple(noise.shape) != (b, c, h, w) or noise.dtype != torch.float32 or not noise.is_contiguous():
        raise MfhipError(f"train_batch_assemble: noise must be contiguous fp32 [{b}, {c}, {h}, {w}]")
    t_len = sqrt_alpha.numel()
    for tab in (sqrt_alpha, sqrt_one_minus_alpha, loss_weight):
        if tab is not None and (tab.dtype != torch.float32 or tab.numel() != t_len or not tab.is_contiguous()):
            raise MfhipError("train_batch_assemble: the schedule tables are contiguous fp32 tensors of one length")
    if timesteps.dtype != torch.int64 or timesteps.numel() != b:
        raise MfhipError(f"train_batch_assemble: timesteps is an int64 tensor of {b} entries")
    if not timesteps.is_cuda:
        if int(timesteps.min()) < 0 or int(timesteps.max()) >= t_len:
            raise MfhipError(f"train_batch_assemble: timesteps outside [0, {t_len})")
        timesteps = timesteps.to(dev)
    timesteps = timesteps.contiguous()
    ph, pw = masks.shape[-2:]
    for name, pl, ch in (("masks", masks, 1), ("depths", depths, 1), ("normals", normals, 3)):
        if pl is not None and (tuple(pl.shape) != (b, ch, ph, pw) or pl.dtype != torch.float32 or not pl.is_contiguous()):
            raise MfhipError(f"train_batch_assemble: {name} must be contiguous fp32 [{b}, {ch}, {ph}, {pw}], got {pl.dtype} {tuple(pl.shape)}")
    if (depths is not None and n > 2 and moments[2] is not None) or (normals is not None and n > 3 and moments[3] is not None):
        raise MfhipError("train_batch_assemble: depth / normals come as latents or as planes, not both")
    nlat = sum(1 for m in moments[2:] if m is not None)
    ctot = c + 1 + nlat * c + (1 if depths is not None else 0) + (3 if normals is not None else 0)
    shapes = {"latents": (b, c, h, w), "noisy_latents": (b, c, h, w), "target": (b, c, h, w), "conditioning_latents": (b, ctot, h, w),
              "timesteps_f32": (b,), "loss_weights": (b,)}
    res = {}
    for name in ASSEMBLE_OUTPUTS:
        if name == "loss_weights" and loss_weight is None:
            continue
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shapes[name], dtype=torch.float32, device=dev)
        elif not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != shapes[name] or not t.is_contiguous():
            raise MfhipError(f"train_batch_assemble: out[{name!r}] must be a contiguous fp32 device tensor of shape {shapes[name]}")
        res[name] = t
    arr = (C.c_void_p * n)(*[_ptr(m) for m in moments])
    pna = (C.c_void_p * n)(*[_ptr(p) for p in posterior_noise])
    _launch("mf_train_batch_assemble", arr, pna, n, dt_code(dt), ld, c, b, h, w, float(scaling), noise, timesteps, sqrt_alpha,
            sqrt_one_minus_alpha, loss_weight, t_len, masks, depths, normals, ph, pw, int(bool(v_prediction)), res["latents"],
            res["noisy_latents"], res["target"], res["conditioning_latents"], res["timesteps_f32"], res.get("loss_weights"))
    return res


# ---- random numbers (csrc/rng.hip; include/mfhip.h states the stream; rng.PhiloxGenerator keeps the (seed, offset) pair) ---------------
def _s64(v: int) -> int:
    """A 64-bit value as the int64_t the ABI carries it in (2^63 + 1 -> -(2^63 - 1)): the library reads the same 64 bits unsigned."""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def _philox_state(state: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if state is not None and (not state.is_cuda or state.dtype != torch.int64 or state.numel() != 2 or not state.is_contiguous()):
        raise MfhipError("a Philox device state is a contiguous int64 device tensor {seed, offset}")
    return state


def _count(what: str, **counts) -> None:
    """Counts are checked here, before an empty tensor's null address could speak for them; an empty draw launches nothing."""
    bad = {k: v for k, v in counts.items() if int(v) < 0}
    if bad:
        raise MfhipError(f"{what}: {', '.join(f'{k} = {v}' for k, v in bad.items())} must not be negative")


def philox_normal_blocks(samples: int, per_sample: int) -> int:
    n = load().mf_philox_normal_blocks(samples, per_sample)
    _check(-1 if n < 0 else 0, "mf_philox_normal_blocks")
    return n


def philox_int_blocks(n: int) -> int:
    r = load().mf_philox_int_blocks(n)
    _check(-1 if r < 0 else 0, "mf_philox_int_blocks")
    return r


def philox_bits_host(n: int, seed: int, offset: int = 0) -> torch.Tensor:
    """The stream's raw bits computed on the host (mf_philox_bits_host): an int32 host tensor holding the uint32 bit patterns."""
    _count("philox_bits_host", n=n)
    out = torch.empty(int(n), dtype=torch.int32)
    if n:
        _check(load().mf_philox_bits_host(out.data_ptr(), n, _s64(seed), _s64(offset)), "mf_philox_bits_host")
    return out


def philox_bits(n: int, seed: int, offset: int, device, state: Optional[torch.Tensor] = None) -> torch.Tensor:
    """n raw uint32 of the stream as an int32 device tensor (the bit patterns); `state` overrides (seed, offset)."""
    _count("philox_bits", n=n)
    out = torch.empty(int(n), dtype=torch.int32, device=device)
    _req_cuda(out, state)
    if n:
        _launch("mf_philox_bits", out, n, _s64(seed), _s64(offset), _philox_state(state))
    return out


def philox_normal(shape, seed: int, offset: int, device, scale: float = 1.0, first_sample: int = 0, global_batch: Optional[int] = None,
                  state: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 normals of shape [B, ...], drawn per sample: the rows [first_sample, first_sample + B) of a draw of global_batch rows."""
    shape = tuple(int(d) for d in shape)
    if not shape:
        raise MfhipError("philox_normal: a shape [B, ...] is needed (the draw is per sample)")
    b = shape[0]
    per = 1
    for d in shape[1:]:
        per *= d
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise MfhipError(f"philox_normal: out must be a contiguous fp32 tensor of shape {shape}")
    _req_cuda(out, state)
    g = b + first_sample if global_batch is None else int(global_batch)
    _count("philox_normal", first_sample=first_sample)
    if g < first_sample + b:
        raise MfhipError(f"philox_normal: global_batch {g} < first_sample {first_sample} + samples {b}")
    if out.numel():
        _launch("mf_philox_normal", out, b, per, float(scale), first_sample, g, _s64(seed), _s64(offset), _philox_state(state))
    return out


def philox_randint(high: int, n: int, seed: int, offset: int, device, first: int = 0, total: Optional[int] = None,
                   state: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [n] below `high`: the elements [first, first + n) of a draw of `total` integers."""
    _count("philox_randint", n=n, first=first)
    total = first + n if total is None else int(total)
    if not 0 < high <= 1 << 31 or total < first + n:
        raise MfhipError(f"philox_randint: high = {high} outside (0, 2^31], or total {total} < first {first} + n {n}")
    if out is None:
        out = torch.empty(int(n), dtype=torch.int64, device=device)
    elif out.dtype != torch.int64 or out.numel() != n or not out.is_contiguous():
        raise MfhipError(f"philox_randint: out must be a contiguous int64 tensor of {n} entries")
    _req_cuda(out, state)
    if n:
        _launch("mf_philox_randint", out, n, high, first, total, _s64(seed), _s64(offset), _philox_state(state))
    return out


def philox_advance(state: torch.Tensor, blocks: int) -> None:
    _req_cuda(state)
    _launch("mf_philox_advance", _philox_state(state), blocks)


def train_batch_draw(posterior_noise, noise: torch.Tensor, timesteps: torch.Tensor, high: int, seed: int, offset: int, first_sample: int = 0,
                     global_batch: Optional[int] = None, state: Optional[torch.Tensor] = None) -> int:
    """Everything train_batch_assemble reads as random input in one launch (mf_train_batch_draw): posterior_noise is 2 .. 4 fp32
    [B, c, h, w] tensors to fill (image, conditioning image, depth, normals; the last two may be None), then noise, then timesteps
    (int64 [B], below `high`).  Returns the blocks the draw consumes (what the generator advances by)."""
    pns = list(posterior_noise)
    if not 2 <= len(pns) <= 4 or pns[0] is None or pns[1] is None:
        raise MfhipError("train_batch_draw: 2 .. 4 posterior noise tensors, the image's and the conditioning image's present")
    b = noise.shape[0]
    per = noise.numel() // max(b, 1)
    for t in (*pns, noise):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != tuple(noise.shape) or not t.is_contiguous()):
            raise MfhipError(f"train_batch_draw: every noise tensor must be contiguous fp32 {tuple(noise.shape)}")
    if timesteps.dtype != torch.int64 or timesteps.numel() != b or not timesteps.is_contiguous():
        raise MfhipError(f"train_batch_draw: timesteps is a contiguous int64 tensor of {b} entries")
    _req_cuda(*pns, noise, timesteps, state)
    g = b + first_sample if global_batch is None else global_batch
    if noise.numel():
        arr = (C.c_void_p * len(pns))(*[_ptr(p) for p in pns])
        _launch("mf_train_batch_draw", arr, len(pns), noise, timesteps, b, per, high, first_sample, g, _s64(seed), _s64(offset), _philox_state(state))
    return (sum(1 for p in pns if p is not None) + 1) * philox_normal_blocks(g, per) + philox_int_blocks(g)


def postprocess(x: torch.Tensor, denormalize: bool = True, uint8: bool = False) -> torch.Tensor:
    """clamp(x / 2 + 0.5, 0, 1) as fp32 NCHW, or (uint8=True) round(. * 255) as uint8 NHWC."""
    _f32(x)
    x = x.contiguous()
    b, c, h, w = x.shape
    out = torch.empty((b, h, w, c) if uint8 else (b, c, h, w), dtype=torch.uint8 if uint8 else torch.float32, device=x.device)
    _launch("mf_postprocess", x, None if uint8 else out, out if uint8 else None, b, c, h * w, int(denormalize))
    return out


REGIONS = {None: 0, "": 0, "none": 0, "mask": 1, "mirror": 2}        # mf_image_metrics' region codes (dataset.py:62-68)


def image_metrics(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None, region=0,
                  data_range: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mf_image_metrics on uint8 NHWC device tensors [B, H, W, C] (mask: uint8 [B, H, W]): one mf_metrics_row per image as a uint8
    [B, sizeof(MetricsRow)] DEVICE tensor.  Nothing synchronises with the host; metrics_rows() reads the rows."""
    _req_cuda(pred, target, mask)
    region = REGIONS[region] if region in REGIONS else int(region)
    if pred.dtype != torch.uint8 or target.dtype != torch.uint8 or pred.dim() != 4 or pred.shape != target.shape:
        raise MfhipError("image_metrics: two uint8 [batch, height, width, channels] tensors of one shape")
    b, h, w, c = pred.shape
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (b, h, w)):
        raise MfhipError(f"image_metrics: the mask must be uint8 [{b}, {h}, {w}], got {mask.dtype} {tuple(mask.shape)}")
    pred, target = pred.contiguous(), target.contiguous()
    mask = None if mask is None else mask.contiguous()
    nbytes = load().mf_image_metrics_ws_bytes(b, h, w, c)
    if nbytes < 0:
        raise MfhipError(f"image_metrics: {load().mf_last_error().decode()}")
    ws = scratch("image_metrics", (nbytes + 3) // 4, pred.device)
    if out is None:
        out = torch.empty(b, C.sizeof(MetricsRow), dtype=torch.uint8, device=pred.device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != b * C.sizeof(MetricsRow) or out.device != pred.device:
        raise MfhipError(f"image_metrics: out must be a contiguous uint8 [{b}, {C.sizeof(MetricsRow)}] tensor on {pred.device}")
    _launch("mf_image_metrics", pred, target, mask, region, b, h, w, c, float(data_range), out, ws)
    return out


def metrics_rows(rows: torch.Tensor):
    """The rows of image_metrics() on the host, as a numpy record array with MetricsRow's fields (this is the synchronisation)."""
    import numpy as np
    return np.frombuffer(rows.cpu().numpy().tobytes(), dtype=np.dtype(MetricsRow))


def clip_preprocess(images: torch.Tensor, size: int, crop: int, patch: int, htab: Optional[torch.Tensor], hk: int,
                    vtab: Optional[torch.Tensor], vk: int, mean, std, out_dtype: torch.dtype, want_u8: bool = False):
    """mf_clip_preprocess on a uint8 [B, H, W, 3] device tensor: (patch matrix [B, (crop / patch)^2, K8] in out_dtype, the cropped uint8
    image [B, crop, crop, 3] or None).  htab / vtab: the int32 device tables of frontend.clip_resize_table (None: that pass is skipped)."""
    _req_cuda(images, htab, vtab)
    if images.dtype != torch.uint8 or images.dim() != 4:
        raise MfhipError("clip_preprocess: a uint8 [batch, height, width, 3] tensor")
    images = images.contiguous()
    b, h, w, c = images.shape
    nbytes = load().mf_clip_preprocess_ws_bytes(b, h, w, size, crop)
    if nbytes < 0:
        raise MfhipError(f"clip_preprocess: {load().mf_last_error().decode()}")
    ws = scratch("clip_preprocess", (nbytes + 3) // 4, images.device)
    k8 = (3 * patch * patch + 7) // 8 * 8
    n = (crop // max(patch, 1)) ** 2
    out = torch.empty(b, n, k8, dtype=out_dtype, device=images.device)
    u8 = torch.empty(b, crop, crop, 3, dtype=torch.uint8, device=images.device) if want_u8 else None
    _launch("mf_clip_preprocess", images, b, h, w, c, size, crop, patch, htab, hk, vtab, vk, *[float(v) for v in mean], *[float(v) for v in std],
            out, dt_code(out_dtype), k8, u8, ws)
    return out, u8


def clip_vision_embed(patches: torch.Tensor, class_embedding: torch.Tensor, pos_table: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """out[b][0] = class_embedding + pos_table[0], out[b][1 + i] = patches[b][i] + pos_table[1 + i] (mf_clip_vision_embed)."""
    _req_cuda(patches, class_embedding, pos_table)
    b, n, hidden = patches.shape
    if (not patches.is_contiguous() or not pos_table.is_contiguous() or tuple(pos_table.shape) != (n + 1, hidden)
            or tuple(class_embedding.shape) != (hidden,) or not patches.dtype == class_embedding.dtype == pos_table.dtype):
        raise MfhipError(f"clip_vision_embed: contiguous patches [B, n, hidden], class_embedding [hidden] and pos_table [n + 1, hidden] of one "
                         f"dtype (got {tuple(patches.shape)}, {tuple(class_embedding.shape)}, {tuple(pos_table.shape)})")
    out = torch.empty(b, n + 1, hidden, dtype=out_dtype, device=patches.device)
    _launch("mf_clip_vision_embed", patches, class_embedding, pos_table, dt_code(patches.dtype), out, dt_code(out_dtype), b, n + 1, hidden)
    return out


def clip_score(image_feats: torch.Tensor, text_feats: torch.Tensor):
    """mf_clip_score: (100 cos(i, t) per row [B], the norms [B, 2]) of two fp32 [B, P] device tensors.  Nothing synchronises."""
    _req_cuda(image_feats, text_feats)
    if image_feats.dtype != torch.float32 or text_feats.dtype != torch.float32 or image_feats.dim() != 2 or image_feats.shape != text_feats.shape:
        raise MfhipError(f"clip_score: two fp32 [batch, dim] tensors of one shape (got {tuple(image_feats.shape)}, {tuple(text_feats.shape)})")
    i, t = image_feats.contiguous(), text_feats.contiguous()
    out = torch.empty(i.shape[0], dtype=torch.float32, device=i.device)
    norms = torch.empty(i.shape[0], 2, dtype=torch.float32, device=i.device)
    _launch("mf_clip_score", i, t, i.shape[0], i.shape[1], out, norms)
    return out, norms


LPIPS_LAYERS = 7


def lpips_prepare(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor], region, unit_range: bool,
                  out_dtype: torch.dtype) -> torch.Tensor:
    """mf_lpips_prepare on uint8 NHWC device tensors [B, H, W, 3] (mask: uint8 [B, H, W]): the normalised, scaled input of the LPIPS
    network as [2 B, H, W, 8] in out_dtype (pred images first, channels 3 .. 7 zero)."""
    _req_cuda(pred, gt, mask)
    region = REGIONS[region] if region in REGIONS else int(region)
    if pred.dtype != torch.uint8 or gt.dtype != torch.uint8 or pred.dim() != 4 or pred.shape != gt.shape:
        raise MfhipError("lpips_prepare: two uint8 [batch, height, width, 3] tensors of one shape")
    b, h, w, c = pred.shape
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (b, h, w)):
        raise MfhipError(f"lpips_prepare: the mask must be uint8 [{b}, {h}, {w}], got {mask.dtype} {tuple(mask.shape)}")
    pred, gt = pred.contiguous(), gt.contiguous()
    mask = None if mask is None else mask.contiguous()
    out = torch.empty(2 * b, h, w, 8, dtype=out_dtype, device=pred.device)
    _launch("mf_lpips_prepare", pred, gt, mask, region, b, h, w, c, int(bool(unit_range)), out, dt_code(out_dtype))
    return out


def relu_(x: torch.Tensor) -> torch.Tensor:
    """mf_relu: max(x, 0) in place.  x is [..., channels] with unit channel stride and ONE stride between its rows (a contiguous tensor
    or a channel slice of one): what a GEMM wrote through out / ldc."""
    _req_cuda(x)
    c = x.shape[-1]
    rows = x.numel() // max(c, 1)
    ld = x.stride(-2) if x.dim() >= 2 else c
    flat = x.dim() < 2 or all(x.stride(i) == x.stride(i + 1) * x.shape[i + 1] for i in range(x.dim() - 2))
    if x.stride(-1) != 1 or not flat:
        raise MfhipError(f"relu_: rows of unit-stride channels, one stride apart (got shape {tuple(x.shape)}, strides {x.stride()})")
    _launch("mf_relu", x, dt_code(x.dtype), rows, c, ld)
    return x


def maxpool3s2_ceil(x: torch.Tensor) -> torch.Tensor:
    """mf_maxpool3s2_ceil: MaxPool2d(3, 2, ceil_mode=True) over a contiguous NHWC tensor."""
    _req_cuda(x)
    if x.dim() != 4 or not x.is_contiguous():
        raise MfhipError("maxpool3s2_ceil: a contiguous [batch, height, width, channels] tensor")
    b, h, w, c = x.shape
    out = torch.empty(b, max(-(-(h - 3) // 2) + 1, 1), max(-(-(w - 3) // 2) + 1, 1), c, dtype=x.dtype, device=x.device)
    _launch("mf_maxpool3s2_ceil", x, out, dt_code(x.dtype), b, h, w, c)
    return out


def lpips_ws(batch: int, device) -> torch.Tensor:
    nbytes = load().mf_lpips_ws_bytes(batch)
    if nbytes < 0:
        raise MfhipError(f"lpips: {load().mf_last_error().decode()}")
    return scratch("lpips", (nbytes + 3) // 4 + 2, device)


def lpips_layer(feat: torch.Tensor, weight: torch.Tensor, layer: int, ws: torch.Tensor) -> None:
    """mf_lpips_layer: feat [2 B, h, w, C] (image b against image B + b), weight fp32 [C]; the partial sums go to slot `layer` of ws."""
    _req_cuda(feat, weight, ws)
    if feat.dim() != 4 or feat.shape[0] % 2 or not feat.is_contiguous() or weight.dtype != torch.float32 or weight.numel() != feat.shape[-1]:
        raise MfhipError(f"lpips_layer: a contiguous [2 B, h, w, C] feature and C fp32 weights (got {tuple(feat.shape)}, {tuple(weight.shape)})")
    b2, h, w, c = feat.shape
    _launch("mf_lpips_layer", feat, dt_code(feat.dtype), weight.contiguous(), b2 // 2, h * w, c, layer, ws)


def lpips_finish(ws: torch.Tensor, batch: int) -> torch.Tensor:
    """mf_lpips_finish: the fp32 [B, 7] DEVICE row of per-layer sums.  Nothing synchronises with the host."""
    _req_cuda(ws)
    out = torch.empty(batch, LPIPS_LAYERS, dtype=torch.float32, device=ws.device)
    _launch("mf_lpips_finish", ws, batch, out)
    return out


def _sel_ws(device) -> torch.Tensor:
    return scratch("select", load().mf_select_ws_bytes() // 4 + 8, device)


def depth_percentile_normalize(depth: torch.Tensor, signed_range: bool = True) -> torch.Tensor:
    """apply_transforms_depth(normalization_method="percentile"): clip to the [2 %, 98 %] percentiles and map to the range."""
    import math
    _f32(depth)
    depth = depth.contiguous()
    n = depth.numel()
    ranks, ts = [], []
    for q in (2.0, 98.0):
        pos = q / 100.0 * (n - 1)
        lo = math.floor(pos)
        ranks += [lo, min(lo + 1, n - 1)]
        ts.append(pos - lo)
    rk = torch.tensor(ranks, dtype=torch.int64).to(depth.device)
    vals = torch.empty(4, dtype=torch.float32, device=depth.device)
    out = torch.empty_like(depth)
    _launch("mf_depth_percentile_normalize", depth, out, n, rk, ts[0], ts[1], int(signed_range), vals, _sel_ws(depth.device))
    return out


def select_ranks(x: torch.Tensor, ranks) -> torch.Tensor:
    """The order statistics x_(r) (0-based, ascending) for up to four ranks, on the device."""
    _f32(x)
    x = x.contiguous()
    rk = torch.tensor(list(ranks), dtype=torch.int64).to(x.device)
    vals = torch.empty(len(ranks), dtype=torch.float32, device=x.device)
    _launch("mf_select_ranks", x, x.numel(), rk, len(ranks), vals, _sel_ws(x.device))
    return vals


def bicubic_resize_crop(x: torch.Tensor, resized: tuple, crop: tuple, out_hw: tuple, a: float = 1.0, b: float = 0.0,
                        antialias: bool = False) -> torch.Tensor:
    """x [planes, H, W] fp32 -> a * bicubic(x -> resized)[crop window of out_hw at (top, left) = crop] + b.  antialias: PyTorch's
    antialiased kernel (F.interpolate(..., antialias=True): torchvision 0.18's Resize on tensors) instead of the plain one."""
    _f32(x)
    x = x.contiguous()
    planes, h, w = x.shape
    out = torch.empty(planes, out_hw[0], out_hw[1], dtype=torch.float32, device=x.device)
    _launch("mf_bicubic_aa_resize_crop" if antialias else "mf_bicubic_resize_crop", x, out, planes, h, w, int(resized[0]), int(resized[1]),
            int(crop[0]), int(crop[1]), int(out_hw[0]), int(out_hw[1]), a, b)
    return out


def axpby_affine(x: torch.Tensor, a: float, b: float) -> torch.Tensor:
    """a * x + b on fp32 planes (the bicubic kernel at scale 1 is the identity: reuse it as the affine map)."""
    planes, h, w = x.shape
    return bicubic_resize_crop(x, (h, w), (0, 0), (h, w), a, b)


def hwc_to_chw_affine(x: torch.Tensor, a: float, b: float) -> torch.Tensor:
    _f32(x)
    x = x.contiguous()
    h, w, c = x.shape
    out = torch.empty(c, h, w, dtype=torch.float32, device=x.device)
    _launch("mf_hwc_to_chw_affine", x, out, h * w, c, a, b)
    return out


def depth_normalize(depth: torch.Tensor, mask: Optional[torch.Tensor] = None, max_scene_depth: float = 5.0, delta: float = 0.5,
                    signed_range: bool = True) -> torch.Tensor:
    _f32(depth, mask)
    depth = depth.contiguous()
    out = torch.empty_like(depth)
    _launch("mf_depth_normalize", depth, mask.contiguous() if mask is not None else None, out, depth.numel(), max_scene_depth, delta,
            int(signed_range), _mm_ws(depth.device))
    return out


# ---- LoRA adapters merged on the device (csrc/lora.hip) --------------------------------------------------------------------------
class LoraTables:
    """The target / term tables of mf_lora_merge for `targets` = [(base, out, [(up, down), ...]), ...]: fp32 device tensors, base / out
    [rows, cols], up [rows, rank], down [rank, cols], all contiguous.  Built once per adapter set (host -> device copies: never inside a
    capture); `coef` (one float per term, device) is the only thing a new scale rewrites.  Keeps every tensor it points to alive."""

    def __init__(self, targets, device):
        lib = load()
        self.keep = []
        tg, tm = [], []
        tiles = 0
        for base, out, pairs in targets:
            _f32(base, out)
            rows, cols = base.shape
            if tuple(out.shape) != (rows, cols) or not (base.is_contiguous() and out.is_contiguous()):
                raise MfhipError("lora: base and out are contiguous fp32 [rows, cols] of one shape")
            if not pairs:
                raise MfhipError("lora: a target without a term")
            tg.append(LoraTarget(base.data_ptr(), out.data_ptr(), rows, cols, len(tm), len(pairs), tiles))
            n = lib.mf_lora_tiles(rows, cols)
            if n < 0:
                raise MfhipError(f"mf_lora_tiles failed: {lib.mf_last_error().decode()}")
            tiles += n
            self.keep += [base, out]
            for up, down in pairs:
                _f32(up, down)
                if up.dim() != 2 or down.dim() != 2 or up.shape[0] != rows or down.shape[1] != cols or up.shape[1] != down.shape[0] \
                        or not (up.is_contiguous() and down.is_contiguous()):
                    raise MfhipError(f"lora: up {tuple(up.shape)} / down {tuple(down.shape)} do not fit a [{rows}, {cols}] weight")
                tm.append(LoraTerm(up.data_ptr(), down.data_ptr(), up.shape[1], 0))
                self.keep += [up, down]
        if not tg:
            raise MfhipError("lora: no targets")
        self.targets = (LoraTarget * len(tg))(*tg)
        self.terms = (LoraTerm * len(tm))(*tm)
        self.ntargets, self.nterms, self.tiles = len(tg), len(tm), tiles
        as_dev = lambda arr: torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
        self.targets_dev, self.terms_dev = as_dev(self.targets), as_dev(self.terms)
        self.coef = torch.zeros(len(tm), dtype=torch.float32, device=device)
        # bytes one merge moves: base read + out written, and each term's factors once (their re-reads come from the caches)
        self.bytes = sum(8 * b.numel() for b, _, _ in targets) + sum(4 * (u.numel() + d.numel()) for _, _, ps in targets for u, d in ps)


def lora_merge(tables: LoraTables, coef=None) -> None:
    """out_t = base_t + sum_terms coef * up @ down for every target of the tables, one launch (mf_lora_merge).  `coef`: the per-term
    factors (a sequence or tensor of nterms floats) to upload first; None keeps tables.coef as it is."""
    if coef is not None:
        c = torch.as_tensor(coef, dtype=torch.float32).reshape(-1)
        if c.numel() != tables.nterms:
            raise MfhipError(f"lora_merge: {c.numel()} coefficients for {tables.nterms} terms")
        tables.coef.copy_(c)
    _req_cuda(tables.coef, tables.targets_dev, tables.terms_dev)
    _launch("mf_lora_merge", C.cast(tables.targets, C.c_void_p), C.cast(tables.terms, C.c_void_p), tables.targets_dev, tables.terms_dev,
            tables.coef, tables.ntargets, tables.nterms)
