"""mf_conv_up2x without a GPU: the weight fold and the float64 model of the entry's formula (tests/up2x_ref.py) against the conv they
replace, the entry's host-side plan (mf_conv_up2x_plan: every check and choice, nothing launched), its refusals, and its tables."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import abi_header
import up2x_ref
from reflecting_reality_amd import hip, ops, program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MF_EINVAL = -1
# (B, C, H, W, N): borders, a non-square input, a single pixel
SHAPES = [(2, 8, 3, 5, 6), (1, 8, 1, 1, 4), (2, 16, 4, 12, 8)]


@pytest.mark.parametrize("b,c,h,w,n", SHAPES)
def test_fold_and_model_equal_the_conv_over_the_upsampled_image(b, c, h, w, n):
    """fold_phase_weights + the model of the entry's formula == F.conv2d(F.interpolate(x, 2, nearest), w, padding=1) to 1e-12 relative,
    in float64: the identity itself, zero padding included."""
    g = torch.Generator().manual_seed(1000 * h + w)
    x = torch.randn(b, c, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(n, c, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(n, generator=g, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, bias, padding=1).permute(0, 2, 3, 1).reshape(-1, n)
    w4 = ops.fold_phase_weights(wt).reshape(4, n, 4 * c)
    got, s = up2x_ref.model(x.permute(0, 2, 3, 1), w4, bias)
    rel = float((got - want).abs().max() / want.abs().max())
    print(f"({b}, {c}, {h}, {w}, {n}): max |model - conv| / max |conv| = {rel:.3e}")
    assert got.shape == want.shape and rel <= 1e-12
    assert bool((s >= got.abs() - 1e-9).all()), "S bounds the value"


def test_phase_weights_are_summed_in_fp32_and_rounded_once():
    g = torch.Generator().manual_seed(7)
    wt = torch.randn(12, 10, 3, 3, generator=g)
    bias = torch.randn(12, generator=g)
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        pw = ops.PhaseWeight(wt, bias, ops.Precision.get(name), "cpu")
        assert pw.w.shape == (4, 12, 4 * 16) and pw.w.dtype == dt and pw.cin_pad == 16 and pw.n == 12
        want = F.pad(ops.fold_phase_weights(wt.float()), (0, 6)).reshape(4, 12, 64).to(dt)      # fp32 sums, ONE rounding
        assert torch.equal(pw.w, want)
        assert bool((pw.w.view(4, 12, 4, 16)[..., 10:] == 0).all()), "padded channels are zero"
        assert torch.equal(pw.bias, bias)
    with pytest.raises(hip.MfhipError):
        ops.PhaseWeight(wt, bias, ops.Precision.get("fp32"), "cpu")


def _desc(**kw) -> hip.GemmDesc:
    """A bf16 descriptor of the entry on made-up (16-byte aligned, never dereferenced) addresses: B 2, 16 x 16 -> 32 x 32, C 128, N 320."""
    d = hip.GemmDesc()
    d.dtype = d.a_dtype = d.out_dtype = hip.MF_BF16
    d.a0, d.w, d.out, d.bias = 0x10000, 0x20000, 0x30000, 0x40000
    d.c0, d.lda0, d.ldw, d.n, d.ldc = 128, 128, 512, 320, 320
    d.w_zs_o = 320 * 512
    d.batch, d.h_in, d.w_in, d.h_out, d.w_out = 2, 16, 16, 32, 32
    d.kh, d.kw, d.stride, d.pad_t, d.pad_l, d.upsample = 2, 2, 1, 1, 1, 1
    d.nz, d.zdiv, d.alpha = 1, 1, 1.0
    d.ld_res0 = d.ld_res1 = 320
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _plan(d):
    plan = hip.GemmPlan()
    rc = hip.load().mf_conv_up2x_plan(C.byref(d), C.byref(plan))
    return rc, plan


def test_plan_reports_the_launch():
    rc, plan = _plan(_desc())
    assert rc == 0 and plan.tile in hip.UP2X_TILES and plan.splitk == 1 and plan.reduce_launch == 0 and plan.gn_part_rows == 0
    bm = {42: 256, 43: 128, 48: 128}
    for tile in hip.UP2X_TILES:
        rc, plan = _plan(_desc(tile=tile))
        assert rc == 0 and plan.tile == tile and plan.blocks == (512 // bm[tile]) * 2 * 4        # row tiles x column tiles x phases
    rows = C.c_int32(0)
    rc, plan = _plan(_desc(tile=48, gn_part=0x50000, gn_part_floats=2 * 320 * (2048 // 32), gn_part_rows=C.addressof(rows)))
    assert rc == 0 and plan.gn_part_rows == 128, "the epilogue's sums: one block of the tile's rows inside one low-resolution image"
    rc, plan = _plan(_desc(tile=48, splitk=2, ws=0x60000, ws_floats=2 * 2048 * 320))
    assert rc == 0 and plan.splitk == 2 and plan.reduce_launch == 1 and plan.blocks == 4 * 2 * 4 * 2
    rc, _ = _plan(_desc(tile=48, splitk=2, ws=0x60000, ws_floats=2 * 2048 * 320 - 1))
    assert rc == MF_EINVAL, "the slabs hold the full-resolution output"


REFUSED = {
    "nz": dict(nz=2), "temb": dict(temb=0x70000), "ln_colsum": dict(ln_colsum=0x70000, ln_eps=1e-5), "vt_out": dict(vt_out=0x70000, vt_n0=160, vt_tokens=256),
    "geglu": dict(act=hip.ACT_GEGLU4), "two segments": dict(a1=0x70000, c1=128), "a_scale": dict(a_scale=0x70000), "w_scale": dict(w_scale=0x70000),
    "bias_mode": dict(bias_mode=1), "defer_reduce": dict(defer_reduce=1), "3x3 taps": dict(kh=3, kw=3), "stride": dict(stride=2),
    "no upsample": dict(upsample=0), "extent": dict(h_out=16, w_out=16), "fp32": dict(dtype=hip.MF_F32, a_dtype=hip.MF_F32),
    "f16x3": dict(dtype=hip.MF_F16X3, a_dtype=hip.MF_F32), "fp32 activations": dict(a_dtype=hip.MF_F32), "w_split": dict(w_split=1),
    "tile": dict(tile=50), "fp16 output of a bf16 call": dict(out_dtype=hip.MF_F16), "ldw": dict(ldw=256), "channels": dict(c0=4, lda0=4),
    "res1_rows": dict(res1=0x70000, res1_rows=1000),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals(what):
    rc, _ = _plan(_desc(**REFUSED[what]))
    msg = hip.load().mf_last_error().decode()
    assert rc == MF_EINVAL and msg.startswith("mf_conv_up2x"), (what, rc, msg)


def test_the_entry_is_declared_exported_and_bound_and_the_abi_version_stays():
    protos = abi_header.prototypes()
    lib = hip.load()
    for name, sig in (("mf_conv_up2x", "i:Gp"), ("mf_conv_up2x_plan", "i:GP")):
        assert name in protos and name in hip.EXPORTS and hasattr(lib, name) and hip.SIGNATURES[name] == sig
        assert hip.SIGNATURES[name] == hip.SIGNATURES[name.replace("conv_up2x", "gemm_conv")], "the same struct, unchanged"
    assert lib.mf_abi_version() == hip.ABI_VERSION and lib.mf_sizeof_gemm_desc() == C.sizeof(hip.GemmDesc)      # additive entries only


def test_the_thunk_has_a_table_of_its_own():
    """csrc/program.hip's kUpFns restates program.SIGNATURES_UP; the pinned tables of a denoise step and of a call's two ends stay as
    they are, and the recorder takes the entry's descriptor like mf_gemm_conv's."""
    src = open(os.path.join(ROOT, "reflecting-reality_amd", "csrc", "program.hip")).read()
    table = dict(re.findall(r'\{U_\w+,\s*"(mf_\w+)",\s*"(\w+)"\}', src))
    assert table == program.SIGNATURES_UP == {"mf_conv_up2x": "d"}
    assert not set(table) & (set(program.SIGNATURES) | set(program.SIGNATURES_CALL) | set(program.SIGNATURES_NOISE))
    assert program._ALL_SIGNATURES["mf_conv_up2x"] == program.SIGNATURES["mf_gemm_conv"]
    assert "mf_conv_up2x_plan" in program._PASS_THROUGH
