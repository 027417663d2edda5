"""mf_conv_up2x on the GPU: the entry on its own against the float64 model of its own descriptor (tests/up2x_ref.py) with the phase
weights exactly as stored, under the launch audit's bound (tests/gemm_ref.py: 0.5 ulp + 2^-18 S per element of a 16-bit output, the
partial GroupNorm sums within the summed bounds of their rows) on sentinel-filled buffers with guard tails; its accuracy relative to
conv2d(upsample=True) on the same inputs and fp32 master weights; and the routing of the models (attribute, LoRA rebuild, autograd tape)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import gemm_ref as G  # noqa: E402
import up2x_ref  # noqa: E402
from reflecting_reality_amd import autograd, hip, models as M, ops, program, synth  # noqa: E402
from util import ENV_K_LINF, ENV_K_LINF_SMALL, ENV_K_MEAN, ENV_SMALL_NUMEL  # noqa: E402

DEV = "cuda"
GUARD = 4096
MF_EINVAL = -1
DT = {"bf16": (torch.bfloat16, hip.MF_BF16), "fp16": (torch.float16, hip.MF_F16)}
# (B, H, W, C, N): a tile spans two images; W not a power of two and an N tail; W larger than the tile's rows; two K tiles per tap
# and N no multiple of the tile; C no multiple of a K tile (64): a K tile straddles two taps, the general staging path
SHAPES = [(2, 8, 8, 64, 64), (2, 4, 12, 64, 96), (1, 2, 256, 64, 160), (2, 16, 16, 128, 200), (1, 4, 4, 72, 40)]
# res0_silu (both residuals, alpha, SiLU) is held to the per-element bound only: SiLU's flat minimum at -0.278 piles outputs up below a
# binade edge, so e = (got - ref) / ulp(ref) of a CORRECTLY rounded result is not uniform there — an IEEE fp32 evaluation of the same
# epilogue on an exact accumulator gives mean(e^2) = 0.0850 (bf16) / 0.0842 (fp16) on these inputs, above the audit's 1/12 + 6 sigma
VARIANTS = ("bias", "res1", "res1_shared", "res0_silu", "gn_part", "splitk")
_cases = {}


class Buf:
    """`n` elements of `dtype` followed by a GUARD-byte tail, every byte `fill` to begin with."""

    def __init__(self, n, dtype, fill):
        self.es = torch.tensor([], dtype=dtype).element_size()
        self.raw = torch.full((n * self.es + GUARD,), fill, dtype=torch.uint8, device=DEV)
        self.nbytes, self.fill = n * self.es, fill
        self.t = self.raw[: self.nbytes].view(dtype)

    def guard_ok(self):
        return bool((self.raw[self.nbytes:] == self.fill).all())

    def untouched(self):
        return bool((self.raw == self.fill).all())


def case(shape, prec):
    """Inputs of one (shape, dtype), made once and left unchanged: activations, phase weights as stored, bias, a residual."""
    key = (shape, prec)
    if key not in _cases:
        b, h, w, c, n = shape
        dt = DT[prec][0]
        g = torch.Generator().manual_seed(hash(shape) % 1000 + (7 if prec == "fp16" else 0))
        x = torch.randn(b, h, w, c, generator=g).to(dt).to(DEV)
        wt = torch.randn(n, c, 3, 3, generator=g) / (9 * c) ** 0.5
        pw = ops.PhaseWeight(wt, torch.randn(n, generator=g), ops.Precision.get(prec), DEV)
        res = torch.randn(4 * b * h * w, n, generator=g).to(dt).to(DEV)
        _cases[key] = (x, pw, res)
    return _cases[key]


def launch(shape, prec, x, pw, *, tile=0, splitk=0, res0=None, res1=None, res1_rows=0, gn=False, groups=0, alpha=1.0, act=hip.ACT_NONE, **over):
    """One mf_conv_up2x call on sentinel-filled buffers; returns (rc, out Buf, part Buf or None, rows per block, grouped)."""
    b, h, w, c, n = shape
    dt = DT[prec][0]
    m_out = 4 * b * h * w
    out = Buf(m_out * n, dt, G.SENTINEL)
    d = hip._up2x_desc(x, pw.w, out.t, c0=c, batch=b, h_in=h, w_in=w, n=n, bias=pw.bias, res0=res0, res1=res1, res1_rows=res1_rows,
                       alpha=alpha, act=act, splitk=splitk, tile=tile)
    ws = None
    if splitk > 1:
        ws = Buf(splitk * m_out * n, torch.float32, 0xFF)          # NaN: a slab read before it was written shows
        d.ws, d.ws_floats = ws.t.data_ptr(), ws.t.numel()
    part = rows = grouped = None
    if gn:
        part = Buf(2 * n * (m_out // 32), torch.float32, 0xFF)
        rows, grouped = C.c_int32(0), C.c_int32(0)
        d.gn_part, d.gn_part_floats, d.gn_part_rows = part.t.data_ptr(), part.t.numel(), C.addressof(rows)
        d.gn_groups, d.gn_grouped = groups, C.addressof(grouped)
    for k, v in over.items():
        setattr(d, k, v)
    torch.cuda.synchronize()
    rc = hip.load().mf_conv_up2x(C.byref(d), hip._stream())
    torch.cuda.synchronize()
    for name, buf in (("out", out), ("ws", ws), ("gn_part", part)):
        assert buf is None or buf.guard_ok(), f"{name}: the launch wrote into the {GUARD}-byte guard tail"
    return rc, out, part, (rows.value if rows is not None else 0), (grouped.value if grouped is not None else 0), d


def check_gn(part, r, fused, groups, shape, v, bnd):
    """The (sum, sum of squares) per channel of every block of R rows — in the epilogue's (image, phase, block) order when it made
    them, blocks of R consecutive output rows when the column-sum launch did — within the audit's tolerance (gemm_ref.check_gn_part)."""
    b, h, w, c, n = shape
    m_out = 4 * b * h * w
    blocks = up2x_ref.gn_block_rows(b, h, w, r) if fused else torch.arange(m_out).view(-1, r)
    assert blocks.shape[0] == m_out // r and sorted(blocks.flatten().tolist()) == list(range(m_out))
    per_image = blocks.shape[0] // b
    for i in range(b):      # what mf_groupnorm needs of the order: an image's partial rows are contiguous
        rows_i = blocks[i * per_image: (i + 1) * per_image].flatten()
        assert int(rows_i.min()) == i * 4 * h * w and int(rows_i.max()) == (i + 1) * 4 * h * w - 1
    part = part.double()
    fails = []
    for k, rows in enumerate(blocks.to(v.device)):
        vb, bb = v[rows], bnd[rows]
        want = torch.stack([vb.sum(0), (vb * vb).sum(0)], 1)
        tol = torch.stack([bb.sum(0) + 2.0 ** -20 * vb.abs().sum(0), (bb * (2 * vb.abs() + bb)).sum(0) + 2.0 ** -20 * (vb * vb).sum(0)], 1)
        got = part[2 * k * n: 2 * (k + 1) * n].view(n, 2)
        if bool((((got - want).abs() > tol) | ~torch.isfinite(got)).any()):
            fails.append(f"partial row {k}")
        if groups:
            cpg = n // groups
            base = 2 * n * (m_out // r) + 2 * k * groups
            gg = part[base: base + 2 * groups].view(groups, 2)
            gw, gt = want.view(groups, cpg, 2).sum(1), tol.view(groups, cpg, 2).sum(1)
            if bool((((gg - gw).abs() > gt) | ~torch.isfinite(gg)).any()):
                fails.append(f"group sums of partial row {k}")
    return fails


@pytest.mark.parametrize("prec", list(DT))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_entry_against_the_float64_model_of_its_descriptor(shape, prec):
    b, h, w, c, n = shape
    x, pw, res = case(shape, prec)
    code = DT[prec][1]
    m_out = 4 * b * h * w
    bm, bn = C.c_int(), C.c_int()
    fails = []
    for variant in VARIANTS:
        kw, mkw = {}, {}
        if variant == "res1":
            kw, mkw = dict(res1=res), dict(res1=res)
        elif variant == "res1_shared":
            half = res[: m_out // 2].contiguous()
            kw, mkw = dict(res1=half, res1_rows=m_out // 2), dict(res1=half, res1_rows=m_out // 2)
        elif variant == "res0_silu":
            half = res[: m_out // 2].contiguous()
            kw, mkw = dict(res1=half, res1_rows=m_out // 2, res0=res, alpha=0.5, act=hip.ACT_SILU), dict(res1=half, res1_rows=m_out // 2, res0=res, alpha=0.5, silu=True)
        elif variant == "gn_part":
            kw = dict(gn=True, groups=32 if n % 32 == 0 else 0, splitk=1)      # (1: no split-K — the sums come from the epilogue where a block's rows lie in one image)
        elif variant == "splitk":
            kw = dict(splitk=2, gn=True)
        v, s = up2x_ref.model(x, pw.w, pw.bias, **mkw)
        bnd = G.bound(v, s, code)
        for tile in hip.UP2X_TILES:
            what = f"{variant}, tile {tile}"
            rc, out, part, r, grouped, d = launch(shape, prec, x, pw, tile=tile, **kw)
            assert rc == 0, f"{what}: refused: {hip.load().mf_last_error().decode()}"
            assert not bool((out.raw[: out.nbytes].view(-1, out.es) == G.SENTINEL).all(1).any()), f"{what}: elements never written"
            verdict = G.compare(out.t.view(m_out, n), v, s, code, what)
            print(f"{shape} {prec} {what}: max {verdict.max_ulp:.3f} ulp, worst error / bound {verdict.worst:.3f}, mean e {verdict.mean_e:+.4f}, "
                  f"rms e {verdict.rms_e:.4f} over {verdict.n_stat}" + (f", gn rows {r} grouped {grouped}" if part is not None else ""))
            if variant == "res0_silu":
                got = out.t.view(m_out, n).double()
                if not bool((torch.isfinite(got) & ((got - v).abs() <= bnd)).all()):
                    fails.append(f"{what}: elements outside the bound")
            elif not verdict.ok:
                fails.append(verdict.msg)
            if part is not None:
                hip.load().mf_gemm_tile_shape(tile, C.byref(bm), C.byref(bn))
                fused = variant == "gn_part" and (h * w) % bm.value == 0
                assert r == (bm.value if fused else (128 if (4 * h * w) % 128 == 0 else 64 if (4 * h * w) % 64 == 0 else 32)), (what, r)
                assert not grouped or fused
                fails += [f"{what}: {m}" for m in check_gn(part.t, r, fused, kw.get("groups", 0) if grouped else 0, shape, v, bnd)]
    assert not fails, "\n".join(fails)


# what: (a pointer field that gets real device memory, or None; the other fields)
REFUSED = {
    "nz": (None, dict(nz=2)), "temb": ("temb", dict(ld_temb=64)), "ln_colsum": ("ln_colsum", dict(ln_eps=1e-5)),
    "vt_out": ("vt_out", dict(vt_n0=32, vt_tokens=64, vt_ld=64)), "geglu": (None, dict(act=hip.ACT_GEGLU4)),
    "two segments": ("a1", dict(c1=64, lda1=64)), "a_scale": ("a_scale", {}), "w_scale": ("w_scale", {}), "bias_mode": (None, dict(bias_mode=1)),
    "defer_reduce": (None, dict(defer_reduce=1)), "3x3 taps": (None, dict(kh=3, kw=3)), "no upsample": (None, dict(upsample=0)),
    "tile": (None, dict(tile=50)), "extent": (None, dict(h_out=8, w_out=8)), "fp16 output of a bf16 call": (None, dict(out_dtype=hip.MF_F16)),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused_combinations_write_nothing(what):
    shape = SHAPES[0]
    x, pw, res = case(shape, "bf16")
    field, over = REFUSED[what]
    extra = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    if field is not None:
        over = {field: extra.data_ptr(), **over}
    rc, out, part, _, _, _ = launch(shape, "bf16", x, pw, gn=True, **over)
    assert rc == MF_EINVAL and hip.load().mf_last_error().decode().startswith("mf_conv_up2x"), (what, rc)
    assert out.untouched() and part.untouched(), f"{what}: a refused call wrote"


@pytest.mark.parametrize("prec", list(DT))
def test_accuracy_relative_to_the_3x3_path(prec):
    """The same activations and fp32 master weights through conv2d(upsample=True) and through the phase path, each against float64 on the
    UNROUNDED weights: the phase path's error stays inside the project's two-independent-rounding-draws margins of the 3x3 path's."""
    b, h, w, c, n = 2, 16, 16, 128, 320
    g = torch.Generator().manual_seed(5)
    dt = DT[prec][0]
    x = torch.randn(b, h, w, c, generator=g).to(dt)
    wt = torch.randn(n, c, 3, 3, generator=g) / (9 * c) ** 0.5
    bias = torch.randn(n, generator=g)
    ref = F.conv2d(F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), wt.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
    p = ops.Precision.get(prec)
    old = ops.conv2d(x.to(DEV), ops.ConvWeight(wt, bias, p, DEV), upsample=True).double().cpu()
    new = ops.conv_up2x(x.to(DEV), ops.PhaseWeight(wt, bias, p, DEV)).double().cpu()
    e_old, e_new = (old - ref).abs(), (new - ref).abs()
    k_linf = ENV_K_LINF if ref.numel() >= ENV_SMALL_NUMEL else ENV_K_LINF_SMALL
    r_linf, r_mean = float(e_new.max() / e_old.max()), float(e_new.mean() / e_old.mean())
    print(f"UP2X_ACCURACY {prec}: 3x3 path L-inf {float(e_old.max()):.4e} mean {float(e_old.mean()):.4e}; phase path L-inf {float(e_new.max()):.4e} "
          f"mean {float(e_new.mean()):.4e}; ratio L-inf {r_linf:.3f} (limit {k_linf}) mean {r_mean:.3f} (limit {ENV_K_MEAN})")
    assert r_linf <= k_linf and r_mean <= ENV_K_MEAN


# ---- the models' routing ---------------------------------------------------------------------------------------------------------------
CFG = dict(in_channels=4, out_channels=4, block_out_channels=(64, 64), layers_per_block=1, down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
           up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), cross_attention_dim=32, attention_head_dim=8, norm_num_groups=32)
UPCONV = "up_blocks.0.upsamplers.0.conv"


def nets(prec, phases, sd=None):
    """A tiny UNet + BrushNet (16 x 16 latents: the upsamplers run 8 x 8 -> 16 x 16); `phases`: the routing attribute, with the per-level
    table opened for this level (the measured table keeps it on the 3x3 path)."""
    from reflecting_reality_amd.configs import brushnet_config
    unet = M.UNet2DConditionModel(dict(CFG), precision=prec, device=DEV)
    unet.load_state_dict(sd if sd is not None else synth.state_dict_for(unet.param_shapes(), 0))
    bn = M.BrushNetModel(dict(brushnet_config(CFG, 5)), precision=prec, device=DEV)
    bn.load_state_dict(synth.state_dict_for(bn.param_shapes(), 1))
    for m in (unet, bn):
        m.upsample_phases, m.UP2X_MIN_ROWS = phases, 0
    return unet, bn


def forward(unet, bn):
    g = torch.Generator().manual_seed(3)
    x, ehs, cond = torch.randn(2, 4, 16, 16, generator=g), torch.randn(2, 77, 32, generator=g), torch.randn(2, 5, 16, 16, generator=g)
    calls = []
    orig = hip.conv_up2x
    hip.conv_up2x = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        d, m, u = bn(x.to(DEV), 301, ehs.to(DEV), brushnet_cond=cond.to(DEV), return_dict=False)
        y = unet(x.to(DEV), 301, ehs.to(DEV), down_block_add_samples=list(d), mid_block_add_sample=m, up_block_add_samples=list(u), return_dict=False)[0]
    finally:
        hip.conv_up2x = orig
    return y.float().cpu(), len(calls)


@pytest.mark.parametrize("prec", list(DT))
def test_models_with_the_attribute_on_and_off(prec):
    """UNet + BrushNet with the phase routing on and off, each against the same nets in fp32 (which never take the phase path): the
    routed pass stays inside the envelope margins of the unrouted one."""
    ref, n_ref = forward(*nets("fp32", True))
    off, n_off = forward(*nets(prec, False))
    on, n_on = forward(*nets(prec, True))
    assert (n_ref, n_off, n_on) == (0, 0, 2), "fp32 and the attribute keep the 3x3 path; one upsampler per net takes the phase path"
    e_off, e_on = (off - ref).abs(), (on - ref).abs()
    k_linf = ENV_K_LINF if ref.numel() >= ENV_SMALL_NUMEL else ENV_K_LINF_SMALL
    print(f"UP2X_MODEL {prec}: off L-inf {float(e_off.max()):.4e} mean {float(e_off.mean()):.4e}; on L-inf {float(e_on.max()):.4e} mean {float(e_on.mean()):.4e}; "
          f"ratio L-inf {float(e_on.max() / e_off.max()):.3f} (limit {k_linf}) mean {float(e_on.mean() / e_off.mean()):.3f} (limit {ENV_K_MEAN})")
    assert float(e_on.max()) <= k_linf * float(e_off.max()) and float(e_on.mean()) <= ENV_K_MEAN * float(e_off.mean())


def test_a_lora_fuse_rebuilds_the_phase_weights():
    unet, bn = nets("bf16", True)
    base, _ = forward(unet, bn)
    before = unet.P[UPCONV + ".up2x"]
    plan = [t for t in synth.lora_plan(unet.lora_modules()) if t[0] == UPCONV]
    assert plan, "the adapter targets the upsampler's conv"
    asd, alphas = synth.lora_adapter(plan, unet.param_shapes(), 7, 0.3, prefix="")
    unet.load_attn_procs(asd, network_alphas=alphas)
    unet.fuse_lora(0.7)
    assert unet.P[UPCONV + ".up2x"] is not before and not torch.equal(unet.P[UPCONV + ".up2x"].w, before.w), "derived from the merged weight"
    fused, n = forward(unet, bn)
    assert n == 2 and float((fused - base).abs().max()) > 0
    fresh, _ = nets("bf16", True, unet.state_dict())
    assert torch.equal(forward(fresh, bn)[0], fused), "a freshly loaded merged state dict gives the same bits"
    unet.unfuse_lora()
    assert torch.equal(unet.P[UPCONV + ".up2x"].w, before.w)


def test_a_forward_under_an_autograd_tape_keeps_the_3x3_path():
    unet, _ = nets("bf16", True)
    x = torch.randn(2, 8, 8, 64).to(torch.bfloat16).to(DEV)
    calls = []
    o_up, o_conv = ops.conv_up2x, ops.conv2d
    ops.conv_up2x = lambda *a, **k: calls.append("up2x")
    ops.conv2d = lambda *a, **k: calls.append(("conv2d", k.get("upsample")))
    try:
        unet._upsample_conv(UPCONV, x)
        ops.TAPE = autograd.Tape(hip.MF_F32)
        unet._upsample_conv(UPCONV, x)
    finally:
        ops.TAPE, ops.conv_up2x, ops.conv2d = None, o_up, o_conv
    assert calls == ["up2x", ("conv2d", True)]
    ops.TAPE = autograd.Tape(hip.MF_F32)
    try:
        with pytest.raises(hip.MfhipError, match="inference only"):
            ops.conv_up2x(x, unet.P[UPCONV + ".up2x"])
    finally:
        ops.TAPE = None


def test_programs_record_and_replay_the_phase_launches(tmp_path):
    """mf_brushnet_forward / mf_unet_forward programs exported with the routing on hold mf_conv_up2x calls and replay the models' passes
    bit for bit, on the exported inputs and on new ones."""
    unet, bn = nets("bf16", True)
    g = torch.Generator().manual_seed(5)
    x, cond, ehs = torch.randn(2, 4, 16, 16, generator=g).to(DEV), torch.randn(2, 5, 16, 16, generator=g).to(DEV), torch.randn(2, 7, 32, generator=g).to(DEV)
    tvals = torch.tensor([801.0, 401.0], device=DEV)
    tab_b, tab_u = bn.time_embedding_table(tvals, 2), unet.time_embedding_table(tvals, 2)
    t = torch.zeros(1, device=DEV)

    def run(xx, cc, i):
        down, mid, up = bn(xx, t, encoder_hidden_states=None, brushnet_cond=cc, conditioning_scale=1.0, return_dict=False, _temb=tab_b[i].clone())
        eps = unet(xx, t, encoder_hidden_states=ehs, down_block_add_samples=list(down), mid_block_add_sample=mid, up_block_add_samples=list(up),
                   return_dict=False, _temb=tab_u[i].clone())[0]
        return [r.clone() for r in list(down) + [mid] + list(up)], eps.clone(), (down, mid, up)
    res, eps, (down, mid, up) = run(x, cond, 0)
    pb, pu = str(tmp_path / "brushnet.mfprog"), str(tmp_path / "unet.mfprog")
    ib = program.export_brushnet(bn, pb, x, tab_b[0].clone(), cond)
    iu = program.export_unet(unet, pu, x, tab_u[0].clone(), ehs, down, mid, up)
    assert "mf_conv_up2x" in ib["entries"] and "mf_conv_up2x" in iu["entries"], (ib["entries"], iu["entries"])
    x2, cond2 = torch.randn(2, 4, 16, 16, generator=g).to(DEV), torch.randn(2, 5, 16, 16, generator=g).to(DEV)
    res2, eps2, _ = run(x2, cond2, 1)
    lib = hip.load()
    progb, progu = program.Program(pb, DEV), program.Program(pu, DEV)
    outs = [torch.empty_strided(r.shape, r.stride(), dtype=r.dtype, device=DEV) for r in res]
    ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    eps_out = torch.empty_like(eps)
    for xx, cc, i, want_res, want in ((x, cond, 0, res, eps), (x2, cond2, 1, res2, eps2)):
        tb, tu = tab_b[i].clone(), tab_u[i].clone()
        hip._check(lib.mf_brushnet_forward(progb._h, C.c_void_p(xx.data_ptr()), C.c_void_p(tb.data_ptr()), C.c_void_p(cc.data_ptr()), ptrs, len(outs),
                                           hip._stream()), "mf_brushnet_forward")
        torch.cuda.synchronize()
        for k, (o, w) in enumerate(zip(outs, want_res)):
            assert torch.equal(o, w), f"residual {k} differs by {(o.float() - w.float()).abs().max()}"
        rp = (C.c_void_p * len(want_res))(*[r.data_ptr() for r in want_res])
        hip._check(lib.mf_unet_forward(progu._h, C.c_void_p(xx.data_ptr()), C.c_void_p(tu.data_ptr()), rp, len(want_res), C.c_void_p(eps_out.data_ptr()),
                                       hip._stream()), "mf_unet_forward")
        torch.cuda.synchronize()
        assert torch.equal(eps_out, want), f"eps differs by {(eps_out - want).abs().max()}"
    progb.close(); progu.close()
