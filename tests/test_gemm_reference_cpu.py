"""tests/gemm_ref.py, the float64 model of one mf_gemm_desc that tests/test_gemm_launches_gpu.py holds every GEMM launch of the
benchmark step to, checked here without a GPU: the model against plain torch float64 ops on small synthetic descriptors, one per
feature, and the comparator's power to reject subtly wrong results."""
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_ref as G
from reflecting_reality_amd import hip

pytestmark = pytest.mark.filterwarnings("ignore::UserWarning")

GAP = 16384.0        # the value stride gaps hold: a model that reads one is off by far more than any tolerance


def desc(**kw):
    """A GemmDesc with neutral defaults; pointer fields only need to be non-null here (the model reads `ops`)."""
    d = hip.GemmDesc()
    d.dtype = d.a_dtype = d.out_dtype = G.MF_BF16
    d.batch = d.h_in = d.w_in = d.h_out = d.w_out = d.kh = d.kw = d.stride = 1
    d.nz = d.zdiv = 1
    d.alpha = 1.0
    d.a0 = d.w = d.out = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def nhwc_flat(x, lda, dtype):
    """NCHW float tensor -> flat NHWC buffer with pixel stride lda (gaps hold GAP), stored in `dtype`."""
    b, c, h, w = x.shape
    buf = torch.full((b * h * w * lda,), GAP, dtype=dtype)
    buf.view(b * h * w, lda)[:, :c] = x.permute(0, 2, 3, 1).reshape(-1, c).to(dtype)
    return buf


def w_flat(w4, ldw, dtype):
    """[n, C, kh, kw] -> flat [n][ldw] rows in k = (ky * kw + kx) * C + c order, gaps GAP."""
    n = w4.shape[0]
    k = w4[0].numel()
    buf = torch.full((n * ldw,), GAP, dtype=dtype)
    buf.view(n, ldw)[:, :k] = w4.permute(0, 2, 3, 1).reshape(n, k).to(dtype)
    return buf


def stored(buf, c, lda, shape):
    """The values the flat NHWC buffer holds, back as float64 NCHW."""
    b, _, h, w = shape
    return buf.view(-1, lda)[:, :c].double().view(b, h, w, c).permute(0, 3, 1, 2)


def conv_ref(x, w4, stride, pad_t, pad_l, h_out, w_out, upsample):
    if upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    kh, kw = w4.shape[2:]
    xp = F.pad(x, (pad_l, kw + stride * w_out, pad_t, kh + stride * h_out))
    return F.conv2d(xp, w4, stride=stride)[:, :, :h_out, :w_out]


def all_rows(d):
    return torch.arange(G.m_rows(d))


def to_rows(y):
    """NCHW -> [1, B*H*W, C] (the model's layout for nz = 1)."""
    return y.permute(0, 2, 3, 1).reshape(1, -1, y.shape[1])


@pytest.mark.parametrize("case", ["sym_pad", "asym_stride2", "upsample", "two_segments"])
def test_model_matches_conv2d(case):
    g = torch.Generator().manual_seed(7)
    b, h, w, c0, c1, n = 2, 6, 5, 5, 0, 6
    stride, pad_t, pad_l, ups, kh = 1, 1, 1, False, 3
    if case == "asym_stride2":          # diffusers' Downsample2D: F.pad(0, 1, 0, 1), then a 3x3 / stride 2 conv without padding
        stride, pad_t, pad_l = 2, 0, 0
    if case == "upsample":
        ups = True
    if case == "two_segments":
        c1 = 3
    hi, wi = (2 * h, 2 * w) if ups else (h, w)
    h_out = (hi + (1 if case == "asym_stride2" else 2 * pad_t) - kh) // stride + 1
    w_out = (wi + (1 if case == "asym_stride2" else 2 * pad_l) - kh) // stride + 1
    x0 = torch.randn(b, c0, h, w, generator=g)
    x1 = torch.randn(b, c1, h, w, generator=g)
    w4 = torch.randn(n, c0 + c1, kh, kh, generator=g)
    lda0, lda1 = c0 + 3, c1 + 1
    ops = {"a0": nhwc_flat(x0, lda0, torch.bfloat16), "w": w_flat(w4, kh * kh * (c0 + c1) + 2, torch.bfloat16)}
    if c1:
        ops["a1"] = nhwc_flat(x1, lda1, torch.bfloat16)
    d = desc(c0=c0, c1=c1, lda0=lda0, lda1=lda1, batch=b, h_in=h, w_in=w, h_out=h_out, w_out=w_out, kh=kh, kw=kh,
             stride=stride, pad_t=pad_t, pad_l=pad_l, upsample=int(ups), ldw=kh * kh * (c0 + c1) + 2, n=n, a1=1 if c1 else None)
    ref = G.reference(d, ops, all_rows(d))
    xs = stored(ops["a0"], c0, lda0, x0.shape)
    if c1:
        xs = torch.cat([xs, stored(ops["a1"], c1, lda1, x1.shape)], 1)
    ws = ops["w"].view(n, -1)[:, :kh * kh * (c0 + c1)].double().view(n, kh, kh, c0 + c1).permute(0, 3, 1, 2)
    want = conv_ref(xs, ws, stride, pad_t, pad_l, h_out, w_out, ups)
    torch.testing.assert_close(ref.v, to_rows(want), rtol=1e-12, atol=1e-12)
    # S is sum |a| |w| of the same gather
    want_s = conv_ref(xs.abs(), ws.abs(), stride, pad_t, pad_l, h_out, w_out, ups)
    torch.testing.assert_close(ref.s, to_rows(want_s), rtol=1e-12, atol=1e-12)


def test_model_fp32_a_rounds_to_bf16_and_split_codes_keep_fp32():
    g = torch.Generator().manual_seed(8)
    x = torch.randn(16, 32, generator=g)
    w = torch.randn(8, 32, generator=g)
    ops = {"a0": x.flatten(), "w": w.to(torch.bfloat16).flatten()}
    d = desc(a_dtype=G.MF_F32, c0=32, lda0=32, h_in=16, h_out=16, ldw=32, n=8)
    ref = G.reference(d, ops, all_rows(d))
    torch.testing.assert_close(ref.v[0], x.to(torch.bfloat16).double() @ w.to(torch.bfloat16).double().T, rtol=1e-12, atol=1e-12)
    # f16x3 with a pre-split weight: the model multiplies fp32 A by hi + lo of the packed rows (K = 40 pads to 64)
    from reflecting_reality_amd import ops as O
    x = torch.randn(16, 40, generator=g)
    w = torch.randn(8, 40, generator=g)
    packed, kp = O.split_pack(w, hip.MF_F16X3)
    ops = {"a0": x.flatten(), "w": packed.flatten()}
    d = desc(dtype=G.MF_F16X3, a_dtype=G.MF_F32, out_dtype=G.MF_F32, c0=40, lda0=40, h_in=16, h_out=16, ldw=kp, w_split=1, n=8)
    ref = G.reference(d, ops, all_rows(d))
    hi = w.to(torch.float16).double()
    want = x.double() @ (hi + (w - hi.float()).to(torch.float16).double()).T
    torch.testing.assert_close(ref.v[0], want, rtol=1e-12, atol=1e-12)
    assert (ref.v[0] - x.double() @ w.double().T).abs().max() < 1e-5


def test_model_strided_batched_matmul():
    """QK^T of attention as mf_gemm_conv runs it: z = (batch, head), A / W rows of one head are dh-wide slices of a row."""
    g = torch.Generator().manual_seed(9)
    bsz, heads, s, dh = 2, 3, 10, 8
    ld = heads * dh + 4
    q = torch.randn(bsz, s, ld, generator=g)
    k = torch.randn(bsz, s, ld, generator=g)
    d = desc(dtype=G.MF_F32, a_dtype=G.MF_F32, out_dtype=G.MF_F32, c0=dh, lda0=ld, h_in=s, h_out=s, ldw=ld, n=s,
             nz=bsz * heads, zdiv=heads, a_zs_o=s * ld, a_zs_i=dh, w_zs_o=s * ld, w_zs_i=dh, o_zs_o=heads * s * s, o_zs_i=s * s,
             ldc=s, alpha=0.5)
    ref = G.reference(d, {"a0": q.flatten(), "w": k.flatten()}, all_rows(d))
    qh = q[..., :heads * dh].view(bsz, s, heads, dh).transpose(1, 2).double()
    kh = k[..., :heads * dh].view(bsz, s, heads, dh).transpose(1, 2).double()
    want = 0.5 * qh @ kh.transpose(-1, -2)
    torch.testing.assert_close(ref.v, want.reshape(bsz * heads, s, s), rtol=1e-12, atol=1e-12)
    # and the output blocks cover exactly the z slabs
    out, vt = G.out_blocks(d)
    assert vt is None and out[-1] == ((bsz - 1) * heads * s * s + (heads - 1) * s * s, s, s, s)


def test_model_epilogue_bias_rows_temb_alpha_residuals_silu():
    g = torch.Generator().manual_seed(10)
    b, hw, k, n = 3, 4, 16, 8
    m = b * hw
    x = torch.randn(m, k, generator=g).to(torch.bfloat16)
    w = torch.randn(n, k, generator=g).to(torch.bfloat16)
    bias_r = torch.randn(m, generator=g)
    temb = torch.randn(b, n + 5, generator=g)
    res0 = torch.randn(m, n + 2, generator=g).to(torch.bfloat16)
    res1 = torch.randn(hw, n + 1, generator=g).to(torch.bfloat16)        # shared by the b replicas: row m % hw
    ops = {"a0": x.flatten(), "w": w.flatten(), "bias": bias_r, "temb": temb.flatten(), "res0": res0.flatten(), "res1": res1.flatten()}
    d = desc(c0=k, lda0=k, batch=b, h_in=2, w_in=2, h_out=2, w_out=2, ldw=k, n=n, bias=1, bias_mode=1, temb=1, ld_temb=n + 5,
             alpha=0.75, res0=1, res0_dtype=G.MF_BF16, ld_res0=n + 2, res1=1, res1_dtype=G.MF_BF16, ld_res1=n + 1, res1_rows=hw,
             act=G.ACT_SILU)
    ref = G.reference(d, ops, all_rows(d))
    acc = x.double() @ w.double().T
    v = 0.75 * (acc + bias_r.double()[:, None] + temb.double()[:, :n].repeat_interleave(hw, 0))
    v = v + res0.double()[:, :n] + res1.double()[:, :n].repeat(b, 1)
    torch.testing.assert_close(ref.v[0], F.silu(v), rtol=1e-12, atol=1e-12)
    # the column bias form
    d2 = desc(c0=k, lda0=k, batch=b, h_in=2, w_in=2, h_out=2, w_out=2, ldw=k, n=n, bias=1)
    ref2 = G.reference(d2, {"a0": x.flatten(), "w": w.flatten(), "bias": bias_r[:n]}, all_rows(d2))
    torch.testing.assert_close(ref2.v[0], acc + bias_r.double()[:n], rtol=1e-12, atol=1e-12)


def test_model_geglu_interleaved():
    """Weight rows interleaved [4 values | 4 gates] per 8 (ops.py): output column 4 g + j = value * gelu(gate), exact erf."""
    g = torch.Generator().manual_seed(11)
    m, k, half = 20, 24, 16
    x = torch.randn(m, k, generator=g).to(torch.bfloat16)
    wv, wg = torch.randn(half, k, generator=g), torch.randn(half, k, generator=g)
    bv, bg = torch.randn(half, generator=g), torch.randn(half, generator=g)
    wi = torch.cat([wv.view(-1, 4, k), wg.view(-1, 4, k)], 1).reshape(2 * half, k).to(torch.bfloat16)
    bi = torch.cat([bv.view(-1, 4), bg.view(-1, 4)], 1).reshape(-1)
    d = desc(c0=k, lda0=k, h_in=m, h_out=m, ldw=k, n=2 * half, bias=1, act=G.ACT_GEGLU4, ldc=half)
    ref = G.reference(d, {"a0": x.flatten(), "w": wi.flatten(), "bias": bi}, all_rows(d))
    xv = x.double()
    val = xv @ wv.to(torch.bfloat16).double().T + bv.double()
    gate = xv @ wg.to(torch.bfloat16).double().T + bg.double()
    torch.testing.assert_close(ref.v[0], val * F.gelu(gate, approximate="none"), rtol=1e-12, atol=1e-12)
    assert G.out_cols(d) == half


def test_model_folded_layernorm():
    """ln_colsum: LayerNorm(x; gamma, beta) then Linear(W, b) == rstd (x W'^T - mean colsum) + b' with W' = W gamma, b' = b + W beta."""
    g = torch.Generator().manual_seed(12)
    m, k, n = 24, 64, 16
    x = (torch.randn(m, k, generator=g) * torch.rand(m, 1, generator=g) * 3 + torch.randn(m, 1, generator=g) * 2).to(torch.bfloat16)
    gamma, beta = 1 + 0.1 * torch.randn(k, generator=g), 0.1 * torch.randn(k, generator=g)
    w, b = torch.randn(n, k, generator=g), torch.randn(n, generator=g)
    wf = (w * gamma).to(torch.bfloat16)
    cs = wf.double().sum(1).float()
    bf = (b.double() + w.double() @ beta.double()).float()
    d = desc(c0=k, lda0=k, h_in=m, h_out=m, ldw=k, n=n, bias=1, ln_colsum=1, ln_eps=1e-5)
    ref = G.reference(d, {"a0": x.flatten(), "w": wf.flatten(), "bias": bf, "ln_colsum": cs}, all_rows(d))
    want = F.linear(F.layer_norm(x.double(), (k,), gamma.double(), beta.double(), 1e-5), w.double(), b.double())
    # the folded form is exact up to the rounding of W' to bf16 and of colsum / b' to fp32: compare at the bf16 weight level
    want_f = F.linear(F.layer_norm(x.double(), (k,), None, None, 1e-5), wf.double(), bf.double())
    torch.testing.assert_close(ref.v[0], want_f, rtol=1e-6, atol=1e-6)
    assert (ref.v[0] - want).abs().max() < 0.05


def test_model_vt_out_transpose():
    """Columns n >= vt_n0 live in vt_out[m / tokens][n - vt_n0][m % tokens]: gather_got reads a buffer written that way."""
    g = torch.Generator().manual_seed(13)
    imgs, tokens, n, n0, ldc, vt_ld = 2, 16, 24, 8, 8, 24
    m = imgs * tokens
    full = torch.randn(m, n, generator=g).to(torch.bfloat16)
    out = torch.full((m * ldc,), 0.0, dtype=torch.bfloat16)
    out.view(m, ldc)[:, :n0] = full[:, :n0]
    vt = torch.zeros(imgs * (n - n0) * vt_ld, dtype=torch.bfloat16)
    v3 = vt.view(imgs, n - n0, vt_ld)
    for i in range(imgs):
        v3[i, :, :tokens] = full[i * tokens:(i + 1) * tokens, n0:].T
    d = desc(c0=4, lda0=4, h_in=m, h_out=m, ldw=4, n=n, ldc=ldc, vt_out=1, vt_n0=n0, vt_tokens=tokens, vt_ld=vt_ld)
    rows = torch.tensor([0, 5, 17, 31])
    got = G.gather_got(d, out, rows, vt)
    assert torch.equal(got[0], full[rows])
    ob, vb = G.out_blocks(d)
    assert ob == [(0, m, n0, ldc)] and vb == [(0, imgs * (n - n0), tokens, vt_ld)]


def _fp8_case(seed=15, m=5, n=7, k=48, nz=2):
    """A small batched fp8 descriptor with strides of its own everywhere: (d, ops, codes A [nz, m, k], W [nz, n, k], rs, cs, bias)."""
    g = torch.Generator().manual_seed(seed)
    lda, ldw, a_zs, w_zs, rs_zs, cs_zs = k + 16, k + 32, m * (k + 16) + 16, n * (k + 32) + 48, m + 3, n + 2
    qa = (torch.randn(nz, m, k, generator=g) * 100).clamp(-448, 448).to(G.FP8_DT)
    qw = (torch.randn(nz, n, k, generator=g) * 100).clamp(-448, 448).to(G.FP8_DT)
    a = torch.full((nz * a_zs,), 448.0).to(G.FP8_DT)                          # gaps hold 448: a model that reads one is far off
    w = torch.full((nz * w_zs,), 448.0).to(G.FP8_DT)
    rs = torch.full((nz * rs_zs,), GAP)
    cs = torch.full((nz * cs_zs,), GAP)
    for z in range(nz):
        a.view(torch.uint8)[z * a_zs: z * a_zs + m * lda].view(m, lda)[:, :k] = qa[z].view(torch.uint8)
        w.view(torch.uint8)[z * w_zs: z * w_zs + n * ldw].view(n, ldw)[:, :k] = qw[z].view(torch.uint8)
        rs[z * rs_zs: z * rs_zs + m] = torch.exp2(torch.randint(-12, 12, (m,), generator=g).float()) * (1 + torch.rand(m, generator=g))
        cs[z * cs_zs: z * cs_zs + n] = torch.exp2(torch.randint(-12, 12, (n,), generator=g).float()) * (1 + torch.rand(n, generator=g))
    bias = torch.randn(m, generator=g)
    d = desc(dtype=G.MF_FP8, a_dtype=G.MF_FP8, out_dtype=G.MF_F32, c0=k, lda0=lda, h_in=m, h_out=m, ldw=ldw, n=n, nz=nz,
             a_zs_o=a_zs, w_zs_o=w_zs, o_zs_o=m * n, ldc=n, a_scale=1, w_scale=1, a_scale_zs=rs_zs, w_scale_zs=cs_zs,
             bias=1, bias_mode=1, alpha=-0.75)
    ops = {"a0": a, "w": w, "a_scale": rs, "w_scale": cs, "bias": bias}
    return d, ops, qa, qw, rs.view(nz, rs_zs)[:, :m], cs.view(nz, cs_zs)[:, :n], bias


def test_model_fp8_matches_a_brute_force_loop():
    """5 x 7 x 48 with nz = 2: v = alpha (acc rs[m] cs[n] + bias[m]) by a plain float64 loop over every (z, m, n, k); S and the
    fp8 allowance 2e-4 R rs cs |alpha| with R the rms of the unscaled code product."""
    d, ops, qa, qw, rs, cs, bias = _fp8_case()
    nz, m, k = qa.shape
    n = qw.shape[1]
    ref = G.reference(d, ops, all_rows(d))
    fa, fw = qa.float().double().tolist(), qw.float().double().tolist()
    want = torch.zeros(nz, m, n, dtype=torch.float64)
    want_s = torch.zeros_like(want)
    code = torch.zeros_like(want)
    for z in range(nz):
        for i in range(m):
            for j in range(n):
                acc = sabs = 0.0
                for kk in range(k):
                    acc += fa[z][i][kk] * fw[z][j][kk]
                    sabs += abs(fa[z][i][kk] * fw[z][j][kk])
                g = float(rs[z, i].double() * cs[z, j].double())
                code[z, i, j] = acc
                want[z, i, j] = -0.75 * (acc * g + float(bias[i]))
                want_s[z, i, j] = 0.75 * (sabs * g + abs(float(bias[i])))
    torch.testing.assert_close(ref.v, want, rtol=1e-13, atol=0)
    torch.testing.assert_close(ref.s, want_s, rtol=1e-13, atol=0)
    rms = float((code ** 2).mean().sqrt())
    want_a = 2e-4 * rms * 0.75 * rs.double()[:, :, None] * cs.double()[:, None, :]
    torch.testing.assert_close(ref.a, want_a, rtol=1e-12, atol=0)
    assert float(ref.a.max() / ref.a.min()) > 1e3                 # the allowance follows the scales
    exact = G.reference(d, ops, all_rows(d), fp8_allow=0.0)
    assert float(exact.a.abs().max()) == 0.0 and torch.equal(exact.v, ref.v)
    # one z alone, and a GEGLU epilogue: the allowance goes through the gains like LN_A
    one = G.reference(d, ops, all_rows(d), zs=[1])
    torch.testing.assert_close(one.v[0], want[1], rtol=1e-13, atol=0)


def test_model_fp8_geglu_and_what_stays_refused():
    g = torch.Generator().manual_seed(16)
    m, k, n = 6, 32, 16
    qa = (torch.randn(m, k, generator=g) * 60).clamp(-448, 448).to(G.FP8_DT)
    qw = (torch.randn(n, k, generator=g) * 60).clamp(-448, 448).to(G.FP8_DT)
    rs, cs = torch.rand(m, generator=g) * 1e-2, torch.rand(n, generator=g) * 1e-2
    bias = torch.randn(n, generator=g)
    ops = {"a0": qa.flatten(), "w": qw.flatten(), "a_scale": rs, "w_scale": cs, "bias": bias}
    kw = dict(dtype=G.MF_FP8, a_dtype=G.MF_FP8, c0=k, lda0=k, h_in=m, h_out=m, ldw=k, n=n, a_scale=1, w_scale=1, bias=1)
    ref = G.reference(desc(act=G.ACT_GEGLU4, ldc=n // 2, **kw), ops, torch.arange(m))
    v = (qa.float().double() @ qw.float().double().T) * rs.double()[:, None] * cs.double()[None, :] + bias.double()
    v = v.view(m, n // 8, 8)
    torch.testing.assert_close(ref.v[0], (v[..., :4] * F.gelu(v[..., 4:])).reshape(m, n // 2), rtol=1e-12, atol=1e-14)
    assert bool((ref.a > 0).all())
    for bad in (dict(kw, ln_colsum=1), dict(kw, vt_out=1, vt_n0=8, vt_tokens=2),              # as the entry refuses them
                dict(kw, dtype=G.MF_BF16, a_dtype=G.MF_BF16), dict(kw, dtype=G.MF_BF16, a_dtype=G.MF_BF16, a_scale=None),
                dict(kw, a_dtype=G.MF_BF16), dict(kw, dtype=G.MF_BF16)):                    # a scale, or half of fp8, without the code
        with pytest.raises(G.NotModelled):
            G.reference(desc(**bad), ops, torch.arange(m))


def test_model_refuses_what_it_does_not_cover():
    for kw in ({"a_scale": 1}, {"w_scale": 1}, {"dtype": G.MF_BF16X1}, {"defer_reduce": 1}, {"act": 7}):
        d = desc(c0=8, lda0=8, ldw=8, n=8, **kw)
        with pytest.raises(G.NotModelled):
            G.reference(d, {"a0": torch.zeros(8, dtype=torch.bfloat16), "w": torch.zeros(64, dtype=torch.bfloat16)}, torch.arange(1))


# ---- the comparator's power ---------------------------------------------------------------------------------------------------

def _exact(seed=14, m=512, k=320, n=64, res=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g).to(torch.bfloat16)
    w = (torch.randn(n, k, generator=g) / math.sqrt(k)).to(torch.bfloat16)
    acc = x.double() @ w.double().T
    s = x.double().abs() @ w.double().abs().T
    r = torch.randn(m, n, generator=g).to(torch.bfloat16).double() if res else torch.zeros(m, n, dtype=torch.float64)
    return x, w, acc, s, r


def _rne(v):
    return v.to(torch.bfloat16).double()


def _trunc(v):
    """float64 -> bf16 by truncation toward zero."""
    f = v.float()
    bits = f.view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).double()


def test_comparator_passes_round_to_nearest_even():
    _, _, acc, s, r = _exact(res=True)
    ref = acc + r
    s = s + r.abs()
    v = G.compare(_rne(ref), ref, s, G.MF_BF16)
    assert v.ok, v.msg
    assert v.n_stat >= 1000 and abs(v.mean_e) < 0.02 and abs(v.rms_e - 0.2887) < 0.02
    # the fp32-rounded accumulator the kernel actually rounds from passes too (its error is far below the bound)
    v = G.compare(_rne((acc.float() + r.float()).double()), ref, s, G.MF_BF16)
    assert v.ok, v.msg
    v = G.compare(ref.float(), ref, s, G.MF_F32)
    assert v.ok, v.msg


def test_comparator_rejects_truncation():
    _, _, acc, s, _ = _exact()
    v = G.compare(_trunc(acc), acc, s, G.MF_BF16)
    assert not v.ok and "bias" in v.msg


def test_comparator_rejects_a_dropped_k_term():
    x, w, acc, s, _ = _exact()
    dropped = acc - x.double()[:, 100:101] * w.double()[:, 100][None, :]
    v = G.compare(_rne(dropped), acc, s, G.MF_BF16)
    assert not v.ok


def test_comparator_rejects_double_rounding_before_the_residual():
    _, _, acc, s, r = _exact(res=True)
    ref = acc + r
    got = _rne(_rne(acc) + r)
    v = G.compare(got, ref, s + r.abs(), G.MF_BF16)
    assert not v.ok, v.msg


def test_comparator_rejects_a_shifted_row_block():
    _, _, acc, s, _ = _exact()
    got = _rne(acc).clone()
    got[32:64] = _rne(acc[33:65])
    v = G.compare(got, acc, s, G.MF_BF16)
    assert not v.ok and "outside the bound" in v.msg


def test_comparator_rejects_nan():
    _, _, acc, s, _ = _exact()
    got = _rne(acc).clone()
    got[3, 5] = float("nan")
    assert not G.compare(got, acc, s, G.MF_BF16).ok


def test_untouched_memory_catches_a_sentinel_overwritten_past_n():
    m, n, ldc = 16, 24, 32
    d = desc(c0=8, lda0=8, h_in=m, h_out=m, ldw=8, n=n, ldc=ldc)
    blocks, _ = G.out_blocks(d)
    numel = (m - 1) * ldc + n
    buf = torch.full((numel * 2,), G.SENTINEL, dtype=torch.uint8)
    mask = G.region_mask(numel, blocks)
    typed = buf.view(torch.bfloat16)
    typed[mask] = 1.0                                           # a correct launch: every element of the region, nothing else
    bytes_mask = mask[:, None].expand(numel, 2).reshape(-1)
    assert G.untouched(buf, bytes_mask) == 0
    typed[5 * ldc + n] = 1.0                                    # one element past n in row 5
    assert G.untouched(buf, bytes_mask) == 2


def test_sample_rows_takes_whole_blocks():
    assert torch.equal(G.sample_rows(5000, 1), torch.arange(5000))
    r = G.sample_rows(100000 + 37, 2, block=128, budget=4096)
    blocks = sorted({int(x) // 128 for x in r})
    assert blocks[0] == 0 and blocks[-1] == 100037 // 128 and len(blocks) == 32
    assert int(r[-1]) == 100036 and len(r) == 31 * 128 + 100037 % 128
