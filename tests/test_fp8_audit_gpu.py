"""The fp8 (OCP e4m3) path held to float64, launch by launch: the quantiser csrc/fp8.hip against the contract of tests/fp8_ref.py
byte for byte, its fused LayerNorm on inputs whose mean dwarfs their spread, non-finite rows, and the fp8 GEMM
(csrc/gemm_fp8.hip, the dequantising epilogue, split-K) against the float64 model of its descriptor (tests/gemm_ref.py) in
sentinel-filled buffers with guard tails — exact cases that need no tolerance, statistical cases under the scale-aware allowance
G.FP8_A, and every fp8 launch of a tiny-XL UNet forward replayed like tests/test_gemm_launches_gpu.py replays the benchmark step.

profiles/fp8_audit.txt holds what these tests printed on an MI355X."""
import ctypes as C
import math

import pytest
import torch

import fp8_ref as R8
import gemm_audit as A
import gemm_ref as G
import norm_conditioning_ref as NC

pytestmark = pytest.mark.gpu

from reflecting_reality_amd import hip, ops  # noqa: E402

DEV = torch.device("cuda", 0)
FP8_TILES = (1, 2, 3, 6, 7, 13, 14, 15)


# ---- the quantiser ---------------------------------------------------------------------------------------------------------------
def run_quant(x, norm=None, eps=1e-5):
    """mf_quantize_rows_fp8 on x [rows, c] (CPU, fp32 or bf16) with sentinel-filled q / scale buffers and guard tails: returns
    (codes uint8 [rows, c], scale fp32 [rows]) on the CPU."""
    rows, c = x.shape
    xb = A.Buf(x.numel() * x.element_size(), 0, DEV, 0)
    xb.typed(x.dtype).copy_(x.flatten())
    qb = A.Buf(rows * c, 0, DEV, G.SENTINEL)
    sb = A.Buf(rows * 4, 0, DEV, G.SENTINEL)
    g, b = (norm[0].to(DEV), norm[1].to(DEV)) if norm is not None else (None, None)
    hip._launch("mf_quantize_rows_fp8", xb.typed(x.dtype), hip.dt_code(x.dtype), qb.bytes, sb.typed(torch.float32), rows, c, g, b, eps)
    torch.cuda.synchronize()
    for name, buf in (("x", xb), ("q", qb), ("scale", sb)):
        assert buf.guard_ok(), f"{name}: the quantiser wrote into the guard tail"
    assert torch.equal(xb.typed(x.dtype).cpu().view(torch.uint8), x.flatten().view(torch.uint8)), "the quantiser changed its input"
    return qb.bytes.cpu().view(rows, c), sb.typed(torch.float32).cpu()


QUANT_SHAPES = [(c, (1, 7, 8, 9)) for c in (8, 256, 264, 2048, 2056)] + [(c, (1, 3, 4, 5)) for c in (4096, 4104, 8192)]
TIE_DIFFS = {}           # (c, dtype) -> (differences accepted at a near-tie, elements): printed, and summed up by the last case


@pytest.mark.parametrize("c,row_counts", QUANT_SHAPES)
def test_quantiser_writes_the_contracts_bytes(c, row_counts):
    """Codes and scales byte for byte those of fp8_ref.quantize_contract, at the lane and vector edges of both instantiations
    (<32 lanes, 8 vectors> up to C = 2048, <64, 16> above; 8 or 4 rows per block), on ties, subnormal targets, -0, zero rows, the
    smallest normal amax, amax 3e38 and rows scaled 2^-20 ... 2^20 besides Gaussian rows.  A differing code is accepted only one
    step away with the float64 y within 2^-20 relative of the tie; such elements are counted and capped at 1e-4 of the case."""
    pool = torch.cat([R8.special_rows(c), R8.gauss(13, c)])
    off = 0
    for rows in row_counts:
        x32 = pool[off: off + rows]
        off += rows
        for dt in (torch.float32, torch.bfloat16):
            x = x32.to(dt)
            q, s = run_quant(x)
            wq, ws = R8.quantize_contract(x)
            sbad = (s.view(torch.int32) != ws.view(torch.int32)).nonzero().flatten().tolist()
            assert not sbad, f"C {c} rows {rows} {dt}: scale of row {sbad[0]} is {float(s[sbad[0]])!r}, contract {float(ws[sbad[0]])!r}"
            d = q != wq
            nd = int(d.sum())
            if nd:
                _, _, y = R8.quantize_exact(x)
                ok = R8.one_step(q[d], wq[d]) & R8.near_tie(y[d])
                r, j = [int(v[0]) for v in torch.nonzero(d, as_tuple=True)]
                where = (f"C {c} rows {rows} {dt}: {nd} codes differ from the contract; first at row {r} col {j}: x {float(x[r, j])!r} "
                         f"y64 {float(y[r, j])!r} GPU 0x{int(q[r, j]):02x} contract 0x{int(wq[r, j]):02x}")
                print(where)
                assert bool(ok.all()), where + f"; {int((~ok).sum())} of them not at a near-tie"
                assert nd <= 1e-4 * q.numel(), where
            n0, n1 = TIE_DIFFS.get((c, dt), (0, 0))
            TIE_DIFFS[(c, dt)] = (n0 + nd, n1 + q.numel())
    tot = [sum(v[i] for k, v in TIE_DIFFS.items() if k[0] == c) for i in (0, 1)]
    print(f"quantiser C {c}: {tot[0]} of {tot[1]} codes differ from the contract (accepted near-ties), scales bit-equal")


@pytest.mark.parametrize("c", [320, 2048, 2056, 5120])
def test_quantiser_with_layernorm_on_the_conditioning_ladder(c):
    """Every rung of norm_conditioning_ref.LADDER through the fused LayerNorm: per element
    |q s - y64| <= 0.5 e4m3_spacing(y64 / s) s + delta, delta = 2^-20 (|y64 - beta| (1 + |mean| / std) + |beta|)  (fp8_ref.ln_quantize),
    and |s - amax64 / 448| <= (delta at the argmax + 2^-23 amax64) / 448."""
    rows = 9
    gamma, beta = NC.params(c, 83)
    fails = []
    for dt in (torch.float32, torch.bfloat16):
        for name in NC.ladder(dt):
            x = NC.ln_input(name, rows, c, dt, 83)
            q, s = run_quant(x, (gamma, beta), NC.EPS)
            y, _, s64, delta = R8.ln_quantize(x, gamma, beta, NC.EPS)
            sg = s.double()[:, None]
            err = (R8.decode(q) * sg - y).abs()
            bnd = 0.5 * R8.e4m3_spacing(y / sg) * sg + delta
            amax, arg = y.abs().max(1)
            serr = (s.double() - amax / 448.0).abs()
            sbnd = (delta.gather(1, arg[:, None])[:, 0] + 2.0 ** -23 * amax) / 448.0
            nbad, nsbad = int((~(err <= bnd)).sum()), int((~(serr <= sbnd)).sum())
            # how far the LayerNorm itself is off, in units of delta: (q s - y64) less the half step the rounding may add
            ln_part = float(((err - 0.5 * R8.e4m3_spacing(y / sg) * sg).clamp(min=0) / delta).max())
            line = (f"ln+quant C {c} {str(dt)[6:]:8s} {name:12s}: worst err/bound {float((err / bnd).max()):.3f} "
                    f"(beyond the half step: {ln_part:.2f} delta) scale err/bound {float((serr / sbnd).max()):.3f} bad {nbad}/{err.numel()} scales bad {nsbad}/{rows}")
            print(line)
            if nbad or nsbad:
                fails.append(line)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("c", [320, 4096])
@pytest.mark.parametrize("ln", [False, True])
def test_quantiser_non_finite_rows_get_a_nan_scale(c, ln):
    """A row that holds a NaN or an Inf comes out with scale NaN (and every code NaN), with and without the fused LayerNorm;
    the finite rows of the same blocks keep the bits they have without the bad rows beside them.  (Before the change to
    csrc/fp8.hip a NaN left as the finite code -448 of a row with a finite scale: see profiles/fp8_audit.txt.)"""
    rows = 10
    clean = R8.gauss(rows, c, seed=77)
    norm = NC.params(c, 84) if ln else None
    for dt in (torch.float32, torch.bfloat16):
        x = clean.clone()
        x[2, c // 3] = float("nan")
        x[5, c - 1] = float("inf")
        x[7, 0] = float("-inf")
        x[8, 1], x[8, 2] = float("inf"), float("nan")
        q0, s0 = run_quant(clean.to(dt), norm)
        q, s = run_quant(x.to(dt), norm)
        bad = torch.tensor([r in (2, 5, 7, 8) for r in range(rows)])
        assert torch.isnan(s).tolist() == bad.tolist(), f"scales {s.tolist()}"
        assert bool((q[bad] == R8.NAN_CODE).all()), f"codes of the non-finite rows: {q[bad][:, :8].tolist()}"
        assert torch.equal(q[~bad], q0[~bad]) and torch.equal(s[~bad], s0[~bad]), "a finite row changed beside a non-finite one"
        if not ln:
            wq, ws = R8.quantize_contract(x.to(dt))
            assert torch.equal(q, wq) and torch.equal(torch.isnan(s), torch.isnan(ws))


def test_fp8_linear_carries_a_nan_input_row_to_its_output_row():
    """ops.linear on an fp8 weight with a NaN and an Inf in its input: those output rows are non-finite in every column, as the
    bf16 path's are, and the other rows are bit-equal to the run without them."""
    g = torch.Generator().manual_seed(85)
    m, k, n = 70, 320, 72
    x = torch.randn(m, k, generator=g)
    w, b = torch.randn(n, k, generator=g) / math.sqrt(k), torch.randn(n, generator=g)
    xb = x.clone()
    xb[3, 17] = float("nan")
    xb[66, 0] = float("inf")
    bad = torch.tensor([r in (3, 66) for r in range(m)])
    for prec, f8 in (("fp8", True), ("bf16", False)):
        lw = ops.ConvWeight(w, b, ops.Precision.get(prec), DEV, fp8=f8)
        xin = (lambda t: t.to(DEV)) if f8 else (lambda t: t.to(DEV, torch.bfloat16))
        y0 = ops.linear(xin(x), lw, out_dtype=torch.float32).cpu()
        y = ops.linear(xin(xb), lw, out_dtype=torch.float32).cpu()
        assert bool(torch.isfinite(y0).all())
        assert not bool(torch.isfinite(y[bad]).any()), f"{prec}: a non-finite input row gave finite outputs {y[bad][:, :4].tolist()}"
        assert torch.equal(y[~bad], y0[~bad]), prec
    xt = xb[:64].view(1, 64, k)            # the V^T form: the tokens are the W operand, a bad token is a bad output COLUMN
    lw = ops.ConvWeight(w, b, ops.Precision.get("fp8"), DEV, fp8=True)
    vt = ops.linear_t(xt.to(DEV), lw, 64).float().cpu()
    assert not bool(torch.isfinite(vt[0, :, 3]).any()) and bool(torch.isfinite(vt[0, :, :3]).all()) and bool(torch.isfinite(vt[0, :, 4:]).all())


def test_weight_quantiser_codes_and_nan_rows():
    """ConvWeight(..., fp8=True): the stored codes are e4m3_round of the float64 quotient w / w_scale, all-zero rows and rows
    below the 1e-30 clamp included; a weight row with a NaN gets a NaN w_scale."""
    g = torch.Generator().manual_seed(86)
    n, k = 40, 320
    w = torch.randn(n, k, generator=g) * torch.exp2(torch.randint(-12, 12, (n, 1), generator=g).float())
    w[5] = 0.0
    w[6] = torch.randn(k, generator=g) * 1e-33               # amax below the clamp: scale 1e-30 / 448, small codes
    w[7] = torch.randn(k, generator=g) * 1e-38
    w[9, 11] = float("nan")
    lw = ops.ConvWeight(w, None, ops.Precision.get("fp8"), DEV, fp8=True)
    q, s = lw.w.cpu().view(torch.uint8), lw.w_scale.cpu()
    assert torch.isnan(s).tolist() == [r == 9 for r in range(n)]
    ok = torch.tensor([r != 9 for r in range(n)])
    amax = w.double().abs().amax(1).clamp_min(1e-30)
    assert bool(((s.double() - amax / 448.0).abs()[ok] <= 2.0 ** -22 * amax[ok] / 448.0).all())
    y = w.double()[ok] / s.double()[ok, None]
    want = R8.codes(R8.e4m3_round(y))
    d = q[ok] != want
    print(f"weight quantiser: {int(d.sum())} of {want.numel()} codes differ from e4m3_round of the float64 quotient")
    assert bool((R8.one_step(q[ok][d], want[d]) & R8.near_tie(y[d])).all()) and int(d.sum()) <= 1e-4 * want.numel()
    assert int(q[5].max()) == 0 and float(R8.decode(q[6]).abs().max()) < 448.0 and float(R8.decode(q[7]).abs().max()) == 0.0


# ---- the GEMM: exact cases -------------------------------------------------------------------------------------------------------
CODE_SET = torch.tensor([0.0, 1, -1, 2, -2, 3, -3, 4, -4, 6, -6, 8, -8])
# (M, N, K): every M in {1, 63, 65, 129, 193}, N in {8, 40, 77, 168, 200} and K in {16, 48, 112, 128, 144, 272, 528, 2048} at least once
EXACT_TABLE = [(1, 8, 16), (63, 40, 48), (65, 77, 112), (129, 168, 128), (193, 200, 144), (1, 200, 272), (63, 168, 528),
               (65, 8, 2048), (129, 77, 2048), (193, 40, 16), (129, 200, 528), (63, 77, 128)]
VARIANTS = ("plain", "epilogue", "geglu", "linear_t_77", "linear_t_80", "batched")


def _put(bufs, ops_, name, t, mod=0):
    """Tensor t (CPU, flat) into a guard-tailed buffer at an address `mod` modulo 256."""
    b = bufs[name] = A.Buf(t.numel() * t.element_size(), mod, DEV, 0)
    b.typed(torch.uint8).copy_(t.contiguous().view(torch.uint8).flatten())
    ops_[name] = b.typed(t.dtype)


def _codes(gen, shape, ld):
    """Small-integer e4m3 codes [..., rows, k] in rows of stride ld, the gaps holding 448."""
    *lead, r, k = shape
    buf = torch.full((*lead, r, ld), 448.0)
    buf[..., :k] = CODE_SET[torch.randint(len(CODE_SET), shape, generator=gen)]
    return buf.to(G.FP8_DT).flatten()


def _pow2(gen, count, total=None):
    v = torch.full((total or count,), A.GAP)
    v[:count] = torch.exp2(torch.randint(-3, 4, (count,), generator=gen).float())
    return v


def _ints(gen, shape, hi=8):
    return torch.randint(-hi, hi + 1, shape, generator=gen).float()


def exact_case(variant, m, n, k, tile, out_code, seed, splitk=1, w_scale_mod=0):
    """(descriptor, bufs, ops) of one exact case: integer codes, power-of-two scales, integer biases and residuals."""
    gen = torch.Generator().manual_seed(seed)
    lda, ldw = k + 16, k + 32
    d = hip.GemmDesc()
    d.dtype = d.a_dtype = G.MF_FP8
    d.out_dtype = out_code
    d.batch, d.h_in, d.w_in, d.h_out, d.w_out, d.kh, d.kw, d.stride = m, 1, 1, 1, 1, 1, 1, 1
    d.c0, d.lda0, d.ldw, d.n, d.nz, d.zdiv, d.alpha = k, lda, ldw, n, 1, 1, 1.0
    d.tile, d.splitk = tile, splitk
    d.ldc = n + 8
    d.a0 = d.w = d.out = d.a_scale = 256
    d.w_scale = 256 + w_scale_mod
    bufs, ops_ = {}, {}
    t = variant.startswith("linear_t")
    nz = 2 if t or variant == "batched" else 1
    if variant == "batched":         # both operands and both scale vectors per z, every stride its own
        d.nz, d.a_zs_o, d.w_zs_o, d.o_zs_o, d.a_scale_zs, d.w_scale_zs = nz, m * lda, n * ldw, m * (n + 8), m + 3, n + 4
        _put(bufs, ops_, "a0", _codes(gen, (nz, m, k), lda))
        _put(bufs, ops_, "a_scale", torch.cat([_pow2(gen, m, m + 3), _pow2(gen, m)]))
    else:
        _put(bufs, ops_, "a0", _codes(gen, (m, k), lda))
        _put(bufs, ops_, "a_scale", _pow2(gen, m))
    _put(bufs, ops_, "w", _codes(gen, (nz, n, k), ldw))
    if t:            # ops.linear_t: the weight is A, the tokens of every batch element W; bias per row; the scalar or the vector epilogue
        zs = int(variant[-2:])
        d.nz, d.w_zs_o, d.o_zs_o, d.w_scale_zs, d.bias_mode, d.ldc = nz, n * ldw, m * (n + 8), zs, 1, n + 8
        cs = torch.full((zs + n,), A.GAP)
        for z in range(nz):          # (vectors closer than n overlap: the second one wins where they do, and the model reads the same)
            cs[z * zs: z * zs + n] = _pow2(gen, n)
        _put(bufs, ops_, "w_scale", cs, w_scale_mod)
        d.bias = 256
        _put(bufs, ops_, "bias", _ints(gen, (m,)))
    elif variant == "batched":
        _put(bufs, ops_, "w_scale", torch.cat([_pow2(gen, n, n + 4), _pow2(gen, n)]), w_scale_mod)
    else:
        _put(bufs, ops_, "w_scale", _pow2(gen, n), w_scale_mod)
    if variant in ("epilogue", "geglu"):
        d.bias = 256
        _put(bufs, ops_, "bias", _ints(gen, (n,), 2 if variant == "geglu" else 8))
    if variant == "epilogue":
        d.alpha = 0.5
        d.res0, d.res0_dtype, d.ld_res0 = 256, G.MF_BF16, n + 16
        d.res1, d.res1_dtype, d.ld_res1 = 256, G.MF_F32, n + 8
        _put(bufs, ops_, "res0", _ints(gen, (m, n + 16), 64).to(torch.bfloat16).flatten())
        _put(bufs, ops_, "res1", _ints(gen, (m, n + 8), 64).flatten())
    if variant == "geglu":
        d.act, d.ldc = G.ACT_GEGLU4, n // 2 + 4
    if splitk != 1:
        d.ws, d.ws_floats = 256, 4 * nz * m * n
    return d, bufs, ops_


def run_exact(d, bufs, ops_, what):
    """Launches and holds the output to the model: bit for bit (fp32: the float64 value itself; bf16: its RNE rounding), GEGLU
    under the model's GELU_A allowance.  Returns the verdict."""
    v, problems, _, got, ref = A.finish(d, d, None, bufs, ops_, 0, DEV, fp8_allow=0.0)
    assert not problems, f"{what}: {problems}"
    if d.act == G.ACT_GEGLU4:
        assert v.ok, f"{what}: {v.msg}"
    else:
        want = ref.v.to(G.TORCH_DT[d.out_dtype])
        assert float(ref.v.abs().max()) < 2.0 ** 24
        if d.out_dtype == G.MF_F32:
            assert torch.equal(want.double(), ref.v), f"{what}: the case is not exact in fp32"
        ne = got != want
        assert not bool(ne.any()), (f"{what}: {int(ne.sum())}/{ne.numel()} elements differ from the exact result; first at (z, m, n) "
                                    f"{[int(i[0]) for i in torch.nonzero(ne, as_tuple=True)]}: got {float(got[ne][0])!r} want {float(want[ne][0])!r}")
    return v


@pytest.mark.parametrize("m,n,k", EXACT_TABLE)
def test_fp8_gemm_exact_cases(m, n, k):
    """Integer codes {0, +-1, +-2, +-3, +-4, +-6, +-8}, power-of-two scales 2^-3 ... 2^3, integer biases / residuals, K <= 2048:
    every product is an integer <= 64 and every partial sum stays below 2^24 (with the scales: 2^17 x 2^6), so the result is exact
    in fp32 under any summation order.  Every fp8 tile, fp32 and bf16 outputs; plain, bias + res0 + res1 with alpha, GEGLU, and
    the linear_t form (bias per row, nz = 2) with w_scale_zs = 77 (scalar epilogue) and 80 (vector epilogue where n % 8 == 0),
    and a batched form whose two z have operands and scale vectors of their own (a_scale_zs = m + 3, w_scale_zs = n + 4).
    GEGLU with n % 8 != 0 is a combination the entry refuses: it must return an error and leave the output's sentinel intact."""
    worst = 0.0
    launches = 0
    for vi, variant in enumerate(VARIANTS):
        for tile in FP8_TILES:
            for out_code in (G.MF_F32, G.MF_BF16):
                d, bufs, ops_ = exact_case(variant, m, n, k, tile, out_code, 1000 * vi + k + m)
                what = f"{variant} M{m} N{n} K{k} tile {tile} out {out_code}"
                if variant == "geglu" and n % 8:
                    ob = A.Buf(m * d.ldc * 4, 0, DEV, G.SENTINEL)
                    for name, b in bufs.items():
                        setattr(d, name, b.ptr)
                    d.out = ob.ptr
                    rc = hip.load().mf_gemm_conv(C.byref(d), hip._stream())
                    torch.cuda.synchronize()
                    assert rc != 0, f"{what}: the entry accepted GEGLU with n % 8 != 0"
                    assert bool((ob.raw == G.SENTINEL).all()), f"{what}: a refused call wrote to its output"
                    continue
                v = run_exact(d, bufs, ops_, what)
                worst = max(worst, v.worst)
                launches += 1
    print(f"fp8 exact M{m} N{n} K{k}: {launches} launches bit-exact (GEGLU worst err/bound {worst:.3f})")


def test_fp8_gemm_exact_w_scale_at_4_mod_16():
    """w_scale at an address that is 4 modulo 16: the 8-wide epilogue would load it with 16-byte vectors, so the entry must route
    the call to the scalar epilogue; the result stays exact."""
    for variant in ("plain", "epilogue", "linear_t_80"):
        for tile in (1, 3, 14):
            d, bufs, ops_ = exact_case(variant, 129, 168, 272, tile, G.MF_F32, 7, w_scale_mod=4)
            assert bufs["w_scale"].ptr % 16 == 4
            run_exact(d, bufs, ops_, f"{variant} tile {tile} w_scale at 4 mod 16")


def test_fp8_gemm_split_k_exact():
    """M 154, N 640, K 2048 (77 tokens x 2, the shape of a cross-attention K / V projection of the 640-wide level): forced split-K
    2 and 3, and splitk = 0, which the plan must split on its own.  The workspace starts as NaN; a_scale / w_scale reach the output
    through the reduce kernel's epilogue."""
    for splitk in (2, 3, 0):
        for variant in ("plain", "epilogue"):
            for out_code in (G.MF_F32, G.MF_BF16):
                d, bufs, ops_ = exact_case(variant, 154, 640, 2048, 0, out_code, 40 + splitk, splitk=splitk)
                p = hip.GemmPlan()
                assert hip.load().mf_gemm_conv_plan(C.byref(d), C.byref(p)) == 0, hip.load().mf_last_error().decode()
                if splitk == 0:
                    assert p.splitk > 1, f"the plan no longer splits M154 N640 K2048 on its own (splitk {p.splitk})"
                else:
                    assert p.splitk == splitk
                d.tile, d.splitk = 0, splitk
                run_exact(d, bufs, ops_, f"split-K {splitk} (plan: tile {p.tile} splitk {p.splitk}) {variant} out {out_code}")
                print(f"fp8 split-K {splitk}: plan tile {p.tile} splitk {p.splitk} reduce_launch {p.reduce_launch}, {variant} out {out_code} bit-exact")


# ---- the GEMM: statistical cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,n", [(300, 320, 72), (154, 2048, 640), (64, 1280, 160)])
def test_fp8_gemm_on_quantised_operands_with_wide_scale_spreads(m, k, n):
    """Operands out of hip.quantize_rows_fp8, Gaussian rows times 2^U(-10, 10) per row (activations and weights alike), so that
    rs and cs span six orders of magnitude: every element inside G.bound() + 2e-4 R rs[m] cs[n] |alpha| (G.FP8_A).  Every fp8 tile
    and the plan's own choice on the first half of the operands, and one batched launch (nz = 2, a_scale_zs = m, w_scale_zs = n) on
    both halves."""
    g = torch.Generator().manual_seed(91)
    x = torch.randn(2 * m, k, generator=g) * torch.exp2(20 * torch.rand(2 * m, 1, generator=g) - 10)
    w = torch.randn(2 * n, k, generator=g) * torch.exp2(20 * torch.rand(2 * n, 1, generator=g) - 10) / math.sqrt(k)
    xq, xs = hip.quantize_rows_fp8(x.to(DEV))
    wq, ws = hip.quantize_rows_fp8(w.to(DEV))
    assert float(xs[:m].max() / xs[:m].min()) > 1e5 and float(ws[:n].max() / ws[:n].min()) > 1e4
    bias = torch.randn(n, generator=g)
    for tile in (0, -2) + FP8_TILES:            # -2: the batched launch, on the plan's tile
        for out_code, with_bias in ((G.MF_F32, True), (G.MF_BF16, False)):
            d = hip.GemmDesc()
            d.dtype = d.a_dtype = G.MF_FP8
            d.out_dtype = out_code
            d.batch, d.h_in, d.w_in, d.h_out, d.w_out, d.kh, d.kw, d.stride = m, 1, 1, 1, 1, 1, 1, 1
            d.c0, d.lda0, d.ldw, d.n, d.nz, d.zdiv, d.alpha, d.ldc = k, k, k, n, 1, 1, 1.0, n
            d.tile, d.splitk = max(tile, 0), 0
            d.a0 = d.w = d.out = d.a_scale = d.w_scale = d.ws = 256
            d.ws_floats = 8 * m * n
            if tile == -2:
                d.nz, d.a_zs_o, d.w_zs_o, d.o_zs_o, d.a_scale_zs, d.w_scale_zs = 2, m * k, n * k, m * n, m, n
            bufs, ops_ = {}, {}
            _put(bufs, ops_, "a0", xq.cpu().flatten())
            _put(bufs, ops_, "w", wq.cpu().flatten())
            _put(bufs, ops_, "a_scale", xs.cpu())
            _put(bufs, ops_, "w_scale", ws.cpu())
            if with_bias:
                d.bias = 256
                _put(bufs, ops_, "bias", bias)
            p = hip.GemmPlan()
            assert hip.load().mf_gemm_conv_plan(C.byref(d), C.byref(p)) == 0, hip.load().mf_last_error().decode()
            v, problems, _, got, ref = A.finish(d, d, None, bufs, ops_, 0, DEV)
            print(f"fp8 statistical M{m} K{k} N{n} nz {d.nz} tile {p.tile} splitk {p.splitk} out {out_code}: worst err/bound {v.worst:.3f} "
                  f"max ulp {v.max_ulp:.3f}")
            assert v.ok and not problems, f"M{m} K{k} N{n} nz {d.nz} tile {p.tile} splitk {p.splitk} out {out_code}: {v.msg} {problems}"


# ---- the forms the model launches --------------------------------------------------------------------------------------------------
def _fp8_cases(launches):
    cases = {}
    for x in launches:
        if not x.tuner and x.rc == 0 and x.d.dtype == G.MF_FP8:
            cases.setdefault(A.case_key(x.d), []).append(x)
    return cases


def _replay_all(cases, tag):
    fails = []
    for i, group in enumerate(cases.values()):
        d = group[0].d
        feat = [f for f, on in (("bias", d.bias and not d.bias_mode), ("biasM", d.bias and d.bias_mode), ("res0", d.res0), ("res1", d.res1),
                                ("geglu", d.act == G.ACT_GEGLU4), (f"nz{d.nz}", d.nz > 1), (f"a{d.alpha:g}", d.alpha != 1.0)) if on]
        p = hip.GemmPlan()
        hip.load().mf_gemm_conv_plan(C.byref(d), C.byref(p))
        head = (f"  {tag} case {i:2d} M{G.m_rows(d)} N{d.n} K{G.k_depth(d)} tile {d.tile} (plan {p.tile}) sk {d.splitk} (plan {p.splitk}) "
                f"out {d.out_dtype} x{len(group)} [{','.join(feat)}]")
        try:
            v, extra, nrows = A.replay(d, group[0], 3000 + i, DEV)
        except (AssertionError, G.NotModelled, hip.MfhipError) as e:
            fails.append(f"{head}: {type(e).__name__}: {e}")
            print(f"{head} FAILED {e}")
            continue
        print(f"{head} rows {nrows} worst err/bound {v.worst:.3f} max ulp {v.max_ulp:.3f}" + ("" if v.ok and not extra else "  FAIL"))
        if not v.ok or extra:
            fails.append(f"{head}: {v.msg} {' | '.join(extra)}")
    return fails


def _plan_splitk(d):
    p = hip.GemmPlan()
    return p.splitk if hip.load().mf_gemm_conv_plan(C.byref(d), C.byref(p)) == 0 else 0


def test_every_fp8_launch_of_a_tiny_xl_unet_forward(monkeypatch):
    """One forward of the tiny-XL UNet in precision "fp8" (the model of test_fp8_gpu.test_tiny_xl_models_and_pipeline_in_fp8) is
    traced; every fp8 mf_gemm_conv case is replayed with fresh codes and scales, sentinels and guards against the float64 model.
    The trace must hold a GEGLU, a residual and a linear_t (bias per row, nz > 1) fp8 launch.  No Linear of the tiny
    configuration is deep enough to split (K <= 256: two K tiles, the plan wants eight), so the split-K launch comes from a second
    trace: the same configuration with a 256-wide last level, whose FeedForward output projection has K = 1024, with the tile and
    split left to the library's own plan as for any shape the tune cache does not hold."""
    from oracle import mirrorfusion_ref as R
    from reflecting_reality_amd import models as M
    from reflecting_reality_amd import synth
    g = torch.Generator().manual_seed(43)
    x = torch.randn(2, 4, 8, 8, generator=g)
    ehs = torch.randn(2, 77, 48, generator=g)
    added = dict(text_embeds=torch.randn(2, 24, generator=g), time_ids=torch.tensor([[16., 16., 0., 0., 16., 16.], [32., 24., 4., 2., 16., 16.]]))
    wide = dict(R.TINY_XL_UNET, block_out_channels=(32, 64, 256), attention_head_dim=(2, 4, 16))
    traces = {}
    for tag, cfg in (("tiny-XL", dict(R.TINY_XL_UNET)), ("wide", wide)):
        if tag == "wide":
            monkeypatch.setattr(hip, "AUTOTUNE", False)
        unet = M.UNet2DConditionModel(cfg, precision="fp8", device=DEV)
        unet.load_state_dict(synth.state_dict_for(unet.param_shapes(), 20))
        assert sum(1 for v in unet.P.values() if getattr(v, "fp8", False)) > 10, "no fp8 layers were built"
        with A.trace_gemms() as tr:
            unet(x, 401, ehs, added_cond_kwargs=added, return_dict=False)
        traces[tag] = _fp8_cases(tr.launches)
        del unet
    fails = []
    for tag, cases in traces.items():
        n_launch = sum(len(v) for v in cases.values())
        print(f"\n[{tag}] {n_launch} fp8 launches, {len(cases)} cases")
        assert cases, f"{tag}: no fp8 mf_gemm_conv launch was traced"
        fails += _replay_all(cases, tag)
    assert not fails, f"{len(fails)} fp8 cases failed:\n" + "\n".join(fails)
    tiny = [v[0].d for v in traces["tiny-XL"].values()]
    every = tiny + [v[0].d for v in traces["wide"].values()]
    need = {"GEGLU": any(d.act == G.ACT_GEGLU4 for d in tiny), "residual": any(d.res0 for d in tiny),
            "linear_t": any(d.bias_mode == 1 and d.nz > 1 and d.w_scale_zs for d in tiny),
            "split-K": any(_plan_splitk(d) > 1 for d in every)}
    missing = [k for k, v in need.items() if not v]
    assert not missing, f"the traced fp8 forwards no longer launch: {missing}"
