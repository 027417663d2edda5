"""Every flash-attention flavour through the C ABI against float64, on inputs that move the running maximum after the first key
tile (tests/attention_ref.py: the reference, the per-element bound |got - o| <= B with factor 1, and the input families;
tests/test_attention_reference_cpu.py shows on the CPU that these inputs catch a kernel that rescales wrongly, which `randn` does not).

Every launch writes into a sentinel-filled output with gap columns (ldo > C), 128 spare rows behind the last query block and a
4 KB guard tail, all of which must come back untouched; q and k rows carry gap columns as well.  B = 2 and heads = 3 keep batch and
head offsets from aliasing; the grids have 6 (sq <= 128) or 12 (sq > 128) blocks: fewer than the 8 XCDs, and not a multiple of 8.
Every case is launched twice and must be bit-reproducible."""
import math
import os
import sys

import pytest
import torch

import attention_ref as A
from gemm_audit import Buf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from reflecting_reality_amd import hip, ops  # noqa: E402

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
B, HEADS = 2, 3
GAP = 16384.0                 # what the gap columns of q / k rows hold
SENTINEL = 0x7B               # output fill: 0x7B7B = 3.3e36 (bf16), 61280 (fp16); 0x7B7B7B7B = 1.3e36 (fp32)
SPARE_ROWS = 128
STORE = {"bf16": torch.bfloat16, "fp16": torch.float16, "f16x3": torch.float32}
FAMILIES = tuple(f for f in A.FAMILIES if f != "dense")
SHAPES = ((1, 1), (33, 63), (128, 64), (130, 65), (200, 77), (96, 190), (64, 200))
DIMS = {"bf16": (8, 40, 64, 80, 160), "fp16": (8, 40, 64, 80, 160), "f16x3": (8, 40, 64, 80)}
WORST = {}                    # (group, flavour, family) -> worst err/B, printed as a table when the module is done


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    yield
    groups = sorted({g for g, _, _ in WORST})
    for grp in groups:
        fams = sorted({f for g, _, f in WORST if g == grp})
        print(f"\nworst err/B, {grp}:\n" + "flavour".ljust(8) + "".join(f.rjust(14) for f in fams))
        for fl in sorted({x for g, x, _ in WORST if g == grp}):
            print(fl.ljust(8) + "".join((f"{WORST[(grp, fl, f)]:.3f}" if (grp, fl, f) in WORST else "-").rjust(14) for f in fams))


def rows_tensor(x64, ld, dtype, extra_rows=0):
    """[B, S, C] float64 (already rounded to storage) -> a device [B * S + extra_rows, ld] tensor of `dtype`, gaps filled with GAP."""
    b, s, c = x64.shape
    t = torch.full((b * s + extra_rows, ld), GAP, dtype=dtype, device=DEV)
    t[: b * s, :c] = x64.reshape(b * s, c).to(DEV, dtype)
    return t


def vt_tensor(v64, ldvt, dtype, pad=0.0):
    b, s, c = v64.shape
    t = torch.full((b, c, ldvt), pad, dtype=dtype, device=DEV)
    t[:, :, :s] = v64.transpose(1, 2).to(DEV, dtype)
    return t


def planes(t, flavour):
    """What the entry point takes for a stored tensor: the tensor itself, or its (hi, lo) fp16 planes."""
    return hip.split_halves(t) if flavour == "f16x3" else t


def seen(p, flavour):
    """float64 value of the operand as the kernel reads it."""
    return p[0].double() + p[1].double() if flavour == "f16x3" else p.double()


def cols(p, c0, c1):
    return tuple(x[:, c0:c1] for x in p) if isinstance(p, tuple) else p[:, c0:c1]


class Out:
    """Sentinel-filled [B * sq + SPARE_ROWS, ldo] output (and optionally [B, heads, sq] lse) in guarded buffers."""

    def __init__(self, flavour, sq, c, with_lse=False):
        self.dtype = torch.float32 if flavour == "f16x3" else STORE[flavour]
        self.es = 4 if flavour == "f16x3" else 2
        self.sq, self.c, self.ldo = sq, c, c + 8
        self.rows = B * sq + SPARE_ROWS
        self.buf = Buf(self.rows * self.ldo * self.es, 0, DEV, SENTINEL)
        self.lse = Buf(B * HEADS * sq * 4, 0, DEV, SENTINEL) if with_lse else None

    def tensor(self):
        return self.buf.typed(self.dtype)

    def lse_tensor(self):
        return self.lse.typed(torch.float32) if self.lse is not None else None

    def values(self):
        return self.tensor().view(self.rows, self.ldo)[: B * self.sq, : self.c].double().reshape(B, self.sq, self.c)

    def lse_values(self):
        return self.lse_tensor().double().view(B, HEADS, self.sq)

    def untouched(self):
        raw = self.buf.bytes.view(self.rows, self.ldo * self.es)
        assert bool((raw[: B * self.sq, self.c * self.es:] == SENTINEL).all()), "gap columns of the output were written"
        assert bool((raw[B * self.sq:] == SENTINEL).all()), "rows past sq of the last query block were written"
        assert self.buf.guard_ok(), "the output's guard tail was written"
        assert self.lse is None or self.lse.guard_ok(), "the lse guard tail was written"


def launch(flavour, qp, kp, vp, out, *, ldq, ldk, ldvt, sq, skv, d, causal=False):
    fn = hip.attention_f16x3 if flavour == "f16x3" else hip.attention_bf16
    kw = dict(ldq=ldq, ldk=ldk, ldvt=ldvt, ldo=out.ldo, batch=B, heads=HEADS, sq=sq, skv=skv, head_dim=d, scale=d ** -0.5)
    if causal:
        fn(qp, kp, vp, out.tensor(), causal=True, **kw)
    else:
        fn(qp, kp, vp, out.tensor(), lse=out.lse_tensor(), **kw)
    torch.cuda.synchronize()


def check(name, key, flavour, d, got, q64, k64, v64, causal=False, lse=None, units_as=None):
    """Holds `got` (and `lse`) to the bound; returns the list of failure messages (empty: inside)."""
    ref = A.reference(q64, k64, v64, HEADS, d ** -0.5, causal)
    bnd, bnd_lse = A.bound(q64, k64, v64, HEADS, d ** -0.5, ref, units_as or flavour)
    r = (got - ref[0]).abs() / bnd
    worst, rms = float(r.nan_to_num(math.inf).max()), float(r.pow(2).mean().sqrt())
    smax = float(ref[2].masked_fill(torch.isinf(ref[2]), 0.0).abs().max())
    msg = f"{name}: worst err/B {worst:.3f}, rms err/B {rms:.3f}, |o|max {float(ref[0].abs().max()):.2f}, |s|max {smax:.1f}"
    bad = []
    if not bool(((got - ref[0]).abs() <= bnd).all()):
        n = int((~((got - ref[0]).abs() <= bnd)).sum())
        bad.append(f"{name}: {n} of {got.numel()} outputs outside B, worst err/B {worst:.3g}")
    if lse is not None:
        r_lse = (lse - ref[3]).abs() / bnd_lse
        msg += f", lse worst err/B {float(r_lse.nan_to_num(math.inf).max()):.3f}"
        if not bool(((lse - ref[3]).abs() <= bnd_lse).all()):
            bad.append(f"{name}: lse outside B_lse, worst err/B {float(r_lse.nan_to_num(math.inf).max()):.3g}")
    print(msg)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    return bad


def run(group, flavour, d, family, sq, skv, *, causal=False, with_lse=False, fused=False, seed=0):
    c = HEADS * d
    name = f"{group}[{flavour}, d{d}, {family}, {sq}x{skv}]"
    q64, k64, v64 = A.make_inputs(family, B, HEADS, sq, skv, d, seed=seed + 31 * d + 1000 * sq + skv, rnd=flavour)
    dt = STORE[flavour]
    if fused:          # self-attention's projection layout: q and k are column slices of one [B, S, 2C] tensor
        assert sq == skv
        qk = planes(rows_tensor(torch.cat([q64, k64], -1), 2 * c, dt), flavour)
        qp, kp, ldq, ldk = cols(qk, 0, c), cols(qk, c, 2 * c), 2 * c, 2 * c
    else:
        qp, kp = planes(rows_tensor(q64, c + 8, dt), flavour), planes(rows_tensor(k64, c + 16, dt), flavour)
        ldq, ldk = c + 8, c + 16
    ldvt = (skv + 7) // 8 * 8
    vp = planes(vt_tensor(v64, ldvt, dt), flavour)
    qs, ks = (seen(cols(p, 0, c), flavour).reshape(B, -1, c) for p in (qp, kp))
    vs = seen(vp, flavour)[:, :, :skv].transpose(1, 2)
    outs = []
    for _ in range(2):
        out = Out(flavour, sq, c, with_lse)
        launch(flavour, qp, kp, vp, out, ldq=ldq, ldk=ldk, ldvt=ldvt, sq=sq, skv=skv, d=d, causal=causal)
        out.untouched()
        outs.append(out)
    bad = check(name, (group, flavour, family), flavour, d, outs[0].values(), qs, ks, vs, causal,
                outs[0].lse_values() if with_lse else None)
    if not torch.equal(outs[0].buf.bytes, outs[1].buf.bytes) or (with_lse and not torch.equal(outs[0].lse.bytes, outs[1].lse.bytes)):
        bad.append(f"{name}: two launches differ")
    if with_lse:       # the entry without the row statistics writes the same bits
        plain = Out(flavour, sq, c)
        launch(flavour, qp, kp, vp, plain, ldq=ldq, ldk=ldk, ldvt=ldvt, sq=sq, skv=skv, d=d)
        if not torch.equal(plain.buf.bytes, outs[0].buf.bytes):
            bad.append(f"{name}: the _lse entry's output differs from the plain entry's")
    return bad


FLAVOUR_DIMS = [(fl, d) for fl in A.FLAVOURS for d in DIMS[fl]]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("flavour,d", FLAVOUR_DIMS)
def test_flavours(flavour, d, family):
    bad = []
    for sq, skv in SHAPES:
        bad += run("flash", flavour, d, family, sq, skv)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("family", ["stairs_up", "peaked"])
@pytest.mark.parametrize("flavour", A.FLAVOURS)
def test_long_row(flavour, family):
    """64 key tiles: the DMA offsets step 63 times and both LDS buffers are used 32 times each."""
    bad = run("long", flavour, 40, family, 128, 4096)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("family", ["peaked", "stairs_up", "forbidden"])
@pytest.mark.parametrize("d", [8, 64])
@pytest.mark.parametrize("flavour", A.FLAVOURS)
def test_causal(flavour, d, family):
    bad = []
    for s in (1, 64, 65, 77, 130, 200):
        bad += run("causal", flavour, d, family, s, s, causal=True)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("family", ["peaked", "stairs_up"])
@pytest.mark.parametrize("d", [8, 40, 64, 80])
@pytest.mark.parametrize("flavour", A.FLAVOURS)
def test_fused_qk_layout(flavour, d, family):
    bad = []
    for s in (77, 130):
        bad += run("fused", flavour, d, family, s, s, fused=True)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("family", ["peaked", "stairs_down", "all_negative", "flat"])
@pytest.mark.parametrize("flavour,d", [(fl, d) for fl, d in FLAVOUR_DIMS if fl != "fp16"])
def test_lse(flavour, d, family):
    """mf_attention_bf16_lse / mf_attention_f16x3_lse: the row statistic against log2 sum exp, and the same output bits as the
    plain entry."""
    bad = []
    for sq, skv in ((130, 65), (200, 77), (64, 200)):
        bad += run("lse", flavour, d, family, sq, skv, with_lse=True)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("skv", [63, 65, 77])
@pytest.mark.parametrize("d", [40, 64])
@pytest.mark.parametrize("flavour", A.FLAVOURS)
def test_decoys_past_skv(flavour, d, skv):
    """What lies past skv inside the last key tile must not count (include/mfhip.h, mf_attention_bf16).  The K rows there are the next
    batch's first keys — made hot for this batch's queries here — or, past the last batch, rows the kernel must not read (allocated
    and hot as well); the V^T columns from skv to ldvt (64 columns and more past skv) hold 1e4."""
    sq, c = 64, HEADS * d
    name = f"decoy[{flavour}, d{d}, peaked, {sq}x{skv}]"
    q64, k64, v64 = A.make_inputs("peaked", B, HEADS, sq, skv, d, seed=77 + d + skv, rnd=flavour)
    hot = 3.0 * math.sqrt(d) * q64 / A.split_heads(q64, HEADS).norm(dim=-1).transpose(1, 2).repeat_interleave(d, -1)    # scores 3 |q| each
    n = min(64, skv)
    k64[1, :n] = A.stored(hot[0, :n], flavour)               # batch 0's tile tail reads these; for batch 1 they are ordinary keys
    dt = STORE[flavour]
    kt = rows_tensor(k64, c + 16, dt, extra_rows=64)
    kt[B * skv:, :c] = hot[B - 1].to(DEV, dt)
    ldvt = (skv + 64 + 7) // 8 * 8
    qp, kp, vp = planes(rows_tensor(q64, c + 8, dt), flavour), planes(kt, flavour), planes(vt_tensor(v64, ldvt, dt, pad=1e4), flavour)
    qs, vs = seen(cols(qp, 0, c), flavour).reshape(B, sq, c), seen(vp, flavour)[:, :, :skv].transpose(1, 2)
    ks = seen(cols(kp, 0, c), flavour)[: B * skv].reshape(B, skv, c)
    outs = []
    for _ in range(2):
        out = Out(flavour, sq, c)
        launch(flavour, qp, kp, vp, out, ldq=c + 8, ldk=c + 16, ldvt=ldvt, sq=sq, skv=skv, d=d)
        out.untouched()
        outs.append(out)
    bad = check(name, ("decoy", flavour, "peaked"), flavour, d, outs[0].values(), qs, ks, vs)
    assert torch.equal(outs[0].buf.bytes, outs[1].buf.bytes)
    assert not bad, "\n".join(bad)


DISPATCH = [("f16x3", 160, HEADS, 130, 77),          # no split flash kernel at 160: the unfused split GEMMs and mf_softmax_rows
            ("fp32", 40, HEADS, 130, 77),            # the fp32 mode is unfused at every head dim
            ("bf16", 512, 1, 96, 96)]                # the VAE's single 512-wide head


@pytest.mark.parametrize("family", ["peaked", "stairs_up", "all_negative", "flat"])
@pytest.mark.parametrize("prec_name,d,heads,sq,skv", DISPATCH)
def test_dispatcher(prec_name, d, heads, sq, skv, family):
    """ops.attention on the shapes that leave the flash kernel: the same bound with that precision's constants."""
    prec = ops.Precision.get(prec_name)
    c = heads * d
    rnd = {"f16x3": "f16x3", "fp32": "f32", "bf16": "bf16"}[prec_name]       # f16x3: 22-bit operands, so the GEMMs' own split is exact
    q64, k64, v64 = A.make_inputs(family, B, heads, sq, skv, d, seed=5 + d, rnd=rnd)
    ldv = (skv + 7) // 8 * 8
    vt = torch.zeros(B, c, ldv, dtype=prec.act, device=DEV)
    vt[:, :, :skv] = v64.transpose(1, 2).to(DEV, prec.act)
    q, k = q64.to(DEV, prec.act), k64.to(DEV, prec.act)
    o1 = ops.attention(q, k, vt, heads, skv, d ** -0.5, prec)
    o2 = ops.attention(q, k, vt, heads, skv, d ** -0.5, prec)
    torch.cuda.synchronize()
    assert o1.dtype == (torch.float32 if prec_name != "bf16" else torch.bfloat16) and o1.shape == (B, sq, c)
    ref = A.reference(q.double(), k.double(), v64.to(DEV), heads, d ** -0.5)
    bnd, _ = A.bound(q.double(), k.double(), v64.to(DEV), heads, d ** -0.5, ref,
                     "f16x3_unfused" if prec_name == "f16x3" else prec_name)
    r = (o1.double() - ref[0]).abs() / bnd
    worst = float(r.nan_to_num(math.inf).max())
    print(f"dispatch[{prec_name}, d{d}, {family}, {sq}x{skv}]: worst err/B {worst:.3f}, rms err/B {float(r.pow(2).mean().sqrt()):.3f}, "
          f"|o|max {float(ref[0].abs().max()):.2f}, |s|max {float(ref[2].abs().max()):.1f}")
    WORST[("dispatch", f"{prec_name}/{d}", family)] = worst
    assert torch.equal(o1, o2)
    assert bool(((o1.double() - ref[0]).abs() <= bnd).all()), f"worst err/B {worst:.3g}"
