"""Every GEMM launch of the benchmark step, each on its own, against the float64 model of its descriptor (tests/gemm_ref.py).

One bench.py pass (num_inference_steps = 1: the eager first step, so VAE encode, BrushNet, the UNet and VAE decode all launch) is
traced through a proxy of the library handle that copies every mf_gemm_conv descriptor.  The tile each launch ran is the one the
shipped tune cache, hip.PREFER_PERS or the library heuristic chose for that call at that position; the fused epilogue forms are the
ones the step turned on.  Launches that agree on every non-pointer field and on each pointer's null-ness and address modulo 256 are
one case.  Every case is replayed with fresh seeded data in buffers sized from its descriptor (each pointer keeps its address
modulo 256, so the alignment paths take the same branch), sentinel-filled output, 4 KB guard tails, and checked against float64:
16-bit outputs to 0.5 ulp + 2^-18 S per element and unbiased, correctly-rounded statistics; fp32 outputs to 2^-19 S."""
import ctypes as C
import math
import os
import sys
import time
from collections import Counter, OrderedDict

import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from reflecting_reality_amd import hip, synth  # noqa: E402

GUARD = 4096
GAP = 16384.0            # what stride gaps of the inputs hold (lda > c, ldw > K, ld_res > n, ld_temb > n)
PTR_FIELDS = ("a0", "a1", "w", "bias", "temb", "a_scale", "w_scale", "res0", "res1", "out", "ws", "ln_colsum", "vt_out",
              "sk_tickets", "gn_part")
HOST_PTR_FIELDS = ("gn_part_rows", "gn_grouped", "deferred_splits")      # host ints: only their null-ness is part of a case


class Launch:
    def __init__(self, d, rc, part_rows, grouped, deferred, tuner, ctx, key):
        self.d, self.rc, self.part_rows, self.grouped, self.deferred, self.tuner, self.ctx = d, rc, part_rows, grouped, deferred, tuner, ctx
        self.key = key          # the tune key hip.gemm_conv looked up for this call; None: the tile was not the tuner's to choose


def _host_int(addr):
    return int(C.c_int32.from_address(addr).value) if addr else 0


class _LibProxy:
    """Forwards every attribute of the library handle; copies each mf_gemm_conv descriptor before the call and records what the
    call returned and wrote to the host ints."""

    def __init__(self, lib, log, state):
        self._lib, self._log, self._state = lib, log, state

    def __getattr__(self, name):
        if name == "mf_gemm_conv":
            return self._gemm
        return getattr(self._lib, name)

    def _gemm(self, dref, stream):
        src = dref._obj
        d = hip.GemmDesc()
        C.memmove(C.addressof(d), C.addressof(src), C.sizeof(hip.GemmDesc))
        rc = self._lib.mf_gemm_conv(dref, stream)
        tuner, key = self._state["tuner"] > 0, None
        if not tuner and len(hip.KEY_LOG) > self._state["keys"]:
            self._state["keys"], key = len(hip.KEY_LOG), hip.KEY_LOG[-1]
        self._log.append(Launch(d, rc, _host_int(src.gn_part_rows), _host_int(src.gn_grouped), _host_int(src.deferred_splits),
                                tuner, hip.TUNE_CTX, key))
        return rc


class trace_gemms:
    """Context manager: every mf_gemm_conv launch in the block goes to self.launches (the tuner's trial launches flagged); the tune
    cache is held to the shipped file's entries and hip.KEY_LOG collects the tune keys looked up."""

    def __enter__(self):
        self.launches, self.state = [], {"tuner": 0, "keys": 0}
        lib = hip.load()
        self._saved = (hip._lib, hip._tune, hip._tuned_config, hip.KEY_LOG, hip._tune_misses)
        hip._tune = hip._tune_read(hip._TUNE_PATH, lib.mf_gemm_tile_table_version())
        self.shipped = dict(hip._tune)
        hip.KEY_LOG = []
        inner = hip._tuned_config

        def tuned(d, key):
            self.state["tuner"] += 1
            try:
                return inner(d, key)
            finally:
                self.state["tuner"] -= 1
        hip._tuned_config = tuned
        hip._lib = _LibProxy(lib, self.launches, self.state)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.keys = hip.KEY_LOG
        self.misses = hip._tune_misses - self._saved[4]
        hip._lib, hip._tune, hip._tuned_config, hip.KEY_LOG, _ = self._saved
        return False


def case_key(d):
    key = []
    for name, _ in hip.GemmDesc._fields_:
        v = getattr(d, name)
        if name in PTR_FIELDS:
            key.append((name, v is None, (v or 0) % 256))
        elif name in HOST_PTR_FIELDS:
            key.append((name, v is None))
        else:
            key.append((name, v))
    return tuple(key)


# ---- replay ------------------------------------------------------------------------------------------------------------------

ES = {G.MF_F32: 4, G.MF_BF16: 2, G.MF_F16: 2}


class Buf:
    """`nbytes` at an address congruent to `mod` modulo 256, followed by a GUARD-byte tail; everything starts as `fill`."""

    def __init__(self, nbytes, mod, dev, fill):
        self.raw = torch.full((nbytes + 256 + GUARD,), fill, dtype=torch.uint8, device=dev)
        self.off = (mod - self.raw.data_ptr()) % 256
        self.nbytes, self.fill = nbytes, fill
        self.bytes = self.raw[self.off: self.off + nbytes]
        assert self.bytes.data_ptr() % 256 == mod % 256

    def typed(self, dtype):
        es = torch.tensor([], dtype=dtype).element_size()
        return self.bytes[: self.nbytes // es * es].view(dtype)

    @property
    def ptr(self):
        return self.bytes.data_ptr()

    def guard_ok(self):
        return bool((self.raw[self.off + self.nbytes: self.off + self.nbytes + GUARD] == self.fill).all())


def _max_z(nz, zdiv, o, i):
    return max(G.zoff(z, zdiv, o, i) for z in range(nz))


def _fill_strided(t, shape, strides, offset, gen, scale=1.0, rowscale=None, rowoff=None):
    v = torch.randn(shape, generator=gen, device=t.device) * scale
    if rowscale is not None:
        v = v * rowscale[:, None] + rowoff[:, None]
    t.as_strided(shape, strides, offset).copy_(v.to(t.dtype))


def replay(d0, rec, seed, dev):
    """Replays one case; returns (verdict, gn messages, row count) or raises with what went wrong."""
    d = hip.GemmDesc()
    C.memmove(C.addressof(d), C.addressof(d0), C.sizeof(hip.GemmDesc))
    d.defer_reduce, d.deferred_splits = 0, None
    G.check_supported(d)
    gen = torch.Generator(device=dev).manual_seed(seed)
    m, k, n = G.m_rows(d), G.k_depth(d), d.n
    rows_in = d.batch * d.h_in * d.w_in
    bufs, ops = {}, {}
    a_es = ES[d.a_dtype]
    a_dt = G.TORCH_DT[d.a_dtype]
    ln = bool(d.ln_colsum)
    rs = ro = None
    if ln:      # folded LayerNorm: rows with their own offset and scale, so that mean and rstd matter
        rs = torch.exp(0.5 * torch.randn(rows_in, generator=gen, device=dev))
        ro = 2.0 * torch.randn(rows_in, generator=gen, device=dev)
    for name, c, lda in (("a0", d.c0, d.lda0), ("a1", d.c1, d.lda1)):
        if not getattr(d, name):
            continue
        zmax = _max_z(d.nz, d.zdiv, d.a_zs_o, d.a_zs_i) if name == "a0" else 0
        ne = zmax + (rows_in - 1) * lda + c
        b = bufs[name] = Buf(ne * a_es, getattr(d, name), dev, 0)
        t = b.typed(a_dt)
        t.fill_(GAP)
        for z in range(d.nz if name == "a0" else 1):
            _fill_strided(t, (rows_in, c), (lda, 1), G.zoff(z, d.zdiv, d.a_zs_o, d.a_zs_i) if name == "a0" else 0, gen,
                          rowscale=rs, rowoff=ro)
        ops[name] = t
    # W: N(0, 1 / K) rows, so that outputs, biases and residuals are of one scale
    wscale = 1.0 / math.sqrt(k)
    if d.w_split:
        w32 = torch.randn(n, k, generator=gen, device=dev) * wscale
        packed, kp = hip.split_pack(w32, d.dtype)
        assert kp == d.ldw, f"split_pack ldw {kp} != recorded {d.ldw}"
        b = bufs["w"] = Buf(packed.numel() * 2, d.w, dev, 0)
        b.typed(packed.dtype).copy_(packed.flatten())
        ops["w"] = b.typed(packed.dtype)
    else:
        w_dt = torch.float32 if d.dtype in G.SPLIT_CODES else G.TORCH_DT[d.dtype]
        zmax = _max_z(d.nz, d.zdiv, d.w_zs_o, d.w_zs_i)
        ne = zmax + (n - 1) * d.ldw + k
        b = bufs["w"] = Buf(ne * torch.tensor([], dtype=w_dt).element_size(), d.w, dev, 0)
        t = b.typed(w_dt)
        t.fill_(GAP)
        for z in range(d.nz):
            _fill_strided(t, (n, k), (d.ldw, 1), G.zoff(z, d.zdiv, d.w_zs_o, d.w_zs_i), gen, scale=wscale)
        ops["w"] = t
    if ln:
        cs = ops["w"].as_strided((n, k), (d.ldw, 1), 0).double().sum(1).float()
        b = bufs["ln_colsum"] = Buf(n * 4, d.ln_colsum, dev, 0)
        b.typed(torch.float32).copy_(cs)
        ops["ln_colsum"] = b.typed(torch.float32)
    if d.bias:
        nb = m if d.bias_mode else n
        b = bufs["bias"] = Buf(nb * 4, d.bias, dev, 0)
        _fill_strided(b.typed(torch.float32), (nb,), (1,), 0, gen)
        ops["bias"] = b.typed(torch.float32)
    if d.temb:
        ne = (d.batch - 1) * d.ld_temb + n
        b = bufs["temb"] = Buf(ne * 4, d.temb, dev, 0)
        t = b.typed(torch.float32)
        t.fill_(GAP)
        _fill_strided(t, (d.batch, n), (d.ld_temb, 1), 0, gen)
        ops["temb"] = t
    for name in ("res0", "res1"):
        if not getattr(d, name):
            continue
        rows = d.res1_rows if (name == "res1" and 0 < d.res1_rows < m) else m
        ld = getattr(d, "ld_" + name)
        dt = G.TORCH_DT[getattr(d, name + "_dtype")]
        ne = (rows - 1) * ld + n
        b = bufs[name] = Buf(ne * ES[getattr(d, name + "_dtype")], getattr(d, name), dev, 0)
        t = b.typed(dt)
        t.fill_(GAP)
        _fill_strided(t, (rows, n), (ld, 1), 0, gen)
        ops[name] = t
    # outputs: sentinel bytes
    o_dt = G.TORCH_DT[d.out_dtype]
    blocks, vblocks = G.out_blocks(d)
    o_ne = max(off + (r - 1) * ld + c for off, r, c, ld in blocks)
    bufs["out"] = Buf(o_ne * ES[d.out_dtype], d.out, dev, G.SENTINEL)
    if d.vt_out:
        v_ne = max(off + (r - 1) * ld + c for off, r, c, ld in vblocks)
        bufs["vt_out"] = Buf(v_ne * ES[d.out_dtype], d.vt_out, dev, G.SENTINEL)
    if d.ws:
        bufs["ws"] = Buf(d.ws_floats * 4, d.ws, dev, 0xFF)          # NaN: a split-K slab read before it was written shows
    if d.sk_tickets:
        bufs["sk_tickets"] = Buf(d.sk_ticket_cap * 4, d.sk_tickets, dev, 0)
    if d.gn_part:
        bufs["gn_part"] = Buf(d.gn_part_floats * 4, d.gn_part, dev, 0xFF)
    for name, b in bufs.items():
        setattr(d, name, b.ptr)
    part_rows, grouped = C.c_int32(0), C.c_int32(0)
    d.gn_part_rows = C.addressof(part_rows) if d0.gn_part_rows else None
    d.gn_grouped = C.addressof(grouped) if d0.gn_grouped else None
    tile, splitk = d.tile, d.splitk
    torch.cuda.synchronize()
    rc = hip.load().mf_gemm_conv(C.byref(d), hip._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"replay refused (rc={rc}): {hip.load().mf_last_error().decode()}"
    assert (d.tile, d.splitk) == (tile, splitk)
    if d.gn_part:
        assert (part_rows.value, grouped.value) == (rec.part_rows, rec.grouped), \
            f"gn_part rows / grouped {(part_rows.value, grouped.value)} != recorded {(rec.part_rows, rec.grouped)}"
    for name, b in bufs.items():
        assert b.guard_ok(), f"{name}: the launch wrote into the {GUARD}-byte guard tail"
    # untouched memory and NaN-free region
    problems = []
    for name, blks in (("out", blocks), ("vt_out", vblocks)):
        if blks is None:
            continue
        b = bufs[name]
        es = ES[d.out_dtype]
        ne = b.nbytes // es
        mask = G.region_mask(ne, blks, dev)
        nb = G.untouched(b.bytes.view(ne, es), mask[:, None].expand(ne, es))
        if nb:
            problems.append(f"{name}: {nb} bytes outside the written region lost their sentinel")
        vals = b.typed(o_dt)
        if bool(torch.isnan(vals[mask]).any()):
            problems.append(f"{name}: NaN in the output region")
        if not bool((b.bytes.view(ne, es)[mask] != G.SENTINEL).any(1).all()):
            problems.append(f"{name}: elements of the output region were never written")
    # values of the sampled rows
    blk = 128
    if d.gn_part:
        blk = 128 * rec.part_rows // math.gcd(128, rec.part_rows)
    rows = G.sample_rows(m, seed, block=blk)
    ref = G.reference(d, ops, rows)
    got = G.gather_got(d, bufs["out"].typed(o_dt), rows, bufs["vt_out"].typed(o_dt) if d.vt_out else None)
    v = G.compare(got, ref.v, ref.s, d.out_dtype, a=ref.a)
    gn = []
    if d.gn_part:
        gn = G.check_gn_part(bufs["gn_part"].typed(torch.float32), rec.part_rows, d.gn_groups if rec.grouped else 0, d, ref,
                             d.out_dtype)
    return v, problems + gn, len(rows)


def features(d, rec):
    f = []
    if d.kh > 1:
        f.append(f"{d.kh}x{d.kw}")
    if d.c1:
        f.append("2seg")
    if d.stride > 1:
        f.append(f"s{d.stride}")
    if d.upsample:
        f.append("ups")
    if d.nz > 1:
        f.append(f"nz{d.nz}")
    if d.a_dtype != d.dtype:
        f.append("aF32")
    if d.w_split:
        f.append("wsplit")
    if d.bias:
        f.append("biasM" if d.bias_mode else "bias")
    if d.temb:
        f.append("temb")
    if d.alpha != 1.0:
        f.append(f"a{d.alpha:g}")
    if d.res0:
        f.append("res0")
    if d.res1:
        f.append(f"res1/{d.res1_rows}" if d.res1_rows else "res1")
    f += {G.ACT_SILU: ["silu"], G.ACT_GEGLU4: ["geglu"]}.get(d.act, [])
    if d.ln_colsum:
        f.append("ln")
    if d.vt_out:
        f.append("vt")
    if d.gn_part:
        f.append(f"gn{rec.part_rows}" + ("g" if rec.grouped else ""))
    if rec.deferred:
        f.append(f"defer{rec.deferred}")
    if d.sk_tickets:
        f.append("skf")
    return f


def run_precision(prec):
    import bench
    dev = torch.device("cuda", 0)
    pipe, _ = bench.build_pipeline(prec, dev)
    inp = {k: v.to(dev) for k, v in synth.pipeline_inputs(4, 512, 512, seed=1234, cross_dim=768).items()}
    torch.cuda.synchronize()
    with trace_gemms() as tr:
        pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"],
             mask=inp["mask"], depth=inp["depth"], num_inference_steps=1, guidance_scale=7.5, latents=inp["latents"],
             output_type="pt", brushnet_conditioning_scale=1.0, height=512, width=512, conditioning_noise=inp["vae_noise"])
    del pipe, inp
    torch.cuda.empty_cache()
    return tr


def plan_disagreements(x):
    """mf_gemm_conv_plan on a recorded descriptor against what its launch reported through the host ints (the plan never reads them).
    A launch on tile 70 gives every block hip.PERS_MIN_NLOOP output tiles or more — unless tile 70 was not hip.PREFER_PERS' choice but the
    tuner's (the call looked up a tune key, so its tile is the cache's or a fresh measurement's).  Asserted for every tile-70 launch
    alike, 6 of the bf16 step's 131 cases fail it with ONE tile per block: M8192 N640 K320; M8192 N640 K640 plain, with a residual and
    with a folded LayerNorm; M2048 N1280 K1280 with a folded LayerNorm; M512 N10240 K1280 GEGLU.  The shipped tune cache holds tile 70
    for them (measured the winner there), and they launched the same way before the plan existed."""
    p = hip.GemmPlan()
    if hip.load().mf_gemm_conv_plan(C.byref(x.d), C.byref(p)) != 0:
        return [f"the plan refuses a call that launched: {hip.load().mf_last_error().decode()}"]
    out = []
    got, want = (p.gn_part_rows, p.gn_grouped, p.deferred_splits), (x.part_rows, x.grouped, x.deferred)
    if got != want:
        out.append(f"plan (gn_part_rows, gn_grouped, deferred_splits) {got} != launch {want}")
    if x.d.tile == hip.PERS_TILE and p.tiles_per_block < hip.PERS_MIN_NLOOP:
        if x.key is None:
            out.append(f"routed to tile {hip.PERS_TILE} with {p.tiles_per_block} output tiles per block")
    return out


def audit(prec):
    t0 = time.time()
    tr = run_precision(prec)
    launches = [x for x in tr.launches if not x.tuner]
    refused = [x for x in launches if x.rc != 0]
    cases = OrderedDict()
    for x in launches:
        if x.rc == 0:
            cases.setdefault(case_key(x.d), []).append(x)
    tagged = sorted({k for k in tr.keys if "@" in k and k in tr.shipped})
    print(f"\n[{prec}] traced {len(tr.launches)} launches ({len(tr.launches) - len(launches)} tuner trials), {len(cases)} cases, "
          f"{len(refused)} refused, trace {time.time() - t0:.1f}s")
    fails = []
    worst_mean = worst_rms = 0.0
    for i, (key, group) in enumerate(cases.items()):
        rec = group[0]
        d = rec.d
        m, k = G.m_rows(d), G.k_depth(d)
        shape = f"M{m} N{d.n} K{k}"
        fails += [f"case {i} {shape} tile {d.tile} sk {d.splitk} {features(d, rec)}: {msg}" for x in group for msg in plan_disagreements(x)]
        try:
            v, extra, nrows = replay(d, rec, 1000 + i, torch.device("cuda", 0))
        except (AssertionError, G.NotModelled, hip.MfhipError) as e:
            fails.append(f"case {i} {shape} tile {d.tile} sk {d.splitk} {features(d, rec)}: {type(e).__name__}: {e}")
            print(f"  case {i:3d} {shape:24s} tile {d.tile:2d} sk {d.splitk:2d} FAILED {type(e).__name__}: {e}")
            continue
        if d.out_dtype != G.MF_F32 and v.n_stat >= 1000:
            worst_mean = max(worst_mean, abs(v.mean_e))
            worst_rms = max(worst_rms, v.rms_e)
        ok = v.ok and not extra
        print(f"  case {i:3d} {shape:24s} tile {d.tile:2d} sk {d.splitk:2d} out {'f32' if d.out_dtype == G.MF_F32 else 'b16' if d.out_dtype == G.MF_BF16 else 'f16'} "
              f"x{len(group):<3d} rows {nrows:5d} maxulp {v.max_ulp:8.3f} mean(e) {v.mean_e:+.4f} rms(e) {v.rms_e:.4f} "
              f"bound {v.worst:.3f} [{','.join(features(d, rec))}]" + ("" if ok else "  FAIL"))
        if not ok:
            fails.append(f"case {i} {shape} tile {d.tile} sk {d.splitk} {features(d, rec)}: {v.msg} {' | '.join(extra)}")
        torch.cuda.empty_cache()
    tiles = Counter(x.d.tile for x in launches)
    print(f"[{prec}] summary: {len(cases)} cases, {len(launches)} launches, tiles {dict(sorted(tiles.items()))}, "
          f"tune misses {tr.misses}, tagged cache hits {len(tagged)}, worst |mean(e)| {worst_mean:.4f}, worst rms(e) {worst_rms:.4f}, "
          f"{time.time() - t0:.1f}s")
    return tr, launches, refused, cases, tagged, fails


@pytest.mark.parametrize("prec", ["bf16", "fp16", "f16x3"])
def test_every_gemm_launch_of_the_benchmark_step(prec):
    tr, launches, refused, cases, tagged, fails = audit(prec)
    assert launches, "no mf_gemm_conv launch was traced"
    assert not refused, "the library refused cached (tile, split-K) choices: " + "; ".join(
        f"tile {x.d.tile} sk {x.d.splitk} M{G.m_rows(x.d)} N{x.d.n} K{G.k_depth(x.d)}" for x in refused[:8])
    assert not fails, f"{len(fails)} of {len(cases)} cases failed:\n" + "\n".join(fails)
    if prec == "bf16":
        ds = [(x.d, x) for x in launches]
        need = {
            # (the decoder's cat(h, skip) reaches a conv as two segments in the 1x1 shortcut; its 3x3 conv1 reads the GroupNorm output)
            "two-segment conv": any(d.c1 for d, _ in ds),
            "stride 2": any(d.stride == 2 for d, _ in ds),
            "upsample": any(d.upsample for d, _ in ds),
            "tile 70": any(d.tile == hip.PERS_TILE for d, _ in ds),
            "folded LN with vt_out": any(d.ln_colsum and d.vt_out for d, _ in ds),
            "GEGLU": any(d.act == G.ACT_GEGLU4 for d, _ in ds),
            "gn_part": any(d.gn_part for d, _ in ds),
            "deferred split-K": any(r.deferred for _, r in ds),
            "@-tagged cache hit": bool(tagged),
        }
        missing = [k for k, v in need.items() if not v]
        assert not missing, f"the traced bf16 step no longer uses: {missing}"
