"""What tests/test_gemm_launches_gpu.py and tests/test_fp8_audit_gpu.py share: tracing every mf_gemm_conv launch of a block of
code through a proxy of the library handle, grouping the launches into cases, and replaying one case with fresh seeded data in
sentinel-filled, guard-tailed buffers against the float64 model of its descriptor (tests/gemm_ref.py)."""
import ctypes as C
import math

import torch

import gemm_ref as G
from reflecting_reality_amd import hip

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

ES = {G.MF_F32: 4, G.MF_BF16: 2, G.MF_F16: 2, G.MF_FP8: 1}
FP8_GAP = 0x7E           # what stride gaps of fp8 operands hold: the code of 448


class Buf:
    """`nbytes` at an address congruent to `mod` modulo 256, followed by a GUARD-byte tail; everything starts as `fill`."""

    def __init__(self, nbytes, mod, dev, fill):
        self.raw = torch.full((nbytes + 256 + GUARD,), fill, dtype=torch.uint8, device=dev)
        self.off = (mod - self.raw.data_ptr()) % 256
        self.nbytes, self.fill = nbytes, fill
        self.bytes = self.raw[self.off: self.off + nbytes]
        assert self.bytes.data_ptr() % 256 == mod % 256

    def typed(self, dtype):
        es = torch.empty(0, dtype=dtype).element_size()
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


def fp8_rows(shape, gen, dev):
    """fp8 codes [..., rows, c] as the quantiser leaves them: Gaussian rows, every row scaled to amax 448 (bytes, uint8)."""
    v = torch.randn(shape, generator=gen, device=dev)
    v = v * (448.0 / v.abs().amax(-1, keepdim=True))
    return v.clamp(-448.0, 448.0).to(G.FP8_DT).view(torch.uint8)


def _fill_fp8(buf, shape, strides, offset, gen):
    t = buf.typed(torch.uint8)
    t.as_strided(shape, strides, offset).copy_(fp8_rows(shape, gen, t.device))


def _fill_scales(d, name, count, zs, gen, dev, bufs, ops):
    """a_scale / w_scale: `count` positive values per outer z, 2^U(-4, 4) apart, the gaps between the vectors GAP."""
    nq = (d.nz - 1) // d.zdiv + 1
    b = bufs[name] = Buf(((nq - 1) * zs + count) * 4, getattr(d, name), dev, 0)
    t = b.typed(torch.float32)
    t.fill_(GAP)
    for q in range(nq):
        t[q * zs: q * zs + count] = torch.exp2(8.0 * torch.rand(count, generator=gen, device=dev) - 4.0) / 448.0
    ops[name] = t


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
    fp8 = d.dtype == G.MF_FP8
    a_es = ES[d.a_dtype]
    a_dt = G.FP8_DT if fp8 else G.TORCH_DT[d.a_dtype]
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
        if fp8:
            b.bytes.fill_(FP8_GAP)
            for z in range(d.nz):
                _fill_fp8(b, (rows_in, c), (lda, 1), G.zoff(z, d.zdiv, d.a_zs_o, d.a_zs_i), gen)
            ops[name] = t
            continue
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
    elif fp8:
        zmax = _max_z(d.nz, d.zdiv, d.w_zs_o, d.w_zs_i)
        b = bufs["w"] = Buf(zmax + (n - 1) * d.ldw + k, d.w, dev, FP8_GAP)
        for z in range(d.nz):
            _fill_fp8(b, (n, k), (d.ldw, 1), G.zoff(z, d.zdiv, d.w_zs_o, d.w_zs_i), gen)
        ops["w"] = b.typed(G.FP8_DT)
        # scales that bring the outputs to the order of 1, like the biases and residuals: code products have rms ~ 448^2 sqrt(K) / 9
        if d.a_scale:
            _fill_scales(d, "a_scale", m, d.a_scale_zs, gen, dev, bufs, ops)
        if d.w_scale:
            _fill_scales(d, "w_scale", n, d.w_scale_zs, gen, dev, bufs, ops)
            ops["w_scale"].mul_(9.0 / math.sqrt(k))
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
    v, problems, nrows, _, _ = finish(d, d0, rec, bufs, ops, seed, dev)
    return v, problems, nrows


def finish(d, d0, rec, bufs, ops, seed, dev, fp8_allow=G.FP8_A):
    """The second half of a replay, for a descriptor `d` whose input pointers already sit in `bufs` (name -> Buf) with `ops` the
    typed views the model reads: sentinel-filled outputs, NaN workspace, the launch, guards, untouched memory, and the float64
    comparison of the sampled rows.  Returns (verdict, problems, row count, got, Ref)."""
    m, n = G.m_rows(d), d.n
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
    ref = G.reference(d, ops, rows, fp8_allow=fp8_allow)
    got = G.gather_got(d, bufs["out"].typed(o_dt), rows, bufs["vt_out"].typed(o_dt) if d.vt_out else None)
    v = G.compare(got, ref.v, ref.s, d.out_dtype, a=ref.a)
    gn = []
    if d.gn_part:
        gn = G.check_gn_part(bufs["gn_part"].typed(torch.float32), rec.part_rows, d.gn_groups if rec.grouped else 0, d, ref,
                             d.out_dtype)
    return v, problems + gn, len(rows), got, ref
