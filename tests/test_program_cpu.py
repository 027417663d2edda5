"""Step programs without a GPU: the recorder's signature table, the replay thunks' table in csrc/program.hip and the prototypes of
include/mfhip.h must say the same thing about every replayable entry (a wrong letter would pass a float where an int64 is read)."""
import os
import re

import abi_header
from reflecting_reality_amd import program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# program.SIGNATURES is derived from hip.SIGNATURES: this is what it must come to (the table csrc/program.hip's kFns restates)
EXPECTED = {
    "mf_gemm_conv": "d", "mf_groupnorm": "d",
    "mf_layernorm": "pipipplif", "mf_softmax_rows": "ppilii",
    "mf_attention_bf16": "plplplpliiiiif", "mf_attention_f16": "plplplpliiiiif",
    "mf_attention_f16x3": "pplpplpplpliiiiif", "mf_attention_f16x3_lse": "pplpplpplplpiiiiif", "mf_split_halves": "pppl",
    "mf_quantize_rows_fp8": "pipplippf",
    "mf_pack_nhwc": "pipipiiii", "mf_unpack_nchw": "pilpiii",
    "mf_add": "pipipil", "mf_cast_bf16": "ppl", "mf_geglu": "pipili",
    "mf_timestep_embedding": "ppiiif", "mf_silu_f32": "ppl",
    "mf_cfg_ddim_step_dev": "ppfpppifl", "mf_cfg_combine": "ppfpl", "mf_sched_step_dev": "ppfpppl",
    "mf_vae_sample": "pilppiiif", "mf_nearest_resize": "ppiiiii",
    "mf_transpose": "ppiiillll", "mf_transpose_bf16": "ppiiillll", "mf_transpose_bf16_bf16": "ppiiillll",
    "mf_memcpy2d": "plplll", "mf_memset": "pil",
}


def _header_signatures():
    """The int-returning, stream-taking prototypes in the recorder's alphabet: the arguments before the stream, 'd' for the two descriptors
    that have a replay thunk."""
    out = {}
    for name, (ret, params) in abi_header.prototypes().items():
        if ret != "i" or not params or params[-1] != "p":
            continue
        out[name] = "".join("d" if k in ("mf_gemm_desc", "mf_groupnorm_desc") else k if len(k) == 1 else "?" for k in params[:-1])
    return out


def test_signature_tables_agree_with_the_header():
    assert program.SIGNATURES == EXPECTED
    hdr = _header_signatures()
    for name, sig in program.SIGNATURES.items():
        assert name in hdr, f"{name} is not declared in include/mfhip.h with a trailing stream argument"
        assert hdr[name] == sig, f"{name}: program.SIGNATURES says {sig!r}, the header's prototype reads {hdr[name]!r}"
    src = open(os.path.join(ROOT, "reflecting-reality_amd", "csrc", "program.hip")).read()
    table = dict(re.findall(r'\{"(mf_\w+)",\s*"(\w+)"\}', src))
    assert table == program.SIGNATURES, "csrc/program.hip's kFns and program.SIGNATURES differ"
    # one thunk per table entry, and every thunk reads exactly the arguments its signature has
    enum = re.search(r"enum Fn \{(.*?)F_COUNT", src, flags=re.S).group(1)
    assert len([e for e in enum.replace("\n", " ").split(",") if e.strip()]) == len(table)


def test_two_d_copy_decomposition():
    import torch
    a = torch.zeros(4, 6, 8)
    assert program._rows_runs(a) == (1, 192, 192)
    assert program._rows_runs(a[:, :, :4]) == (24, 8, 4)
    assert program._rows_runs(a[:, :3]) == (4, 48, 24)
    assert program._rows_runs(a[:, ::2, :4]) == (12, 16, 4)             # every second row: still one pitch
    try:
        program._rows_runs(a[:, :2, :4])                               # rows 8 apart, then a jump of 48: two pitches
    except program.ProgramError:
        pass
    else:
        raise AssertionError("a copy with two different outer pitches is not a 2-D copy")


def _blob(calls, buffers, nevents=0, meta="{}"):
    return program.serialize_header(calls, buffers, nevents, meta)[0]


def test_program_header_round_trips_through_the_library_without_a_gpu():
    """program.serialize_header -> mf_program_load: the parser accepts what the writer writes (buffers, names, data offsets, meta, calls on
    two streams with an event between them) and refuses malformed or foreign input with a message — no device call is made."""
    import ctypes as C
    import struct
    from reflecting_reality_amd import hip
    lib = hip.load()
    bufs = [dict(kind=program.KIND_IO, name="x", bytes=256), dict(kind=program.KIND_WORKSPACE, name="workspace.0", bytes=4096),
            dict(kind=program.KIND_CONST, name="const.abc", bytes=512)]
    calls = [("@record", [(program.A_I32, 0)], 0), ("@wait", [(program.A_I32, 0)], 1),
             ("mf_silu_f32", [(program.A_PTR, 0, 0), (program.A_PTR, 1, 128), (program.A_I64, 64)], 1),
             ("mf_cfg_combine", [(program.A_PTR, 0, 0), (program.A_PTR, -1, 0), (program.A_F32, 7.5), (program.A_PTR, 2, 16), (program.A_I64, 8)], 0)]
    blob = _blob(calls, bufs, nevents=1, meta='{"entry": "test"}')
    h = C.c_void_p()
    assert lib.mf_program_load(blob, C.c_int64(len(blob)), C.byref(h)) == 0, lib.mf_last_error()
    assert lib.mf_program_num_buffers(h) == 3 and lib.mf_program_num_calls(h) == 4 and lib.mf_program_meta(h) == b'{"entry": "test"}'
    assert lib.mf_program_find_buffer(h, b"const.abc") == 2 and lib.mf_program_find_buffer(h, b"nope") == -1
    kind, nbytes, off, name = C.c_int32(), C.c_int64(), C.c_int64(), C.c_char_p()
    assert lib.mf_program_buffer_info(h, 1, C.byref(kind), C.byref(nbytes), C.byref(off), C.byref(name)) == 0
    assert (kind.value, nbytes.value, off.value, name.value) == (program.KIND_WORKSPACE, 4096, -1, b"workspace.0")
    assert lib.mf_program_buffer_info(h, 2, C.byref(kind), C.byref(nbytes), C.byref(off), C.byref(name)) == 0
    assert off.value % 256 == 0 and off.value >= len(blob) + 256 and nbytes.value == 512
    assert lib.mf_program_bind(h, 0, C.c_void_p(0x1008)) != 0 and b"aligned" in lib.mf_last_error()
    assert lib.mf_program_bind(h, 7, C.c_void_p(0x1000)) != 0
    assert lib.mf_program_bind(h, 0, C.c_void_p(0x1000)) == 0
    assert lib.mf_program_run(h, None) != 0 and b"not bound" in lib.mf_last_error()       # refused before anything is launched
    lib.mf_program_destroy(h)
    # refusals: an entry without a thunk, a signature mismatch, a buffer index out of range, a stream the header does not declare, a foreign ABI
    for bad_calls, nev, what in (([("mf_adamw", [(program.A_PTR, 0, 0)], 0)], 0, b"no replay thunk"),
                                 ([("mf_silu_f32", [(program.A_PTR, 0, 0), (program.A_I64, 1), (program.A_I64, 64)], 0)], 0, b"signature"),
                                 ([("mf_silu_f32", [(program.A_PTR, 0, 0), (program.A_PTR, 9, 0), (program.A_I64, 64)], 0)], 0, b"signature"),
                                 ([("@wait", [(program.A_I32, 3)], 0)], 1, b"malformed")):
        b2 = _blob(bad_calls, bufs, nevents=nev)
        assert lib.mf_program_load(b2, C.c_int64(len(b2)), C.byref(h)) != 0 and what in lib.mf_last_error(), (what, lib.mf_last_error())
    b3 = bytearray(blob)
    b3[8:12] = struct.pack("<I", hip.ABI_VERSION + 1)
    assert lib.mf_program_load(bytes(b3), C.c_int64(len(b3)), C.byref(h)) != 0 and b"ABI" in lib.mf_last_error()
    assert lib.mf_program_load(blob[:-8], C.c_int64(len(blob) - 8), C.byref(h)) != 0
