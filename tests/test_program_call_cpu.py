"""The two ends of a call as step programs, without a GPU: the new entries in the three descriptions of the ABI, the second thunk table of
csrc/program.hip against program.SIGNATURES_CALL, a program header exported for mf_encode_prompt through the loader, and the manifest
the exporter writes through the reader the C host uses (examples/c_host/manifest_reader.h, built into a stand-alone program)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import abi_header
from reflecting_reality_amd import hip, program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mf_u8_to_planes", "mf_encode_prompt", "mf_build_conditioning", "mf_decode_image")
NEW_THUNKS = ("mf_embed_tokens", "mf_act", "mf_attention_causal_bf16", "mf_attention_causal_f16", "mf_attention_causal_f16x3",
              "mf_softmax_rows_causal", "mf_minmax", "mf_image_normalize", "mf_mask_keep", "mf_postprocess", "mf_u8_to_planes", "mf_axpby_n")


def test_new_entries_exist_and_the_abi_version_stays():
    assert hip.ABI_VERSION == 23
    protos = abi_header.prototypes()
    lib = hip.load()
    for name in NEW_ENTRIES:
        assert name in hip.SIGNATURES and name in protos and hasattr(lib, name), name
    assert protos["mf_u8_to_planes"] == ("i", list("ppiiilp"))
    assert protos["mf_encode_prompt"] == ("i", list("pppp")) and protos["mf_build_conditioning"] == ("i", list("ppppppp"))
    assert protos["mf_decode_image"] == ("i", list("pppp"))
    assert lib.mf_abi_version() == 23


def test_every_new_replayable_entry_has_a_thunk_of_its_signature():
    """csrc/program.hip's kCallFns restates program.SIGNATURES_CALL; each signature is the header's prototype without the stream —
    except mf_axpby_n, whose two host arrays the recorder writes out flat; the thunk reads exactly the arguments the signature has."""
    src = open(os.path.join(ROOT, "reflecting-reality_amd", "csrc", "program.hip")).read()
    table = dict(re.findall(r'\{G_\w+,\s*"(mf_\w+)",\s*"(\w+)"\}', src))
    assert table == program.SIGNATURES_CALL and set(table) == set(NEW_THUNKS)
    assert not set(table) & set(program.SIGNATURES), "an entry belongs to one of the two tables"
    enum = re.search(r"enum CallFn \{(.*?)G_END", src, flags=re.S).group(1)
    ids = [e.split("=")[0].strip() for e in enum.replace("\n", " ").split(",") if e.strip()]
    assert len(ids) == len(table)
    protos = abi_header.prototypes()
    for name, sig in table.items():
        if name != "mf_axpby_n":
            assert "".join(protos[name][1][:-1]) == sig, name
    assert table["mf_axpby_n"] == "ppppppffffffipl"
    # every thunk indexes the arguments 0 .. len(sig) - 1 of its call, with the accessor of each one's kind
    kinds = {"P": "p", "FP": "p", "I": "i", "L": "l", "F": "f"}
    for gid, name in re.findall(r'\{(G_\w+),\s*"(mf_\w+)"', src):
        body = re.search(r"case %s:(.*?)(?=\n    case |\n    default:)" % gid, src, flags=re.S).group(1)
        used = {int(i): kinds[k] for k, i in re.findall(r"\b(FP|P|I|L|F)\((\d+)\)", body)}
        assert used == dict(enumerate(table[name])), f"{name}: the thunk reads {used}, the signature is {table[name]!r}"
    # the entries existing tests pin as not replayable stay so
    for name in ("mf_attention_ip_bf16", "mf_attention_ip_f16", "mf_attention_ip_f16x3", "mf_adamw", "mf_silu_bwd", "mf_concat_channels"):
        assert name not in program.SIGNATURES and name not in program.SIGNATURES_CALL


def test_flat_form_of_axpby():
    xs = (C.c_void_p * 2)(0x1000, 0x2000)
    cf = (C.c_float * 2)(0.5, -2.0)
    flat = program._flat_axpby((xs, cf, 2, 0x3000, 64, None))
    assert flat == (0x1000, 0x2000, None, None, None, None, 0.5, -2.0, 0.0, 0.0, 0.0, 0.0, 2, 0x3000, 64, None)
    assert len(flat) == len(program.SIGNATURES_CALL["mf_axpby_n"]) + 1
    with pytest.raises(program.ProgramError):
        program._flat_axpby((xs, cf, 7, 0x3000, 64, None))


def test_a_prompt_program_header_loads_and_the_entries_check_it():
    """A header as export_encode_prompt writes it (entry meta, the new entries' calls) loads without a GPU; the typed entries refuse a
    program exported for another one and an unbound one before anything is launched; a malformed header is refused."""
    lib = hip.load()
    bufs = [dict(kind=program.KIND_IO, name="input_ids", bytes=2 * 77 * 4), dict(kind=program.KIND_CONST, name="const.a", bytes=4096),
            dict(kind=program.KIND_WORKSPACE, name="workspace.0", bytes=1 << 16), dict(kind=program.KIND_IO, name="prompt_embeds", bytes=2 * 77 * 32 * 2)]
    P, I, L, F = program.A_PTR, program.A_I32, program.A_I64, program.A_F32
    calls = [("mf_embed_tokens", [(P, 0, 0), (P, 1, 0), (P, 1, 2048), (I, 1), (P, 2, 0), (I, 1), (I, 2), (I, 77), (I, 32), (I, 1000)], 0),
             ("mf_act", [(P, 2, 0), (P, 2, 0), (I, 1), (I, 3), (L, 2 * 77 * 32)], 0),
             ("mf_axpby_n", [(P, 2, 0)] + [(P, -1, 0)] * 5 + [(F, 0.5)] + [(F, 0.0)] * 5 + [(I, 1), (P, 2, 0), (L, 64)], 0),
             ("mf_u8_to_planes", [(P, 0, 0), (P, 2, 0), (I, 1), (I, 3), (I, 3), (L, 35)], 0)]
    blob = program.serialize_header(calls, bufs, 0, '{"entry": "mf_encode_prompt", "precision": "bf16"}')[0]
    h = C.c_void_p()
    assert lib.mf_program_load(blob, C.c_int64(len(blob)), C.byref(h)) == 0, lib.mf_last_error()
    assert lib.mf_program_num_calls(h) == 4 and lib.mf_program_find_buffer(h, b"prompt_embeds") == 3
    assert lib.mf_decode_image(h, None, None, None) != 0 and b"mf_decode_image" in lib.mf_last_error()
    assert lib.mf_build_conditioning(h, None, None, None, None, None, None) != 0 and b"not exported for this entry" in lib.mf_last_error()
    assert lib.mf_encode_prompt(h, None, None, None) != 0 and b"not bound" in lib.mf_last_error()       # the right entry: refused at the unbound buffers
    lib.mf_program_destroy(h)
    assert lib.mf_encode_prompt(None, None, None, None) != 0
    # a wrong argument kind, a wrong count, a truncated header
    bad = [("mf_act", [(P, 2, 0), (P, 2, 0), (I, 1), (L, 3), (L, 64)], 0)]
    b2 = program.serialize_header(bad, bufs, 0, "{}")[0]
    assert lib.mf_program_load(b2, C.c_int64(len(b2)), C.byref(h)) != 0 and b"signature" in lib.mf_last_error()
    bad = [("mf_u8_to_planes", [(P, 0, 0), (P, 2, 0), (I, 1), (I, 3), (L, 35)], 0)]
    b2 = program.serialize_header(bad, bufs, 0, "{}")[0]
    assert lib.mf_program_load(b2, C.c_int64(len(b2)), C.byref(h)) != 0 and b"no replay thunk" in lib.mf_last_error()
    assert lib.mf_program_load(blob[:-16], C.c_int64(len(blob) - 16), C.byref(h)) != 0


MANIFEST = dict(abi_version=23, precision="bf16", scheduler="UniPCMultistepScheduler", steps=5, batch=1, brushnet_once=False, cond_noise_batch=2,
                depth=True, init_noise_sigma=1.0,
                files=dict(encode_prompt="encode_prompt.mfprog", bind_prompt="bind_prompt.mfprog", conditioning="conditioning.mfprog",
                           step="step.mfprog", decode="decode.mfprog"),
                io=dict(conditioning=dict(image_u8=dict(shape=[1, 16, 16, 3], dtype="uint8"), cond=dict(shape=[2, 6, 8, 8], dtype="float32"))),
                shared_buffers=dict(cond=["conditioning", "step"]))

READER_MAIN = r'''
#include "manifest_reader.h"
int main(int argc, char** argv) {
    static mf_manifest m;
    char err[1280];
    int i;
    long long v;
    if (argc < 2) return 2;
    if (mf_manifest_read(argv[1], &m, err, sizeof(err)) != 0) { fprintf(stderr, "%s\n", err); return 1; }
    for (i = 0; i < m.n; ++i) printf("%s=%s\n", m.e[i].key, m.e[i].value);
    if (mf_manifest_int(&m, "steps", &v) != 0) return 3;
    printf("#steps %lld\n", v);
    if (mf_manifest_int(&m, "precision", &v) == 0 || mf_manifest_get(&m, "nope")) return 4;
    return 0;
}
'''


def test_manifest_round_trips_through_the_c_hosts_reader(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc is not None, "the C host's manifest reader is checked with gcc"
    program.write_manifest(str(tmp_path), MANIFEST)
    import json
    assert json.load(open(tmp_path / "manifest.json")) == MANIFEST
    (tmp_path / "reader.c").write_text(READER_MAIN)
    exe = str(tmp_path / "reader")
    subprocess.run([gcc, "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'examples', 'c_host')}",
                    str(tmp_path / "reader.c"), "-o", exe], check=True, capture_output=True, text=True)
    out = subprocess.run([exe, str(tmp_path / "manifest.txt")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict(line.split("=", 1) for line in out.stdout.splitlines() if not line.startswith("#"))
    want = dict(program._flat_items("", MANIFEST))
    assert got == want and "#steps 5" in out.stdout
    assert got["files.step"] == "step.mfprog" and got["io.conditioning.cond.shape"] == "2,6,8,8" and got["brushnet_once"] == "0" and got["depth"] == "1"
    # refused with a message: a missing file, a line without a value, a line that does not fit
    for text, what in ((None, "cannot open"), ("steps\n", "key value"), ("k " + "v" * 400 + "\n", "too long"), ("k" * 120 + " v\n", "too long")):
        path = tmp_path / "bad.txt"
        if text is None:
            path = tmp_path / "absent.txt"
        else:
            path.write_text(text)
        out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and what in out.stderr, (text, out.stderr)
    with pytest.raises(program.ProgramError):
        program.write_manifest(str(tmp_path), {"a key": 1})
