"""The library's own random stream without a GPU: the numpy oracle (philox_ref.py) against Random123's known answers, the host bits
(mf_philox_bits_host: the kernels' block function compiled for the host) against the oracle, the ABI surface, the block-count query, the
argument checks, and PhiloxGenerator's host-side bookkeeping."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import philox_ref as PR
from reflecting_reality_amd import _build, hip
from reflecting_reality_amd.rng import PhiloxGenerator, randn_tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mf_philox_normal_blocks", "mf_philox_int_blocks", "mf_philox_bits_host", "mf_philox_bits", "mf_philox_normal", "mf_philox_randint",
       "mf_philox_advance", "mf_train_batch_draw"]
SEEDS = [0, 1234, 2 ** 32 + 5, 2 ** 63 + 1]


def test_the_oracle_reproduces_random123s_known_answers():
    for ctr, key, want in PR.KNOWN_ANSWERS:
        got = tuple(int(x[0]) for x in PR.philox4x32(ctr, key))
        assert got == want, [f"{v:08x}" for v in got]


def _host_bits(n, seed, offset):
    return hip.philox_bits_host(n, seed, offset).numpy().view(np.uint32)


@pytest.mark.parametrize("seed", SEEDS)
def test_host_bits_equal_the_oracle(seed):
    for n in (1, 3, 4, 5, 1027):
        assert np.array_equal(_host_bits(n, seed, 0), PR.bits(seed, 0, n)), n
    for offset in (0, 1, 2 ** 32 - 2):          # the last one carries into the high counter word inside the draw
        assert np.array_equal(_host_bits(16, seed, offset), PR.bits(seed, offset, 16)), offset


def test_a_seed_above_2_63_travels_as_a_negative_int64():
    lib = hip.load()
    out = (C.c_uint32 * 8)()
    assert lib.mf_philox_bits_host(out, 8, -(2 ** 63 - 1), 0) == 0          # the same 64 bits as 2^63 + 1
    assert np.array_equal(np.frombuffer(out, dtype=np.uint32), PR.bits(2 ** 63 + 1, 0, 8))
    assert hip._s64(2 ** 63 + 1) == -(2 ** 63 - 1) and hip._s64(5) == 5 and hip._s64(2 ** 64 - 1) == -1


def test_an_empty_host_draw_is_an_empty_tensor_and_a_negative_count_is_named():
    assert tuple(hip.philox_bits_host(0, 1234, 0).shape) == (0,)
    with pytest.raises(hip.MfhipError, match="negative"):
        hip.philox_bits_host(-1, 1234, 0)


def test_consecutive_draws_continue_the_stream():
    whole = _host_bits(24, 1234, 7)
    assert np.array_equal(whole[:8], _host_bits(8, 1234, 7)) and np.array_equal(whole[8:], _host_bits(16, 1234, 7 + 2))


def test_the_new_entries_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "mfhip.h")).read()
    lib = hip.load()
    for name in NEW:
        assert name + "(" in header and name in hip.SIGNATURES and name in hip.EXPORTS and hasattr(lib, name), name
    assert lib.mf_abi_version() == 23 and hip.ABI_VERSION == 23
    assert "rng.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "rng.hip"))
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "T / 2^32"):       # the specification is in the header
        assert word in header, word


def test_block_counts_are_ceil_arithmetic():
    for samples, per in ((1, 1), (1, 4), (3, 7), (2, 256), (5, 0), (0, 9)):
        assert hip.philox_normal_blocks(samples, per) == samples * -(-per // 4)
    for n in (0, 1, 4, 5, 2 ** 20 + 3, 2 ** 40 + 1):
        assert hip.philox_int_blocks(n) == -(-n // 4)
    lib = hip.load()
    assert lib.mf_philox_normal_blocks(-1, 4) == -1 and b"negative" in lib.mf_last_error()
    assert lib.mf_philox_int_blocks(-1) == -1 and b"negative" in lib.mf_last_error()


def test_argument_errors_are_reported_without_a_gpu():
    """Every check runs before any HIP call: -1 and a message on a machine with no device (pointers only need to be non-null here)."""
    lib = hip.load()
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    arr = (C.c_void_p * 4)(p, p, None, None)

    def refused(rc, text):
        assert rc == -1 and text in lib.mf_last_error(), (rc, lib.mf_last_error())

    refused(lib.mf_philox_bits_host(None, 4, 0, 0), b"null output")
    refused(lib.mf_philox_bits_host(p, -1, 0, 0), b"negative")
    refused(lib.mf_philox_bits(None, 4, 0, 0, None, None), b"null output")
    refused(lib.mf_philox_bits(p, -4, 0, 0, None, None), b"negative")
    refused(lib.mf_philox_normal(None, 1, 4, 1.0, 0, 1, 0, 0, None, None), b"null output")
    refused(lib.mf_philox_normal(p, -1, 4, 1.0, 0, 1, 0, 0, None, None), b"negative")
    refused(lib.mf_philox_normal(p, 1, -4, 1.0, 0, 1, 0, 0, None, None), b"negative")
    refused(lib.mf_philox_normal(p, 2, 4, 1.0, 3, 4, 0, 0, None, None), b"global_batch 4 < first_sample 3 + samples 2")
    refused(lib.mf_philox_randint(None, 4, 10, 0, 4, 0, 0, None, None), b"null output")
    refused(lib.mf_philox_randint(p, -1, 10, 0, 4, 0, 0, None, None), b"negative")
    refused(lib.mf_philox_randint(p, 4, 0, 0, 4, 0, 0, None, None), b"outside (0, 2^31]")
    refused(lib.mf_philox_randint(p, 4, 2 ** 31 + 1, 0, 4, 0, 0, None, None), b"outside (0, 2^31]")
    refused(lib.mf_philox_randint(p, 4, 10, 2, 5, 0, 0, None, None), b"total 5 < first 2 + n 4")
    refused(lib.mf_philox_advance(None, 1, None), b"null state")
    refused(lib.mf_philox_advance(p, -1, None), b"negative")
    refused(lib.mf_train_batch_draw(None, 2, p, p, 1, 4, 1000, 0, 1, 0, 0, None, None), b"null output")
    refused(lib.mf_train_batch_draw(arr, 2, None, p, 1, 4, 1000, 0, 1, 0, 0, None, None), b"null output")
    refused(lib.mf_train_batch_draw(arr, 2, p, None, 1, 4, 1000, 0, 1, 0, 0, None, None), b"null output")
    refused(lib.mf_train_batch_draw((C.c_void_p * 2)(p, None), 2, p, p, 1, 4, 1000, 0, 1, 0, 0, None, None), b"null output")
    refused(lib.mf_train_batch_draw(arr, 5, p, p, 1, 4, 1000, 0, 1, 0, 0, None, None), b"sources")
    refused(lib.mf_train_batch_draw(arr, 4, p, p, -1, 4, 1000, 0, 1, 0, 0, None, None), b"negative")
    refused(lib.mf_train_batch_draw(arr, 4, p, p, 1, 4, 0, 0, 1, 0, 0, None, None), b"outside (0, 2^31]")
    refused(lib.mf_train_batch_draw(arr, 4, p, p, 2, 4, 1000, 3, 4, 0, 0, None, None), b"global_batch 4 < first_sample 3 + samples 2")


def test_generator_bookkeeping_is_host_arithmetic():
    g = PhiloxGenerator(1234)
    assert (g.seed, g.offset) == (1234, 0) and g.get_state() == (1234, 0)
    g.note_advanced(hip.philox_normal_blocks(3, 7))
    assert g.offset == 6
    g.note_advanced(hip.philox_int_blocks(5))
    assert g.get_state() == (1234, 8)
    h = PhiloxGenerator().set_state(g.get_state())
    assert h.get_state() == (1234, 8) and PhiloxGenerator(7).manual_seed(9).get_state() == (9, 0)
    big = PhiloxGenerator(2 ** 63 + 1)
    big.set_state((2 ** 63 + 1, 2 ** 64 - 1))
    big.note_advanced(2)                                   # the offset is a 64-bit counter: it wraps
    assert big.get_state() == (2 ** 63 + 1, 1)
    assert PhiloxGenerator(-1).seed == 2 ** 64 - 1


def test_randn_tensor_keeps_its_torch_semantics():
    """What tests/test_host_logic.py pins, restated here beside the new generator kind: a CPU generator draws on the host, a list draws
    one sample per generator, a wrong-sized list is refused; a PhiloxGenerator cannot produce a host tensor."""
    a = randn_tensor((2, 4, 8, 8), torch.Generator().manual_seed(5))
    assert torch.equal(a, torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(5))) and a.device.type == "cpu"
    gs = [torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)]
    b = randn_tensor((2, 4, 8, 8), gs)
    assert torch.equal(b[1:], torch.randn((1, 4, 8, 8), generator=torch.Generator().manual_seed(2)))
    with pytest.raises(ValueError):
        randn_tensor((3, 4, 8, 8), gs)
    with pytest.raises(ValueError, match="PhiloxGenerator"):
        randn_tensor((2, 4), PhiloxGenerator(1), "cpu")
    with pytest.raises(ValueError, match="mix"):
        randn_tensor((2, 4), [PhiloxGenerator(1), torch.Generator()], "cuda")
