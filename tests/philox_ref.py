"""The library's random stream restated in numpy from its specification (include/mfhip.h, "random numbers"): Philox4x32-10, the layout
of bits, per-sample normals (Box-Muller, evaluated here in float64 from the same exact u and phi) and multiply-shift integers.  A plain
helper module, like gemm_ref.py; nothing here calls the library."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

# Random123's known answers for philox4x32-10: (counter, key, output)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32(ctr, key, rounds=10):
    """ctr: four arrays (or ints) of 32-bit words, key: two ints.  Returns four uint32 arrays."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k = [np.uint64(key[0]), np.uint64(key[1])]
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> S32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return [x.astype(np.uint32) for x in c]


def blocks(seed, first_block, count):
    """uint32 [count, 4]: the blocks first_block .. first_block + count - 1 (mod 2^64) of the generator `seed` (any int, read mod 2^64)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over="ignore"):
        idx = np.uint64(int(first_block) & 0xFFFFFFFFFFFFFFFF) + np.arange(count, dtype=np.uint64)
    x = philox4x32((idx & MASK, idx >> S32, np.zeros_like(idx), np.zeros_like(idx)), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(x, axis=1)


def ceil4(n):
    return (n + 3) // 4


def bits(seed, offset, n):
    return blocks(seed, offset, ceil4(n)).reshape(-1)[:n]


def randint(high, seed, offset, n, first=0):
    """Elements [first, first + n) of an integer draw below `high` that starts at `offset`."""
    x = blocks(seed, offset, ceil4(first + n)).reshape(-1)[first:first + n]
    return ((x.astype(np.uint64) * np.uint64(high)) >> S32).astype(np.int64)


def _unit(x):
    u = ((x >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert np.all(u.astype(np.float32) == u)          # exact in fp32, as the specification says
    return u


def normals_of(x, per):
    """float64 [per]: the normals the blocks x (uint32 [ceil(per / 4), 4]) give."""
    out = np.empty((x.shape[0], 4), dtype=np.float64)
    for a in (0, 2):
        u, phi = _unit(x[:, a]), _unit(x[:, a + 1])
        s = np.sqrt(-2.0 * np.log(u))
        out[:, a], out[:, a + 1] = s * np.cos(2.0 * np.pi * phi), s * np.sin(2.0 * np.pi * phi)
    return out.reshape(-1)[:per]


def normal_row(seed, first_block, per):
    """float64 [per]: one sample's normals from the blocks that start at first_block."""
    return normals_of(blocks(seed, first_block, ceil4(per)), per)


def normal(shape, seed, offset, first_sample=0):
    """float64 normals of shape [B, ...]: the rows [first_sample, first_sample + B) of a per-sample draw that starts at `offset`."""
    b, per = shape[0], int(np.prod(shape[1:], dtype=np.int64))
    rows = [normal_row(seed, offset + (first_sample + s) * ceil4(per), per) for s in range(b)]
    return np.stack(rows).reshape(shape)
