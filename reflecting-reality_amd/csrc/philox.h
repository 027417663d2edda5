// The library's random stream, shared by every kernel that draws from it (csrc/rng.hip: the draws into memory; csrc/elementwise.hip:
// mf_sched_step_noise_dev, which draws into a register): the Philox4x32-10 block function and the transform to normals.  include/mfhip.h
// states the stream; one definition here, so that two kernels cannot disagree about a bit of it.
#pragma once
#include "mf_common.h"

namespace {

// ---- the block function: the same code on the host (mf_philox_bits_host) and in the kernels -----------------------------------------
// key = (seed low, seed high), counter = (block low, block high, 0, 0); the 64-bit block index is split here, in plain C++
__host__ __device__ inline void philox_block(uint64_t seed, uint64_t block, uint32_t x[4]) {
    uint32_t c0 = (uint32_t)block, c1 = (uint32_t)(block >> 32), c2 = 0u, c3 = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

__host__ __device__ inline int64_t blocks_of(int64_t n) { return (n + 3) / 4; }

// lanes (a, b) -> one Box-Muller pair.  u and phi are exact in fp32 (23 bits + the half), u in (0, 1); logf / sqrtf / sinpif / cospif
// are the accurate library functions (no native forms), the products are single roundings.
__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float scale, float& z0, float& z1) {
    const float u = ((float)(xa >> 9) + 0.5f) * 0x1p-23f, phi = ((float)(xb >> 9) + 0.5f) * 0x1p-23f;
    const float s = sqrtf(__fmul_rn(-2.0f, logf(u)));
    const float t = __fmul_rn(2.0f, phi);
    z0 = __fmul_rn(__fmul_rn(s, cospif(t)), scale);
    z1 = __fmul_rn(__fmul_rn(s, sinpif(t)), scale);
}

}  // namespace
