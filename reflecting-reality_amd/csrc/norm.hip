// GroupNorm(+SiLU), LayerNorm and row softmax for NHWC / token-major activations on gfx950.
// All three are HBM-bound: one read + one write of the tensor (GroupNorm above 16x16 reads it twice: stats,
// then apply), fp32 statistics, vectorised 4-channel accesses, no atomics (bitwise reproducible).
#include <type_traits>
#include "mf_common.h"

namespace {

// Settled by sweeps (profiles/r03_groupnorm_grid_sweep.txt, profiles/gn_streaming_ab.txt: "the block target stays 1024 and U stays 4"):
constexpr int GN_MAX_CHUNKS = 64;          // chunks of rows per image in the statistics pass (and slots per group in ws)
constexpr int GN_TARGET_BLOCKS = 1024;     // blocks of the apply pass: ~4 row blocks per CU
constexpr int GN_ROWS_IN_FLIGHT = 4;       // whole rows a thread of either pass has in flight (U); 8 were slower or the same everywhere
constexpr int GN_BLK = 512;

struct GnArgs {
    const char* x0; const char* x1;
    int C0, C1, C, in_dt, HW, G, cpg, rows_per_chunk, nchunks;
    int cvn, tpr, rif;                 // vector columns per row, threads per row, rows in flight per block
    float eps;
    const float* gamma; const float* beta;
    int silu;
    char* out; int out_dt;
    float* ws;   // [batch][G][nchunks][2] = (mean, M2) of each chunk
    float* ws_ab;   // [batch][2][C] per-channel scale / shift (separate-finalize path)
    int fuse_finalize;
    // fp32 output: the apply pass forms y = ((x - mean_hi) - mean_lo) * a + beta with the group's mean as TWO floats, not x * a + shift:
    // the fp32 shift beta - mean * a rounds a term of size |mean| * rstd * |gamma| (1000 |gamma| for mean 100 / std 0.1), which alone
    // exceeds the 1e-4 the fp32-class modes promise.  centered: a separate finalize launch hands (mean_hi, mean_lo, rstd) of every group
    // to the apply pass in the image's own (by then consumed, or unused) chunk-statistics slots of ws, 3 floats per group.
    int centered;
    float* stats_out;   // nullable [batch][G][2]: (mean, rstd) of every group, kept for mf_groupnorm_bwd (training)
    // statistics handed over by the producers (mf_gemm_desc.gn_part): per-channel (sum, sum of squares) of every block of rows
    const float2* part0; const float2* part1; int pr0, pr1;
    const float2* grp0; int nch0;      // per-GROUP sums of x0 from its producer: [batch][nch0][G]; fuse_finalize == 2
    // the input as a deferred split-K reduce (mf_groupnorm_desc.sk_ws): slabs [split][batch * HW][C] fp32, bias / temb / alpha
    const float* sk_ws; int sk_splits; const float* sk_bias; const float* sk_temb; int64_t sk_ld_temb; float sk_alpha; int64_t sk_mn;
};

template <bool F16>
__device__ __forceinline__ float4 load4(const char* p, int dt, int64_t idx) {
    if (dt == MF_F32) return *reinterpret_cast<const float4*>(p + idx * 4);
    const uint2 u = *reinterpret_cast<const uint2*>(p + idx * 2);
    float4 r;
    unpack_h2<F16>(u.x, r.x, r.y);
    unpack_h2<F16>(u.y, r.z, r.w);
    return r;
}
template <bool F16>
__device__ __forceinline__ void store4(char* p, int dt, int64_t idx, float4 v) {
    if (dt == MF_F32) {
        *reinterpret_cast<float4*>(p + idx * 4) = v;
    } else {
        uint2 u;
        u.x = pack_h2<F16>(v.x, v.y);
        u.y = pack_h2<F16>(v.z, v.w);
        *reinterpret_cast<uint2*>(p + idx * 2) = u;
    }
}

template <bool F16>
__device__ __forceinline__ void load8(const char* p, int dt, int64_t idx, float* o) {
    if (dt == MF_F32) {
        const float4 a = *reinterpret_cast<const float4*>(p + idx * 4);
        const float4 b = *reinterpret_cast<const float4*>(p + idx * 4 + 16);
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
    } else {
        unpack_h8<F16>(*reinterpret_cast<const uint4*>(p + idx * 2), o);
    }
}
template <bool F16>
__device__ __forceinline__ void store8(char* p, int dt, int64_t idx, const float* v) {
    if (dt == MF_F32) {
        *reinterpret_cast<float4*>(p + idx * 4) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(p + idx * 4 + 16) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        *reinterpret_cast<uint4*>(p + idx * 2) = pack_h8<F16>(v);
    }
}

// A row piece of VW channels as it lies in memory, with the storage dtype a TEMPLATE argument (MF_F32 / MF_BF16 / MF_F16): a dtype
// code tested at run time makes hipcc merge the fp32 and 16-bit paths of every access (a dword + dwordx3 pair behind a uniform
// branch with a full vmcnt wait behind each), which left ONE row in flight per wave however far the loops were unrolled.  Rows stay
// packed (4 VGPRs for eight 16-bit channels) until they are used, so that U of them in flight cost U x 4 registers.
template <int DT, int VW>
struct gn_raw { uint4 q[DT == MF_F32 ? VW / 4 : 1]; };

// (every tensor of these kernels lies in global memory: the accesses say so, since a pointer rebuilt from its uniform halves,
// gn_uniform below, is otherwise a flat one, and a flat load waits on both counters)
#if defined(__HIP_DEVICE_COMPILE__)
#define GN_GLOBAL(T, p) reinterpret_cast<__attribute__((address_space(1))) T*>(reinterpret_cast<uintptr_t>(p))
#else
#define GN_GLOBAL(T, p) reinterpret_cast<T*>(p)
#endif
template <int DT, int VW>
__device__ __forceinline__ void gn_load(const char* p, gn_raw<DT, VW>& r) {
    if constexpr (DT == MF_F32) {
#pragma unroll
        for (int j = 0; j < VW / 4; ++j) r.q[j] = *GN_GLOBAL(const uint4, p + 16 * j);
    } else if constexpr (VW == 8) {
        r.q[0] = *GN_GLOBAL(const uint4, p);
    } else {
        const uint2 u = *GN_GLOBAL(const uint2, p);
        r.q[0].x = u.x; r.q[0].y = u.y;
    }
}
template <int DT, int VW>
__device__ __forceinline__ void gn_unpack(const gn_raw<DT, VW>& r, float* o) {
    if constexpr (DT == MF_F32) {
#pragma unroll
        for (int j = 0; j < VW / 4; ++j) {
            o[4 * j] = __uint_as_float(r.q[j].x); o[4 * j + 1] = __uint_as_float(r.q[j].y);
            o[4 * j + 2] = __uint_as_float(r.q[j].z); o[4 * j + 3] = __uint_as_float(r.q[j].w);
        }
    } else {
        constexpr bool F16 = DT == MF_F16;
        unpack_h2<F16>(r.q[0].x, o[0], o[1]);
        unpack_h2<F16>(r.q[0].y, o[2], o[3]);
        if constexpr (VW == 8) {
            unpack_h2<F16>(r.q[0].z, o[4], o[5]);
            unpack_h2<F16>(r.q[0].w, o[6], o[7]);
        }
    }
}
template <int DT, int VW>
__device__ __forceinline__ void gn_store(char* p, const float* v) {
    if constexpr (DT == MF_F32) {
#pragma unroll
        for (int j = 0; j < VW / 4; ++j) *GN_GLOBAL(float4, p + 16 * j) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    } else {
        constexpr bool F16 = DT == MF_F16;
        if constexpr (VW == 8) *GN_GLOBAL(uint4, p) = pack_h8<F16>(v);
        else *GN_GLOBAL(uint2, p) = uint2{pack_h2<F16>(v[0], v[1]), pack_h2<F16>(v[2], v[3])};
    }
}
// A wave-uniform pointer, opaque to the optimizer: base + 32-bit lane offset then stays a scalar base with a VGPR offset in the
// access itself.  Left alone, hipcc folds the lane offset into every row's pointer and keeps one 64-bit VGPR pair per row in flight.
template <typename T>
__device__ __forceinline__ T* gn_uniform(T* p) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return reinterpret_cast<T*>((uint64_t)hi << 32 | lo);
}
// A per-lane pointer the optimizer does not see through: row u's address is formed from it where it is used, not kept as one more
// 64-bit induction variable per row in flight
template <typename T>
__device__ __forceinline__ T* gn_lane_ptr(T* p) {
    asm("" : "+v"(p));
    return p;
}
// The packed form of 8 values that the storage dtype holds exactly (so that unpacking gives the same bits back)
template <int DT>
__device__ __forceinline__ void gn_repack(const float* v, gn_raw<DT, 8>& r) {
    if constexpr (DT == MF_F32) {
        r.q[0] = uint4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
        r.q[1] = uint4{__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7])};
    } else {
        r.q[0] = pack_h8<DT == MF_F16>(v);
    }
}
// The optimizer forgets what a packed row holds: values unpacked from it before are not kept alive in their fp32 form
template <int DT, int VW>
__device__ __forceinline__ void gn_forget(gn_raw<DT, VW>& r) {
#pragma unroll
    for (int j = 0; j < (int)(sizeof(r.q) / sizeof(uint4)); ++j) asm volatile("" : "+v"(r.q[j].x), "+v"(r.q[j].y), "+v"(r.q[j].z), "+v"(r.q[j].w));
}
// VW fp32 parameters (gamma / beta / the per-channel affine), 16-byte aligned
template <int VW>
__device__ __forceinline__ void gn_loadf(const float* p, float* o) {
    gn_raw<MF_F32, VW> r;
    gn_load<MF_F32, VW>(reinterpret_cast<const char*>(p), r);
    gn_unpack<MF_F32, VW>(r, o);
}

// Thread geometry shared by both passes: a row of C channels is cvn = C/VW vector columns; tpr = min(cvn, 512)
// threads cover one row and rif = 512/tpr rows are in flight per block, so every lane issues a 16-byte access
// (VW = 8 bf16 / 2 x 16 bytes fp32) and a block's footprint is whole contiguous rows.  A thread keeps the same
// column(s) for all of its rows: per-channel state (sums, or scale/shift) lives in registers.
//
// Pass 1, grid (nchunks, batch): per-(thread-row, channel) fp32 sums -> LDS -> one (mean, M2) per group of the
// chunk, in double.  No atomics: bitwise reproducible.
//
// The sums are those of x - pivot, one pivot per (image, group): the stored value at the image's first row, first channel of the
// group (gn_pivot).  Sums of the raw values lose the variance once the mean dwarfs the spread (mean 100, std 0.1: sum x^2 is 1e4 n,
// its fp32 rounding as large as the M2 = 0.01 n it is subtracted down to; tests/test_norm_conditioning_gpu.py).  A pivot inside the
// data leaves |x - pivot| of the order of the spread, all partial sums stay additive, and the double combine restores
// mean = pivot + S / n, M2 = SS - S^2 / n.  The pivot depends on the image's own data only.
template <int IN_DT>
__device__ __forceinline__ float gn_pivot(const GnArgs& p, int b, int g) {
    constexpr int esz = IN_DT == MF_F32 ? 4 : 2;
    const int c = g * p.cpg;
    const char* q = c < p.C0 ? p.x0 + ((int64_t)b * p.HW * p.C0 + c) * esz : p.x1 + ((int64_t)b * p.HW * p.C1 + (c - p.C0)) * esz;
    if constexpr (IN_DT == MF_F32) {
        return *GN_GLOBAL(const float, q);
    } else {
        float lo, hi;
        unpack_h2<IN_DT == MF_F16>((uint32_t)*GN_GLOBAL(const uint16_t, q), lo, hi);
        return lo;
    }
}
template <int IN_DT, int VW>
__global__ __launch_bounds__(GN_BLK) void gn_stats_kernel(const GnArgs p) {
    constexpr int U = GN_ROWS_IN_FLIGHT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float2* chan = reinterpret_cast<float2*>(smem_raw);   // [rif][C] (sum, sum of squares)
    const int chunk = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int lcol = t % p.tpr, trow = t / p.tpr;
    const int r0 = chunk * p.rows_per_chunk;
    int r1 = r0 + p.rows_per_chunk;
    if (r1 > p.HW) r1 = p.HW;
    constexpr int esz = IN_DT == MF_F32 ? 4 : 2;
    if (trow < p.rif) {
        for (int col = lcol; col < p.cvn; col += p.tpr) {
            const int c = col * VW;
            const char* base; int64_t ld; int cc;
            if (c < p.C0) { base = p.x0; ld = p.C0; cc = c; }
            else { base = p.x1; ld = p.C1; cc = c - p.C0; }
            float s[VW], ss[VW], piv[VW];
            {   // channel c + e lies in group (c + e) / cpg: one pivot load per group the column touches
                int g = c / p.cpg, rem = c - g * p.cpg;
                float pv = gn_pivot<IN_DT>(p, b, g);
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    s[e] = 0.0f; ss[e] = 0.0f; piv[e] = pv;
                    if (++rem == p.cpg && e + 1 < VW) { rem = 0; pv = gn_pivot<IN_DT>(p, b, ++g); }
                }
            }
            const int64_t step = (int64_t)p.rif * ld * esz;
            const char* ptr = base + (((int64_t)b * p.HW + r0 + trow) * ld + cc) * esz;
            int r = r0 + trow;
            for (; r + (U - 1) * p.rif < r1; r += U * p.rif, ptr += U * step) {
                gn_raw<IN_DT, VW> raw[U];
#pragma unroll
                for (int u = 0; u < U; ++u) gn_load<IN_DT, VW>(ptr + u * step, raw[u]);      // U whole rows in flight
#pragma unroll
                for (int u = 0; u < U; u += 4) {
                    float v[4][VW];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        gn_unpack<IN_DT, VW>(raw[u + k], v[k]);
#pragma unroll
                        for (int e = 0; e < VW; ++e) v[k][e] -= piv[e];
                    }
#pragma unroll
                    for (int e = 0; e < VW; ++e) {
                        s[e] += (v[0][e] + v[1][e]) + (v[2][e] + v[3][e]);
                        ss[e] += (v[0][e] * v[0][e] + v[1][e] * v[1][e]) + (v[2][e] * v[2][e] + v[3][e] * v[3][e]);
                    }
                }
            }
            for (; r < r1; r += p.rif, ptr += step) {
                gn_raw<IN_DT, VW> raw0;
                gn_load<IN_DT, VW>(ptr, raw0);
                float v0[VW];
                gn_unpack<IN_DT, VW>(raw0, v0);
#pragma unroll
                for (int e = 0; e < VW; ++e) { const float d = v0[e] - piv[e]; s[e] += d; ss[e] += d * d; }
            }
#pragma unroll
            for (int e = 0; e < VW; ++e) chan[trow * p.C + c + e] = make_float2(s[e], ss[e]);
        }
    }
    __syncthreads();
    {   // 8 lanes per group: fixed-order partial sums over the (thread-row, channel) list, then a butterfly
        const int l = t & 7;
        const int items = p.rif * p.cpg;
        for (int g = t >> 3; g < p.G; g += (int)blockDim.x >> 3) {
            double s = 0.0, ss = 0.0;
            for (int it = l; it < items; it += 8) {
                const int tr = it / p.cpg;
                const float2 v = chan[tr * p.C + g * p.cpg + (it - tr * p.cpg)];
                s += (double)v.x;
                ss += (double)v.y;
            }
#pragma unroll
            for (int off = 1; off < 8; off <<= 1) {
                s += __shfl_xor(s, off, 8);
                ss += __shfl_xor(ss, off, 8);
            }
            if (l == 0) {
                const double n = (double)(r1 - r0) * p.cpg;
                const double mean = s / n;                              // (of x - pivot)
                double m2 = ss - s * mean;
                if (m2 < 0.0) m2 = 0.0;
                float* o = p.ws + (((int64_t)b * p.G + g) * p.nchunks + chunk) * 2;
                o[0] = (float)((double)gn_pivot<IN_DT>(p, b, g) + mean);
                o[1] = (float)m2;
            }
        }
    }
}

// Pass 1b, grid (batch): combine the chunk statistics of every group in a fixed order (double) and write the
// per-channel affine y = x*a[c] + b[c].  (An in-kernel "last block finalizes" variant needs agent-scope fences,
// whose L2 writeback/invalidate on this multi-XCD part cost more than this launch: measured 95 us vs 34 us.)
// (mean, rstd) of every group of sample b from the per-chunk (mean_k, M2_k) of pass 1, by all threads of the block:
// chunk k holds (mean_k, M2_k) over n_k elements: mean = sum n_k mean_k / N, M2 = sum M2_k + n_k (mean_k - mean)^2.
// 8 lanes per group, each over chunks j, j+8, ...; fixed-order butterflies (xor partners add the same two values), so
// every block that evaluates it gets the same bits.
__device__ __forceinline__ void gn_group_mean_rstd(const GnArgs& p, int b, float* gm, float* gr, float* gl) {
    const int t = threadIdx.x;
    for (int g0 = 0; g0 < p.G; g0 += (int)blockDim.x >> 3) {
        const int g = g0 + (t >> 3), j = t & 7;
        const bool on = g < p.G;
        const float* st = p.ws + ((int64_t)b * p.G + (on ? g : 0)) * p.nchunks * 2;
        // Both passes read the chunk statistics with all eight loads in flight (the second pass hits the cache): a chunk past the
        // end is read from a clamped address and counts as zeros.  A branch around each load put a full wait behind every one of
        // them (eight dependent round trips in front of the apply loop).  `pass` is opaque to the optimizer, so that the second pass
        // re-reads instead of keeping 24 values (and their double forms, hoisted out of the g0 loop) alive across the butterflies:
        // that cost the fused apply kernel its occupancy.
        auto chunks = [&](int pass, float* m, float* q, float* cnt) {
            float2 v[GN_MAX_CHUNKS / 8];
#pragma unroll
            for (int u = 0; u < GN_MAX_CHUNKS / 8; ++u) {
                const int k = j + 8 * u + pass;
                v[u] = *reinterpret_cast<const float2*>(st + 2 * (k < p.nchunks ? k : 0));
            }
#pragma unroll
            for (int u = 0; u < GN_MAX_CHUNKS / 8; ++u) {
                asm volatile("" : "+v"(v[u].x), "+v"(v[u].y));      // (keeps the optimizer from sinking the load into the select below)
                const int k = j + 8 * u + pass;
                const bool have = on && k < p.nchunks;
                int rows = p.rows_per_chunk;
                if ((k + 1) * p.rows_per_chunk > p.HW) rows = p.HW - k * p.rows_per_chunk;
                m[u] = have ? v[u].x : 0.0f; q[u] = have ? v[u].y : 0.0f; cnt[u] = have ? (float)(rows * p.cpg) : 0.0f;
            }
        };
        int pass0 = 0, pass1 = 0;
        asm volatile("" : "+v"(pass0));
        double s1 = 0.0;
        {
            float pm[GN_MAX_CHUNKS / 8], pq[GN_MAX_CHUNKS / 8], pn[GN_MAX_CHUNKS / 8];
            chunks(pass0, pm, pq, pn);
#pragma unroll
            for (int u = 0; u < GN_MAX_CHUNKS / 8; ++u) s1 += (double)pn[u] * (double)pm[u];
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) s1 += __shfl_xor(s1, off, 8);
        asm volatile("" : "+v"(pass1), "+v"(s1));      // the second pass starts behind the butterfly
        const double n = (double)p.HW * p.cpg;
        const double mean = s1 / n;
        double m2 = 0.0;
        {
            float pm[GN_MAX_CHUNKS / 8], pq[GN_MAX_CHUNKS / 8], pn[GN_MAX_CHUNKS / 8];
            chunks(pass1, pm, pq, pn);
#pragma unroll
            for (int u = 0; u < GN_MAX_CHUNKS / 8; ++u) {
                const double d = (double)pm[u] - mean;
                m2 += (double)pq[u] + (double)pn[u] * d * d;
            }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) m2 += __shfl_xor(m2, off, 8);
        if (on && j == 0) {
            gm[g] = (float)mean;
            gl[g] = (float)(mean - (double)gm[g]);                  // mean = gm + gl to 2^-48
            gr[g] = (float)(1.0 / sqrt(m2 / n + (double)p.eps));
        }
    }
}

// (mean, rstd) of every group of sample b from the per-(row block, group) sums the producing GEMM left (GnArgs::grp0): 8 lanes per
// group, each over blocks j, j + 8, ... in double; fixed-order butterflies, so every block that evaluates it gets the same bits.
__device__ __forceinline__ void gn_group_from_sums(const GnArgs& p, int b, float* gm, float* gr, float* gl) {
    const int t = threadIdx.x;
    for (int g0 = 0; g0 < p.G; g0 += (int)blockDim.x >> 3) {
        const int g = g0 + (t >> 3), j = t & 7;
        const bool on = g < p.G;
        double s = 0.0, q = 0.0;
        if (on) {
            const float2* src = p.grp0 + (int64_t)b * p.nch0 * p.G + g;
            for (int k0 = j; k0 < p.nch0; k0 += 32) {                  // up to four independent loads in flight (nch0 <= 64), added in order
                float2 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {                           // (a block past the end: clamped address, counted as zeros)
                    const bool have = k0 + 8 * u < p.nch0;
                    v[u] = src[(int64_t)(have ? k0 + 8 * u : k0) * p.G];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    asm volatile("" : "+v"(v[u].x), "+v"(v[u].y));      // (keeps the optimizer from sinking the load into the select)
                    v[u] = k0 + 8 * u < p.nch0 ? v[u] : make_float2(0.0f, 0.0f);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) { s += (double)v[u].x; q += (double)v[u].y; }
            }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            s += __shfl_xor(s, off, 8);
            q += __shfl_xor(q, off, 8);
        }
        if (on && j == 0) {
            const double n = (double)p.HW * p.cpg;
            const double mean = s / n;
            double m2 = q - s * mean;
            if (m2 < 0.0) m2 = 0.0;
            gm[g] = (float)mean;
            gl[g] = (float)(mean - (double)gm[g]);
            gr[g] = (float)(1.0 / sqrt(m2 / n + (double)p.eps));
        }
    }
}

// Where a finalize launch leaves (mean_hi, mean_lo, rstd) of group g of image b for a centered apply pass (GnArgs::centered): the
// first 3 G floats of the image's own chunk-statistics slots ([G][nchunks][2] floats, nchunks >= 2).  Only the block(s) of image b
// touch them: gn_finalize_kernel has read all of them (a barrier lies in between), gn_finalize_part_kernel's route never fills them.
__device__ __forceinline__ float* gn_group_triple(const GnArgs& p, int b, int g) {
    return p.ws + (int64_t)b * p.G * p.nchunks * 2 + g * 3;
}

__global__ __launch_bounds__(GN_BLK) void gn_finalize_kernel(const GnArgs p) {
    __shared__ float gm[64], gr[64], gl[64];
    const int b = blockIdx.x, t = threadIdx.x;
    gn_group_mean_rstd(p, b, gm, gr, gl);
    __syncthreads();
    if (p.centered)
        for (int g = t; g < p.G; g += blockDim.x) {
            float* o = gn_group_triple(p, b, g);
            o[0] = gm[g]; o[1] = gl[g]; o[2] = gr[g];
        }
    if (p.stats_out)
        for (int g = t; g < p.G; g += blockDim.x) {
            p.stats_out[((int64_t)b * p.G + g) * 2] = gm[g];
            p.stats_out[((int64_t)b * p.G + g) * 2 + 1] = gr[g];
        }
    float* ab = p.ws_ab + (int64_t)b * 2 * p.C;
    for (int c = t; c < p.C; c += blockDim.x) {
        const int g = c / p.cpg;
        const float a = gr[g] * p.gamma[c];
        ab[c] = a;
        ab[p.C + c] = p.beta[c] - gm[g] * a;
    }
}

// Pass 1 replaced (round 6): the producing GEMMs left per-channel (sum, sum of squares) of every block of pr rows of their output
// (gemm_conv_kernel.h, GemmArgs::gn_part), so the statistics pass over the tensor is this launch over HW / pr * C float pairs per
// image.  grid (batch, slices): a block takes a contiguous run of groups; a thread sums one channel's blocks in block order
// (double), 8 lanes then combine a group's channels in a fixed order — every bit is reproducible.  Writes the per-channel
// affine y = x * a[c] + b[c] like gn_finalize_kernel.
__global__ __launch_bounds__(GN_BLK) void gn_finalize_part_kernel(const GnArgs p, int gps, int kparts) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double2* chan = reinterpret_cast<double2*>(smem_raw);          // [kparts][gps * cpg] partial (sum, sum of squares), then row 0 = the totals
    __shared__ float gm[64], gr[64];
    const int b = blockIdx.x, t = threadIdx.x;
    const int g0 = blockIdx.y * gps;
    int g1 = g0 + gps;
    if (g1 > p.G) g1 = p.G;
    const int c0 = g0 * p.cpg, nc = (g1 - g0) * p.cpg, ncmax = gps * p.cpg;
    // (the affine parameters of the last stage are requested first: their latency hides under the partial sums')
    const float gam = t < nc ? p.gamma[c0 + t] : 0.0f, bet = t < nc ? p.beta[c0 + t] : 0.0f;
    // thread (channel j, part kp) sums the blocks kp, kp + kparts, ... of its channel: the launch is latency-bound (the partial sums
    // come from other XCDs' L2s through the fabric), so the loads of a channel are spread over kparts threads and issued together —
    // one thread per channel walking 32 blocks measured 11 us, as long as the statistics pass this launch replaces
    for (int idx = t; idx < nc * kparts; idx += blockDim.x) {
        const int kp = idx / nc, j = idx - kp * nc;
        const int c = c0 + j;
        const float2* src; int nb; int64_t ld;
        if (c < p.C0) { nb = p.HW / p.pr0; ld = p.C0; src = p.part0 + (int64_t)b * nb * ld + c; }
        else { nb = p.HW / p.pr1; ld = p.C1; src = p.part1 + (int64_t)b * nb * ld + (c - p.C0); }
        double s = 0.0, q = 0.0;
        int k = kp;
        for (; k + 3 * kparts < nb; k += 4 * kparts) {             // four independent loads in flight
            const float2 v0 = src[(int64_t)k * ld], v1 = src[(int64_t)(k + kparts) * ld], v2 = src[(int64_t)(k + 2 * kparts) * ld],
                         v3 = src[(int64_t)(k + 3 * kparts) * ld];
            s += (double)v0.x; q += (double)v0.y; s += (double)v1.x; q += (double)v1.y;
            s += (double)v2.x; q += (double)v2.y; s += (double)v3.x; q += (double)v3.y;
        }
        for (; k < nb; k += kparts) {
            const float2 v = src[(int64_t)k * ld];
            s += (double)v.x; q += (double)v.y;
        }
        chan[kp * ncmax + j] = make_double2(s, q);
    }
    __syncthreads();
    for (int j = t; j < nc; j += blockDim.x) {                     // parts in order: reproducible
        double s = 0.0, q = 0.0;
        for (int kp = 0; kp < kparts; ++kp) { const double2 v = chan[kp * ncmax + j]; s += v.x; q += v.y; }
        chan[j] = make_double2(s, q);                              // (row 0 is written by the thread that read column j of every row)
    }
    __syncthreads();
    {
        const int l = t & 7;
        for (int g = g0 + (t >> 3); g < g1; g += (int)blockDim.x >> 3) {
            double s = 0.0, q = 0.0;
            for (int it = l; it < p.cpg; it += 8) {
                const double2 v = chan[(g - g0) * p.cpg + it];
                s += v.x; q += v.y;
            }
#pragma unroll
            for (int off = 1; off < 8; off <<= 1) {
                s += __shfl_xor(s, off, 8);
                q += __shfl_xor(q, off, 8);
            }
            if (l == 0) {
                const double n = (double)p.HW * p.cpg;
                const double mean = s / n;
                double m2 = q - s * mean;
                if (m2 < 0.0) m2 = 0.0;
                gm[g - g0] = (float)mean;
                gr[g - g0] = (float)(1.0 / sqrt(m2 / n + (double)p.eps));
                if (p.centered) {
                    float* o = gn_group_triple(p, b, g);
                    o[0] = gm[g - g0]; o[1] = (float)(mean - (double)gm[g - g0]); o[2] = gr[g - g0];
                }
                if (p.stats_out) {
                    p.stats_out[((int64_t)b * p.G + g) * 2] = gm[g - g0];
                    p.stats_out[((int64_t)b * p.G + g) * 2 + 1] = gr[g - g0];
                }
            }
        }
    }
    __syncthreads();
    float* ab = p.ws_ab + (int64_t)b * 2 * p.C;
    for (int j = t; j < nc; j += blockDim.x) {
        const int c = c0 + j, g = j / p.cpg;
        const float a = gr[g] * (j == t ? gam : p.gamma[c]);
        ab[c] = a;
        ab[p.C + c] = (j == t ? bet : p.beta[c]) - gm[g] * a;
    }
}

// Waves per SIMD the apply kernel is compiled for.  With U = 4 packed 16-bit rows (4 VGPRs each) and the scale / shift of 8 channels
// the row loop needs about 60 VGPRs, but the statistics combine in the prologue (double-precision divisions, a square root) spills
// below 80: 6 waves per SIMD = three resident blocks of 8 waves per CU.  Two segments (per-lane row pointers) take the
// 96 VGPRs of 5 waves; fp32 rows need more.  tests/test_groupnorm_resources_cpu.py holds the 16-bit kernels to 96 and no scratch.
constexpr int gn_apply_waves(int in_dt, int out_dt, bool seg2) {
    return in_dt == MF_F32 || out_dt == MF_F32 ? 4 : !seg2 ? 6 : 5;
}

// Pass 2, grid (row blocks, batch): pure streaming y = silu(x*a[c] + b[c]) with the thread's a/b in registers.
// Storage dtypes, vector width and SiLU are template arguments, the rows in flight (U) a constant, and everything else a launch decides (the three
// fuse_finalize modes, the segment a column lies in) is settled before the row loop, so that the loop is U whole-row loads issued
// back to back, counted waits, branch-free arithmetic on one unpacked row at a time and whole-row stores.
template <int IN_DT, int OUT_DT, int VW, bool SILU, bool SEG2>
__global__ __launch_bounds__(GN_BLK, gn_apply_waves(IN_DT, OUT_DT, SEG2)) void gn_apply_kernel(const GnArgs p, int rows_per_block) {
    constexpr int U = GN_ROWS_IN_FLIGHT;
    const int b = blockIdx.y, t = threadIdx.x;
    const int lcol = t % p.tpr, trow = t / p.tpr;
    __shared__ float gm[64], gr[64], gl[64];
    constexpr bool CENTERED = OUT_DT == MF_F32;      // y = ((x - sm) - sl) * sa + sb (GnArgs::centered); else y = x * sa + sb
    // the statistics of the groups are in LDS (combined here, or left by a finalize launch): the affine is formed from gamma / beta
    const bool from_stats = p.fuse_finalize || (CENTERED && p.centered);
    float ga[VW], be[VW];
    if (!p.fuse_finalize && from_stats) {
        gn_loadf<VW>(p.gamma + lcol * VW, ga);
        gn_loadf<VW>(p.beta + lcol * VW, be);
        for (int g = t; g < p.G; g += blockDim.x) {
            const float* o = gn_group_triple(p, b, g);
            gm[g] = o[0]; gl[g] = o[1]; gr[g] = o[2];
        }
        __syncthreads();
    }
    if (p.fuse_finalize) {       // every block combines the chunk statistics itself: one launch (and its gap) less
        // (the affine parameters of the thread's first column are requested first: their latency hides under the combine)
        gn_loadf<VW>(p.gamma + lcol * VW, ga);
        gn_loadf<VW>(p.beta + lcol * VW, be);
        if (p.fuse_finalize == 2) gn_group_from_sums(p, b, gm, gr, gl);
        else gn_group_mean_rstd(p, b, gm, gr, gl);
        __syncthreads();
        if (p.stats_out && blockIdx.x == 0)
            for (int g = t; g < p.G; g += blockDim.x) {
                p.stats_out[((int64_t)b * p.G + g) * 2] = gm[g];
                p.stats_out[((int64_t)b * p.G + g) * 2 + 1] = gr[g];
            }
    }
    if (trow >= p.rif) return;
    const int r0 = blockIdx.x * rows_per_block;
    int r1 = r0 + rows_per_block;
    if (r1 > p.HW) r1 = p.HW;
    constexpr int esz = IN_DT == MF_F32 ? 4 : 2, osz = OUT_DT == MF_F32 ? 4 : 2;
    constexpr bool fast_silu = OUT_DT != MF_F32;        // 16-bit output: __expf is far inside the rounding
    const float* ab = p.ws_ab + (int64_t)b * 2 * p.C;
    float sa[VW], sb[VW], sm[CENTERED ? VW : 1], sl[CENTERED ? VW : 1];
    auto affine = [&](int c, const float* gam, const float* bet) {
        int g = c / p.cpg, rem = c - g * p.cpg;          // one division per column: channel c + e lies in group (c + e) / cpg
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            sa[e] = gr[g] * gam[e];
            if constexpr (CENTERED) { sb[e] = bet[e]; sm[e] = gm[g]; sl[e] = gl[g]; }
            else sb[e] = bet[e] - gm[g] * sa[e];
            if (++rem == p.cpg) { rem = 0; ++g; }
        }
    };
    if (from_stats) affine(lcol * VW, ga, be);
    // the output of a block: a wave-uniform base plus a 32-bit lane offset that is the same for every row of the thread
    char* const obase = p.out + ((int64_t)b * p.HW + r0) * p.C * osz;
    const int64_t ostep = (int64_t)p.rif * p.C * osz;
    for (int col = lcol; col < p.cvn; col += p.tpr) {
        const int c = col * VW;
        if (!from_stats) {
            gn_loadf<VW>(ab + c, sa);
            gn_loadf<VW>(ab + p.C + c, sb);
            if constexpr (CENTERED) {                    // (not centered — gamma / beta off 16 bytes, one chunk: the per-channel shift, around a mean of 0)
#pragma unroll
                for (int e = 0; e < VW; ++e) { sm[e] = 0.0f; sl[e] = 0.0f; }
            }
        } else if (col != lcol) {
            float g2[VW], b2[VW];
            gn_loadf<VW>(p.gamma + c, g2);
            gn_loadf<VW>(p.beta + c, b2);
            affine(c, g2, b2);
        }
        // One segment (SEG2 = false): like the output, a wave-uniform row pointer plus one 32-bit lane offset — the addresses of
        // all rows in flight cost one VGPR.  Two segments: the segment, and with it the row pitch, differs from lane to lane, so
        // the row pointer is per lane (ioff = 0) and the pitch a 32-bit lane value.
        const char* ptr; unsigned ioff;
        typename std::conditional<SEG2, unsigned, int64_t>::type step;
        if constexpr (SEG2) {
            const bool first = c < p.C0;
            const int ld = first ? p.C0 : p.C1, cc = first ? c : c - p.C0;
            ptr = (first ? p.x0 : p.x1) + (((int64_t)b * p.HW + r0 + trow) * ld + cc) * esz;
            ioff = 0;
            step = (unsigned)(p.rif * ld) * esz;
        } else {
            ptr = p.x0 + ((int64_t)b * p.HW + r0) * p.C0 * esz;
            ioff = (unsigned)(trow * p.C0 + c) * esz;
            step = (int64_t)p.rif * p.C0 * esz;
        }
        const unsigned ooff = (unsigned)(trow * p.C + c) * osz;
        char* optr = obase;
        auto finish = [&](const gn_raw<IN_DT, VW>& raw, char* o) {
            float v[VW];
            gn_unpack<IN_DT, VW>(raw, v);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                float y;
                if constexpr (CENTERED) y = ((v[e] - sm[e]) - sl[e]) * sa[e] + sb[e];
                else y = v[e] * sa[e] + sb[e];
                if constexpr (SILU) y = fast_silu ? silu_f(y) : silu_precise(y);
                v[e] = y;
            }
            gn_store<OUT_DT, VW>(gn_uniform(o) + ooff, v);
        };
        int r = r0 + trow;
        for (; r + (U - 1) * p.rif < r1; r += U * p.rif, ptr += U * step, optr += U * ostep) {
            gn_raw<IN_DT, VW> raw[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {                                                       // U whole rows in flight
                if constexpr (SEG2) gn_load<IN_DT, VW>(gn_lane_ptr(ptr) + u * step, raw[u]);
                else gn_load<IN_DT, VW>(gn_uniform(ptr + u * step) + ioff, raw[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) finish(raw[u], optr + u * ostep);
        }
        // at most U - 1 rows are left: TB at a time, their loads go out together too (a row past the end re-reads row r)
        constexpr int TB = U - 1;
        for (; r < r1; r += TB * p.rif, ptr += TB * step, optr += TB * ostep) {
            gn_raw<IN_DT, VW> raw[TB];
#pragma unroll
            for (int u = 0; u < TB; ++u) gn_load<IN_DT, VW>((r + u * p.rif < r1 ? ptr + u * step : ptr) + ioff, raw[u]);
#pragma unroll
            for (int u = 0; u < TB; ++u)
                if (r + u * p.rif < r1) finish(raw[u], optr + u * ostep);
        }
    }
}

// One-launch GroupNorm for the lowest-resolution levels (HW <= 256: 16x16 / 8x8 latents), where the two-launch form
// above is a chain of dependent launches and memory round trips, not bytes (tools/bench_gn.py: 12 us at 8x8 for 2 MB).
// grid (C / SC, batch): a block owns a SLAB of SC = lcm(cpg, 8) channels = whole groups = nv 16-byte vector columns
// over ALL HW rows of one sample, so the statistics never leave the block and the rows never leave the registers.
// Thread t = lane * nv + vcol keeps vector column vcol of rows lane, lane + P, ... (at most ROWS): per-channel fp32
// (sum, sum of squares) of x - pivot -> LDS -> one wave per group combines them in double in a fixed order (bitwise
// reproducible) -> y = silu(x * a[c] + b[c]) from the registers.
// Storage dtypes, SiLU and the deferred split-K input (SK: GnArgs::sk_ws) are template arguments.  Everything the block needs from
// memory is requested at the top, before the first wait: gamma / beta (and bias / temb of a deferred reduce), then all ROWS rows —
// a row past HW is read from a clamped address and replaced by zeros, not branched around.
template <int IN_DT, int OUT_DT, bool SILU, bool SK, int ROWS = 4>
__global__ __launch_bounds__(1024, IN_DT != MF_F32 && OUT_DT != MF_F32 ? 5 : 4) void gn_slab_kernel(const GnArgs p, int SC, int nv, int P) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float2* chan = reinterpret_cast<float2*>(smem_raw);              // [P][SC or SC/8] (sum, sum of squares) of x - pivot
    __shared__ float gm[8], gr[8], gp[8];                            // per group of the slab: mean, rstd, pivot
    const int slab = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int vcol = t % nv, lane = t / nv;
    const bool active = lane < P;                      // the block is padded to whole waves for the butterflies
    const int c = slab * SC + vcol * 8;
    constexpr int esz = IN_DT == MF_F32 ? 4 : 2, osz = OUT_DT == MF_F32 ? 4 : 2;
    const bool whole = p.cpg % 8 == 0;                 // a thread's 8 channels lie in one group: pre-reduce them
    const int W = whole ? SC / 8 : SC;                 // LDS items per lane
    float sa[8], sb[8];
    if constexpr (!SK) {
        gn_loadf<8>(p.gamma + c, sa);
        gn_loadf<8>(p.beta + c, sb);
    }
    // the rows of the thread stay PACKED from here to the stores behind the two barriers (4 VGPRs per 16-bit row, not 8): they
    // are unpacked once for the statistics and once more for the output
    gn_raw<IN_DT, 8> raw[ROWS];
    if constexpr (!SK) {
        const char* base; int64_t ld; int cc;
        if (c < p.C0) { base = p.x0; ld = p.C0; cc = c; }
        else { base = p.x1; ld = p.C1; cc = c - p.C0; }
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int row = lane + i * P < p.HW ? lane + i * P : p.HW - 1;
            gn_load<IN_DT, 8>(base + (((int64_t)b * p.HW + row) * ld + cc) * esz, raw[i]);
        }
    } else {
        // the producer's split-K slabs: summed in slab order, + bias + temb, * alpha, rounded to the storage dtype — what
        // splitk_reduce_kernel + epilogue_store8 (csrc/gemm_conv.hip) would have stored and this kernel read back
        const bool has_bias = p.sk_bias != nullptr, has_temb = p.sk_temb != nullptr;
        float bt[8], tb[8];                            // (an absent term is read from gamma and never added)
        gn_loadf<8>(has_bias ? p.sk_bias + c : p.gamma + c, bt);
        gn_loadf<8>(has_temb ? p.sk_temb + (int64_t)b * p.sk_ld_temb + c : p.gamma + c, tb);
        float v[ROWS][8];
#pragma unroll
        for (int i = 0; i < ROWS; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] = 0.0f;
        unsigned roff[ROWS];                            // a slab of one image is below 4 GB: uniform slab pointer + 32-bit lane offsets
#pragma unroll
        for (int i = 0; i < ROWS; ++i) roff[i] = (unsigned)((lane + i * P < p.HW ? lane + i * P : p.HW - 1) * p.C + c) * 4u;
        const char* src = reinterpret_cast<const char*>(p.sk_ws + (int64_t)b * p.HW * p.C);
        for (int z = 0; z < p.sk_splits; ++z, src += p.sk_mn * 4) {  // a slab's ROWS rows in flight together; the additions keep the slab order
            gn_raw<MF_F32, 8> part[ROWS];
#pragma unroll
            for (int i = 0; i < ROWS; ++i) gn_load<MF_F32, 8>(gn_uniform(src) + roff[i], part[i]);
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                float x[8];
                gn_unpack<MF_F32, 8>(part[i], x);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[i][e] += x[e];
            }
        }
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const bool in = lane + i * P < p.HW;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float x = v[i][e];
                x = has_bias ? x + bt[e] : x;
                x = has_temb ? x + tb[e] : x;
                x *= p.sk_alpha;
                v[i][e] = in ? x : 0.0f;
            }
            // rounded to the storage dtype (nearest-even, the conversion epilogue_store8 uses) by packing; the statistics take the
            // rounded values
            gn_repack<IN_DT>(v[i], raw[i]);
            gn_forget(raw[i]);                         // (fp32 storage: what the reduce would have stored, not a product to contract into the sums below)
        }
    }
    // (the rows wait for the barrier in their packed form: the statistics unpack them once more, channel by channel)
#pragma unroll
    for (int i = 0; i < ROWS; ++i) gn_forget(raw[i]);
    // The pivot of every group of the slab (see gn_stats_kernel): the value at row 0, first channel of the group, as stored (or as
    // the deferred reduce would have stored it), published by the thread that holds it.  Row 0 is the first row of lane 0.
    if (lane == 0) {
        float x0[8];
        gn_unpack<IN_DT, 8>(raw[0], x0);
        int g = vcol * 8 / p.cpg, rem = vcol * 8 - g * p.cpg;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (rem == 0) gp[g] = x0[e];
            if (++rem == p.cpg) { rem = 0; ++g; }
        }
    }
    __syncthreads();
    if (active) {
        float s[8], ss[8];
        int g = vcol * 8 / p.cpg, rem = vcol * 8 - g * p.cpg;
#pragma unroll
        for (int e = 0; e < 8; ++e) {                              // channel by channel: one pivot and one element of every row at a time
            const float pv = gp[g];
            if (++rem == p.cpg) { rem = 0; ++g; }
            float d[ROWS];
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                float x[8];
                gn_unpack<IN_DT, 8>(raw[i], x);
                d[i] = lane + i * P < p.HW ? x[e] - pv : 0.0f;     // (a row past the end counts as zeros, not as minus the pivot)
            }
            s[e] = 0.0f; ss[e] = 0.0f;
            // The squares are summed as one explicit fma chain: left to the compiler, d0 * d0 + d1 * d1 is contracted one way in
            // one instantiation and the other way in the next, and the deferred split-K form (SK) must give the bits of the plain one.
#pragma unroll
            for (int i = 0; i < ROWS; i += 4) {
                s[e] += (d[i] + d[i + 1]) + (d[i + 2] + d[i + 3]);
                ss[e] += fmaf(d[i + 3], d[i + 3], fmaf(d[i + 2], d[i + 2], fmaf(d[i + 1], d[i + 1], __fmul_rn(d[i], d[i]))));
            }
        }
        if (whole) {
            const float s8 = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
            const float q8 = ((ss[0] + ss[1]) + (ss[2] + ss[3])) + ((ss[4] + ss[5]) + (ss[6] + ss[7]));
            chan[lane * W + vcol] = make_float2(s8, q8);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) chan[lane * W + vcol * 8 + e] = make_float2(s[e], ss[e]);
        }
    }
#pragma unroll
    for (int i = 0; i < ROWS; ++i) gn_forget(raw[i]);
    if constexpr (SK) {
        // (the slab sums, bias and temb, then the shifted sums took the registers until here: gamma / beta are requested now, a
        // barrier and the combine ahead of their use)
        gn_loadf<8>(p.gamma + c, sa);
        gn_loadf<8>(p.beta + c, sb);
    }
    __syncthreads();
    {   // one wave per group of the slab: fixed-order partial sums in double, then a butterfly
        const int l = t & 63, ipg = whole ? p.cpg / 8 : p.cpg, items = P * ipg, gps = SC / p.cpg;
        for (int g = t >> 6; g < gps; g += (int)blockDim.x >> 6) {
            double s = 0.0, ss = 0.0;
            for (int it = l; it < items; it += 64) {
                const int tr = it / ipg;
                const float2 x = chan[tr * W + g * ipg + (it - tr * ipg)];
                s += (double)x.x;
                ss += (double)x.y;
            }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                s += __shfl_xor(s, off, 64);
                ss += __shfl_xor(ss, off, 64);
            }
            if (l == 0) {
                const double n = (double)p.HW * p.cpg;
                const double mean = s / n;                              // (of x - pivot)
                double m2 = ss - s * mean;
                if (m2 < 0.0) m2 = 0.0;
                gm[g] = (float)((double)gp[g] + mean);
                gr[g] = (float)(1.0 / sqrt(m2 / n + (double)p.eps));
                if (p.stats_out) {
                    p.stats_out[((int64_t)b * p.G + slab * gps + g) * 2] = gm[g];
                    p.stats_out[((int64_t)b * p.G + slab * gps + g) * 2 + 1] = gr[g];
                }
            }
        }
    }
    __syncthreads();
    if (!active) return;
    {
        int g = vcol * 8 / p.cpg, rem = vcol * 8 - g * p.cpg;       // channel vcol * 8 + e of the slab lies in its group (vcol * 8 + e) / cpg
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sa[e] = gr[g] * sa[e];
            sb[e] = sb[e] - gm[g] * sa[e];
            if (++rem == p.cpg) { rem = 0; ++g; }
        }
    }
    constexpr bool fast_silu = OUT_DT != MF_F32;
    const int64_t ostep = (int64_t)P * p.C * osz;
    char* optr = p.out + (((int64_t)b * p.HW + lane) * p.C + c) * osz;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        if (lane + i * P < p.HW) {
            float y[8];
            gn_unpack<IN_DT, 8>(raw[i], y);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                y[e] = y[e] * sa[e] + sb[e];
                if constexpr (SILU) y[e] = fast_silu ? silu_f(y[e]) : silu_precise(y[e]);
            }
            gn_store<OUT_DT, 8>(optr + i * ostep, y);
        }
    }
}

// Half a wave per row (two rows per wave, 8 per block), 8-channel (16-byte) vectors: C % 8 == 0, C <= 2048.
// For the transformer widths of the path (320 / 640 / 1280) this moves twice the bytes per instruction of the
// 4-channel kernel below and halves the dependent shuffle chain (5 steps inside 32 lanes).
template <bool F16>
__global__ __launch_bounds__(256) void layernorm8_kernel(const char* x, int in_dt, char* out, int out_dt,
                                                         const float* gamma, const float* beta, int64_t rows, int C,
                                                         float eps) {
    const int l32 = threadIdx.x & 31;
    const int64_t row = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool live = row < rows;                       // keep every lane alive for the shuffles
    constexpr int MAXV = 8;
    float v[MAXV][8];
    const int c8n = C >> 3;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int c8 = l32 + 32 * j;
        if (live && c8 < c8n) {
            load8<F16>(x, in_dt, row * C + c8 * 8, v[j]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[j][e] = 0.0f;
        }
    }
    // The mean is pivot + sum(x - pivot) / C with the row's first element as the pivot: the fp32 sum of the raw values carries a
    // rounding error of the order of |mean|, which rstd then multiplies (a constant row came out as beta + 1e-2)
    const float piv = __shfl(v[0][0], 0, 32);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        if (l32 + 32 * j < c8n) {
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[j][e] - piv;
        }
    }
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) s += __shfl_xor(s, off, 32);
    const float mean = piv + s / (float)C;
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        if (l32 + 32 * j < c8n) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[j][e] - mean; q += d * d; }
        }
    }
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) q += __shfl_xor(q, off, 32);
    const float rstd = 1.0f / sqrtf(q / (float)C + eps);
    if (!live) return;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int c8 = l32 + 32 * j;
        if (c8 < c8n) {
            const int c = c8 * 8;
            float g[8], bb[8], y[8];
            load8<false>(reinterpret_cast<const char*>(gamma), MF_F32, c, g);
            load8<false>(reinterpret_cast<const char*>(beta), MF_F32, c, bb);
#pragma unroll
            for (int e = 0; e < 8; ++e) y[e] = (v[j][e] - mean) * rstd * g[e] + bb[e];
            store8<F16>(out, out_dt, row * C + c, y);
        }
    }
}

// One wave per row, up to 8 x 256 channels.
template <bool F16>
__global__ __launch_bounds__(256) void layernorm_kernel(const char* x, int in_dt, char* out, int out_dt,
                                                        const float* gamma, const float* beta, int64_t rows, int C,
                                                        float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    constexpr int MAXV = 8;
    float4 v[MAXV];
    const int c4n = C >> 2;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int c4 = lane + 64 * j;
        v[j] = c4 < c4n ? load4<F16>(x, in_dt, row * C + c4 * 4) : make_float4(0, 0, 0, 0);
    }
    const float piv = __shfl(v[0].x, 0, 64);             // (the mean as pivot + sum(x - pivot) / C: see layernorm8_kernel)
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        if (lane + 64 * j < c4n) s += ((v[j].x - piv) + (v[j].y - piv)) + ((v[j].z - piv) + (v[j].w - piv));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    const float mean = piv + s / (float)C;
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int c4 = lane + 64 * j;
        if (c4 < c4n) {
            const float dx = v[j].x - mean, dy = v[j].y - mean, dz = v[j].z - mean, dw = v[j].w - mean;
            q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
    const float rstd = 1.0f / sqrtf(q / (float)C + eps);
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int c4 = lane + 64 * j;
        if (c4 < c4n) {
            const int c = c4 * 4;
            const float4 g = *reinterpret_cast<const float4*>(gamma + c);
            const float4 bb = *reinterpret_cast<const float4*>(beta + c);
            float4 y;
            y.x = (v[j].x - mean) * rstd * g.x + bb.x;
            y.y = (v[j].y - mean) * rstd * g.y + bb.y;
            y.z = (v[j].z - mean) * rstd * g.z + bb.z;
            y.w = (v[j].w - mean) * rstd * g.w + bb.w;
            store4<F16>(out, out_dt, row * C + c, y);
        }
    }
}

// One wave per row: max, sum(exp), normalise; pad columns [cols, ld) are zeroed.
// CAUSAL (sq > 0): row r is query r % sq and keeps columns 0 .. r % sq; the rest of the row is written as 0 like the pad.
template <bool CAUSAL>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* s, char* out, int out_dt, int64_t rows,
                                                           int cols, int ld, int sq) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* r = s + row * ld;
    if constexpr (CAUSAL) {
        const int keep = (int)(row % sq) + 1;
        if (keep < cols) cols = keep;
    }
    float mx = -INFINITY;
    for (int c = lane; c < cols; c += 64) mx = fmaxf(mx, r[c]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    float sum = 0.0f;
    for (int c = lane; c < cols; c += 64) sum += expf(r[c] - mx);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    const float inv = 1.0f / sum;
    for (int c = lane; c < ld; c += 64) {
        const float pv = c < cols ? expf(r[c] - mx) * inv : 0.0f;
        store_from_f32(out, out_dt, row * ld + c, pv);
    }
}

// ---- dispatch of the dtype-templated GroupNorm kernels: every (in, out) storage pair mf_groupnorm accepts — all pairs of
// {fp32, bf16, fp16} except fp16 mixed with bf16.  A pair outside the table is an error of the call, never another pair's kernel.
template <int V> struct gn_int { static constexpr int value = V; };

template <typename F>
bool gn_for_dtypes(int in_dt, int out_dt, F&& f) {
#define MF_GN_PAIR(I_, O_) if (in_dt == I_ && out_dt == O_) { f(gn_int<I_>{}, gn_int<O_>{}); return true; }
    MF_GN_PAIR(MF_BF16, MF_BF16) MF_GN_PAIR(MF_F16, MF_F16) MF_GN_PAIR(MF_F32, MF_F32)
    MF_GN_PAIR(MF_F32, MF_BF16) MF_GN_PAIR(MF_F32, MF_F16) MF_GN_PAIR(MF_BF16, MF_F32) MF_GN_PAIR(MF_F16, MF_F32)
#undef MF_GN_PAIR
    return false;
}

// The one-launch slab form of mf_groupnorm, shape half: 8-channel vectors, slabs of sc = lcm(cpg, 8) channels x P rows of an image of at
// most 4 P rows, at most 1024 threads and 64 KB of LDS per block.  (The alignment half is gn_plan's.)
struct GnSlab { int sc, nv, P, nthr; size_t smem; };
bool gn_slab_shape(int hw, int c0, int c1, int groups, GnSlab* sl) {
    const int C = c0 + c1;
    if (hw < 1 || groups <= 0 || C % groups || c0 % 8 || c1 % 8) return false;
    const int cpg = C / groups;
    sl->sc = cpg;                                    // lcm(cpg, 8)
    while (sl->sc % 8) sl->sc += cpg;
    sl->nv = sl->sc / 8;
    sl->P = hw < 64 ? hw : 64;     // (rows = 4; 32x32 with P 128, 8 rows, 128 blocks measured no faster: 17.3 vs 17.6 us)
    sl->nthr = (sl->nv * sl->P + 63) / 64 * 64;
    sl->smem = (size_t)sl->P * sl->sc * sizeof(float2);
    return hw <= sl->P * 4 && C % sl->sc == 0 && sl->sc / cpg <= 8 && sl->nthr <= 1024 && sl->smem <= 64 * 1024;
}

// ---- plan, then launch: gn_plan makes every check and every decision of a call on the host (no HIP runtime call; of the descriptor's
// pointers only null-ness and 16-byte alignment count), gn_launch issues what the plan says.  mf_groupnorm is one after the other.
enum GnForm { kGnSlab = 0, kGnOwnStats = 1, kGnChannelSums = 2, kGnGroupSums = 3 };      // mf_gn_plan::form

struct GnPlan {
    GnArgs a;                 // what the kernels take
    mf_gn_plan r;             // the decisions, as mf_groupnorm_plan reports them: gn_launch reads grids, blocks and LDS sizes from here
    GnSlab sl;                // kGnSlab: the geometry of a slab
    int batch, slices, gps;   // kGnChannelSums: slices of the groups per image and groups per slice of the finalize launch
};

int gn_plan(const mf_groupnorm_desc* d, GnPlan* plan) {
    MF_CHECK_ARG(d && d->x0 && d->out && d->gamma && d->beta && d->ws, "mf_groupnorm: null pointer");
    MF_CHECK_ARG((d->x1 != nullptr) == (d->c1 > 0) && d->c0 > 0, "mf_groupnorm: bad segments");
    const int C = d->c0 + d->c1;
    MF_CHECK_ARG(d->groups > 0 && C % d->groups == 0, "mf_groupnorm: C=%d not divisible by groups=%d", C, d->groups);
    MF_CHECK_ARG(d->c0 % 4 == 0 && d->c1 % 4 == 0, "mf_groupnorm: channel counts must be multiples of 4");
    MF_CHECK_ARG(d->batch >= 1 && d->hw >= 1, "mf_groupnorm: bad batch/hw");
    MF_CHECK_ARG(!(mf_any_f16(d->in_dtype, d->out_dtype) && mf_any_bf16(d->in_dtype, d->out_dtype)), "mf_groupnorm: fp16 and bf16 operands in one launch");
    MF_CHECK_ARG(d->groups <= 64, "mf_groupnorm: at most 64 groups");
    *plan = GnPlan{};
    plan->batch = d->batch;
    GnArgs& a = plan->a;
    a.x0 = (const char*)d->x0; a.x1 = (const char*)d->x1;
    a.C0 = d->c0; a.C1 = d->c1; a.C = C; a.in_dt = d->in_dtype; a.HW = d->hw; a.G = d->groups;
    a.cpg = C / d->groups;
    a.eps = d->eps; a.gamma = d->gamma; a.beta = d->beta; a.silu = d->silu;
    a.out = (char*)d->out; a.out_dt = d->out_dtype; a.ws = d->ws; a.stats_out = d->stats_out;
    a.ws_ab = d->ws + (int64_t)d->batch * d->groups * GN_MAX_CHUNKS * 2;
    const bool affine16 = mf_aligned16(d->gamma) && mf_aligned16(d->beta);
    const bool known = gn_for_dtypes(d->in_dtype, d->out_dtype, [](auto, auto) {});
    // The one-launch slab kernel for the low-resolution levels.  Measured against the two-launch form (tools/bench_gn.py, batch 8, us):
    // 8x8 C 1280: 11.7 -> 5.0, 2560: 13.0 -> 6.0; 16x16 C 1280: 12.8 -> 8.1, 2560: 17.4 -> 9.8
    const GnSlab& sl = plan->sl;
    const bool slab_ok = gn_slab_shape(d->hw, d->c0, d->c1, d->groups, &plan->sl) && affine16 && mf_aligned16(d->x0) && mf_aligned16(d->out) && (!d->x1 || mf_aligned16(d->x1));
    if (d->sk_ws) {
        MF_CHECK_ARG(slab_ok && d->c1 == 0 && d->sk_splits >= 2 && d->stats_out == nullptr && mf_aligned16(d->sk_ws) &&
                         (!d->sk_bias || mf_aligned16(d->sk_bias)) && (!d->sk_temb || (mf_aligned16(d->sk_temb) && d->sk_ld_temb % 4 == 0)),
                     "mf_groupnorm: a deferred split-K input (sk_ws) needs the one-launch form (hw <= 256, channels %% 8 == 0, one segment), "
                     ">= 2 slabs, 16-byte aligned slabs / bias / temb and no stats_out");
        a.sk_ws = d->sk_ws; a.sk_splits = d->sk_splits; a.sk_bias = d->sk_bias; a.sk_temb = d->sk_temb; a.sk_ld_temb = d->sk_ld_temb;
        a.sk_alpha = d->sk_alpha; a.sk_mn = (int64_t)d->batch * d->hw * C;
    }
    if (slab_ok) {
        MF_CHECK_ARG(known, "mf_groupnorm: no kernel for in_dtype %d with out_dtype %d", d->in_dtype, d->out_dtype);
        plan->r = mf_gn_plan{kGnSlab, 1, 8, 0, 0, 0, 0, sl.P, C / sl.sc * d->batch, sl.nthr, (int32_t)sl.smem, 0};
        return MF_OK;
    }
    // The streaming forms.  Statistics from the producers' per-channel sums: every present segment has them and their row blocks divide
    // the image (at most 128 per image: the finalize launch walks them serially per channel).  From the producer's per-GROUP sums: no
    // statistics pass and no finalize launch — every apply block combines its image's row blocks.  Else a pass of its own.
    const bool from_parts = d->part0 != nullptr && d->part0_rows > 0 && d->hw % d->part0_rows == 0 && d->hw / d->part0_rows <= 128 &&
                            (d->c1 == 0 || (d->part1 != nullptr && d->part1_rows > 0 && d->hw % d->part1_rows == 0 && d->hw / d->part1_rows <= 128));
    const bool from_groups = d->grp0 != nullptr && d->c1 == 0 && d->grp0_rows > 0 && d->hw % d->grp0_rows == 0 && d->hw / d->grp0_rows <= 64 && affine16;
    const int form = from_groups ? kGnGroupSums : from_parts ? kGnChannelSums : kGnOwnStats;
    a.part0 = (const float2*)d->part0; a.part1 = (const float2*)d->part1; a.pr0 = d->part0_rows; a.pr1 = d->part1_rows;
    if (from_groups) { a.grp0 = (const float2*)d->grp0; a.nch0 = d->hw / d->grp0_rows; }
    a.rows_per_chunk = d->hw > 16 * GN_MAX_CHUNKS ? (d->hw + GN_MAX_CHUNKS - 1) / GN_MAX_CHUNKS : 16;
    a.nchunks = (d->hw + a.rows_per_chunk - 1) / a.rows_per_chunk;
    // Who turns the statistics into (mean, rstd): every apply block (1: the chunks of the own pass; 2: the producer's group sums) or a
    // finalize launch (0).  Measured (tools/bench_gn.py): -1.5...2 us per GroupNorm up to 32x32, +1 us at 64x64 (64 chunks combined by 256
    // blocks; round 3: fetching a thread's first rows AHEAD of the combine was neutral there, 26.3 vs 25.6 us, and removed).
    a.fuse_finalize = from_groups ? 2 : !from_parts && d->hw <= 1024 && affine16 ? 1 : 0;
    a.centered = d->out_dtype == MF_F32 && a.nchunks >= 2 && affine16;
    const int vw = (d->c0 % 8 == 0 && d->c1 % 8 == 0) ? 8 : 4;
    a.cvn = C / vw;
    a.tpr = a.cvn < GN_BLK ? a.cvn : GN_BLK;
    a.rif = GN_BLK / a.tpr;
    const int nthr = (a.tpr * a.rif + 63) / 64 * 64;
    const size_t smem1 = (size_t)a.rif * C * sizeof(float2);      // the statistics pass's [rif][C] sums
    MF_CHECK_ARG(smem1 <= 64 * 1024, "mf_groupnorm: C=%d too large", C);
    // the apply pass: GN_TARGET_BLOCKS row blocks in all, at least 4 rows per thread
    const int rows_even = (int)(((int64_t)d->hw * d->batch + GN_TARGET_BLOCKS - 1) / GN_TARGET_BLOCKS);
    const int rows_per_block = rows_even < 4 * a.rif ? 4 * a.rif : rows_even;
    const int nblk = (d->hw + rows_per_block - 1) / rows_per_block;
    int kparts = 0;
    if (form == kGnChannelSums) {
        // finalize from partial sums: 8 slices of the groups per image, and as many threads per channel as the block has room for
        plan->slices = d->groups >= 32 ? 8 : 1;
        plan->gps = (d->groups + plan->slices - 1) / plan->slices;
        kparts = GN_BLK / (plan->gps * a.cpg);
        const int nb0 = d->hw / d->part0_rows, nb1 = d->c1 ? d->hw / d->part1_rows : nb0, nbmin = nb0 < nb1 ? nb0 : nb1;
        kparts = kparts > nbmin ? nbmin : kparts < 1 ? 1 : kparts;
        while ((size_t)kparts * plan->gps * a.cpg * sizeof(double2) > 48 * 1024 && kparts > 1) --kparts;
    }
    MF_CHECK_ARG(known, "mf_groupnorm: no kernel for in_dtype %d with out_dtype %d", d->in_dtype, d->out_dtype);
    const size_t smem = form == kGnOwnStats ? smem1 : (size_t)kparts * plan->gps * a.cpg * sizeof(double2);      // (group sums: 0)
    plan->r = mf_gn_plan{form, from_groups ? 1 : from_parts || a.fuse_finalize ? 2 : 3, vw, a.fuse_finalize, a.centered, a.nchunks,
                         a.rows_per_chunk, rows_per_block, nblk * d->batch, nthr, (int32_t)smem, kparts};
    return MF_OK;
}

template <int I, int O, int VW>
auto* gn_apply_for(bool silu, bool seg2) {
    return silu ? (seg2 ? gn_apply_kernel<I, O, VW, true, true> : gn_apply_kernel<I, O, VW, true, false>)
                : (seg2 ? gn_apply_kernel<I, O, VW, false, true> : gn_apply_kernel<I, O, VW, false, false>);
}

int gn_launch(const GnPlan& p, hipStream_t s) {
    const GnArgs& a = p.a;
    const mf_gn_plan& r = p.r;
    gn_for_dtypes(a.in_dt, a.out_dt, [&](auto in_c, auto out_c) {        // (gn_plan refused a pair without kernels)
        constexpr int I = decltype(in_c)::value, O = decltype(out_c)::value;
        if (r.form == kGnSlab) {
            auto* kern = a.sk_ws ? (a.silu ? gn_slab_kernel<I, O, true, true> : gn_slab_kernel<I, O, false, true>)
                                 : (a.silu ? gn_slab_kernel<I, O, true, false> : gn_slab_kernel<I, O, false, false>);
            hipLaunchKernelGGL(kern, dim3(a.C / p.sl.sc, p.batch), dim3(r.threads), r.lds_bytes, s, a, p.sl.sc, p.sl.nv, p.sl.P);
            return;
        }
        if (r.form == kGnChannelSums) {
            hipLaunchKernelGGL(gn_finalize_part_kernel, dim3(p.batch, p.slices), dim3(GN_BLK), r.lds_bytes, s, a, p.gps, r.finalize_parts);
        } else if (r.form == kGnOwnStats) {
            auto* stats = r.vec == 8 ? gn_stats_kernel<I, 8> : gn_stats_kernel<I, 4>;
            hipLaunchKernelGGL(stats, dim3(a.nchunks, p.batch), dim3(r.threads), r.lds_bytes, s, a);
            if (!a.fuse_finalize) hipLaunchKernelGGL(gn_finalize_kernel, dim3(p.batch), dim3(GN_BLK), 0, s, a);
        }
        auto* apply = r.vec == 8 ? gn_apply_for<I, O, 8>(a.silu, a.C1) : gn_apply_for<I, O, 4>(a.silu, a.C1);
        hipLaunchKernelGGL(apply, dim3(r.blocks / p.batch, p.batch), dim3(r.threads), 0, s, a, r.rows_per_block);
    });
    MF_CHECK_LAUNCH(r.form == kGnSlab ? "mf_groupnorm(slab)" : "mf_groupnorm(apply)");
    return MF_OK;
}

}  // namespace

extern "C" int mf_groupnorm_slab_applies(int32_t hw, int32_t channels, int32_t groups) {
    GnSlab sl;
    return gn_slab_shape(hw, channels, 0, groups, &sl) ? 1 : 0;
}

extern "C" int64_t mf_groupnorm_ws_floats(int32_t batch, int32_t groups, int32_t channels) {
    return (int64_t)batch * groups * GN_MAX_CHUNKS * 2 + (int64_t)batch * channels * 2;
}

extern "C" int mf_groupnorm(const mf_groupnorm_desc* d, void* stream) {
    GnPlan plan;
    const int rc = gn_plan(d, &plan);
    return rc != MF_OK ? rc : gn_launch(plan, (hipStream_t)stream);
}

extern "C" int mf_sizeof_gn_plan(void) { return (int)sizeof(mf_gn_plan); }
extern "C" int mf_groupnorm_plan(const mf_groupnorm_desc* d, mf_gn_plan* out) {
    MF_CHECK_ARG(out != nullptr, "mf_groupnorm_plan: null plan");
    GnPlan p;
    const int rc = gn_plan(d, &p);
    if (rc == MF_OK) *out = p.r;
    return rc;
}

extern "C" int mf_layernorm(const void* x, int32_t in_dtype, void* out, int32_t out_dtype, const float* gamma,
                            const float* beta, int64_t rows, int32_t c, float eps, void* stream) {
    MF_CHECK_ARG(x && out && gamma && beta, "mf_layernorm: null pointer");
    MF_CHECK_ARG(c % 4 == 0 && c >= 4 && c <= 2048, "mf_layernorm: C=%d must be a multiple of 4 and <= 2048", c);
    if (rows <= 0) return MF_OK;
    MF_CHECK_ARG(!(mf_any_f16(in_dtype, out_dtype) && mf_any_bf16(in_dtype, out_dtype)), "mf_layernorm: fp16 and bf16 operands in one launch");
    const bool f16 = mf_any_f16(in_dtype, out_dtype);
    const bool v8 = c % 8 == 0 && mf_aligned16(x) && mf_aligned16(out) && mf_aligned16(gamma) && mf_aligned16(beta);
    const dim3 grid((unsigned)(v8 ? (rows + 7) / 8 : (rows + 3) / 4));
    auto* kern = v8 ? (f16 ? layernorm8_kernel<true> : layernorm8_kernel<false>) : (f16 ? layernorm_kernel<true> : layernorm_kernel<false>);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, (const char*)x, in_dtype, (char*)out, out_dtype, gamma, beta, rows, c, eps);
    MF_CHECK_LAUNCH("mf_layernorm");
    return MF_OK;
}

extern "C" int mf_softmax_rows(const float* scores, void* out, int32_t out_dtype, int64_t rows, int32_t cols,
                               int32_t ld, void* stream) {
    MF_CHECK_ARG(scores && out && cols >= 1 && ld >= cols, "mf_softmax_rows: bad arguments");
    if (rows <= 0) return MF_OK;
    hipLaunchKernelGGL(softmax_rows_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       scores, (char*)out, out_dtype, rows, cols, ld, 0);
    MF_CHECK_LAUNCH("mf_softmax_rows");
    return MF_OK;
}

extern "C" int mf_softmax_rows_causal(const float* scores, void* out, int32_t out_dtype, int64_t rows, int32_t cols,
                                      int32_t ld, int32_t sq, void* stream) {
    MF_CHECK_ARG(scores && out && cols >= 1 && ld >= cols, "mf_softmax_rows_causal: bad arguments");
    MF_CHECK_ARG(sq >= 1 && sq == cols && rows % sq == 0, "mf_softmax_rows_causal: the causal mask needs sq == cols and rows %% sq == 0");
    if (rows <= 0) return MF_OK;
    hipLaunchKernelGGL(softmax_rows_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       scores, (char*)out, out_dtype, rows, cols, ld, sq);
    MF_CHECK_LAUNCH("mf_softmax_rows_causal");
    return MF_OK;
}
