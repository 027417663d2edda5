// LoRA merge on the device (models/lora.py:324,410 `_fuse_lora`: W + scale * alpha / rank * mm(up.flatten(1), down.flatten(1))), for a
// whole TABLE of weights in one launch:
//   out_t[i][k] = base_t[i][k] + sum over the target's terms of coef[term] * ( sum_{j < rank} up[i][j] * down[j][k] )
// base / out are the reference's own row-major fp32 weights ([rows][cols], cols = Cin * kh * kw), so a conv LoRA needs no layout
// knowledge.  Arithmetic contract (mfhip.h): every output element is computed by exactly one thread; per term s = 0, then
// s = fmaf(up[i][j], down[j][k], s) for ascending j; the element starts as base and takes fmaf(coef, s, element) per term in table
// order.  No atomics, nothing depends on the grid.
//
// The kernel is bandwidth-bound (8 bytes per weight element; 2 * rank flops per element stay under the fp32 vector rate up to rank 128),
// so a block owns a 32 x 256 tile of one target: 256 threads, a wave per 8 rows, a lane per 4 consecutive columns (16-byte loads and
// stores along cols; a target whose cols or addresses do not allow them takes scalar accesses with the same tile).  The rank loop runs
// in chunks of 16: the chunk's down rows [16][256] and up columns [32][16] are staged in LDS once per tile (18 KB), a lane keeps its
// 8 x 4 partial sums and the 8 x 4 up values of four j in registers, and reads down as one 16-byte LDS access per j (conflict-free:
// consecutive lanes, consecutive slots; the up reads are broadcasts).  The 32-row tile bounds the re-read of down from L2 to
// rank / 32 floats per element.
#include "mf_common.h"

namespace {

constexpr int LR_ROWS = 32, LR_COLS = 256, LR_RK = 16, LR_THREADS = 256;
constexpr int LR_RPW = LR_ROWS / (LR_THREADS / 64);       // rows per wave
constexpr int64_t LR_MAX_GRID = (int64_t)1 << 22;

__global__ __launch_bounds__(LR_THREADS) void lora_merge_kernel(const mf_lora_target* __restrict__ targets, const mf_lora_term* __restrict__ terms,
                                                                const float* __restrict__ coef, int ntargets, int64_t total_tiles) {
    __shared__ __align__(16) float down_s[LR_RK][LR_COLS];
    __shared__ __align__(16) float up_s[LR_ROWS][LR_RK];
    const int tid = threadIdx.x, cg = tid & 63, rg = tid >> 6;
    for (int64_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        int lo = 0, hi = ntargets - 1;                     // the last target whose first tile is <= tile (block-uniform)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (targets[mid].first_tile <= tile) lo = mid; else hi = mid - 1;
        }
        const mf_lora_target t = targets[lo];
        const int rows = t.rows, cols = t.cols;
        const int ct = (cols + LR_COLS - 1) / LR_COLS;
        const int64_t local = tile - t.first_tile;
        const int row0 = (int)(local / ct) * LR_ROWS, col0 = (int)(local % ct) * LR_COLS;
        const bool vec = (cols & 3) == 0 && ((((uintptr_t)t.base) | ((uintptr_t)t.out)) & 15) == 0;
        const int c = col0 + cg * 4;                       // this lane's first column
        const int r0 = row0 + rg * LR_RPW;                 // this wave's first row
        const bool wave_live = r0 < rows;

        float acc[LR_RPW][4];
#pragma unroll
        for (int i = 0; i < LR_RPW; ++i) {
            acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0f;
            const int r = r0 + i;
            if (r < rows && c < cols) {
                const float* p = t.base + (int64_t)r * cols + c;
                if (vec) {
                    const float4 v = *reinterpret_cast<const float4*>(p);
                    acc[i][0] = v.x; acc[i][1] = v.y; acc[i][2] = v.z; acc[i][3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < cols) acc[i][e] = p[e];
                }
            }
        }

        for (int ti = 0; ti < t.nterms; ++ti) {
            const mf_lora_term tm = terms[t.first_term + ti];
            const float cf = coef[t.first_term + ti];
            const int rank = tm.rank;
            const bool dvec = (cols & 3) == 0 && (((uintptr_t)tm.down) & 15) == 0;
            float s[LR_RPW][4];
#pragma unroll
            for (int i = 0; i < LR_RPW; ++i) s[i][0] = s[i][1] = s[i][2] = s[i][3] = 0.0f;

            for (int k0 = 0; k0 < rank; k0 += LR_RK) {
                const int jn = min(LR_RK, rank - k0);
                __syncthreads();                           // the previous chunk (or tile) has been read
                // down rows k0 .. k0 + 15, columns col0 .. col0 + 255: four 16-byte pieces per thread, zeros past the rank / the matrix
#pragma unroll
                for (int q = 0; q < LR_RK * LR_COLS / 4 / LR_THREADS; ++q) {
                    const int jj = q * (LR_THREADS / 64) + rg;
                    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (jj < jn && c < cols) {
                        const float* p = tm.down + (int64_t)(k0 + jj) * cols + c;
                        if (dvec) {
                            v = *reinterpret_cast<const float4*>(p);
                        } else {
                            v.x = p[0];
                            if (c + 1 < cols) v.y = p[1];
                            if (c + 2 < cols) v.z = p[2];
                            if (c + 3 < cols) v.w = p[3];
                        }
                    }
                    *reinterpret_cast<float4*>(&down_s[jj][cg * 4]) = v;
                }
                // up rows row0 .. row0 + 31, columns k0 .. k0 + 15: two floats per thread, consecutive lanes along j
#pragma unroll
                for (int q = 0; q < LR_ROWS * LR_RK / LR_THREADS; ++q) {
                    const int idx = q * LR_THREADS + tid, r = idx / LR_RK, jj = idx % LR_RK;
                    float v = 0.0f;
                    if (row0 + r < rows && jj < jn) v = tm.up[(int64_t)(row0 + r) * rank + k0 + jj];
                    up_s[r][jj] = v;
                }
                __syncthreads();
                if (wave_live) {
                    const int j4n = (jn + 3) >> 2;         // whole groups of four j: the padding is zeros on both sides
                    for (int j4 = 0; j4 < j4n; ++j4) {
                        float4 u[LR_RPW];
#pragma unroll
                        for (int i = 0; i < LR_RPW; ++i) u[i] = *reinterpret_cast<const float4*>(&up_s[rg * LR_RPW + i][j4 * 4]);
#pragma unroll
                        for (int jq = 0; jq < 4; ++jq) {
                            const float4 d = *reinterpret_cast<const float4*>(&down_s[j4 * 4 + jq][cg * 4]);
#pragma unroll
                            for (int i = 0; i < LR_RPW; ++i) {
                                const float uu = jq == 0 ? u[i].x : (jq == 1 ? u[i].y : (jq == 2 ? u[i].z : u[i].w));
                                s[i][0] = fmaf(uu, d.x, s[i][0]);
                                s[i][1] = fmaf(uu, d.y, s[i][1]);
                                s[i][2] = fmaf(uu, d.z, s[i][2]);
                                s[i][3] = fmaf(uu, d.w, s[i][3]);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < LR_RPW; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][e] = fmaf(cf, s[i][e], acc[i][e]);
        }

#pragma unroll
        for (int i = 0; i < LR_RPW; ++i) {
            const int r = r0 + i;
            if (r < rows && c < cols) {
                float* p = t.out + (int64_t)r * cols + c;
                if (vec) {
                    *reinterpret_cast<float4*>(p) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < cols) p[e] = acc[i][e];
                }
            }
        }
    }
}

inline int64_t tiles_of(int64_t rows, int64_t cols) { return ((rows + LR_ROWS - 1) / LR_ROWS) * ((cols + LR_COLS - 1) / LR_COLS); }

}  // namespace

extern "C" int mf_sizeof_lora_target(void) { return (int)sizeof(mf_lora_target); }
extern "C" int mf_sizeof_lora_term(void) { return (int)sizeof(mf_lora_term); }

extern "C" int64_t mf_lora_tiles(int32_t rows, int32_t cols) {
    if (rows < 1 || cols < 1) {
        mf_set_error("mf_lora_tiles: rows %d and cols %d must be at least 1", rows, cols);
        return -1;
    }
    return tiles_of(rows, cols);
}

extern "C" int mf_lora_merge(const mf_lora_target* targets, const mf_lora_term* terms, const mf_lora_target* targets_dev,
                             const mf_lora_term* terms_dev, const float* coef_dev, int32_t ntargets, int32_t nterms, void* stream) {
    MF_CHECK_ARG(targets && terms, "mf_lora_merge: null host table");
    MF_CHECK_ARG(targets_dev && terms_dev && coef_dev, "mf_lora_merge: null device table");
    MF_CHECK_ARG(ntargets >= 1 && nterms >= 1, "mf_lora_merge: %d targets and %d terms (at least 1 each)", ntargets, nterms);
    MF_CHECK_ARG((((uintptr_t)targets_dev | (uintptr_t)terms_dev) & 7) == 0 && ((uintptr_t)coef_dev & 3) == 0,
                 "mf_lora_merge: the device tables must be 8-byte, coef 4-byte aligned");
    int64_t tiles = 0;
    int32_t next_term = 0;
    for (int32_t i = 0; i < ntargets; ++i) {
        const mf_lora_target& t = targets[i];
        MF_CHECK_ARG(t.base && t.out, "mf_lora_merge: target %d: null base or out", i);
        MF_CHECK_ARG(t.rows >= 1 && t.cols >= 1, "mf_lora_merge: target %d: rows %d and cols %d must be at least 1", i, t.rows, t.cols);
        MF_CHECK_ARG((((uintptr_t)t.base | (uintptr_t)t.out) & 3) == 0, "mf_lora_merge: target %d: base and out must be 4-byte aligned", i);
        const uintptr_t bytes = (uintptr_t)t.rows * (uintptr_t)t.cols * 4, b = (uintptr_t)t.base, o = (uintptr_t)t.out;
        MF_CHECK_ARG(o + bytes <= b || b + bytes <= o, "mf_lora_merge: target %d: out must not alias base (the base is kept, never subtracted back)", i);
        MF_CHECK_ARG(t.first_term == next_term && t.nterms >= 1 && (int64_t)t.first_term + t.nterms <= nterms,
                     "mf_lora_merge: target %d: terms [%d, %d + %d) are not the next run of the %d-term table", i, t.first_term, t.first_term,
                     t.nterms, nterms);
        MF_CHECK_ARG(t.first_tile == tiles, "mf_lora_merge: target %d: first_tile %lld is not the running sum of mf_lora_tiles (%lld)", i,
                     (long long)t.first_tile, (long long)tiles);
        for (int32_t k = t.first_term; k < t.first_term + t.nterms; ++k) {
            MF_CHECK_ARG(terms[k].up && terms[k].down, "mf_lora_merge: term %d (target %d): null up or down", k, i);
            MF_CHECK_ARG(terms[k].rank >= 1, "mf_lora_merge: term %d (target %d): rank %d must be at least 1", k, i, terms[k].rank);
            MF_CHECK_ARG((((uintptr_t)terms[k].up | (uintptr_t)terms[k].down) & 3) == 0,
                         "mf_lora_merge: term %d (target %d): up and down must be 4-byte aligned", k, i);
        }
        next_term += t.nterms;
        tiles += tiles_of(t.rows, t.cols);
    }
    MF_CHECK_ARG(next_term == nterms, "mf_lora_merge: the targets use %d of the %d terms", next_term, nterms);
    const int64_t grid = tiles < LR_MAX_GRID ? tiles : LR_MAX_GRID;
    hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)grid), dim3(LR_THREADS), 0, (hipStream_t)stream, targets_dev, terms_dev, coef_dev,
                       (int)ntargets, tiles);
    MF_CHECK_LAUNCH("mf_lora_merge");
    return 0;
}
