// Image scoring on the device: what the reference's evaluation side computes with torchmetrics on fp32 copies of the images
// (metrics/metrics.py:51-67 compute_metrics, :108-165 MetricsCalculator.compute_metric; train_brushnet_mirror.py:224-250).
//   peak_signal_noise_ratio (defaults)              10 log10(range(target)^2 / mean (pred - target)^2)
//   structural_similarity_index_measure (defaults)  11 x 11 Gaussian window, sigma 1.5, mean over the (H - 10)(W - 10) C valid positions
//   the "mask" / "mirror" regions                   (dataset.py:62-68: pixels with mask == 255 / mask == 0 blacked out in both images)
// The images are uint8 NHWC in device memory (what mf_postprocess / mf_decode_image leave there); every image of a batch is scored on its
// own.  The device writes one mf_metrics_row per image: integers for everything that is exact (the squared-error sum, the extrema after
// the region step), a float64 sum of the per-position SSIM values; PSNR and the SSIM mean are two float64 divisions the caller finishes.
// Two passes over the bytes at most: the statistics (c1 / c2 of SSIM come from the data) and the SSIM tiles; with a given data_range the
// statistics ride in the tile pass.  A tile is staged as bytes in LDS with its 10-pixel halo, the region applied while loading, and
// the separable 11-tap filter runs on the five moment maps out of LDS: no moment map ever reaches global memory.  Reductions are per-block
// partials summed in a fixed order by one block per image: no floating-point atomics, the same inputs give the same bits on every run.
#include <math.h>
#include "mf_common.h"

namespace {

constexpr int MT = 32;                   // output positions per tile edge
constexpr int MI = MT + 10;              // input pixels per tile edge (the window reaches 10 pixels further)
constexpr int MROW = MI * 4 + 4;         // LDS bytes of a staged image row: 4 channels, up to 3 bytes of alignment phase, whole dwords
constexpr int MMROW = (MI + 3 + 3) / 4 * 4;   // the same for a mask row
constexpr int MSTAT_BLOCKS = 128;        // stage-1 blocks per image of the stand-alone statistics pass

struct StatPart { unsigned long long sq; int pmin, pmax, tmin, tmax; };
struct Taps { float w[11]; };

__device__ __forceinline__ bool region_zero(int region, unsigned m) { return region == 1 ? m == 255u : (region == 2 ? m == 0u : false); }

// bytes [j0, j0 + 4) of src[0 .. len), little-endian in one word, zero outside the range.  One dword read when all four lie inside AND
// their address is dword aligned, byte reads otherwise: every global read is at its natural alignment (an RGB row is 3 W bytes, in
// general not a multiple of 4) and none leaves the range.
__device__ __forceinline__ unsigned load4(const unsigned char* src, int64_t j0, int64_t len) {
    if (j0 >= 0 && j0 + 4 <= len && (((uintptr_t)(src + j0)) & 3) == 0) return *reinterpret_cast<const unsigned*>(src + j0);
    unsigned v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t j = j0 + i;
        if (j >= 0 && j < len) v |= (unsigned)src[j] << (8 * i);
    }
    return v;
}

struct Stat {
    unsigned long long sq = 0;
    int pmin = 255, pmax = 0, tmin = 255, tmax = 0;
    __device__ __forceinline__ void add(int p, int t) {
        const int d = p - t;
        sq += (unsigned)(d * d);
        pmin = min(pmin, p); pmax = max(pmax, p); tmin = min(tmin, t); tmax = max(tmax, t);
    }
    __device__ __forceinline__ void merge(const StatPart& o) {
        sq += o.sq;
        pmin = min(pmin, o.pmin); pmax = max(pmax, o.pmax); tmin = min(tmin, o.tmin); tmax = max(tmax, o.tmax);
    }
};

// the block's 256 Stats folded by a fixed tree; the result is valid in thread 0
__device__ __forceinline__ StatPart block_reduce_stat(const Stat& s) {
    __shared__ StatPart red[256];
    const int t = threadIdx.x;
    red[t] = StatPart{s.sq, s.pmin, s.pmax, s.tmin, s.tmax};
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            const StatPart o = red[t + w];
            StatPart& a = red[t];
            a.sq += o.sq;
            a.pmin = min(a.pmin, o.pmin); a.pmax = max(a.pmax, o.pmax); a.tmin = min(a.tmin, o.tmin); a.tmax = max(a.tmax, o.tmax);
        }
        __syncthreads();
    }
    const StatPart r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double block_reduce_sum(double v) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// ---- pass 1 (only when the data range comes from the data): squared error and extrema of image blockIdx.y, per-block partials --------
template <int C>
__global__ __launch_bounds__(256) void metrics_stats_kernel(const unsigned char* pred, const unsigned char* target, const unsigned char* mask,
                                                            int region, int64_t pixels, StatPart* part) {
    const int b = blockIdx.y;
    const int64_t n = pixels * C;
    const unsigned char* pb = pred + b * n;
    const unsigned char* tb = target + b * n;
    const unsigned char* mb = mask ? mask + b * pixels : nullptr;
    const int phase = (int)(((uintptr_t)pb) & 3);            // groups are the aligned dwords of pred (and of target when it is laid out alike)
    const int64_t groups = (n + phase + 3) / 4;
    Stat s;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < groups; k += (int64_t)gridDim.x * 256) {
        const int64_t j0 = 4 * k - phase;
        const unsigned vp = load4(pb, j0, n), vt = load4(tb, j0, n);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t j = j0 + i;
            if (j < 0 || j >= n) continue;
            int p = (vp >> (8 * i)) & 255, t = (vt >> (8 * i)) & 255;
            if (region && region_zero(region, mb[j / C])) p = t = 0;
            s.add(p, t);
        }
    }
    const StatPart r = block_reduce_stat(s);
    if (threadIdx.x == 0) part[(int64_t)b * gridDim.x + blockIdx.x] = r;
}

// ---- pass 2: one 32 x 32 tile of SSIM positions of image blockIdx.z, all channels --------------------------------------------------------
// LDS: the (32 + 10)^2 pixels of both images as bytes (a row keeps its global dword phase, so aligned dwords land on aligned dwords), the
// mask tile, and the five horizontally filtered moment maps of ONE channel (42 rows x 32 columns fp32).
// The moments are taken of (byte - ref), ref = the rounded mean of the tile's bytes of that channel over both images (an integer: the
// subtraction is exact).  Variances and the covariance do not move with ref and the means get it back, but E[x^2] - E[x]^2 no longer
// cancels two numbers of the order 255^2: on a flat area plain fp32 moments leave a variance of either sign of ~1e-2, which the
// max(., 0) of the definition turns into a bias of 1e-4 in s.
template <int C, bool RIDE>
__global__ __launch_bounds__(256) void metrics_ssim_kernel(const unsigned char* pred, const unsigned char* target, const unsigned char* mask,
                                                           int region, int h, int w, Taps taps, float data_range, const float* c12,
                                                           double* ssim_part, StatPart* stat_part) {
    __shared__ __attribute__((aligned(16))) unsigned char sp[MI][MROW];
    __shared__ __attribute__((aligned(16))) unsigned char st[MI][MROW];
    __shared__ __attribute__((aligned(16))) unsigned char sm[MI][MMROW];
    __shared__ float hm[5][MI][MT];
    const int tid = threadIdx.x;
    const int b = blockIdx.z, x0 = blockIdx.x * MT, y0 = blockIdx.y * MT;
    const int cols = min(MI, w - x0), rows = min(MI, h - y0);          // input pixels this tile has (>= 11 each)
    const int64_t img = (int64_t)b * h * w;
    auto pix = [&](int ly) { return img + (int64_t)(y0 + ly) * w + x0; };          // pixel index of the tile row's first pixel
    auto phase_of = [](const unsigned char* p) { return (int)(((uintptr_t)p) & 3); };
    __shared__ int php[MI], pht[MI];                                              // LDS byte offset of each staged row's first pixel
    if (tid < MI) {
        php[tid] = tid < rows ? phase_of(pred + pix(tid) * C) : 0;
        pht[tid] = tid < rows ? phase_of(target + pix(tid) * C) : 0;
    }

    if (region) {
        for (int item = tid; item < MI * (MMROW / 4); item += 256) {
            const int ly = item / (MMROW / 4), k = item - ly * (MMROW / 4);
            unsigned v = 0;
            if (ly < rows) {
                const unsigned char* src = mask + pix(ly);
                v = load4(src, 4 * k - phase_of(src), cols);
            }
            *reinterpret_cast<unsigned*>(&sm[ly][4 * k]) = v;
        }
        __syncthreads();
    }
    for (int item = tid; item < MI * (MROW / 4); item += 256) {
        const int ly = item / (MROW / 4), k = item - ly * (MROW / 4);
        unsigned vp = 0, vt = 0;
        if (ly < rows) {
            const int len = cols * C;
            const unsigned char* ps = pred + pix(ly) * C;
            const unsigned char* ts = target + pix(ly) * C;
            const int jp = 4 * k - phase_of(ps), jt = 4 * k - phase_of(ts);
            vp = load4(ps, jp, len);
            vt = load4(ts, jt, len);
            if (region) {
                const unsigned char* mrow = &sm[ly][phase_of(mask + pix(ly))];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (jp + i >= 0 && jp + i < len && region_zero(region, mrow[(jp + i) / C])) vp &= ~(0xffu << (8 * i));
                    if (jt + i >= 0 && jt + i < len && region_zero(region, mrow[(jt + i) / C])) vt &= ~(0xffu << (8 * i));
                }
            }
        }
        *reinterpret_cast<unsigned*>(&sp[ly][4 * k]) = vp;
        *reinterpret_cast<unsigned*>(&st[ly][4 * k]) = vt;
    }
    __syncthreads();

    if constexpr (RIDE) {
        // every pixel of the image belongs to exactly one tile: its first 32 rows / columns, and the halo too on the last tile of an axis
        const int own_rows = blockIdx.y == gridDim.y - 1 ? rows : MT, own_bytes = (blockIdx.x == gridDim.x - 1 ? cols : MT) * C;
        Stat s;
        for (int item = tid; item < own_rows * own_bytes; item += 256) {
            const int ly = item / own_bytes, j = item - ly * own_bytes;
            s.add(sp[ly][php[ly] + j], st[ly][pht[ly] + j]);
        }
        const StatPart r = block_reduce_stat(s);
        if (tid == 0) stat_part[((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = r;
    }

    float c1, c2;
    if (data_range > 0.0f) {
        const double k1 = 0.01 * (double)data_range, k2 = 0.03 * (double)data_range;
        c1 = (float)(k1 * k1); c2 = (float)(k2 * k2);
    } else {
        c1 = c12[2 * b]; c2 = c12[2 * b + 1];
    }
    const int ox = tid & (MT - 1), oy0 = (tid >> 5) * 4;       // vertical pass: one column, four consecutive output rows per thread
    double acc = 0.0;
    for (int c = 0; c < C; ++c) {
        int bsum = 0;
        for (int item = tid; item < rows * cols; item += 256) {
            const int ly = item / cols, lx = item - ly * cols;
            bsum += sp[ly][php[ly] + lx * C + c] + st[ly][pht[ly] + lx * C + c];
        }
        const int nb = 2 * rows * cols;
        const float ref = (float)(((int)block_reduce_sum((double)bsum) + nb / 2) / nb);       // (integers below 2^53: the sum is exact)
        // horizontal pass: hm[m][ly][x] = sum_d w[d] * moment_m(ly, x + d) for the 42 rows
        for (int item = tid; item < MI * MT; item += 256) {
            const int ly = item >> 5, x = item & (MT - 1);
            const unsigned char* pr = &sp[ly][php[ly] + x * C + c];
            const unsigned char* tr = &st[ly][pht[ly] + x * C + c];
            float mp = 0.0f, mt = 0.0f, mpp = 0.0f, mtt = 0.0f, mpt = 0.0f;
#pragma unroll
            for (int d = 0; d < 11; ++d) {
                const float p = (float)pr[d * C] - ref, t = (float)tr[d * C] - ref, wd = taps.w[d];
                mp = fmaf(wd, p, mp); mt = fmaf(wd, t, mt);
                mpp = fmaf(wd, p * p, mpp); mtt = fmaf(wd, t * t, mtt); mpt = fmaf(wd, p * t, mpt);
            }
            hm[0][ly][x] = mp; hm[1][ly][x] = mt; hm[2][ly][x] = mpp; hm[3][ly][x] = mtt; hm[4][ly][x] = mpt;
        }
        __syncthreads();
        float e[5][4];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            float col[14];
#pragma unroll
            for (int r = 0; r < 14; ++r) col[r] = hm[m][oy0 + r][ox];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                float a = 0.0f;
#pragma unroll
                for (int d = 0; d < 11; ++d) a = fmaf(taps.w[d], col[o + d], a);
                e[m][o] = a;
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (y0 + oy0 + o < h - 10 && x0 + ox < w - 10) {
                const float up = e[0][o], ut = e[1][o];                       // means of (byte - ref)
                const float vp = fmaxf(e[2][o] - up * up, 0.0f), vt = fmaxf(e[3][o] - ut * ut, 0.0f), cpt = e[4][o] - up * ut;
                const float mup = up + ref, mut = ut + ref;
                const float s = ((2.0f * mup * mut + c1) * (2.0f * cpt + c2)) / ((mup * mup + mut * mut + c1) * (vp + vt + c2));
                acc += (double)s;
            }
        }
        __syncthreads();
    }
    const double total = block_reduce_sum(acc);
    if (tid == 0) ssim_part[((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = total;
}

// ---- stage 2: the partials of image blockIdx.x in a fixed order -> its row (and c1 / c2 for the tile pass) --------------------------------
__global__ __launch_bounds__(256) void metrics_finish_kernel(const StatPart* stat_part, int nstat, const double* ssim_part, int ntiles,
                                                             mf_metrics_row* rows, float* c12, int64_t count) {
    const int b = blockIdx.x;
    if (nstat > 0) {
        Stat s;
        for (int i = threadIdx.x; i < nstat; i += 256) s.merge(stat_part[(int64_t)b * nstat + i]);
        const StatPart r = block_reduce_stat(s);
        if (threadIdx.x == 0) {
            rows[b].sq_err = (int64_t)r.sq;
            rows[b].pred_min = r.pmin; rows[b].pred_max = r.pmax; rows[b].target_min = r.tmin; rows[b].target_max = r.tmax;
            const double dr = (double)max(r.pmax - r.pmin, r.tmax - r.tmin);
            c12[2 * b] = (float)((0.01 * dr) * (0.01 * dr));
            c12[2 * b + 1] = (float)((0.03 * dr) * (0.03 * dr));
        }
    }
    if (ntiles > 0) {
        double a = 0.0;
        for (int i = threadIdx.x; i < ntiles; i += 256) a += ssim_part[(int64_t)b * ntiles + i];
        const double total = block_reduce_sum(a);
        if (threadIdx.x == 0) { rows[b].ssim_sum = total; rows[b].count = count; }
    }
}

inline int tiles_of(int n) { return (n - 10 + MT - 1) / MT; }
inline bool dims_ok(int batch, int h, int w, int channels) {
    return batch >= 1 && batch <= 65535 && h >= 11 && w >= 11 && h <= 32768 && w <= 32768 && channels >= 1 && channels <= 4;
}
struct WsLayout { int64_t ntiles, stat_bytes, ssim_bytes, total; };
inline WsLayout ws_layout(int batch, int h, int w) {
    WsLayout l;
    l.ntiles = (int64_t)tiles_of(h) * tiles_of(w);
    const int64_t nstat = l.ntiles > MSTAT_BLOCKS ? l.ntiles : MSTAT_BLOCKS;
    l.stat_bytes = (int64_t)batch * nstat * (int64_t)sizeof(StatPart);
    l.ssim_bytes = (int64_t)batch * l.ntiles * 8;
    l.total = l.stat_bytes + l.ssim_bytes + (int64_t)batch * 8;
    return l;
}

template <int C>
int launch_metrics(const unsigned char* pred, const unsigned char* target, const unsigned char* mask, int region, int batch, int h, int w,
                   float data_range, mf_metrics_row* rows, void* ws, hipStream_t s) {
    const WsLayout l = ws_layout(batch, h, w);
    StatPart* stat_part = (StatPart*)ws;
    double* ssim_part = (double*)((char*)ws + l.stat_bytes);
    float* c12 = (float*)((char*)ws + l.stat_bytes + l.ssim_bytes);
    const bool ride = data_range > 0.0f;
    const int64_t pixels = (int64_t)h * w, count = (int64_t)(h - 10) * (w - 10) * C;
    Taps taps;
    double g[11], sum = 0.0;
    for (int d = 0; d < 11; ++d) { g[d] = exp(-((d - 5) / 1.5) * ((d - 5) / 1.5) / 2.0); sum += g[d]; }
    for (int d = 0; d < 11; ++d) taps.w[d] = (float)(g[d] / sum);
    const dim3 grid((unsigned)tiles_of(w), (unsigned)tiles_of(h), (unsigned)batch);
    if (!ride) {
        const int64_t groups = (pixels * C + 3 + 3) / 4;
        int64_t blocks = (groups + 255) / 256;
        if (blocks > MSTAT_BLOCKS) blocks = MSTAT_BLOCKS;
        hipLaunchKernelGGL(metrics_stats_kernel<C>, dim3((unsigned)blocks, (unsigned)batch), dim3(256), 0, s, pred, target, mask, region, pixels,
                           stat_part);
        MF_CHECK_LAUNCH("mf_image_metrics(statistics)");
        hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)batch), dim3(256), 0, s, (const StatPart*)stat_part, (int)blocks,
                           (const double*)nullptr, 0, rows, c12, count);
        MF_CHECK_LAUNCH("mf_image_metrics(statistics, stage 2)");
        hipLaunchKernelGGL((metrics_ssim_kernel<C, false>), grid, dim3(256), 0, s, pred, target, mask, region, h, w, taps, data_range,
                           (const float*)c12, ssim_part, stat_part);
        MF_CHECK_LAUNCH("mf_image_metrics(ssim)");
        hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)batch), dim3(256), 0, s, (const StatPart*)nullptr, 0, (const double*)ssim_part,
                           (int)l.ntiles, rows, c12, count);
    } else {
        hipLaunchKernelGGL((metrics_ssim_kernel<C, true>), grid, dim3(256), 0, s, pred, target, mask, region, h, w, taps, data_range,
                           (const float*)c12, ssim_part, stat_part);
        MF_CHECK_LAUNCH("mf_image_metrics(ssim)");
        hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)batch), dim3(256), 0, s, (const StatPart*)stat_part, (int)l.ntiles,
                           (const double*)ssim_part, (int)l.ntiles, rows, c12, count);
    }
    MF_CHECK_LAUNCH("mf_image_metrics(stage 2)");
    return MF_OK;
}

}  // namespace

extern "C" int mf_sizeof_metrics_row(void) { return (int)sizeof(mf_metrics_row); }

extern "C" int64_t mf_image_metrics_ws_bytes(int32_t batch, int32_t h, int32_t w, int32_t channels) {
    if (!dims_ok(batch, h, w, channels)) {
        mf_set_error("mf_image_metrics_ws_bytes: batch %d, %d x %d x %d (batch 1 .. 65535, 11 .. 32768 pixels per edge, 1 .. 4 channels)", batch, h,
                     w, channels);
        return -1;
    }
    return ws_layout(batch, h, w).total;
}

extern "C" int mf_image_metrics(const void* pred_u8_nhwc, const void* target_u8_nhwc, const void* mask_u8, int32_t region, int32_t batch,
                                int32_t h, int32_t w, int32_t channels, float data_range, mf_metrics_row* rows_out, void* ws, void* stream) {
    MF_CHECK_ARG(pred_u8_nhwc && target_u8_nhwc && rows_out && ws, "mf_image_metrics: null pointer (pred, target, rows_out and ws are required)");
    MF_CHECK_ARG(h >= 11 && w >= 11, "mf_image_metrics: %d x %d image: the 11 x 11 window needs at least 11 pixels per edge", h, w);
    MF_CHECK_ARG(channels >= 1 && channels <= 4, "mf_image_metrics: %d channels (1 .. 4)", channels);
    MF_CHECK_ARG(dims_ok(batch, h, w, channels), "mf_image_metrics: batch %d, %d x %d (batch 1 .. 65535, at most 32768 pixels per edge)", batch, h, w);
    MF_CHECK_ARG(region >= 0 && region <= 2, "mf_image_metrics: region %d (0 none, 1 \"mask\", 2 \"mirror\")", region);
    MF_CHECK_ARG(region == 0 || mask_u8, "mf_image_metrics: region %d needs a mask", region);
    MF_CHECK_ARG((((uintptr_t)rows_out) & 7) == 0 && (((uintptr_t)ws) & 7) == 0, "mf_image_metrics: rows_out and ws must be 8-byte aligned");
    const unsigned char* p = (const unsigned char*)pred_u8_nhwc;
    const unsigned char* t = (const unsigned char*)target_u8_nhwc;
    const unsigned char* m = region ? (const unsigned char*)mask_u8 : nullptr;
    hipStream_t s = (hipStream_t)stream;
    switch (channels) {
        case 1: return launch_metrics<1>(p, t, m, region, batch, h, w, data_range, rows_out, ws, s);
        case 2: return launch_metrics<2>(p, t, m, region, batch, h, w, data_range, rows_out, ws, s);
        case 3: return launch_metrics<3>(p, t, m, region, batch, h, w, data_range, rows_out, ws, s);
        default: return launch_metrics<4>(p, t, m, region, batch, h, w, data_range, rows_out, ws, s);
    }
}
