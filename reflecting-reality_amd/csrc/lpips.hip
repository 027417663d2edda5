// LPIPS on the device (metrics/metrics.py:51-67 compute_metrics, :150-151 calculate_lpips, :202-204: torchmetrics'
// learned_perceptual_image_patch_similarity(net_type="squeeze", normalize=False) over torchvision's squeezenet1_1.features).  The
// convolutions are mf_gemm_conv calls (lpips.py); this file holds the arithmetic around them:
//   mf_lpips_prepare      get_normalised_tensor (metrics.py:24-48) + the "mask" / "mirror" blackening (dataset.py:62-68) + the LPIPS scaling
//                         layer, written as the first conv's A operand: [2B][H][W][8], three channels and five zero channels, pred images first
//   mf_relu               in place over a strided [rows][channels] block (the squeeze output, the concatenated expand outputs)
//   mf_maxpool3s2_ceil    MaxPool2d(3, 2, ceil_mode=True) over NHWC: the last window may hang over the edge
//   mf_lpips_layer        per image pair sum over the pixels of sum_c w_c (a_c / n(a) - b_c / n(b))^2, n(x) = sqrt(1e-8 + sum_c x_c^2)
//   mf_lpips_finish       the per-block partials of the seven layers in a fixed order -> one fp32 [B][7] row
// A pixel's channels stay in registers between the norm and the difference: 8 per lane, C / 8 lanes (rounded up to a power of two) per
// pixel, so a wave reads consecutive pixels as one contiguous run of 16-byte (32-byte in fp32) pieces; the two channel sums of a pixel are
// xor butterflies inside its lanes.  Every block owns a fixed run of pixels and writes one double; no floating-point atomics: the same
// inputs give the same bits on every run.
#include <math.h>
#include "mf_common.h"

namespace {

constexpr int LP_PARTS = 512;            // blocks (and partial sums) per image and layer: 8 waves per SIMD at batch 4, 128 pixels per block at 255 x 255
constexpr int LP_LAYERS = 7;

inline unsigned grid_for(int64_t n, int per_block = 256, int cap = 8192) {
    int64_t b = (n + per_block - 1) / per_block;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// DT: 0 fp32, 1 bf16, 2 fp16 (compiled in: a run-time test per packed pair splits the unrolled loads into basic blocks)
template <int DT>
__device__ __forceinline__ void load8(const char* p, int64_t i, float* v) {
    if constexpr (DT == 0) {
        const float4 a = *reinterpret_cast<const float4*>(p + i * 4), b = *reinterpret_cast<const float4*>(p + i * 4 + 16);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        unpack_h8<DT == 2>(*reinterpret_cast<const uint4*>(p + i * 2), v);
    }
}
template <int DT>
__device__ __forceinline__ void store8(char* p, int64_t i, const float* v) {
    if constexpr (DT == 0) {
        *reinterpret_cast<float4*>(p + i * 4) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(p + i * 4 + 16) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        *reinterpret_cast<uint4*>(p + i * 2) = pack_h8<DT == 2>(v);
    }
}
inline int dt_index(int dt) { return dt == MF_F32 ? 0 : (dt == MF_BF16 ? 1 : 2); }

struct Scale3 { float shift[3], scale[3]; };

// ---- one pixel of one image per thread: bytes -> region -> normalise -> scaling layer -> 8 stored channels ---------------------------------
template <int DT>
__global__ __launch_bounds__(256) void lpips_prepare_kernel(const unsigned char* pred, const unsigned char* gt, const unsigned char* mask, int region,
                                                            int64_t pixels, int batch, int unit_range, Scale3 sc, char* out) {
    const int64_t total = 2 * (int64_t)batch * pixels;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t img = i / pixels, p = i - img * pixels;
        const int b = (int)(img < batch ? img : img - batch);
        const unsigned char* src = (img < batch ? pred : gt) + ((int64_t)b * pixels + p) * 3;
        bool black = false;
        if (region) {
            const unsigned m = mask[(int64_t)b * pixels + p];
            black = region == 1 ? m == 255u : m == 0u;
        }
        float v[8];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = black ? 0.0f : (float)src[c];
            // every step rounded on its own, as torch evaluates it (no contraction into an fma)
            const float n = unit_range ? __fdiv_rn(x, 255.0f) : __fsub_rn(__fdiv_rn(x, 127.5f), 1.0f);
            v[c] = __fdiv_rn(__fsub_rn(n, sc.shift[c]), sc.scale[c]);
        }
#pragma unroll
        for (int c = 3; c < 8; ++c) v[c] = 0.0f;
        store8<DT>(out, i * 8, v);
    }
}

// ---- relu in place: 8 channels per thread of a [rows][channels] block whose rows are ld elements apart --------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void relu_kernel(char* x, int64_t rows, int c8, int64_t ld) {
    const int64_t total = rows * c8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / c8;
        const int64_t at = row * ld + (i - row * c8) * 8;
        float v[8];
        load8<DT>(x, at, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] < 0.0f ? 0.0f : v[e];          // (a NaN stays a NaN, as in torch)
        store8<DT>(x, at, v);
    }
}

// ---- MaxPool2d(3, 2, ceil_mode=True): 8 channels of one output pixel per thread; the window is clipped to the image ------------------------
template <int DT>
__global__ __launch_bounds__(256) void maxpool_kernel(const char* x, char* out, int batch, int h, int w, int ho, int wo, int c8) {
    const int64_t total = (int64_t)batch * ho * wo * c8;
    const int c = c8 * 8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t opix = i / c8;
        const int cv = (int)(i - opix * c8);
        const int64_t brow = opix / wo;                       // b * ho + oy
        const int ox = (int)(opix - brow * wo);
        const int b = (int)(brow / ho), oy = (int)(brow - (int64_t)b * ho);
        const int y1 = min(2 * oy + 3, h), x1 = min(2 * ox + 3, w);
        float m[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
        for (int y = 2 * oy; y < y1; ++y)
            for (int xx = 2 * ox; xx < x1; ++xx) {
                float v[8];
                load8<DT>(x, (((int64_t)b * h + y) * w + xx) * c + cv * 8, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) m[e] = (v[e] > m[e] || v[e] != v[e]) ? v[e] : m[e];      // (torch's max_pool2d propagates a NaN)
            }
        store8<DT>(out, opix * c + cv * 8, m);
    }
}

// ---- the layer distance: L lanes per pixel (L * 8 >= C), 256 / L pixels per block and pass ------------------------------------------------
// grid (LP_PARTS, B): block x of image b owns pixels [x * per, (x + 1) * per) and writes part[b][x] (0 when it owns none).
template <int L, int DT>
__global__ __launch_bounds__(256) void lpips_layer_kernel(const char* feat, const float* wgt, int64_t pixels, int C, int batch, double* part) {
    constexpr int G = 256 / L;
    __shared__ double red[G];
    const int tid = threadIdx.x, sub = tid & (L - 1), grp = tid / L;
    const int b = blockIdx.y;
    const int c0 = sub * 8;
    const bool live = c0 < C;
    constexpr int es = DT == 0 ? 4 : 2;
    const char* fa = feat + (int64_t)b * pixels * C * es;
    const char* fb = feat + (int64_t)(batch + b) * pixels * C * es;
    float wv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) wv[e] = live ? wgt[c0 + e] : 0.0f;
    const int64_t per = (pixels + LP_PARTS - 1) / LP_PARTS;
    const int64_t p0 = (int64_t)blockIdx.x * per;
    const int64_t p1 = p0 + per < pixels ? p0 + per : pixels;
    float acc = 0.0f;
    for (int64_t base = p0; base < p1; base += G) {          // (uniform over the block: a lane without a pixel carries zeros, which add 0)
        const int64_t p = base + grp;
        const bool have = live && p < p1;
        float a[8], bb[8];
        if (have) {
            load8<DT>(fa, p * C + c0, a);
            load8<DT>(fb, p * C + c0, bb);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = bb[e] = 0.0f;
        }
        float sa = 0.0f, sb = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { sa = fmaf(a[e], a[e], sa); sb = fmaf(bb[e], bb[e], sb); }
#pragma unroll
        for (int m = L / 2; m > 0; m >>= 1) { sa += __shfl_xor(sa, m, 64); sb += __shfl_xor(sb, m, 64); }
        const float na = __fsqrt_rn(__fadd_rn(1e-8f, sa)), nb = __fsqrt_rn(__fadd_rn(1e-8f, sb));
        float d = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            // the two quotients and their difference rounded on their own: equal inputs give exactly 0
            const float t = __fsub_rn(__fdiv_rn(a[e], na), __fdiv_rn(bb[e], nb));
            d = fmaf(wv[e], __fmul_rn(t, t), d);
        }
#pragma unroll
        for (int m = L / 2; m > 0; m >>= 1) d += __shfl_xor(d, m, 64);
        acc += d;
    }
    if (sub == 0) red[grp] = (double)acc;
    __syncthreads();
    for (int s = G / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) part[(int64_t)b * LP_PARTS + blockIdx.x] = red[0];
}

// ---- one wave per (image, layer): its LP_PARTS partials in a fixed order -------------------------------------------------------------------
__global__ __launch_bounds__(64) void lpips_finish_kernel(const double* part, int batch, float* rows) {
    const int b = blockIdx.x, l = blockIdx.y, lane = threadIdx.x;
    const double* p = part + ((int64_t)l * batch + b) * LP_PARTS;
    double v = 0.0;
    for (int i = lane; i < LP_PARTS; i += 64) v += p[i];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) rows[b * LP_LAYERS + l] = (float)v;
}

template <int DT>
void launch_layer(const char* feat, const float* wgt, int64_t pixels, int c, int batch, double* part, hipStream_t s) {
    const dim3 grid(LP_PARTS, (unsigned)batch);
    const int nvec = c / 8;
    if (nvec <= 8) hipLaunchKernelGGL((lpips_layer_kernel<8, DT>), grid, dim3(256), 0, s, feat, wgt, pixels, c, batch, part);
    else if (nvec <= 16) hipLaunchKernelGGL((lpips_layer_kernel<16, DT>), grid, dim3(256), 0, s, feat, wgt, pixels, c, batch, part);
    else if (nvec <= 32) hipLaunchKernelGGL((lpips_layer_kernel<32, DT>), grid, dim3(256), 0, s, feat, wgt, pixels, c, batch, part);
    else hipLaunchKernelGGL((lpips_layer_kernel<64, DT>), grid, dim3(256), 0, s, feat, wgt, pixels, c, batch, part);
}

inline bool act_dtype(int dt) { return dt == MF_F32 || mf_is16(dt); }

}  // namespace

extern "C" int64_t mf_lpips_ws_bytes(int32_t batch) {
    if (batch < 1 || batch > 32767) {
        mf_set_error("mf_lpips_ws_bytes: batch %d (1 .. 32767 image pairs)", batch);
        return -1;
    }
    return (int64_t)LP_LAYERS * batch * LP_PARTS * (int64_t)sizeof(double);
}

extern "C" int mf_lpips_prepare(const void* pred_u8_nhwc, const void* gt_u8_nhwc, const void* mask_u8, int32_t region, int32_t batch, int32_t h,
                                int32_t w, int32_t channels, int32_t unit_range, void* out, int32_t out_dtype, void* stream) {
    MF_CHECK_ARG(pred_u8_nhwc && gt_u8_nhwc && out, "mf_lpips_prepare: null pointer (pred, gt and out are required)");
    MF_CHECK_ARG(channels == 3, "mf_lpips_prepare: %d channels (the scaling layer's shift / scale are RGB: 3)", channels);
    MF_CHECK_ARG(batch >= 1 && batch <= 32767 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768,
                 "mf_lpips_prepare: batch %d, %d x %d (batch 1 .. 32767, 1 .. 32768 pixels per edge)", batch, h, w);
    MF_CHECK_ARG(region >= 0 && region <= 2, "mf_lpips_prepare: region %d (0 none, 1 \"mask\", 2 \"mirror\")", region);
    MF_CHECK_ARG(region == 0 || mask_u8, "mf_lpips_prepare: region %d needs a mask", region);
    MF_CHECK_ARG(unit_range == 0 || unit_range == 1, "mf_lpips_prepare: unit_range %d (0: x / 127.5 - 1, 1: x / 255)", unit_range);
    MF_CHECK_ARG(act_dtype(out_dtype), "mf_lpips_prepare: out is fp32, bf16 or fp16");
    if (!mf_aligned16(out)) {
        mf_set_error("mf_lpips_prepare: out must be 16-byte aligned");
        return MF_EALIGN;
    }
    const Scale3 sc = {{-0.030f, -0.088f, -0.188f}, {0.458f, 0.448f, 0.450f}};
    const int64_t pixels = (int64_t)h * w;
    const dim3 grid(grid_for(2 * (int64_t)batch * pixels));
    hipStream_t s = (hipStream_t)stream;
    const unsigned char* p = (const unsigned char*)pred_u8_nhwc;
    const unsigned char* g = (const unsigned char*)gt_u8_nhwc;
    const unsigned char* m = region ? (const unsigned char*)mask_u8 : nullptr;
    switch (dt_index(out_dtype)) {
        case 0: hipLaunchKernelGGL(lpips_prepare_kernel<0>, grid, dim3(256), 0, s, p, g, m, region, pixels, batch, unit_range, sc, (char*)out); break;
        case 1: hipLaunchKernelGGL(lpips_prepare_kernel<1>, grid, dim3(256), 0, s, p, g, m, region, pixels, batch, unit_range, sc, (char*)out); break;
        default: hipLaunchKernelGGL(lpips_prepare_kernel<2>, grid, dim3(256), 0, s, p, g, m, region, pixels, batch, unit_range, sc, (char*)out); break;
    }
    MF_CHECK_LAUNCH("mf_lpips_prepare");
    return MF_OK;
}

extern "C" int mf_relu(void* x, int32_t dtype, int64_t rows, int32_t channels, int64_t ld, void* stream) {
    MF_CHECK_ARG(x, "mf_relu: null pointer");
    MF_CHECK_ARG(act_dtype(dtype), "mf_relu: x is fp32, bf16 or fp16");
    MF_CHECK_ARG(rows >= 1 && channels >= 8 && channels % 8 == 0 && ld >= channels && rows <= (1ll << 40) / ld,
                 "mf_relu: %lld rows of %d channels, %lld apart (channels %% 8 == 0, ld >= channels)", (long long)rows, channels, (long long)ld);
    if (!mf_aligned16(x) || ld % 8) {
        mf_set_error("mf_relu: x must be 16-byte aligned and ld a multiple of 8 elements");
        return MF_EALIGN;
    }
    const dim3 grid(grid_for(rows * (channels / 8)));
    hipStream_t s = (hipStream_t)stream;
    switch (dt_index(dtype)) {
        case 0: hipLaunchKernelGGL(relu_kernel<0>, grid, dim3(256), 0, s, (char*)x, rows, channels / 8, ld); break;
        case 1: hipLaunchKernelGGL(relu_kernel<1>, grid, dim3(256), 0, s, (char*)x, rows, channels / 8, ld); break;
        default: hipLaunchKernelGGL(relu_kernel<2>, grid, dim3(256), 0, s, (char*)x, rows, channels / 8, ld); break;
    }
    MF_CHECK_LAUNCH("mf_relu");
    return MF_OK;
}

extern "C" int mf_maxpool3s2_ceil(const void* x, void* out, int32_t dtype, int32_t batch, int32_t h, int32_t w, int32_t channels, void* stream) {
    MF_CHECK_ARG(x && out, "mf_maxpool3s2_ceil: null pointer");
    MF_CHECK_ARG(act_dtype(dtype), "mf_maxpool3s2_ceil: x is fp32, bf16 or fp16");
    MF_CHECK_ARG(batch >= 1 && batch <= 65535 && h >= 3 && w >= 3 && h <= 32768 && w <= 32768 && channels >= 8 && channels % 8 == 0 && channels <= 65536,
                 "mf_maxpool3s2_ceil: batch %d, %d x %d x %d (at least one whole 3 x 3 window, channels %% 8 == 0)", batch, h, w, channels);
    if (!mf_aligned16(x) || !mf_aligned16(out)) {
        mf_set_error("mf_maxpool3s2_ceil: x and out must be 16-byte aligned");
        return MF_EALIGN;
    }
    const int ho = (h - 3 + 1) / 2 + 1, wo = (w - 3 + 1) / 2 + 1;          // ceil((n - 3) / 2) + 1: the last window starts inside the image
    const dim3 grid(grid_for((int64_t)batch * ho * wo * (channels / 8)));
    hipStream_t s = (hipStream_t)stream;
    switch (dt_index(dtype)) {
        case 0: hipLaunchKernelGGL(maxpool_kernel<0>, grid, dim3(256), 0, s, (const char*)x, (char*)out, batch, h, w, ho, wo, channels / 8); break;
        case 1: hipLaunchKernelGGL(maxpool_kernel<1>, grid, dim3(256), 0, s, (const char*)x, (char*)out, batch, h, w, ho, wo, channels / 8); break;
        default: hipLaunchKernelGGL(maxpool_kernel<2>, grid, dim3(256), 0, s, (const char*)x, (char*)out, batch, h, w, ho, wo, channels / 8); break;
    }
    MF_CHECK_LAUNCH("mf_maxpool3s2_ceil");
    return MF_OK;
}

extern "C" int mf_lpips_layer(const void* feat, int32_t dtype, const float* weight, int32_t batch, int64_t pixels, int32_t channels, int32_t layer,
                              void* ws, void* stream) {
    MF_CHECK_ARG(feat && weight && ws, "mf_lpips_layer: null pointer (feat, weight and ws are required)");
    MF_CHECK_ARG(act_dtype(dtype), "mf_lpips_layer: feat is fp32, bf16 or fp16");
    MF_CHECK_ARG(batch >= 1 && batch <= 32767 && pixels >= 1 && pixels < (1ll << 31),
                 "mf_lpips_layer: batch %d, %lld pixels (batch 1 .. 32767 pairs, pixels below 2^31)", batch, (long long)pixels);
    MF_CHECK_ARG(channels >= 8 && channels <= 512 && channels % 8 == 0, "mf_lpips_layer: %d channels (8 .. 512, a multiple of 8: they stay in registers)",
                 channels);
    MF_CHECK_ARG(layer >= 0 && layer < LP_LAYERS, "mf_lpips_layer: layer %d (0 .. %d)", layer, LP_LAYERS - 1);
    if (!mf_aligned16(feat) || !mf_aligned16(weight) || (((uintptr_t)ws) & 7)) {
        mf_set_error("mf_lpips_layer: feat and weight must be 16-byte aligned, ws 8-byte aligned");
        return MF_EALIGN;
    }
    double* part = (double*)ws + (int64_t)layer * batch * LP_PARTS;
    hipStream_t s = (hipStream_t)stream;
    switch (dt_index(dtype)) {
        case 0: launch_layer<0>((const char*)feat, weight, pixels, channels, batch, part, s); break;
        case 1: launch_layer<1>((const char*)feat, weight, pixels, channels, batch, part, s); break;
        default: launch_layer<2>((const char*)feat, weight, pixels, channels, batch, part, s); break;
    }
    MF_CHECK_LAUNCH("mf_lpips_layer");
    return MF_OK;
}

extern "C" int mf_lpips_finish(const void* ws, int32_t batch, float* rows_out, void* stream) {
    MF_CHECK_ARG(ws && rows_out, "mf_lpips_finish: null pointer");
    MF_CHECK_ARG(batch >= 1 && batch <= 32767, "mf_lpips_finish: batch %d (1 .. 32767 image pairs)", batch);
    if ((((uintptr_t)ws) & 7) || (((uintptr_t)rows_out) & 3)) {
        mf_set_error("mf_lpips_finish: ws must be 8-byte aligned, rows_out 4-byte aligned");
        return MF_EALIGN;
    }
    hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)batch, LP_LAYERS), dim3(64), 0, (hipStream_t)stream, (const double*)ws, batch, rows_out);
    MF_CHECK_LAUNCH("mf_lpips_finish");
    return MF_OK;
}
