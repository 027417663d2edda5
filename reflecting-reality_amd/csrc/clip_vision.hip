// The image side of CLIP scoring on the device (metrics/metrics.py:156-157 calculate_clip_similarity: torchmetrics' clip_score on
// openai/clip-vit-large-patch14, which runs transformers' CLIPProcessor on the host and CLIPModel in a second framework).
//   mf_clip_preprocess     replaces CLIPImageProcessor (PIL backend): Image.resize(BICUBIC) of the shortest edge on 8-bit pixels, centre crop,
//                          rescale by 1/255, normalise; and the unfold of CLIPVisionEmbeddings.patch_embedding (a stride-p conv) into the A
//                          operand of a GEMM.  The fp32 pixel_values tensor is never written.
//   mf_clip_vision_embed   replaces CLIPVisionEmbeddings.forward's cat([class_embedding, patch_embeds]) + position_embedding
//   mf_clip_score          replaces torchmetrics' _clip_score_update tail: both features L2-normalised, 100 * their dot product
// PIL's resize is integer arithmetic (Resample.c ImagingResampleHorizontal_8bpc / Vertical_8bpc): per output index a window [xmin, xmin + n)
// and n coefficients in 22-bit fixed point, an int32 accumulator that starts at 2^21, the result clip8(acc >> 22), and a uint8 image between
// the horizontal and the vertical pass.  The coefficient tables are built on the host in float64 (frontend.py) and only read here, so every
// pixel is a sum of integer products: no floating-point ordering can change it.  Only what the crop keeps is computed: the horizontal pass
// writes the crop's columns of every input row, the vertical pass runs inside the kernel that normalises and writes the patch matrix.
#include <math.h>
#include "mf_common.h"

namespace {

inline unsigned grid_for(int64_t n, int per_block = 256, int cap = 8192) {
    int64_t b = (n + per_block - 1) / per_block;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (unsigned)b;
}

__device__ __forceinline__ void load8_as_f32(const char* p, int dt, int64_t i, float* v) {
    if (dt == MF_F32) {
        const float4 a = *reinterpret_cast<const float4*>(p + i * 4), b = *reinterpret_cast<const float4*>(p + i * 4 + 16);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        const uint4 u = *reinterpret_cast<const uint4*>(p + i * 2);
        if (dt == MF_F16) unpack_h8<true>(u, v);
        else unpack_h8<false>(u, v);
    }
}
__device__ __forceinline__ void store8_from_f32(char* p, int dt, int64_t i, const float* v) {
    if (dt == MF_F32) {
        *reinterpret_cast<float4*>(p + i * 4) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(p + i * 4 + 16) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        *reinterpret_cast<uint4*>(p + i * 2) = dt == MF_F16 ? pack_h8<true>(v) : pack_h8<false>(v);
    }
}

// A resize table of n_out output indices with at most ksize taps each: int32 [n_out][2] (xmin, count), then int32 [n_out][ksize].
// One output sample: sum over the window of src[(xmin + j) * stride] * k[j] from 2^21, >> 22, clipped to a byte.  xmin and count are
// clamped to the source extent, so a table that does not belong to these sizes still reads inside the image.
__device__ __forceinline__ int resample_u8(const unsigned char* src, int64_t stride, const int32_t* tab, int n_out, int ksize, int i, int extent) {
    int xmin = tab[2 * i], cnt = tab[2 * i + 1];
    xmin = xmin < 0 ? 0 : (xmin > extent - 1 ? extent - 1 : xmin);
    cnt = cnt > ksize ? ksize : cnt;
    cnt = cnt > extent - xmin ? extent - xmin : cnt;
    const int32_t* k = tab + 2 * (int64_t)n_out + (int64_t)i * ksize;
    int acc = 1 << 21;
    for (int j = 0; j < cnt; ++j) acc += (int)src[(int64_t)(xmin + j) * stride] * k[j];
    acc >>= 22;
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

// ---- horizontal pass: mid[b][y][x][c] for the crop's columns x of every input row y; four bytes (one dword store) per thread ------------
__global__ __launch_bounds__(256) void clip_resize_h_kernel(const unsigned char* img, unsigned* mid, const int32_t* htab, int w1, int hk, int64_t rows,
                                                            int w, int crop, int left) {
    const int rowb = crop * 3;
    const int64_t total = rows * rowb, groups = (total + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        unsigned v = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = g * 4 + e;
            if (i >= total) break;
            const int64_t row = i / rowb;
            const int xc = (int)(i - row * rowb);
            const int x = xc / 3, c = xc - 3 * x;
            v |= (unsigned)resample_u8(img + row * w * 3 + c, 3, htab, w1, hk, left + x, w) << (8 * e);
        }
        mid[g] = v;
    }
}

// ---- vertical pass + crop + rescale + normalise + unfold: eight consecutive K columns of one patch row per thread -------------------------
// src: the image the vertical pass reads ([b][h][src_w][3]; the horizontal pass' output with col0 = 0, or the input itself with col0 = left
// when no horizontal pass ran).  vtab == nullptr: the heights agree and the row is read as it is.
struct Norm3 { float mean[3], std[3]; };

__global__ __launch_bounds__(256) void clip_patchify_kernel(const unsigned char* src, int src_w, int col0, int h, const int32_t* vtab, int h1, int vk,
                                                            int top, int crop, int patch, int kdim, int k8, Norm3 nm, char* out, int odt,
                                                            unsigned char* crop_u8, int64_t total) {
    const int np = crop / patch, g8 = k8 / 8, pp = patch * patch;
    const int64_t rstride = (int64_t)src_w * 3;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t prow = t / g8;                      // b * np^2 + patch index
        const int k0 = (int)(t - prow * g8) * 8;
        const int b = (int)(prow / ((int64_t)np * np));
        const int pi = (int)(prow - (int64_t)b * np * np);
        const int y0 = (pi / np) * patch, x0 = (pi % np) * patch;
        const unsigned char* sb = src + (int64_t)b * h * rstride;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + e;
            if (k >= kdim) { v[e] = 0.0f; continue; }
            const int c = k / pp, r = k - c * pp;
            const int y = y0 + r / patch, x = x0 + r % patch;
            const unsigned char* col = sb + (int64_t)(col0 + x) * 3 + c;
            const int u = vtab ? resample_u8(col, rstride, vtab, h1, vk, top + y, h) : (int)col[(int64_t)(top + y) * rstride];
            if (crop_u8) crop_u8[(((int64_t)b * crop + y) * crop + x) * 3 + c] = (unsigned char)u;
            // three fp32 operations, each rounded on its own (no contraction into an fma): rescale, subtract, divide
            v[e] = __fdiv_rn(__fsub_rn(__fmul_rn((float)u, 1.0f / 255.0f), nm.mean[c]), nm.std[c]);
        }
        store8_from_f32(out, odt, prow * k8 + k0, v);
    }
}

// ---- out[b][0] = class_embedding + pos[0]; out[b][1 + i] = patches[b][i] + pos[1 + i]; eight columns per thread --------------------------
__global__ __launch_bounds__(256) void clip_vision_embed_kernel(const char* patches, const char* cls, const char* pos, int idt, char* out, int odt,
                                                                int64_t rows, int tokens, int h8) {
    const int64_t total = rows * h8;
    const int hidden = h8 * 8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / h8;
        const int c = (int)(i - row * h8) * 8;
        const int64_t b = row / tokens;
        const int s = (int)(row - b * tokens);
        float a[8], p[8];
        if (s == 0) load8_as_f32(cls, idt, c, a);
        else load8_as_f32(patches, idt, (b * (tokens - 1) + (s - 1)) * hidden + c, a);
        load8_as_f32(pos, idt, (int64_t)s * hidden + c, p);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += p[e];
        store8_from_f32(out, odt, row * hidden + c, a);
    }
}

// ---- one wave per pair: the three sums of a row in fp32, folded by a fixed butterfly (the same inputs give the same bits) ------------------
__global__ __launch_bounds__(64) void clip_score_kernel(const float* img, const float* txt, int dim, float* out, float* norms) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* ib = img + (int64_t)b * dim;
    const float* tb = txt + (int64_t)b * dim;
    float dot = 0.0f, ii = 0.0f, tt = 0.0f;
    for (int j = lane; j < dim; j += 64) {
        const float x = ib[j], y = tb[j];
        dot = fmaf(x, y, dot); ii = fmaf(x, x, ii); tt = fmaf(y, y, tt);
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        dot += __shfl_xor(dot, m, 64); ii += __shfl_xor(ii, m, 64); tt += __shfl_xor(tt, m, 64);
    }
    if (lane == 0) {
        const float ni = sqrtf(ii), nt = sqrtf(tt);
        norms[2 * b] = ni; norms[2 * b + 1] = nt;
        out[b] = 100.0f * (dot / (ni * nt));          // no epsilon: a zero vector gives NaN, as x / x.norm() does in the reference
    }
}

struct Geometry { int h1, w1, top, left; };

// CLIPImageProcessor.resize (get_resize_output_image_size, default_to_square False): the shortest edge becomes `size`, the other
// int(size * long / short); center_crop: top = (h1 - crop) // 2, left = (w1 - crop) // 2
inline Geometry geometry(int h, int w, int size, int crop) {
    Geometry g;
    const int shorter = h <= w ? h : w, longer = h <= w ? w : h;
    const int nl = (int)((double)((int64_t)size * longer) / (double)shorter);
    g.h1 = h <= w ? size : nl;
    g.w1 = h <= w ? nl : size;
    g.top = (g.h1 - crop) / 2;
    g.left = (g.w1 - crop) / 2;
    return g;
}

inline bool pre_dims_ok(int batch, int h, int w, int size, int crop) {
    return batch >= 1 && batch <= 65535 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768 && size >= 1 && size <= 32768 && crop >= 1 && crop <= size &&
           (int64_t)size * (h > w ? h : w) / (h < w ? h : w) <= 32768;
}

}  // namespace

extern "C" int64_t mf_clip_preprocess_ws_bytes(int32_t batch, int32_t h, int32_t w, int32_t size, int32_t crop) {
    if (!pre_dims_ok(batch, h, w, size, crop)) {
        mf_set_error("mf_clip_preprocess_ws_bytes: batch %d, %d x %d -> %d, crop %d (batch 1 .. 65535, edges 1 .. 32768, crop <= size)", batch, h, w,
                     size, crop);
        return -1;
    }
    const Geometry g = geometry(h, w, size, crop);
    const int64_t mid = g.w1 == w ? 0 : (int64_t)batch * h * crop * 3;
    return (mid + 15) / 16 * 16 + 16;
}

extern "C" int mf_clip_preprocess(const void* images_u8_nhwc, int32_t batch, int32_t h, int32_t w, int32_t channels, int32_t size, int32_t crop,
                                  int32_t patch, const int32_t* htab, int32_t hk, const int32_t* vtab, int32_t vk, float mean0, float mean1,
                                  float mean2, float std0, float std1, float std2, void* patches_out, int32_t out_dtype, int32_t k8,
                                  void* crop_u8_out, void* ws, void* stream) {
    MF_CHECK_ARG(images_u8_nhwc && patches_out && ws, "mf_clip_preprocess: null pointer (images, patches_out and ws are required)");
    MF_CHECK_ARG(channels == 3, "mf_clip_preprocess: %d channels (the processor's mean / std are RGB: 3)", channels);
    MF_CHECK_ARG(pre_dims_ok(batch, h, w, size, crop), "mf_clip_preprocess: batch %d, %d x %d -> %d, crop %d (batch 1 .. 65535, edges 1 .. 32768, crop <= size)",
                 batch, h, w, size, crop);
    MF_CHECK_ARG(patch >= 1 && crop % patch == 0, "mf_clip_preprocess: crop %d is not a multiple of the patch size %d", crop, patch);
    const int kdim = 3 * patch * patch;
    MF_CHECK_ARG(k8 == (kdim + 7) / 8 * 8, "mf_clip_preprocess: K8 = %d, but 3 * %d * %d = %d rounds up to %d", k8, patch, patch, kdim, (kdim + 7) / 8 * 8);
    MF_CHECK_ARG(out_dtype == MF_F32 || mf_is16(out_dtype), "mf_clip_preprocess: patches_out is fp32, bf16 or fp16");
    MF_CHECK_ARG(std0 != 0.0f && std1 != 0.0f && std2 != 0.0f, "mf_clip_preprocess: a zero std");
    const Geometry g = geometry(h, w, size, crop);
    MF_CHECK_ARG((g.w1 != w) == (htab != nullptr) && (g.h1 != h) == (vtab != nullptr),
                 "mf_clip_preprocess: %d x %d -> %d x %d needs %s horizontal and %s vertical table (a pass whose size does not change is skipped)", h, w,
                 g.h1, g.w1, g.w1 != w ? "a" : "no", g.h1 != h ? "a" : "no");
    MF_CHECK_ARG((!htab || hk >= 1) && (!vtab || vk >= 1), "mf_clip_preprocess: table widths %d / %d", hk, vk);
    if (!mf_aligned16(patches_out) || !mf_aligned16(ws) || (((uintptr_t)htab) & 3) || (((uintptr_t)vtab) & 3)) {
        mf_set_error("mf_clip_preprocess: patches_out and ws must be 16-byte aligned, the tables 4-byte aligned");
        return MF_EALIGN;
    }
    hipStream_t s = (hipStream_t)stream;
    const unsigned char* img = (const unsigned char*)images_u8_nhwc;
    const unsigned char* src = img;
    int src_w = w, col0 = g.left;
    if (htab) {
        const int64_t rows = (int64_t)batch * h;
        hipLaunchKernelGGL(clip_resize_h_kernel, dim3(grid_for((rows * crop * 3 + 3) / 4)), dim3(256), 0, s, img, (unsigned*)ws, htab, g.w1, hk, rows,
                           w, crop, g.left);
        MF_CHECK_LAUNCH("mf_clip_preprocess(horizontal)");
        src = (const unsigned char*)ws;
        src_w = crop;
        col0 = 0;
    }
    const int np = crop / patch;
    const int64_t total = (int64_t)batch * np * np * (k8 / 8);
    const Norm3 nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
    hipLaunchKernelGGL(clip_patchify_kernel, dim3(grid_for(total)), dim3(256), 0, s, src, src_w, col0, h, vtab, g.h1, vk, g.top, crop, patch, kdim, k8,
                       nm, (char*)patches_out, out_dtype, (unsigned char*)crop_u8_out, total);
    MF_CHECK_LAUNCH("mf_clip_preprocess(patches)");
    return MF_OK;
}

extern "C" int mf_clip_vision_embed(const void* patches, const void* class_embedding, const void* pos_table, int32_t in_dtype, void* out,
                                    int32_t out_dtype, int32_t batch, int32_t tokens, int32_t hidden, void* stream) {
    MF_CHECK_ARG(patches && class_embedding && pos_table && out, "mf_clip_vision_embed: null pointer");
    MF_CHECK_ARG(batch >= 1 && tokens >= 2 && hidden >= 8 && hidden % 8 == 0, "mf_clip_vision_embed: bad sizes (tokens >= 2, hidden %% 8 == 0)");
    MF_CHECK_ARG((in_dtype == MF_F32 || mf_is16(in_dtype)) && (out_dtype == MF_F32 || mf_is16(out_dtype)),
                 "mf_clip_vision_embed: the operands and out are fp32, bf16 or fp16");
    MF_CHECK_ARG(!(mf_any_f16(in_dtype, out_dtype) && mf_any_bf16(in_dtype, out_dtype)), "mf_clip_vision_embed: fp16 and bf16 operands in one launch");
    if (!mf_aligned16(patches) || !mf_aligned16(class_embedding) || !mf_aligned16(pos_table) || !mf_aligned16(out)) {
        mf_set_error("mf_clip_vision_embed: the operands and out must be 16-byte aligned");
        return MF_EALIGN;
    }
    const int64_t rows = (int64_t)batch * tokens;
    hipLaunchKernelGGL(clip_vision_embed_kernel, dim3(grid_for(rows * (hidden / 8))), dim3(256), 0, (hipStream_t)stream, (const char*)patches,
                       (const char*)class_embedding, (const char*)pos_table, in_dtype, (char*)out, out_dtype, rows, tokens, hidden / 8);
    MF_CHECK_LAUNCH("mf_clip_vision_embed");
    return MF_OK;
}

extern "C" int mf_clip_score(const float* image_feats, const float* text_feats, int32_t batch, int32_t dim, float* out, float* norms_out,
                             void* stream) {
    MF_CHECK_ARG(image_feats && text_feats && out && norms_out, "mf_clip_score: null pointer (both features, out and norms_out are required)");
    MF_CHECK_ARG(batch >= 1 && dim >= 1, "mf_clip_score: batch %d, dim %d", batch, dim);
    if ((((uintptr_t)image_feats) | ((uintptr_t)text_feats) | ((uintptr_t)out) | ((uintptr_t)norms_out)) & 3) {
        mf_set_error("mf_clip_score: the features, out and norms_out are fp32 arrays: 4-byte aligned");
        return MF_EALIGN;
    }
    hipLaunchKernelGGL(clip_score_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, image_feats, text_feats, dim, out, norms_out);
    MF_CHECK_LAUNCH("mf_clip_score");
    return MF_OK;
}
