// Tiled VAE encode / decode (models/autoencoders/autoencoder_kl.py:311-423): the two data-movement ends of a tile.
//   mf_crop_pack_nhwc   x[:, :, i : i + tile, j : j + tile] of an NCHW fp32 tensor -> one slot range of a stacked NHWC group buffer
//                       (mf_pack_nhwc with a window and a batch offset)
//   mf_vae_tile_blend   blend_v, then blend_h, the crop [:row_limit, :row_limit] and the two torch.cat of tiled_decode / tiled_encode
//                       for ONE tile, launched per tile in raster order on the stream
// Both are bandwidth-bound streaming kernels without LDS: one thread per pixel, adjacent lanes on adjacent x (the NCHW planes on
// either side coalesce), the channels of a pixel moved as 16-byte vectors, 64-bit offsets throughout.
#include "mf_common.h"

namespace {

inline unsigned tgrid(int64_t n, int cap = 8192) {
    int64_t b = (n + 255) / 256;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

// ---- mf_crop_pack_nhwc -----------------------------------------------------------------------------------------------------------
struct CropArgs {
    const float* src;
    char* dst;
    int64_t plane, total;      // h * w of the source; batch * th * tw
    int c, w, y0, x0, th, tw, dt, c_pad, vec;
};

__device__ __forceinline__ void store4(char* dst, int dt, int64_t i, const float* v) {
    if (dt == MF_F32) *reinterpret_cast<float4*>(dst + i * 4) = float4{v[0], v[1], v[2], v[3]};
    else if (dt == MF_F16) *reinterpret_cast<uint2*>(dst + i * 2) = uint2{pack_f16x2(v[0], v[1]), pack_f16x2(v[2], v[3])};
    else *reinterpret_cast<uint2*>(dst + i * 2) = uint2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
}

__global__ __launch_bounds__(256) void crop_pack_nhwc_kernel(const CropArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % a.tw);
        const int64_t r = i / a.tw;
        const int y = (int)(r % a.th);
        const int64_t b = r / a.th;
        const float* sp = a.src + b * a.c * a.plane + (int64_t)(a.y0 + y) * a.w + (a.x0 + x);
        const int64_t o = i * a.c_pad;                                  // dst is already at its batch offset
        for (int c4 = 0; c4 < a.c_pad; c4 += 4) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = c4 + j < a.c ? sp[(int64_t)(c4 + j) * a.plane] : 0.0f;
            if (a.vec) store4(a.dst, a.dt, o + c4, v);
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c4 + j < a.c_pad) store_from_f32(a.dst, a.dt, o + c4 + j, v[j]);
            }
        }
    }
}

// ---- mf_vae_tile_blend -----------------------------------------------------------------------------------------------------------
struct BlendArgs {
    float* tile;
    const float *above, *left;
    float* out;
    int64_t ld, total;
    int th, tw, ah, lw, ev, eh, c, ch, cw, nhwc, out_h, out_w, oy, ox;
};

// a * wa + b * wb as ATen evaluates the reference's one-line loops: two products and a sum, each rounded to fp32.  HIP's __fmul_rn /
// __fadd_rn are plain operators the compiler may still contract into an FMA after inlining, so contraction is switched off here.
__device__ __forceinline__ float ramp(float a, float wa, float b, float wb) {
#pragma clang fp contract(off)
    const float p = a * wa, q = b * wb;
    return p + q;
}

__device__ __forceinline__ float4 ramp4(const float4 a, float wa, const float4 b, float wb) {
    return float4{ramp(a.x, wa, b.x, wb), ramp(a.y, wa, b.y, wb), ramp(a.z, wa, b.z, wb), ramp(a.w, wa, b.w, wb)};
}

// Each thread finishes its own pixel: vertical ramp against the finished tile above, then horizontal ramp against the finished tile
// to the left (the reference's order); it reads no other pixel of its own tile.  All ld floats of a pixel are blended (the pad
// channels ride along), the strips go back into the tile (a later neighbour reads them), the crop goes to the output.
__global__ __launch_bounds__(256) void vae_tile_blend_kernel(const BlendArgs a) {
    const int nv = (int)(a.ld / 4);
    const int64_t out_plane = (int64_t)a.out_h * a.out_w;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % a.tw);
        const int64_t r = i / a.tw;
        const int y = (int)(r % a.th);
        const int64_t b = r / a.th;
        const bool bv = y < a.ev, bh = x < a.eh, crop = y < a.ch && x < a.cw;
        if (!bv && !bh && !crop) continue;
        float w0 = 1.0f, w1 = 0.0f, u0 = 1.0f, u1 = 0.0f;
        if (bv) {                                                       // Python: (1 - y / e) and (y / e) in double, cast by ATen to fp32
            const double t = (double)y / (double)a.ev;
            w0 = (float)t; w1 = (float)(1.0 - t);
        }
        if (bh) {
            const double t = (double)x / (double)a.eh;
            u0 = (float)t; u1 = (float)(1.0 - t);
        }
        float4* tp = reinterpret_cast<float4*>(a.tile + i * a.ld);
        const float4* ap = bv ? reinterpret_cast<const float4*>(a.above + ((b * a.ah + (a.ah - a.ev + y)) * a.tw + x) * a.ld) : nullptr;
        const float4* lp = bh ? reinterpret_cast<const float4*>(a.left + ((b * a.th + y) * a.lw + (a.lw - a.eh + x)) * a.ld) : nullptr;
        const int64_t opix = (int64_t)(a.oy + y) * a.out_w + (a.ox + x);
        for (int k = 0; k < nv; ++k) {
            float4 v = tp[k];
            if (bv) v = ramp4(ap[k], w1, v, w0);
            if (bh) v = ramp4(lp[k], u1, v, u0);
            if (bv || bh) tp[k] = v;
            if (!crop) continue;
            if (a.nhwc) reinterpret_cast<float4*>(a.out + (b * out_plane + opix) * a.ld)[k] = v;
            else {
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * k + j < a.c) a.out[(b * a.c + 4 * k + j) * out_plane + opix] = e[j];
            }
        }
    }
}

}  // namespace

extern "C" int mf_crop_pack_nhwc(const float* src, int32_t batch, int32_t c, int32_t h, int32_t w, int32_t y0, int32_t x0, int32_t th,
                                 int32_t tw, void* dst, int32_t dst_dtype, int32_t c_pad, int32_t dst_batch, int32_t batch_offset,
                                 void* stream) {
    MF_CHECK_ARG(src && dst, "mf_crop_pack_nhwc: null pointer");
    MF_CHECK_ARG(batch >= 1 && c >= 1 && h >= 1 && w >= 1 && th >= 1 && tw >= 1,
                 "mf_crop_pack_nhwc: batch %d, channels %d, source %d x %d, window %d x %d must be positive", batch, c, h, w, th, tw);
    MF_CHECK_ARG(y0 >= 0 && x0 >= 0 && (int64_t)y0 + th <= h && (int64_t)x0 + tw <= w,
                 "mf_crop_pack_nhwc: window (%d, %d) + %d x %d lies outside the %d x %d source", y0, x0, th, tw, h, w);
    MF_CHECK_ARG(dst_dtype == MF_F32 || dst_dtype == MF_BF16 || dst_dtype == MF_F16, "mf_crop_pack_nhwc: bad dst_dtype %d", dst_dtype);
    MF_CHECK_ARG(c_pad >= c, "mf_crop_pack_nhwc: c_pad %d < c = %d", c_pad, c);
    MF_CHECK_ARG(dst_batch >= 1 && batch_offset >= 0 && (int64_t)batch_offset + batch <= dst_batch,
                 "mf_crop_pack_nhwc: samples %d .. %d lie outside the buffer's %d", batch_offset, batch_offset + batch, dst_batch);
    const int es = dst_dtype == MF_F32 ? 4 : 2;
    CropArgs a;
    a.src = src;
    a.dst = (char*)dst + (int64_t)batch_offset * th * tw * c_pad * es;
    a.plane = (int64_t)h * w; a.total = (int64_t)batch * th * tw;
    a.c = c; a.w = w; a.y0 = y0; a.x0 = x0; a.th = th; a.tw = tw; a.dt = dst_dtype; a.c_pad = c_pad;
    a.vec = c_pad % 4 == 0 && ((uintptr_t)a.dst & (es == 4 ? 15 : 7)) == 0;
    hipLaunchKernelGGL(crop_pack_nhwc_kernel, dim3(tgrid(a.total)), dim3(256), 0, (hipStream_t)stream, a);
    MF_CHECK_LAUNCH("mf_crop_pack_nhwc");
    return MF_OK;
}

extern "C" int mf_vae_tile_blend(float* tile, const float* above, const float* left, int32_t batch, int32_t th, int32_t tw, int32_t above_h,
                                 int32_t above_w, int32_t left_h, int32_t left_w, int64_t ld, int32_t c, int32_t blend_extent,
                                 int32_t row_limit, float* out, int32_t out_nhwc, int32_t out_h, int32_t out_w, int32_t out_y,
                                 int32_t out_x, void* stream) {
    MF_CHECK_ARG(tile && out, "mf_vae_tile_blend: null tile or output");
    MF_CHECK_ARG(batch >= 1 && th >= 1 && tw >= 1 && c >= 1 && out_h >= 1 && out_w >= 1,
                 "mf_vae_tile_blend: batch %d, tile %d x %d, c %d, output %d x %d must be positive", batch, th, tw, c, out_h, out_w);
    MF_CHECK_ARG(ld >= c, "mf_vae_tile_blend: ld %lld < c = %d", (long long)ld, c);
    MF_CHECK_ARG(ld % 4 == 0, "mf_vae_tile_blend: ld %lld is not a multiple of 4 floats", (long long)ld);
    MF_CHECK_ARG(blend_extent >= 0 && row_limit >= 1, "mf_vae_tile_blend: blend_extent %d (>= 0), row_limit %d (>= 1)", blend_extent, row_limit);
    MF_CHECK_ARG(out_nhwc == 0 || out_nhwc == 1, "mf_vae_tile_blend: out_nhwc is 0 (NCHW) or 1, got %d", out_nhwc);
    MF_CHECK_ARG(!above || (above_h >= 1 && above_w == tw), "mf_vae_tile_blend: the tile above is %d x %d, this one %d x %d: widths differ",
                 above_h, above_w, th, tw);
    MF_CHECK_ARG(!left || (left_w >= 1 && left_h == th), "mf_vae_tile_blend: the tile to the left is %d x %d, this one %d x %d: heights differ",
                 left_h, left_w, th, tw);
    const int ch = th < row_limit ? th : row_limit, cw = tw < row_limit ? tw : row_limit;
    MF_CHECK_ARG(out_y >= 0 && out_x >= 0 && (int64_t)out_y + ch <= out_h && (int64_t)out_x + cw <= out_w,
                 "mf_vae_tile_blend: the crop %d x %d at (%d, %d) lies outside the %d x %d output", ch, cw, out_y, out_x, out_h, out_w);
    MF_CHECK_ARG((((uintptr_t)tile | (uintptr_t)above | (uintptr_t)left) & 15) == 0 && (!out_nhwc || ((uintptr_t)out & 15) == 0) &&
                     ((uintptr_t)out & 3) == 0,
                 "mf_vae_tile_blend: the tiles (and an NHWC output) must be 16-byte aligned");
    auto min3 = [](int p, int q, int e) { return p < q ? (p < e ? p : e) : (q < e ? q : e); };
    BlendArgs a;
    a.tile = tile; a.above = above; a.left = left; a.out = out;
    a.ld = ld; a.total = (int64_t)batch * th * tw;
    a.th = th; a.tw = tw; a.ah = above ? above_h : 0; a.lw = left ? left_w : 0;
    a.ev = above ? min3(above_h, th, blend_extent) : 0;                // blend_v: min(a.shape[2], b.shape[2], blend_extent)
    a.eh = left ? min3(left_w, tw, blend_extent) : 0;                  // blend_h: min(a.shape[3], b.shape[3], blend_extent)
    a.c = c; a.ch = ch; a.cw = cw; a.nhwc = out_nhwc; a.out_h = out_h; a.out_w = out_w; a.oy = out_y; a.ox = out_x;
    hipLaunchKernelGGL(vae_tile_blend_kernel, dim3(tgrid(a.total)), dim3(256), 0, (hipStream_t)stream, a);
    MF_CHECK_LAUNCH("mf_vae_tile_blend");
    return MF_OK;
}
