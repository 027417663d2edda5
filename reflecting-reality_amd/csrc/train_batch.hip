// The training batch on the device: what the reference does between a decoded sample and the model call.
//   dataset.py:61-96, 216-221      get_masked_image, apply_transforms_rgb / _mask (the resolution-sized case), np.fliplr
//   train_brushnet_mirror.py:1351-1449 minus the networks: DiagonalGaussianDistribution.sample * scaling_factor of up to four encodes,
//                                  F.interpolate (nearest) of mask / depth / normals, torch.cat, add_noise, the epsilon / v target, the
//                                  per-sample loss weight — one launch (mf_train_batch_assemble)
// Bandwidth-bound streaming kernels: adjacent lanes walk adjacent pixels of the NCHW outputs; nothing synchronises with the host (the
// timesteps are read from device memory and their coefficients gathered from device tables).
#include "mf_common.h"

namespace {

inline unsigned tgrid(int64_t n, int cap = 8192) {
    int64_t b = (n + 255) / 256;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

// ---- mf_train_example_u8 ---------------------------------------------------------------------------------------------------------
// Four output pixels of one row per thread.  The bytes come in as dwords when the group is whole and its address allows it (a flipped
// group is the same contiguous bytes read in reverse), each plane gets one 16-byte store when ITS address allows it.  Every register
// array is indexed by literals only (no scratch).
__device__ __forceinline__ float px_value(unsigned px, int normalize) {
    const float v = __fdiv_rn((float)px, 255.0f);                       // numpy / torch: a correctly rounded fp32 division
    return normalize ? __fmul_rn(__fsub_rn(v, 0.5f), 2.0f) : v;         // Normalize([0.5], [0.5]): (v - 0.5) / 0.5
}

__device__ __forceinline__ void store_group(float* d, const float* v, int np) {
    if (np == 4 && ((uintptr_t)d & 15) == 0) *reinterpret_cast<float4*>(d) = float4{v[0], v[1], v[2], v[3]};
    else {
        d[0] = v[0];
        if (np > 1) d[1] = v[1];
        if (np > 2) d[2] = v[2];
        if (np > 3) d[3] = v[3];
    }
}

__global__ __launch_bounds__(256) void train_example_u8_kernel(const unsigned char* __restrict__ img, const unsigned char* __restrict__ msk,
                                                               const int* __restrict__ flips, float* __restrict__ pix, float* __restrict__ cond,
                                                               float* __restrict__ mout, int batch, int h, int w, int normalize) {
    const int64_t gpr = (w + 3) / 4, total = (int64_t)batch * h * gpr, hw = (int64_t)h * w;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / gpr;                                    // b * h + y
        const int x0 = (int)(i - row * gpr) * 4;
        const int64_t b = row / h, y = row - b * h;
        const int np = w - x0 < 4 ? w - x0 : 4;
        const bool flip = flips != nullptr && flips[b] != 0;
        const int xs = flip ? w - x0 - np : x0;                         // first source column of the group
        const unsigned char* ip = img + (row * w + xs) * 3;
        const unsigned char* mp = msk + row * w + xs;
        unsigned px[12], m[4];                                          // in OUTPUT order
        if (np == 4 && ((uintptr_t)ip & 3) == 0 && ((uintptr_t)mp & 3) == 0) {
            unsigned s[12];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const unsigned v = reinterpret_cast<const unsigned*>(ip)[q];
                s[4 * q] = v & 0xff; s[4 * q + 1] = (v >> 8) & 0xff; s[4 * q + 2] = (v >> 16) & 0xff; s[4 * q + 3] = v >> 24;
            }
            const unsigned mv = reinterpret_cast<const unsigned*>(mp)[0];
            const unsigned sm[4] = {mv & 0xff, (mv >> 8) & 0xff, (mv >> 16) & 0xff, mv >> 24};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) px[3 * j + ch] = flip ? s[3 * (3 - j) + ch] : s[3 * j + ch];
                m[j] = flip ? sm[3 - j] : sm[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int sj = flip ? np - 1 - j : j;                   // source pixel of output pixel j within the group
                const bool in = j < np;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) px[3 * j + ch] = in ? ip[3 * sj + ch] : 0;
                m[j] = in ? mp[sj] : 0;
            }
        }
        float vm[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) vm[j] = __fdiv_rn((float)m[j], 255.0f);
        store_group(mout + b * hw + y * w + x0, vm, np);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float vp[4], vc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                vp[j] = px_value(px[3 * j + ch], normalize);
                vc[j] = px_value(m[j] == 255u ? 0u : px[3 * j + ch], normalize);      // get_masked_image(invert=True): only 255 blackens
            }
            const int64_t o = (b * 3 + ch) * hw + y * w + x0;
            store_group(pix + o, vp, np);
            store_group(cond + o, vc, np);
        }
    }
}

// get_masked_image on the bytes themselves (a caller-side helper: mf_train_example_u8 blackens while it converts)
__global__ __launch_bounds__(256) void masked_image_u8_kernel(const unsigned char* __restrict__ img, const unsigned char* __restrict__ msk,
                                                              unsigned char* __restrict__ out, int64_t pixels, int c, int invert) {
    const int64_t total = pixels * c;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const unsigned char m = msk[i / c];
        out[i] = (invert ? m == 255 : m == 0) ? (unsigned char)0 : img[i];
    }
}

// np.fliplr on [rows][w][c] fp32
__global__ __launch_bounds__(256) void fliplr_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t rows, int w, int c) {
    const int64_t rowlen = (int64_t)w * c, total = rows * rowlen;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / rowlen;
        const int k = (int)(i - r * rowlen);
        const int x = k / c, ch = k - x * c;
        dst[i] = src[r * rowlen + (int64_t)(w - 1 - x) * c + ch];
    }
}

// ---- mf_train_batch_assemble -----------------------------------------------------------------------------------------------------
struct AssembleArgs {
    const char *mom0, *mom1, *mom2, *mom3;          // image, conditioning image, depth ("latents"), normals ("latents"); 2 / 3 may be null
    const float *pn0, *pn1, *pn2, *pn3;             // their posterior noise [B][c][hw]
    const float *noise, *sa, *sb, *lw;
    const int64_t* ts;
    const float *masks, *depths, *normals;          // full-resolution planes [B][1 | 1 | 3][ph][pw]; depths / normals may be null
    float *lat, *noisy, *target, *cond, *tsf, *wout;
    int64_t ld;
    int dt, c, batch, h, w, T, ph, pw, vpred, ctot;
    float scaling;
};

// vae_sample_kernel's value: (mean + std * noise) * scaling with the product contracted into the sum, as the compiler does there
__device__ __forceinline__ float sample_z(const char* mom, int dt, int64_t ld, const float* pn, int c, int64_t hw, int64_t b, int ch, int64_t p,
                                          float scaling) {
    const int64_t row = (b * hw + p) * ld;
    const float mean = load_as_f32(mom, dt, row + ch);
    float logvar = load_as_f32(mom, dt, row + c + ch);
    logvar = fminf(fmaxf(logvar, -30.0f), 20.0f);                      // vae.py:776
    const float std = expf(0.5f * logvar);
    return __fmul_rn(__fmaf_rn(std, pn[(b * c + ch) * hw + p], mean), scaling);
}

// nearest_resize_kernel's rule
__device__ __forceinline__ float nearest_at(const float* plane, int ph, int pw, int y, int x, float sy, float sx) {
    int iy = (int)floorf((float)y * sy), ix = (int)floorf((float)x * sx);
    if (iy > ph - 1) iy = ph - 1;
    if (ix > pw - 1) ix = pw - 1;
    return plane[(int64_t)iy * pw + ix];
}

// One item per (image, channel slot, latent pixel): slots [0, c) are the latents (-> latents, noisy_latents, target), the next ctot
// are the channels of conditioning_latents in the script's order.  The pixel is the fastest index, so a wave writes 64 adjacent floats
// of one output plane; the slot is wave-uniform whenever hw is a multiple of 64.
__global__ __launch_bounds__(256) void train_batch_assemble_kernel(const AssembleArgs a) {
    const int64_t hw = (int64_t)a.h * a.w;
    const int slots = a.c + a.ctot;
    const int64_t total = (int64_t)a.batch * slots * hw;
    const float sy = (float)a.ph / (float)a.h, sx = (float)a.pw / (float)a.w;
    const int64_t phw = (int64_t)a.ph * a.pw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t p = i % hw, bs = i / hw;
        const int slot = (int)(bs % slots);
        const int64_t b = bs / slots;
        if (slot < a.c) {
            int64_t t = a.ts[b];
            t = t < 0 ? 0 : (t > a.T - 1 ? a.T - 1 : t);               // no input reads outside the tables
            const float sa = a.sa[t], sb = a.sb[t];
            const int64_t o = (b * a.c + slot) * hw + p;
            const float z = sample_z(a.mom0, a.dt, a.ld, a.pn0, a.c, hw, b, slot, p, a.scaling);
            const float e = a.noise[o];
            a.lat[o] = z;
            a.noisy[o] = __fmaf_rn(sb, e, __fmul_rn(sa, z));           // axpby_kernel: c0 * x0, then fma(c1, x1, .)
            a.target[o] = a.vpred ? __fmaf_rn(-sb, z, __fmul_rn(sa, e)) : e;
            if (slot == 0 && p == 0) {
                a.tsf[b] = (float)t;
                if (a.wout) a.wout[b] = a.lw[t];
            }
            continue;
        }
        int cc = slot - a.c;                                           // channel of conditioning_latents
        const int64_t o = (b * a.ctot + cc) * hw + p;
        const int y = (int)(p / a.w), x = (int)(p - (int64_t)y * a.w);
        float v;
        if (cc < a.c) v = sample_z(a.mom1, a.dt, a.ld, a.pn1, a.c, hw, b, cc, p, a.scaling);
        else if (cc == a.c) v = nearest_at(a.masks + b * phw, a.ph, a.pw, y, x, sy, sx);
        else {
            cc -= a.c + 1;
            const int nd = a.depths ? 1 : (a.mom2 ? a.c : 0);
            if (cc < nd) {
                v = a.depths ? nearest_at(a.depths + b * phw, a.ph, a.pw, y, x, sy, sx)
                             : sample_z(a.mom2, a.dt, a.ld, a.pn2, a.c, hw, b, cc, p, a.scaling);
            } else {
                cc -= nd;
                v = a.normals ? nearest_at(a.normals + (b * 3 + cc) * phw, a.ph, a.pw, y, x, sy, sx)
                              : sample_z(a.mom3, a.dt, a.ld, a.pn3, a.c, hw, b, cc, p, a.scaling);
            }
        }
        a.cond[o] = v;
    }
}

}  // namespace

extern "C" int mf_train_example_u8(const void* image_u8, const void* mask_u8, const int32_t* flips, float* pixel_values,
                                   float* conditioning_pixel_values, float* masks, int32_t batch, int32_t height, int32_t width,
                                   int32_t normalize, void* stream) {
    MF_CHECK_ARG(image_u8 && mask_u8 && pixel_values && conditioning_pixel_values && masks, "mf_train_example_u8: null pointer");
    MF_CHECK_ARG(batch >= 1 && height >= 1 && width >= 1, "mf_train_example_u8: batch %d, height %d, width %d must be positive", batch, height, width);
    MF_CHECK_ARG(normalize == 0 || normalize == 1, "mf_train_example_u8: normalize is 0 or 1, got %d", normalize);
    MF_CHECK_ARG((((uintptr_t)pixel_values | (uintptr_t)conditioning_pixel_values | (uintptr_t)masks) & 3) == 0,
                 "mf_train_example_u8: the outputs must be 4-byte aligned");
    hipLaunchKernelGGL(train_example_u8_kernel, dim3(tgrid((int64_t)batch * height * ((width + 3) / 4))), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)image_u8, (const unsigned char*)mask_u8, (const int*)flips, pixel_values, conditioning_pixel_values,
                       masks, batch, height, width, normalize);
    MF_CHECK_LAUNCH("mf_train_example_u8");
    return MF_OK;
}

extern "C" int mf_masked_image_u8(const void* image_u8, const void* mask_u8, void* out_u8, int64_t pixels, int32_t channels, int32_t invert,
                                  void* stream) {
    MF_CHECK_ARG(image_u8 && mask_u8 && out_u8, "mf_masked_image_u8: null pointer");
    MF_CHECK_ARG(pixels >= 1 && channels >= 1 && channels <= 4, "mf_masked_image_u8: %lld pixels of %d channels (1 .. 4)", (long long)pixels, channels);
    MF_CHECK_ARG(invert == 0 || invert == 1, "mf_masked_image_u8: invert is 0 or 1, got %d", invert);
    hipLaunchKernelGGL(masked_image_u8_kernel, dim3(tgrid(pixels * channels)), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)image_u8,
                       (const unsigned char*)mask_u8, (unsigned char*)out_u8, pixels, channels, invert);
    MF_CHECK_LAUNCH("mf_masked_image_u8");
    return MF_OK;
}

extern "C" int mf_fliplr(const float* src, float* dst, int64_t rows, int32_t width, int32_t channels, void* stream) {
    MF_CHECK_ARG(src && dst, "mf_fliplr: null pointer");
    MF_CHECK_ARG(src != dst, "mf_fliplr: not in place");
    MF_CHECK_ARG(rows >= 1 && width >= 1, "mf_fliplr: rows %lld and width %d must be positive", (long long)rows, width);
    MF_CHECK_ARG(channels == 1 || channels == 3, "mf_fliplr: 1 or 3 channels, got %d", channels);
    hipLaunchKernelGGL(fliplr_kernel, dim3(tgrid(rows * width * channels)), dim3(256), 0, (hipStream_t)stream, src, dst, rows, width, channels);
    MF_CHECK_LAUNCH("mf_fliplr");
    return MF_OK;
}

extern "C" int mf_train_batch_assemble(const void* const* moments, const float* const* posterior_noise, int32_t nsrc, int32_t m_dtype, int64_t ld,
                                       int32_t c, int32_t batch, int32_t h, int32_t w, float scaling, const float* noise,
                                       const int64_t* timesteps, const float* sqrt_alpha, const float* sqrt_one_minus_alpha,
                                       const float* loss_weight, int32_t T, const float* masks, const float* depths, const float* normals,
                                       int32_t plane_h, int32_t plane_w, int32_t prediction_type, float* latents, float* noisy_latents,
                                       float* target, float* conditioning_latents, float* timesteps_f32, float* loss_weights, void* stream) {
    MF_CHECK_ARG(moments && posterior_noise, "mf_train_batch_assemble: null source arrays");
    MF_CHECK_ARG(nsrc >= 2 && nsrc <= 4, "mf_train_batch_assemble: %d sources (2 .. 4: image, conditioning image, depth, normals)", nsrc);
    MF_CHECK_ARG(moments[0] && moments[1] && posterior_noise[0] && posterior_noise[1],
                 "mf_train_batch_assemble: null moments / posterior noise of the image or the conditioning image");
    for (int s = 2; s < nsrc; ++s)
        MF_CHECK_ARG((moments[s] != nullptr) == (posterior_noise[s] != nullptr),
                     "mf_train_batch_assemble: source %d needs both its moments and its posterior noise (or neither)", s);
    MF_CHECK_ARG(m_dtype == MF_F32 || m_dtype == MF_BF16 || m_dtype == MF_F16, "mf_train_batch_assemble: bad m_dtype %d", m_dtype);
    MF_CHECK_ARG(c > 0, "mf_train_batch_assemble: c = %d latent channels", c);
    MF_CHECK_ARG(ld >= 2 * (int64_t)c, "mf_train_batch_assemble: ld %lld < 2 c = %d", (long long)ld, 2 * c);
    MF_CHECK_ARG(batch >= 1 && h >= 1 && w >= 1 && plane_h >= 1 && plane_w >= 1,
                 "mf_train_batch_assemble: batch %d, latent %d x %d, planes %d x %d must be positive", batch, h, w, plane_h, plane_w);
    MF_CHECK_ARG(T > 0, "mf_train_batch_assemble: T = %d table entries", T);
    MF_CHECK_ARG(prediction_type == 0 || prediction_type == 1, "mf_train_batch_assemble: prediction_type %d (0 epsilon, 1 v)", prediction_type);
    MF_CHECK_ARG(noise && timesteps && sqrt_alpha && sqrt_one_minus_alpha && masks, "mf_train_batch_assemble: null input");
    MF_CHECK_ARG(latents && noisy_latents && target && conditioning_latents && timesteps_f32, "mf_train_batch_assemble: null output");
    MF_CHECK_ARG((loss_weight != nullptr) == (loss_weights != nullptr),
                 "mf_train_batch_assemble: the loss_weight table and the loss_weights output go together");
    const void* m2 = nsrc > 2 ? moments[2] : nullptr;
    const void* m3 = nsrc > 3 ? moments[3] : nullptr;
    MF_CHECK_ARG(!(m2 && depths), "mf_train_batch_assemble: depth comes as latents or as a plane, not both");
    MF_CHECK_ARG(!(m3 && normals), "mf_train_batch_assemble: normals come as latents or as planes, not both");
    AssembleArgs a;
    a.mom0 = (const char*)moments[0]; a.mom1 = (const char*)moments[1]; a.mom2 = (const char*)m2; a.mom3 = (const char*)m3;
    a.pn0 = posterior_noise[0]; a.pn1 = posterior_noise[1]; a.pn2 = m2 ? posterior_noise[2] : nullptr; a.pn3 = m3 ? posterior_noise[3] : nullptr;
    a.noise = noise; a.sa = sqrt_alpha; a.sb = sqrt_one_minus_alpha; a.lw = loss_weight; a.ts = timesteps;
    a.masks = masks; a.depths = depths; a.normals = normals;
    a.lat = latents; a.noisy = noisy_latents; a.target = target; a.cond = conditioning_latents; a.tsf = timesteps_f32; a.wout = loss_weights;
    a.ld = ld; a.dt = m_dtype; a.c = c; a.batch = batch; a.h = h; a.w = w; a.T = T; a.ph = plane_h; a.pw = plane_w; a.vpred = prediction_type;
    a.ctot = c + 1 + (depths ? 1 : (m2 ? c : 0)) + (normals ? 3 : (m3 ? c : 0));
    a.scaling = scaling;
    hipLaunchKernelGGL(train_batch_assemble_kernel, dim3(tgrid((int64_t)batch * (c + a.ctot) * h * w)), dim3(256), 0, (hipStream_t)stream, a);
    MF_CHECK_LAUNCH("mf_train_batch_assemble");
    return MF_OK;
}
