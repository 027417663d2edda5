// The library's own random numbers: a counter-based stream (Philox4x32-10, Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11), so that any element is a function of (seed, position) alone — no grid, device or world size enters, a C host and Python draw
// the same numbers, and a generator kept in device memory lets a captured graph draw fresh numbers at every replay.  include/mfhip.h
// states the stream; DESIGN.md section 6 says why it is not torch's.
//   what it replaces: torch.randn / torch.randint in utils/torch_utils.py randn_tensor, pipeline_brushnet.py:1186-1215 (the VAE posterior
//   noise) and train_brushnet_mirror.py:1351-1449 (posterior noise, noise, timesteps)
// One kernel serves every entry: a launch is up to six segments (one output each), an item is one Philox block = four outputs.
#include "mf_common.h"
#include "philox.h"        // the block function and the normal transform (shared with mf_sched_step_noise_dev)

#include <cstring>

namespace {

enum { KIND_BITS = 0, KIND_NORMAL = 1, KIND_INT = 2 };
constexpr int MAX_SEGS = 6;          // mf_train_batch_draw: four posterior noises, the noise, the timesteps

// One output of a launch: `samples` rows of `per` elements, row s drawn from the blocks that start at first_block +
// s * ceil(per / 4) past the generator's offset.  `skip` (rows == 1 only) starts the row at element `skip` of its stream: a rank's slice of a global integer draw.
struct Seg {
    void* out;
    int64_t begin;                   // first item of the launch that belongs to this segment
    int64_t per, bps, skip;
    uint64_t first_block;
    float scale;
    uint32_t T;                      // KIND_INT: T - 1 (so that T = 2^31 .. fits; the kernel adds the one back in 64 bits)
    int kind;
};

struct DrawArgs {
    Seg seg[MAX_SEGS];
    int nseg;
    int64_t total;
    uint64_t seed, offset;
    const uint64_t* state;           // device {seed, offset}: overrides the two host values (what a captured graph reads)
};

__global__ __launch_bounds__(256) void philox_draw_kernel(const DrawArgs a) {
    const uint64_t seed = a.state ? a.state[0] : a.seed, offset = a.state ? a.state[1] : a.offset;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
        // the item's segment: every field is picked with literal indices (a lane-dependent index would send the struct to scratch)
        char* out = (char*)a.seg[0].out;
        int64_t begin = 0, per = a.seg[0].per, bps = a.seg[0].bps, skip = a.seg[0].skip;
        uint64_t first_block = a.seg[0].first_block;
        float scale = a.seg[0].scale;
        uint32_t tm1 = a.seg[0].T;
        int kind = a.seg[0].kind;
#pragma unroll
        for (int k = 1; k < MAX_SEGS; ++k)
            if (k < a.nseg && i >= a.seg[k].begin) {
                out = (char*)a.seg[k].out; begin = a.seg[k].begin; per = a.seg[k].per; bps = a.seg[k].bps; skip = a.seg[k].skip;
                first_block = a.seg[k].first_block; scale = a.seg[k].scale; tm1 = a.seg[k].T; kind = a.seg[k].kind;
            }
        const int64_t item = i - begin;
        const int64_t s = item / bps, j = item - s * bps + skip / 4;           // row, block within the row's stream
        uint32_t x[4];
        philox_block(seed, offset + first_block + (uint64_t)s * (uint64_t)blocks_of(skip + per) + (uint64_t)j, x);
        // the block's elements [e0, e0 + 4) of the row's stream, of which [lo, hi) are inside [skip, skip + per)
        const int64_t e0 = j * 4;
        const int lo = skip > e0 ? (int)(skip - e0) : 0;
        const int hi = skip + per - e0 < 4 ? (int)(skip + per - e0) : 4;
        const int64_t d0 = s * per + e0 - skip;                                // output index of element e0 (negative only where lo > 0)
        const bool whole = lo == 0 && hi == 4;
        if (kind == KIND_NORMAL) {
            float z[4];
            box_muller(x[0], x[1], scale, z[0], z[1]);
            box_muller(x[2], x[3], scale, z[2], z[3]);
            float* d = (float*)out + d0;
            if (whole && ((uintptr_t)d & 15) == 0) *reinterpret_cast<float4*>(d) = float4{z[0], z[1], z[2], z[3]};
            else {
                if (lo <= 0 && hi > 0) d[0] = z[0];
                if (lo <= 1 && hi > 1) d[1] = z[1];
                if (lo <= 2 && hi > 2) d[2] = z[2];
                if (lo <= 3 && hi > 3) d[3] = z[3];
            }
        } else if (kind == KIND_INT) {
            // (x * T) >> 32: no rejection step, so a value's probability is off by at most T / 2^32 of the uniform one
            const uint64_t T = (uint64_t)tm1 + 1u;
            int64_t* d = (int64_t*)out + d0;
            if (whole && ((uintptr_t)d & 15) == 0) {
                reinterpret_cast<longlong2*>(d)[0] = longlong2{(long long)(((uint64_t)x[0] * T) >> 32), (long long)(((uint64_t)x[1] * T) >> 32)};
                reinterpret_cast<longlong2*>(d)[1] = longlong2{(long long)(((uint64_t)x[2] * T) >> 32), (long long)(((uint64_t)x[3] * T) >> 32)};
            } else {
                if (lo <= 0 && hi > 0) d[0] = (int64_t)(((uint64_t)x[0] * T) >> 32);
                if (lo <= 1 && hi > 1) d[1] = (int64_t)(((uint64_t)x[1] * T) >> 32);
                if (lo <= 2 && hi > 2) d[2] = (int64_t)(((uint64_t)x[2] * T) >> 32);
                if (lo <= 3 && hi > 3) d[3] = (int64_t)(((uint64_t)x[3] * T) >> 32);
            }
        } else {
            uint32_t* d = (uint32_t*)out + d0;
            if (whole && ((uintptr_t)d & 15) == 0) *reinterpret_cast<uint4*>(d) = uint4{x[0], x[1], x[2], x[3]};
            else {
                if (lo <= 0 && hi > 0) d[0] = x[0];
                if (lo <= 1 && hi > 1) d[1] = x[1];
                if (lo <= 2 && hi > 2) d[2] = x[2];
                if (lo <= 3 && hi > 3) d[3] = x[3];
            }
        }
    }
}

// The draws never write the state (all their blocks read it); this follows them on the same stream.
__global__ void philox_advance_kernel(uint64_t* state, uint64_t blocks) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[1] += blocks;
}

// The next segment of a launch under construction; returns the blocks the WHOLE draw (global_rows rows of stream_len elements) consumes.
// The kernel strides rows by blocks_of(skip + per), which is the stream's stride for a [samples, per] draw (skip = 0); a slice (skip > 0)
// has one row.
int64_t add_seg(DrawArgs& a, int kind, void* out, int64_t rows, int64_t per, int64_t skip, int64_t stream_len, int64_t first_row,
                int64_t global_rows, uint64_t base, float scale, int64_t T) {
    const int64_t row_blocks = blocks_of(stream_len);
    if (rows > 0 && per > 0) {
        Seg& g = a.seg[a.nseg++];
        g.out = out; g.begin = a.total; g.per = per; g.skip = skip; g.kind = kind; g.scale = scale; g.T = (uint32_t)(T - 1);
        g.bps = blocks_of(skip + per) - skip / 4;                              // items per row: the blocks that hold [skip, skip + per)
        g.first_block = base + (uint64_t)first_row * (uint64_t)row_blocks;
        a.total += rows * g.bps;
    }
    return global_rows * row_blocks;
}

int launch(DrawArgs& a, int64_t seed, int64_t offset, const uint64_t* state, void* stream, const char* name) {
    if (a.total == 0) return MF_OK;
    a.seed = (uint64_t)seed; a.offset = (uint64_t)offset; a.state = state;
    int64_t b = (a.total + 255) / 256;
    if (b > 8192) b = 8192;
    hipLaunchKernelGGL(philox_draw_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, a);
    MF_CHECK_LAUNCH(name);
    return MF_OK;
}

inline DrawArgs empty_args() {
    DrawArgs a;
    std::memset(&a, 0, sizeof(a));
    return a;
}

}  // namespace

extern "C" int64_t mf_philox_normal_blocks(int64_t samples, int64_t per_sample) {
    if (samples < 0 || per_sample < 0) {
        mf_set_error("mf_philox_normal_blocks: samples %lld and per_sample %lld must not be negative", (long long)samples, (long long)per_sample);
        return -1;
    }
    return samples * blocks_of(per_sample);
}

extern "C" int64_t mf_philox_int_blocks(int64_t n) {
    if (n < 0) {
        mf_set_error("mf_philox_int_blocks: n = %lld must not be negative", (long long)n);
        return -1;
    }
    return blocks_of(n);
}

extern "C" int mf_philox_bits_host(uint32_t* out, int64_t n, int64_t seed, int64_t offset) {
    MF_CHECK_ARG(out, "mf_philox_bits_host: null output");
    MF_CHECK_ARG(n >= 0, "mf_philox_bits_host: n = %lld must not be negative", (long long)n);
    for (int64_t b = 0; b < blocks_of(n); ++b) {
        uint32_t x[4];
        philox_block((uint64_t)seed, (uint64_t)offset + (uint64_t)b, x);
        for (int l = 0; l < 4 && 4 * b + l < n; ++l) out[4 * b + l] = x[l];
    }
    return MF_OK;
}

extern "C" int mf_philox_bits(uint32_t* out, int64_t n, int64_t seed, int64_t offset, const uint64_t* state, void* stream) {
    MF_CHECK_ARG(out, "mf_philox_bits: null output");
    MF_CHECK_ARG(n >= 0, "mf_philox_bits: n = %lld must not be negative", (long long)n);
    MF_CHECK_ARG(((uintptr_t)out & 3) == 0 && ((uintptr_t)state & 7) == 0, "mf_philox_bits: the output must be 4-byte, the state 8-byte aligned");
    DrawArgs a = empty_args();
    add_seg(a, KIND_BITS, out, 1, n, 0, n, 0, 1, 0, 1.0f, 1);
    return launch(a, seed, offset, state, stream, "mf_philox_bits");
}

extern "C" int mf_philox_normal(float* out, int64_t samples, int64_t per_sample, float scale, int64_t first_sample, int64_t global_batch,
                                int64_t seed, int64_t offset, const uint64_t* state, void* stream) {
    MF_CHECK_ARG(out, "mf_philox_normal: null output");
    MF_CHECK_ARG(samples >= 0 && per_sample >= 0 && first_sample >= 0,
                 "mf_philox_normal: samples %lld, per_sample %lld and first_sample %lld must not be negative", (long long)samples,
                 (long long)per_sample, (long long)first_sample);
    MF_CHECK_ARG(global_batch >= first_sample + samples, "mf_philox_normal: global_batch %lld < first_sample %lld + samples %lld",
                 (long long)global_batch, (long long)first_sample, (long long)samples);
    MF_CHECK_ARG(((uintptr_t)out & 3) == 0 && ((uintptr_t)state & 7) == 0, "mf_philox_normal: the output must be 4-byte, the state 8-byte aligned");
    DrawArgs a = empty_args();
    add_seg(a, KIND_NORMAL, out, samples, per_sample, 0, per_sample, first_sample, global_batch, 0, scale, 1);
    return launch(a, seed, offset, state, stream, "mf_philox_normal");
}

extern "C" int mf_philox_randint(int64_t* out, int64_t n, int64_t T, int64_t first, int64_t total, int64_t seed, int64_t offset,
                                 const uint64_t* state, void* stream) {
    MF_CHECK_ARG(out, "mf_philox_randint: null output");
    MF_CHECK_ARG(n >= 0 && first >= 0, "mf_philox_randint: n = %lld and first = %lld must not be negative", (long long)n, (long long)first);
    MF_CHECK_ARG(T > 0 && T <= ((int64_t)1 << 31), "mf_philox_randint: T = %lld outside (0, 2^31]", (long long)T);
    MF_CHECK_ARG(total >= first + n, "mf_philox_randint: total %lld < first %lld + n %lld", (long long)total, (long long)first, (long long)n);
    MF_CHECK_ARG(((uintptr_t)out & 7) == 0 && ((uintptr_t)state & 7) == 0, "mf_philox_randint: the output and the state must be 8-byte aligned");
    DrawArgs a = empty_args();
    add_seg(a, KIND_INT, out, 1, n, first, total, 0, 1, 0, 1.0f, T);
    return launch(a, seed, offset, state, stream, "mf_philox_randint");
}

extern "C" int mf_philox_advance(uint64_t* state, int64_t blocks, void* stream) {
    MF_CHECK_ARG(state, "mf_philox_advance: null state");
    MF_CHECK_ARG(blocks >= 0, "mf_philox_advance: blocks = %lld must not be negative", (long long)blocks);
    MF_CHECK_ARG(((uintptr_t)state & 7) == 0, "mf_philox_advance: the state must be 8-byte aligned");
    hipLaunchKernelGGL(philox_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, (uint64_t)blocks);
    MF_CHECK_LAUNCH("mf_philox_advance");
    return MF_OK;
}

extern "C" int mf_train_batch_draw(float* const* posterior_noise, int32_t nsrc, float* noise, int64_t* timesteps, int64_t samples,
                                   int64_t per_sample, int64_t T, int64_t first_sample, int64_t global_batch, int64_t seed, int64_t offset,
                                   const uint64_t* state, void* stream) {
    MF_CHECK_ARG(posterior_noise && noise && timesteps, "mf_train_batch_draw: null output");
    MF_CHECK_ARG(nsrc >= 2 && nsrc <= 4, "mf_train_batch_draw: %d sources (2 .. 4: image, conditioning image, depth, normals)", nsrc);
    MF_CHECK_ARG(posterior_noise[0] && posterior_noise[1], "mf_train_batch_draw: null output for the image's or the conditioning image's posterior noise");
    MF_CHECK_ARG(samples >= 0 && per_sample >= 0 && first_sample >= 0,
                 "mf_train_batch_draw: samples %lld, per_sample %lld and first_sample %lld must not be negative", (long long)samples,
                 (long long)per_sample, (long long)first_sample);
    MF_CHECK_ARG(T > 0 && T <= ((int64_t)1 << 31), "mf_train_batch_draw: T = %lld outside (0, 2^31]", (long long)T);
    MF_CHECK_ARG(global_batch >= first_sample + samples, "mf_train_batch_draw: global_batch %lld < first_sample %lld + samples %lld",
                 (long long)global_batch, (long long)first_sample, (long long)samples);
    uintptr_t align = (uintptr_t)noise;
    for (int s = 0; s < nsrc; ++s) align |= (uintptr_t)posterior_noise[s];
    MF_CHECK_ARG((align & 3) == 0 && (((uintptr_t)timesteps | (uintptr_t)state) & 7) == 0,
                 "mf_train_batch_draw: fp32 outputs must be 4-byte, the timesteps and the state 8-byte aligned");
    DrawArgs a = empty_args();
    uint64_t base = 0;
    for (int s = 0; s < nsrc; ++s)
        if (posterior_noise[s])
            base += (uint64_t)add_seg(a, KIND_NORMAL, posterior_noise[s], samples, per_sample, 0, per_sample, first_sample, global_batch, base, 1.0f, 1);
    base += (uint64_t)add_seg(a, KIND_NORMAL, noise, samples, per_sample, 0, per_sample, first_sample, global_batch, base, 1.0f, 1);
    base += (uint64_t)add_seg(a, KIND_INT, timesteps, 1, samples, first_sample, global_batch, 0, 1, base, 1.0f, T);
    return launch(a, seed, offset, state, stream, "mf_train_batch_draw");
}
