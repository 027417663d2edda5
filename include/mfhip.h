/*
 * mfhip.h — C ABI of libmfhip.so, the MI355X (gfx950) kernel library behind the
 * MirrorFusion (SD1.5 + BrushNet) denoising hot path.
 *
 * The reference (val-iisc/Reflecting-Reality, MirrorFusion/src/diffusers) is 100 % Python and has
 * no native operator boundary; every arithmetic step is an ATen call.  Each entry point below
 * therefore cites the reference *call site* it replaces (paths relative to
 * MirrorFusion/src/diffusers/).  All entry points:
 *   - are extern "C", take plain pointers / sizes / a hipStream_t (passed as void*),
 *   - never allocate, free, synchronise or retain caller memory (graph-capture safe),
 *   - return 0 on success, a negative MF_E* code otherwise; mf_last_error() gives the text.
 * Device buffers are owned by the caller (PyTorch-ROCm allocates them).
 *
 * Layout conventions: activations are NHWC ("pixel-major": [batch][y][x][channel]) which is
 * bit-identical to the [batch][tokens][channels] layout of the transformer blocks, so no
 * transposes exist between conv and attention.  Weights are [N][K] with K contiguous
 * (conv: [Cout][ky][kx][Cin]).  dtype codes: MF_F32 = 0, MF_BF16 = 1.
 *
 * ABI 23 adds the reference's 'ip_adapter' normals mode (examples/brushnet/train_brushnet_mirror.py:752-756, 858-888): decoupled
 * cross-attention in one launch (mf_attention_ip_bf16 / _f16 / _f16x3), the frequency encoder of the mirror normal (mf_freq_encode)
 * and the mean normal over the mirror mask (mf_masked_mean_normal).  These entries are not part of step programs.
 *
 * Appended since (no struct changed, so the version stays 23): mf_u8_to_planes (uint8 NHWC pixels -> fp32 NCHW planes in [0, 1], the
 * ingest of a host that decoded an image file) and the step-level entries mf_encode_prompt / mf_build_conditioning / mf_decode_image,
 * which with mf_denoise_step_fused run a whole inpainting call from step programs: token ids, pixels, mask and depth in, a uint8
 * image out (examples/c_host/inpaint_host.c); and the training batch (csrc/train_batch.hip): mf_train_example_u8, mf_masked_image_u8,
 * mf_fliplr, mf_train_batch_assemble; and the two ends of a tile of the tiled VAE (csrc/vae_tile.hip): mf_crop_pack_nhwc,
 * mf_vae_tile_blend.
 */
#ifndef MFHIP_H
#define MFHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MF_F32 0
#define MF_BF16 1
/* compute-only codes for mf_gemm_desc.dtype ("split" precision: the mode that meets the reference's fp32 results to
 * 1e-3 on the latents AND runs on the 16-bit matrix pipe).  Operands are fp32 in memory; every value x is split into
 * two 16-bit halves x = hi + lo (hi = x rounded toward zero to 11 / 8 significant bits, lo = x - hi, exact in fp32,
 * rounded to 16 bits) and a product is three MFMAs: hi*hi + hi*lo + lo*hi, fp32 accumulate.  MF_F16X3: fp16 halves
 * (22 significant bits, |x| < 65504); MF_BF16X3: bf16 halves (16 bits, fp32 range). */
#define MF_F16X3 2
#define MF_BF16X3 3
/* OCP fp8 e4m3 operands (1 byte each, a_dtype == MF_FP8 too) on the block-scaled matrix instruction
 * v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales (2x the bf16 MFMA rate); the quantisation scales are
 * per A row / per W row fp32 vectors applied in the epilogue (mf_gemm_desc.a_scale / w_scale) */
#define MF_FP8 4
/* fp32 operands in memory (a_dtype == MF_F32, raw fp32 W), each rounded to bf16 (nearest-even) on its way into ONE bf16
 * MFMA, fp32 accumulate: the arithmetic of the reference's --mixed_precision=bf16 autocast (train_brushnet_mirror.py:567,
 * 1127-1131) with the activations still stored in fp32.  Training compute code (mf_gemm_conv, mf_conv_wgrad). */
#define MF_BF16X1 5
/* fp16 operands and activation storage (torch.float16: the default of the reference's inference script,
 * examples/brushnet/test_brushnet.py:122-126), one v_mfma_f32_*_f16 per product at the bf16 rate, fp32 accumulate / statistics.
 * Storage AND compute code: the byte layout of every tensor equals the MF_BF16 one.  11 significant bits against bf16's 8, range
 * |x| < 65504 (a value beyond it becomes inf, as in the reference's fp16 run). */
#define MF_F16 6

#define MF_OK 0
#define MF_EINVAL (-1)   /* bad argument / unsupported shape */
#define MF_ELAUNCH (-2)  /* hipLaunch failed */
#define MF_EALIGN (-3)   /* pointer / stride alignment not met */

#define MF_ACT_NONE 0
#define MF_ACT_SILU 1
/* GEGLU fused into the GEMM: weight rows interleaved [4 value rows | 4 gate rows]; writes n/2 channels */
#define MF_ACT_GEGLU4 2

/* ABI version, bumped on any struct change; checked by the Python host at load time. */
#define MF_ABI_VERSION 23
int mf_abi_version(void);
const char* mf_last_error(void);
/* sizeof() of the descriptor structs, so a foreign-language binding can verify its layout */
int mf_sizeof_gemm_desc(void);
int mf_sizeof_groupnorm_desc(void);

/* --------------------------------------------------------------------------------------------
 * mf_gemm_conv — implicit-GEMM convolution / linear / strided-batched NT GEMM on MFMA.
 *
 *   out[z][m][n] = alpha * ( sum_k A[z][m][k] * W[z][n][k] + bias + temb[b(m)][n] )
 *                  + res0[m][n] + res1[m][n]              (then optional activation)
 *
 * A is gathered on the fly from up to two NHWC tensors concatenated along channels
 * (torch.cat([h, skip], 1) is never materialised), optionally through a nearest-2x upsample,
 * with zero padding; k = (ky*kw + kx)*(c0+c1) + c.
 *
 * Replaces: LoRACompatibleConv/F.conv2d (models/lora.py:293-366; call sites resnet.py:278,294,
 * 320-327, downsampling.py:118-120,134-154, upsampling.py:170-191, brushnet.py:221,325-447,
 * transformer_2d.py:162,225, unet_2d_condition.py conv_in/conv_out), LoRACompatibleLinear/F.linear
 * (lora.py:368-451; attention_processor.py:190-205, activations.py:92, attention.py:663,
 * resnet.py:282, embeddings.py:225-237), torch.cat (unet_2d_blocks.py:2586,2728), the injection
 * adds (unet_2d_blocks.py:1389,1398,1484,1493,2627,2635,2752,2761; unet_2d_condition.py:1218,1289)
 * and, in batched form, the QK^T / PV products of attention_processor.py:577-622.
 * ------------------------------------------------------------------------------------------ */
typedef struct mf_gemm_desc {
    /* compute dtype: MF_BF16 (bf16 MFMA 32x32x16, fp32 accumulate), MF_F32 (fp32 MFMA 32x32x2) or a split code
     * MF_F16X3 / MF_BF16X3 (fp32 operands, three 16-bit MFMAs per product; a_dtype must be MF_F32), MF_BF16X1 (fp32
     * operands, one bf16 MFMA per product; raw W only) */
    int32_t dtype;
    /* A operand */
    const void* a0;       /* segment 0, NHWC */
    const void* a1;       /* segment 1 or NULL */
    int32_t c0, c1;       /* channels per segment (c1 = 0 when a1 is NULL) */
    int64_t lda0, lda1;   /* pixel stride of each segment, in elements (>= c) */
    int32_t a_dtype;      /* storage dtype of a0/a1: == dtype, or MF_F32 with dtype == MF_BF16 */
    int32_t batch, h_in, w_in;  /* input geometry (before upsample) */
    int32_t h_out, w_out;
    int32_t kh, kw, stride, pad_t, pad_l;
    int32_t upsample;     /* 1: nearest-neighbour 2x before the convolution */
    /* W operand, [n][k] row-major, row stride ldw elements, dtype == dtype (fp32 for the split codes).
     * w_split = 1 (split codes only): W was split ahead of time — per block of 32 k the row holds the 32 high halves
     * then the 32 low halves (16-bit each: the same 128 bytes as 32 floats), rows zero-padded to a multiple of 32 k,
     * ldw counted in 4-byte units.  w_split = 0: raw fp32, split on the fly (activation x activation products). */
    const void* w;
    int64_t ldw;
    int32_t w_split;
    int32_t n;            /* output channels */
    /* strided batching (attention): blockIdx.z = z, offset = (z / zdiv)*zs_o + (z % zdiv)*zs_i */
    int32_t nz, zdiv;
    int64_t a_zs_o, a_zs_i, w_zs_o, w_zs_i, o_zs_o, o_zs_i;
    /* epilogue */
    const float* bias;    /* [n] (bias_mode 0) or [m] (bias_mode 1) or NULL */
    int32_t bias_mode;
    const float* temb;    /* [batch][ld_temb] fp32 or NULL; row = m / (h_out*w_out) */
    int64_t ld_temb;
    /* out = alpha * (a_scale[m] * w_scale[n] * acc + bias + temb) + ... : dequantisation of fp8 operands (either may be
     * NULL = 1; usable with any dtype).  Batched calls: vector z starts at a_scale + (z / zdiv) * a_scale_zs (w alike) */
    const float* a_scale; const float* w_scale;
    int64_t a_scale_zs, w_scale_zs;
    const void* res0; int32_t res0_dtype; int64_t ld_res0;
    const void* res1; int32_t res1_dtype; int64_t ld_res1;
    /* 0 (or >= M): res1 has one row per output row.  0 < res1_rows < M (must divide M): res1 has res1_rows rows and output
     * row m adds row m % res1_rows — one residual shared by batch replicas (the BrushNet residual of both halves of a
     * classifier-free-guidance batch: pipeline_brushnet.py:1256-1296 feeds an attention-free BrushNet the same inputs twice) */
    int32_t res1_rows;
    float alpha;
    int32_t act;
    void* out; int32_t out_dtype; int64_t ldc;
    /* split-K: 0 = library heuristic (uses `ws` when it is large enough), 1 = off, >1 = forced;
     * `ws` is a caller-owned scratch of `ws_floats` floats (splitk*nz*M*N are needed) */
    int32_t splitk;
    float* ws;
    int64_t ws_floats;
    /* tile selection: 0 = library heuristic, else an index into the instantiated tile table (mf_gemm_num_tiles).
     * 1-15: implicit-GEMM tiles (any call); 16-19: 3x3 / stride-1 kernels with the input patch resident in LDS (bf16,
     * image sizes that tile by 8x16 / 16x16); 20-24: implicit GEMM with dx-tap reuse of the A window (3x3 / stride 1,
     * W divides or is divided by BM); 25-30: 16x16x32-MFMA forms (bf16); 31-36: deeper LDS rings; 37-40, 47: warp-specialised
     * dx-reuse convs (bf16: extra waves that only stage operands); 41-46, 48: the warp-specialised form of the plain ring
     * (bf16, any call; the only tiles that serve ln_colsum / vt_out).  A tile that does not apply to the call returns MF_EINVAL (the host autotuner skips it); nothing
     * is silently rerouted. */
    int32_t tile;
    /* LayerNorm folded into the GEMM (attention.py:203,233,261 -> the Linear that follows): ln_colsum[n] = sum_k W[n][k] of the
     * weight handed in, which the caller has already multiplied by the norm's gamma (and whose bias already holds W.beta):
     *   out = rstd[m] * (acc[m][n] - mean[m] * ln_colsum[n]) + bias ...  with mean / rstd of A row m over all K (eps = ln_eps),
     * gathered inside the kernel while the A tiles pass through LDS — the normalised tensor is never written.  bf16 1x1 GEMMs
     * with one A segment and no split-K; served by the warp-specialised ring tiles (41-46, 48).  NULL = off. */
    const float* ln_colsum; float ln_eps;
    /* Transposed output columns (a fused q | k | v projection whose V third attention wants as V^T): columns n >= vt_n0 are not
     * written to `out` but as vt_out[image][n - vt_n0][token] (bf16, row stride vt_ld elements), image = m / vt_tokens,
     * token = m % vt_tokens.  vt_n0 must be a multiple of 640; same tiles as ln_colsum.  NULL = off. */
    void* vt_out; int32_t vt_n0, vt_tokens; int64_t vt_ld;
    /* In-launch split-K combine: sk_tickets = `sk_ticket_cap` 32-bit arrival counters owned by the caller, ALL ZERO when the call
     * is issued (the kernel leaves them zero again; one buffer per stream, like `ws`).  With split-K > 1 and at most
     * sk_ticket_cap output tiles, the K-slice block that arrives last at its tile's counter sums the tile's fp32 slabs in slice
     * order (bit-reproducible) and runs the epilogue itself: the separate reduce launch and the kernel boundary behind the
     * dirty partials disappear.  Built into the tiles small-M / deep-K calls use (1, 2, 3, 6 and the warp-specialised rings 41,
     * 43, 44, 48 in bf16; 1, 2, 3, 6, 41, 44 in MF_F16X3); any other tile, or NULL, keeps the reduce launch — same result. */
    uint32_t* sk_tickets; int32_t sk_ticket_cap;
    /* GroupNorm statistics from the producer (round 6; resnet.py:337-338,381,393, transformer_2d.py:158: every GroupNorm of the
     * path reads the output of one of these launches).  gn_part != NULL: besides `out`, the call leaves per-channel partial sums
     * of the FINAL output values (after bias / temb / residuals / activation; fp32, taken before the storage rounding when the
     * epilogue produces them) in gn_part as float pairs
     *     gn_part[(m / R) * n_channels + n] = (sum, sum of squares) over output rows [R * (m / R), R * (m / R) + R) of channel n,
     * and writes R (> 0, a divisor of h_out * w_out, so a block of rows lies inside one image) to *gn_part_rows (a HOST int).
     * mf_groupnorm takes (gn_part, R) as part0 / part1 and skips its statistics pass over the tensor.  Produced inside the GEMM's
     * epilogue (R = the tile's rows; fixed summation order, bit-reproducible) when the launch has no split-K reduce and the tile
     * is an implicit-GEMM tile with h_out * w_out a multiple of its rows; otherwise by one extra column-sum launch over the
     * stored output (R = 128, 64 or 32) — same contract.  Needs n % 8 == 0, nz == 1, h_out * w_out % 32 == 0, no GEGLU, no
     * vt_out, and gn_part_floats >= 2 * n * (M / 32) (enough for the smallest R).
     * Conditioning of the format: the sums are fp32 and UNSHIFTED, so the variance a consumer forms from them, sum x^2 - (sum x)^2 / n,
     * loses digits as |mean| / std of a group grows, whatever precision the consumer combines them in.  Measured with an fp32 output at
     * 640 channels x 1024 rows in blocks of 128 rows (tests/test_norm_conditioning_gpu.py): from the per-channel sums the normalised
     * values stay inside the suite's fp32 bound (1e-4 + 2e-5 |y|, or 4 x torch's fp32 error) up to |mean| / std = 30 and leave it at
     * 100 (7e-4, 19 x torch's fp32 error); from the per-group sums below they stay inside up to 10 and leave it at 30 (4e-4).  mf_groupnorm's
     * own statistics pass (part0 == NULL) accumulates x - pivot and has no such limit. */
    float* gn_part; int64_t gn_part_floats; int32_t* gn_part_rows;
    /* gn_groups > 0 (with gn_part): the consumer is a GroupNorm over exactly this tensor with gn_groups groups (the common case: every
     * norm of the path but the decoder's concatenated ones).  When the epilogue produces the sums and the tile's columns hold whole
     * groups (n / gn_groups divides the tile's column count: the 160-column tiles for 320 / 640 / 1280 channels in 32 groups), it also
     * leaves PER-GROUP sums behind the per-channel ones,
     *     gn_part[2 * n * (M / R) + 2 * ((m / R) * gn_groups + g)] = (sum, sum of squares) over rows [R (m / R), +R) of group g,
     * and writes 1 to *gn_grouped (a HOST int, else 0): mf_groupnorm then needs no finalize launch at all (grp0 below). */
    int32_t gn_groups; int32_t* gn_grouped;
    /* Split-K reduce left to the consumer (round 6, ABI 20).  The 8 x 8 / 16 x 16 levels run their 3x3 convs with split-K (M = 512 / 2048
     * rows cannot fill 256 CUs otherwise); the first conv of a ResnetBlock2D feeds nothing but norm2 (resnet.py:381-393), so the launch that
     * sums the K slices can be the GroupNorm itself.  defer_reduce != 0: when this call ends with split-K slabs in `ws` and an epilogue of
     * bias (per column) / temb / alpha only — no residual, activation, scales, folded LayerNorm, vt_out, gn_part; nz == 1; the 8-channel
     * vector form — the reduce launch is SKIPPED, `out` is NOT written and *deferred_splits (a HOST int) receives the number of slabs
     * [split][M][n] fp32 in ws; mf_groupnorm takes them as sk_ws (below) and must be the next user of `ws` on this stream.  Otherwise
     * *deferred_splits = 0 and the call is complete as always. */
    int32_t defer_reduce; int32_t* deferred_splits;
} mf_gemm_desc;

int mf_gemm_conv(const mf_gemm_desc* d, void* stream);
/* What mf_gemm_conv would do with a descriptor, decided on the host: mf_gemm_conv is this plan followed by its launches.
 * mf_gemm_conv_plan makes every check and every choice of the call (same return code, same mf_last_error text), launches nothing,
 * needs no GPU and reads neither device memory nor the descriptor's host out-pointers (gn_part_rows, gn_grouped, deferred_splits:
 * only their null-ness counts).  The one refusal left to the launch is "tile not instantiated for this dtype". */
typedef struct mf_gemm_plan {
    int32_t tile;               /* the resolved tile (descriptor's, tuned by the caller, or the library heuristic) */
    int32_t splitk;             /* K slices after "no empty splits" (1 = none) */
    int32_t tiles_per_block;    /* output tiles a block of the persistent tiles 69 / 70 walks; 1 elsewhere */
    int32_t blocks;             /* blocks of the main launch */
    int32_t reduce_launch;      /* 1: a separate split-K reduce launch follows the main one */
    int32_t deferred_splits;    /* what *deferred_splits receives (0: the call completes `out` itself) */
    int32_t gn_part_rows;       /* what *gn_part_rows receives (0 without gn_part) */
    int32_t gn_grouped;         /* what *gn_grouped receives */
} mf_gemm_plan;
int mf_gemm_conv_plan(const mf_gemm_desc* d, mf_gemm_plan* out);
int mf_sizeof_gemm_plan(void);
/* The 3x3 / padding 1 convolution over a nearest-2x upsampled image (the UNet / BrushNet upsamplers: mf_gemm_desc.upsample = 1) as
 * FOUR 2x2 convolutions over the low-resolution image, one per output phase (py, px), in one launch: output pixel (2y + py, 2x + px)
 * reads only the 2x2 low-resolution window that starts at (y - 1 + py, x - 1 + px), with the 3x3 taps that land on the same pixel
 * summed (rows: py = 0 -> {ky0}, {ky1 + ky2}; py = 1 -> {ky0 + ky1}, {ky2}; columns alike) — 4/9 of the multiply-adds, and the zero
 * padding of the upsampled image is the zero padding of the low-resolution one, so the borders are exact.  The descriptor struct is
 * mf_gemm_desc, unchanged, read as follows:
 *   h_in, w_in: the LOW-resolution geometry; h_out = 2 h_in, w_out = 2 w_in; kh = kw = 2, stride = 1, upsample = 1; one A segment
 *   (a1 NULL, c1 0), dtype MF_BF16 / MF_F16 with a_dtype = dtype.
 *   w: four weight matrices [n][ldw >= 4 c0] with k = (ty * 2 + tx) * c0 + c over the window's taps; phase p = 2 py + px starts at
 *   w + p * w_zs_o elements.
 *   out / ldc / out_dtype, res0, res1 (res1_rows counted in OUTPUT rows), bias, alpha, act (none / SiLU), gn_part (+ gn_groups and the
 *   host out-fields) mean what they mean to mf_gemm_conv, over the full-resolution output of 4 * batch * h_in * w_in rows.  The partial
 *   sums of gn_part cover R output rows each and an output image's partial rows are contiguous, which is all mf_groupnorm's part0
 *   asks: (image, phase, block of R low-resolution rows) with R = the tile's rows when the epilogue makes them (no split-K,
 *   h_in * w_in a multiple of the tile's rows), blocks of R consecutive output rows otherwise.
 *   tile: 0 or one of 42 / 43 / 48; splitk: 0 / 1 or a forced count (ws holds splitk full-resolution slabs, summed by a reduce launch).
 *   nz > 1, temb, ln_colsum, vt_out, MF_ACT_GEGLU4, a second segment, scales, bias_mode 1 and defer_reduce: MF_EINVAL, nothing written.
 * mf_conv_up2x_plan: the same checks and choices on the host, nothing launched (as mf_gemm_conv_plan is to mf_gemm_conv).
 * (appended; MF_ABI_VERSION stays 23: no existing entry or struct changed) */
int mf_conv_up2x(const mf_gemm_desc* d, void* stream);
int mf_conv_up2x_plan(const mf_gemm_desc* d, mf_gemm_plan* out);
/* number of instantiated tile configurations and their (BM, BN) */
int mf_gemm_num_tiles(void);
int mf_gemm_tile_shape(int tile, int* bm, int* bn);
/* bumped whenever tile indices are renumbered or change meaning (appending tiles keeps it): a host-side cache of tuned
 * tile indices is only valid for the version it was recorded under */
int mf_gemm_tile_table_version(void);

/* --------------------------------------------------------------------------------------------
 * mf_groupnorm — GroupNorm over NHWC (optionally over the channel-concat of two tensors),
 * fused with SiLU.  Replaces torch.nn.GroupNorm + SiLU (resnet.py:337-338,381,393;
 * transformer_2d.py:158,338; unet_2d_condition.py:1336-1338; vae.py; attention_processor.py:1244).
 * `ws` is a scratch buffer of mf_groupnorm_ws_floats(batch, groups, c0 + c1) floats.
 * ------------------------------------------------------------------------------------------ */
typedef struct mf_groupnorm_desc {
    const void* x0; const void* x1;   /* NHWC segments; x1 may be NULL */
    int32_t c0, c1;
    int32_t in_dtype;                 /* MF_F32 / MF_BF16 */
    int32_t batch, hw;                /* hw = H*W */
    int32_t groups;
    float eps;
    const float* gamma; const float* beta;   /* [c0+c1] fp32 */
    int32_t silu;                     /* 1: y = silu(gn(x)) */
    void* out; int32_t out_dtype;     /* [batch][hw][c0+c1] */
    float* ws;
    float* stats_out;                 /* nullable [batch][groups][2]: (mean, rstd) of every group, for mf_groupnorm_bwd's stats_in */
    /* Statistics handed over by the producer(s) of x0 / x1 (mf_gemm_desc.gn_part and the R it reported): per-channel (sum, sum of
     * squares) of every block of part_rows rows.  When every present segment has its partials (and hw > 256: below that the
     * one-launch form keeps the rows in registers anyway) the statistics pass over the tensor is replaced by a small finalize
     * launch over the partials; otherwise they are ignored.  NULL = compute the statistics from the tensor. */
    const float* part0; int32_t part0_rows;
    const float* part1; int32_t part1_rows;
    /* Per-GROUP sums of x0 from its producer (mf_gemm_desc.gn_groups == groups, *gn_grouped == 1): float pairs [batch * hw / grp0_rows]
     * [groups].  One segment only (x1 == NULL), at most 64 row blocks per image: every block of the apply pass combines its image's
     * blocks itself (fixed order, double) and the normalisation is ONE launch. */
    const float* grp0; int32_t grp0_rows;
    /* The input as a deferred split-K reduce (mf_gemm_desc.defer_reduce): x = round(((sum over sk_splits slabs of sk_ws[split][row][c])
     * + sk_bias[c] + sk_temb[image * sk_ld_temb + c]) * sk_alpha), summed in slab order and rounded to in_dtype — bit for bit what the
     * reduce launch would have stored — instead of reading x0 (ignored; c1 must be 0).  Only where the one-launch form applies
     * (hw <= 256, channels % 8 == 0: the levels that split K); refused otherwise.  sk_bias / sk_temb nullable. */
    const float* sk_ws; int32_t sk_splits;
    const float* sk_bias; const float* sk_temb; int64_t sk_ld_temb; float sk_alpha;
} mf_groupnorm_desc;
int mf_groupnorm(const mf_groupnorm_desc* d, void* stream);
int64_t mf_groupnorm_ws_floats(int32_t batch, int32_t groups, int32_t channels);
/* 1 when the shape of [*, hw, channels] in `groups` groups (one segment) fits mf_groupnorm's one-launch slab form, the form sk_ws needs;
 * the pointer alignments the form also asks for are checked by mf_groupnorm itself.  No GPU needed. */
int mf_groupnorm_slab_applies(int32_t hw, int32_t channels, int32_t groups);
/* What mf_groupnorm would do with a descriptor, decided on the host: mf_groupnorm is this plan followed by its launches.
 * mf_groupnorm_plan makes every check and every choice of the call (same return code, same mf_last_error text), launches nothing,
 * needs no GPU and reads nothing behind the descriptor's pointers (only their null-ness and 16-byte alignment count).
 * (appended; MF_ABI_VERSION stays 23: no existing entry or struct changed) */
typedef struct mf_gn_plan {
    int32_t form;               /* 0 one-launch slab; 1 own statistics pass; 2 producer's per-channel sums (part0 / part1); 3 producer's
                                 * per-group sums (grp0) */
    int32_t launches;           /* kernels the call issues: 1..3 */
    int32_t vec;                /* channels per thread vector: 8 or 4 */
    int32_t finalize;           /* who turns the statistics into (mean, rstd): 0 a finalize launch, 1 every apply block combines the
                                 * chunks, 2 every apply block combines the producer's group sums; 0 for the slab */
    int32_t centered;           /* 1: an fp32 output is formed around the group's mean carried as two floats; 0 for the slab */
    int32_t chunks, rows_per_chunk;     /* of the statistics pass (they place the statistics in ws for forms 1-3); 0 for the slab */
    int32_t rows_per_block;     /* apply pass: rows per block; slab: rows of an image in flight per slab */
    int32_t blocks, threads;    /* of the last launch (the apply pass, or the slab) */
    int32_t lds_bytes;          /* largest dynamic LDS request of any launch of the plan */
    int32_t finalize_parts;     /* form 2: threads per channel of the finalize launch; else 0 */
} mf_gn_plan;
int mf_groupnorm_plan(const mf_groupnorm_desc* d, mf_gn_plan* out);
int mf_sizeof_gn_plan(void);

/* LayerNorm over the last dim of [rows][c]; replaces nn.LayerNorm (attention.py:203,233,261). */
int mf_layernorm(const void* x, int32_t in_dtype, void* out, int32_t out_dtype, const float* gamma,
                 const float* beta, int64_t rows, int32_t c, float eps, void* stream);

/* Row softmax in place over scores[rows][ld] (fp32), valid length `cols`; columns in
 * [cols, ld) are written as 0 so the buffer can feed a K-padded GEMM.  Writes P in `out`
 * ([rows][ld], out_dtype).  Replaces attention_probs.softmax(dim=-1) (attention_processor.py:616). */
int mf_softmax_rows(const float* scores, void* out, int32_t out_dtype, int64_t rows, int32_t cols,
                    int32_t ld, void* stream);

/* mf_softmax_rows under a causal mask (the fp32 mode of the CLIP text encoders, modeling_clip's causal_attention_mask): the rows are
 * [batch * heads][sq] queries, row r keeps columns 0 .. r % sq and everything past them is written as 0.  sq == cols. */
int mf_softmax_rows_causal(const float* scores, void* out, int32_t out_dtype, int64_t rows, int32_t cols,
                           int32_t ld, int32_t sq, void* stream);

/* Fused flash-style attention (bf16): out[b][s][h*d + :] = softmax(q k^T * scale) v.
 * q: [B][Sq][ldq], k: [B][Skv][ldk], vt: V^T as [B][heads*d][ldvt] (keys contiguous),
 * replaces F.scaled_dot_product_attention (attention_processor.py:1266-1268).
 *
 * Memory past skv.  Keys are processed in tiles of 64, and the last tile is loaded whole:
 *   - k: rows skv .. 64 * ceil(skv / 64) - 1 of batch b are the first rows of batch b + 1; behind the last batch, rows past the
 *     B * Skv * ldk elements of the tensor are never read (they count as zeros).  Their scores are overwritten with -inf before the
 *     softmax, so these rows may hold ANY bit pattern, NaN and inf included: they never reach the result.
 *   - vt: columns skv .. 64 * ceil(skv / 64) - 1 of every row — the pad columns up to ldvt and, where ldvt is shorter than the
 *     tile, the start of the next row — are multiplied by probabilities that are exactly zero.  They must be FINITE (0 * inf and
 *     0 * NaN are NaN, in every output channel of the query); any finite value, however large, leaves the result unchanged.  Behind
 *     the last row nothing past the B * heads * d * ldvt elements is read.
 * The same holds for every mf_attention_* entry below (the split flavours: for both planes); gap columns of q, k and out rows
 * (ldq, ldk, ldo wider than heads * d) are neither read nor written.  tests/test_attention_gpu.py::test_decoys_past_skv. */
int mf_attention_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt,
                      void* out, int64_t ldo, int32_t batch, int32_t heads, int32_t sq, int32_t skv,
                      int32_t head_dim, float scale, void* stream);
/* mf_attention_bf16 on fp16 operands (MF_F16 storage: q, k, vt and out are fp16; the f16 MFMA forms, fp32 softmax and accumulation):
 * F.scaled_dot_product_attention of the reference's default torch_dtype=torch.float16 run (examples/brushnet/test_brushnet.py:122-126,
 * models/attention_processor.py:1259-1268).  Same layouts, head dims and constraints. */
int mf_attention_f16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt,
                      void* out, int64_t ldo, int32_t batch, int32_t heads, int32_t sq, int32_t skv,
                      int32_t head_dim, float scale, void* stream);

/* The same kernel in split precision (the parity mode's attention): every operand is given as two fp16 planes
 * (hi, lo) of identical layout with hi + lo = the fp32 value to 22 bits (mf_split_halves makes them), each product is
 * three fp16 MFMAs, P is split in registers, out is fp32 [B][Sq][ldo].  head_dim 8 / 40 / 64 / 80. */
int mf_attention_f16x3(const void* q_hi, const void* q_lo, int64_t ldq, const void* k_hi, const void* k_lo, int64_t ldk,
                       const void* vt_hi, const void* vt_lo, int64_t ldvt, float* out, int64_t ldo, int32_t batch,
                       int32_t heads, int32_t sq, int32_t skv, int32_t head_dim, float scale, void* stream);
/* The three flavours above under a causal mask (query i attends keys 0 .. i): the self-attention of the CLIP text encoders
 * (transformers modeling_clip.py CLIPAttention with causal_attention_mask; pipeline_brushnet.py:335-370 encode_prompt).  Same
 * arguments as their twins; sq == skv (else MF_EINVAL); head_dim 8 / 64.  Key tiles above a block's last query are skipped. */
int mf_attention_causal_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt,
                             void* out, int64_t ldo, int32_t batch, int32_t heads, int32_t sq, int32_t skv,
                             int32_t head_dim, float scale, void* stream);
int mf_attention_causal_f16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt,
                            void* out, int64_t ldo, int32_t batch, int32_t heads, int32_t sq, int32_t skv,
                            int32_t head_dim, float scale, void* stream);
int mf_attention_causal_f16x3(const void* q_hi, const void* q_lo, int64_t ldq, const void* k_hi, const void* k_lo, int64_t ldk,
                              const void* vt_hi, const void* vt_lo, int64_t ldvt, float* out, int64_t ldo, int32_t batch,
                              int32_t heads, int32_t sq, int32_t skv, int32_t head_dim, float scale, void* stream);
/* The same with the row statistics the backward pass needs: lse[b][head][i] = log2 of row i's softmax denominator in the exp2
 * domain (max + log2 sum, with scale * log2 e folded in), fp32 [B][heads][Sq]; lse may be NULL. */
int mf_attention_f16x3_lse(const void* q_hi, const void* q_lo, int64_t ldq, const void* k_hi, const void* k_lo, int64_t ldk,
                           const void* vt_hi, const void* vt_lo, int64_t ldvt, float* out, int64_t ldo, float* lse, int32_t batch,
                           int32_t heads, int32_t sq, int32_t skv, int32_t head_dim, float scale, void* stream);

/* Decoupled cross-attention (ABI 23): the reference's IPAttnProcessor2_0 (ip_adapter/attention_processor.py:282-410), which every
 * attn2 of a UNet trained with --normals_conditioning_mode ip_adapter carries, in ONE launch:
 *   out = softmax(q k^T * scale) v + ip_scale * softmax(q k_ip^T * scale) v_ip,        each softmax over its own keys only.
 * k_ip: [B][skv_ip][ldk_ip], vt_ip: V_ip^T as [B][heads*d][ldvt_ip] (keys contiguous, ldvt_ip a multiple of 8 and >= skv_ip);
 * 1 <= skv_ip <= 64 (one key tile; else MF_EINVAL).  The ip keys are one more tile on the text keys' Q fragments, LDS buffers and epilogue,
 * with a fresh softmax; the two results are added in the fp32 accumulator and rounded to storage once.  Everything said of k / vt above
 * holds for k_ip / vt_ip, with this difference: key rows past skv_ip are never read, and of vt_ip only the columns up to
 * 8 * ceil(skv_ip / 8) are (the pad columns among them must be finite).  Head dims as the plain entries (the split flavour: no 160). */
int mf_attention_ip_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt, const void* k_ip,
                         int64_t ldk_ip, const void* vt_ip, int64_t ldvt_ip, void* out, int64_t ldo, int32_t batch, int32_t heads,
                         int32_t sq, int32_t skv, int32_t skv_ip, int32_t head_dim, float scale, float ip_scale, void* stream);
int mf_attention_ip_f16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt, const void* k_ip,
                        int64_t ldk_ip, const void* vt_ip, int64_t ldvt_ip, void* out, int64_t ldo, int32_t batch, int32_t heads,
                        int32_t sq, int32_t skv, int32_t skv_ip, int32_t head_dim, float scale, float ip_scale, void* stream);
int mf_attention_ip_f16x3(const void* q_hi, const void* q_lo, int64_t ldq, const void* k_hi, const void* k_lo, int64_t ldk,
                          const void* vt_hi, const void* vt_lo, int64_t ldvt, const void* k_ip_hi, const void* k_ip_lo,
                          int64_t ldk_ip, const void* vt_ip_hi, const void* vt_ip_lo, int64_t ldvt_ip, float* out, int64_t ldo,
                          int32_t batch, int32_t heads, int32_t sq, int32_t skv, int32_t skv_ip, int32_t head_dim, float scale,
                          float ip_scale, void* stream);
/* Frequency encoding of the mirror normal (ip_adapter/ip_adapter.py:50-94 FreqEncoder, log sampling, (sin, cos), no input copy):
 * x fp32 [rows][in_dim] -> out fp32 [rows][2 * n_freqs * in_dim], out[r][(2 i + s) * in_dim + j] = (s ? cos : sin)(x[r][j] * f_i),
 * f_i = 2^(i * max_freq_log2 / (n_freqs - 1)). */
int mf_freq_encode(const float* x, float* out, int32_t rows, int32_t in_dim, int32_t n_freqs, float max_freq_log2, void* stream);

/* Flash-style attention BACKWARD in split precision (the training step's backward through
 * F.scaled_dot_product_attention, attention_processor.py:1266-1268 under train_brushnet_mirror.py:1459): dQ, dK, dV from Q, K, V,
 * dO, the forward's lse and dd[b][head][i] = sum_c dO[b][i][head*d + c] * O[b][i][head*d + c] (mf_rowdot_heads).  P is recomputed
 * tile by tile; nothing of size Sq x Skv is written; no atomics (dK / dV and dQ are two passes of one kernel), so the result is
 * bit-reproducible.  Every operand is given as two fp16 planes (mf_split_halves) — row-major [B][S][ld] for Q, K, V, dO and
 * transposed [B][heads*d][ldt] (ldt >= S, a multiple of 8, pad columns finite) for Q, K, dO.  head_dim 8 / 40 (the 4096-token
 * layers of the path; head dims 64 / 80 exceed the LDS of the double-buffered dK / dV pass and keep the unfused backward). */
typedef struct mf_attn_bwd_desc {
    const void* q_hi; const void* q_lo; int64_t ldq;
    const void* k_hi; const void* k_lo; int64_t ldk;
    const void* v_hi; const void* v_lo; int64_t ldv;
    const void* do_hi; const void* do_lo; int64_t lddo;
    const void* qt_hi; const void* qt_lo; int64_t ldqt;
    const void* kt_hi; const void* kt_lo; int64_t ldkt;
    const void* dot_hi; const void* dot_lo; int64_t lddot;
    const float* lse; const float* dd;
    void* dq; void* dk; void* dv; int64_t ldo;         /* [B][S][ldo], fp32 — or bf16 with out_dtype = MF_BF16 (mf_attention_bwd_bf16 only) */
    int32_t batch, heads, sq, skv, head_dim;
    float scale;
    int32_t out_dtype;                                 /* 0 / MF_F32: fp32 gradients; MF_BF16: bf16 (the operands of the q / k / v projections'
                                                          weight and data gradients in the MF_BF16X1 mode, which rounds them anyway) */
} mf_attn_bwd_desc;
int mf_sizeof_attn_bwd_desc(void);
int mf_attention_bwd_f16x3(const mf_attn_bwd_desc* d, void* stream);
/* The same backward on ONE bf16 plane per operand (the *_hi pointers; *_lo are ignored) and one bf16 MFMA per product, P and dS
 * rounded to bf16: the attention backward of the MF_BF16X1 training mode on pre-rounded operands (what the reference's bf16 autocast
 * computes in F.scaled_dot_product_attention's backward, attention_processor.py:1266-1268).  head_dim 8 / 40 / 80. */
int mf_attention_bwd_bf16(const mf_attn_bwd_desc* d, void* stream);
/* mf_attention_bf16 that also writes lse[b][head][q] = log2 of the row's softmax denominator in the exp2 domain (m + log2 l), the row
 * statistic the flash backward recomputes P from.  lse may be NULL. */
int mf_attention_bf16_lse(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt, void* out, int64_t ldo,
                          float* lse, int32_t batch, int32_t heads, int32_t sq, int32_t skv, int32_t head_dim, float scale, void* stream);
/* mf_rowdot_heads with a bf16 second operand (the bf16 forward's output O) */
int mf_rowdot_heads_bf16(const float* a, const void* b, float* out, int32_t batch, int32_t sq, int32_t heads, int32_t head_dim, int64_t ld,
                         void* stream);
/* mf_rowdot_heads_bf16 on contiguous [batch * sq][heads * head_dim] rows that ALSO writes a16 = bf16(a): the flash backward of the
 * MF_BF16X1 mode needs D = rowdot(dO, O) and the rounded dO, both from one read of dO.  head_dim % 8 == 0, heads * head_dim <= 2048. */
int mf_rowdot_heads_cast(const float* a, const void* b16, void* a16, float* out, int32_t batch, int32_t sq, int32_t heads, int32_t head_dim,
                         void* stream);
/* out[b][head][i] = sum_c a[b][i][head*d + c] * b[b][i][head*d + c]  (fp32 [B][S][ld] inputs) */
int mf_rowdot_heads(const float* a, const float* b, float* out, int32_t batch, int32_t sq, int32_t heads, int32_t head_dim, int64_t ld,
                    void* stream);

/* x (n fp32, n % 4 == 0) -> fp16 planes hi = x rounded toward zero, lo = (x - hi) rounded toward zero */
int mf_split_halves(const float* x, void* hi, void* lo, int64_t n, void* stream);
/* Range guard of MF_F16X3.  The fp16 halves hold |x| <= 65504 only and v_cvt_pkrtz_f16_f32 SATURATES above that (no inf, no
 * NaN: nothing downstream would notice), so every kernel that splits operands — mf_gemm_conv and mf_conv_wgrad with
 * MF_F16X3, mf_split_halves — tracks max |operand| and raises a sticky device flag when it leaves the range.  This call
 * copies the flags to *raised (bit 0: mf_gemm_conv, bit 1: mf_split_halves / mf_attention_f16x3 operands, bit 2:
 * mf_conv_wgrad; 0 = every split since the last reset was exact to 22 bits) and clears them when `reset`.  Diagnostic entry:
 * the ONLY one that synchronises `stream`; never call it inside a hipGraph capture.  A caller that sees a flag re-runs the
 * affected work in MF_BF16X3 (fp32 range, 16 bits) or MF_F32. */
int mf_split_overflow(int32_t reset, int32_t* raised, void* stream);

/* Per-row dynamic fp8 (e4m3) quantisation of [rows][c] (c % 8 == 0, c <= 8192), optionally fused behind a LayerNorm
 * (gamma / beta non-NULL: y = LN(x) first, attention.py:203,233,261): out_q[r][j] = fp8(y[r][j] / scale[r]),
 * scale[r] = max_j |y[r][j]| / 448.  The pair (out_q, scale) is an fp8 GEMM's A operand + a_scale.
 * In fp32: scale = amax * fl(1 / 448) (1 for an all-zero row), out_q = RNE_e4m3(clamp(y * (1 / scale), -448, 448)); a row with
 * amax < 2^-64 is multiplied by 2^64 first, so that 1 / scale stays finite.  A row of y that holds a NaN or an Inf (with the
 * LayerNorm: a row of x that does) gets scale[r] = NaN and every code NaN (0x7F), so that the GEMM's output row is NaN as in
 * every other precision; the other rows are not affected. */
int mf_quantize_rows_fp8(const void* x, int32_t in_dtype, void* out_q, float* scale, int64_t rows, int32_t c,
                         const float* gamma, const float* beta, float eps, void* stream);

/* ---- elementwise / layout -------------------------------------------------------------- */
/* NCHW fp32 -> NHWC (dtype), channels zero-padded to c_pad; two sources concatenated along C
 * (brushnet.py:810 torch.concat([sample, brushnet_cond], 1)); src1 may be NULL. */
int mf_pack_nhwc(const float* src0, int32_t c0, const float* src1, int32_t c1, void* dst, int32_t dst_dtype,
                 int32_t c_pad, int32_t batch, int32_t hw, void* stream);
/* NHWC (dtype, channel stride ld) -> NCHW fp32, first c channels */
int mf_unpack_nchw(const void* src, int32_t src_dtype, int64_t ld, float* dst, int32_t c, int32_t batch,
                   int32_t hw, void* stream);
/* out = a + b (elementwise over n elements, dtypes independent) (unet_2d_condition.py:1218) */
int mf_add(const void* a, int32_t a_dtype, const void* b, int32_t b_dtype, void* out, int32_t out_dtype,
           int64_t n, void* stream);
/* out[i] = bf16(x[i]), nearest-even, n elements (x and out 16-byte aligned): the operand copies of the MF_BF16X1 training mode —
 * the reference's autocast rounds every conv / linear operand to bf16 (train_brushnet_mirror.py:567, 1127-1131); rounding them ONCE
 * into a copy lets the step's forward and data-gradient GEMMs run on the LDS-DMA bf16 kernels of the inference path. */
int mf_cast_bf16(const float* x, void* out, int64_t n, void* stream);
/* GEGLU: out[r][j] = h[r][j] * gelu_erf(h[r][c + j]) for h = [rows][2c] (activations.py:100-103) */
int mf_geglu(const void* h, int32_t in_dtype, void* out, int32_t out_dtype, int64_t rows, int32_t c,
             void* stream);
/* sinusoidal timestep embedding, flip_sin_to_cos / freq_shift as embeddings.py:27-67; out [n][dim] fp32 */
int mf_timestep_embedding(const float* t, float* out, int32_t n, int32_t dim, int32_t flip_sin_to_cos,
                          float freq_shift, void* stream);
/* SiLU on fp32 vector (resnet.py:372 nonlinearity(temb)) */
int mf_silu_f32(const float* x, float* out, int64_t n, void* stream);

/* CLIP text encoder (transformers modeling_clip.py CLIPTextEmbeddings / CLIPMLP).
 * mf_embed_tokens: out[b][s][:] = token_table[ids[b][s]][:] + pos_table[s][:], summed in fp32 and rounded once.  ids: int32 in device
 * memory; the tables are [vocab][hidden] and [>= seq][hidden] in table_dtype (fp32, bf16 or fp16), out in out_dtype; hidden % 8 == 0,
 * 16-byte accesses.  An id outside [0, vocab) is clamped to the range: the launch never reads out of bounds.
 * mf_act: elementwise activation over n values (n % 8 == 0), in place when out == x: MF_ACT_QUICK_GELU x * sigmoid(1.702 x),
 * MF_ACT_GELU_ERF the exact erf GELU. */
#define MF_ACT_QUICK_GELU 3   /* mf_act only: mf_gemm_conv has no such epilogue */
#define MF_ACT_GELU_ERF 4
int mf_embed_tokens(const int32_t* ids, const void* token_table, const void* pos_table, int32_t table_dtype, void* out,
                    int32_t out_dtype, int32_t batch, int32_t seq, int32_t hidden, int32_t vocab, void* stream);
int mf_act(const void* x, void* out, int32_t dtype, int32_t kind, int64_t n, void* stream);

/* Fused classifier-free guidance + DDIM step (pipeline_brushnet.py:1310-1315,
 * scheduling_ddim.py:404-450, eta = 0):
 *   e = eu + g*(ec - eu)                       (g < 0: e = eu, no guidance)
 *   pred_type 0 (epsilon):      x0 = (x - sqrt_1m_at*e)/sqrt_at ; eps = e
 *   pred_type 1 (v_prediction): x0 = sqrt_at*x - sqrt_1m_at*e   ; eps = sqrt_at*e + sqrt_1m_at*x
 *   clip > 0: x0 = clamp(x0, -clip, clip)      (clip_sample, :427-430)
 *   x_prev = sqrt_ap*x0 + dir_coef*eps
 * eps_u/eps_c: the two halves of the UNet output in NCHW fp32; eps_out (nullable) receives e. */
int mf_cfg_ddim_step(const float* eps_u, const float* eps_c, float g, const float* x, float* x_prev,
                     float sqrt_at, float sqrt_1m_at, float sqrt_ap, float dir_coef, int32_t pred_type,
                     float clip, float* eps_out, int64_t n, void* stream);
/* Same update with the four coefficients {sqrt_at, sqrt_1m_at, sqrt_ap, dir_coef} read from DEVICE memory, so a
 * captured hipGraph of the whole denoise step can be replayed for every timestep (the host only refreshes the
 * coefficient / timestep buffers between replays).  x_prev may alias x (in-place). */
int mf_cfg_ddim_step_dev(const float* eps_u, const float* eps_c, float g, const float* x, float* x_prev,
                         const float* coef4, int32_t pred_type, float clip, int64_t n, void* stream);
/* CFG combine only (PNDM keeps its own history on the host side): eps = eu + g*(ec-eu) */
int mf_cfg_combine(const float* eps_u, const float* eps_c, float g, float* eps, int64_t n, void* stream);
/* generic y = sum_i c[i]*x[i] (i < nin <= 6) — PNDM/PLMS linear multistep and _get_prev_sample
 * (scheduling_pndm.py:370-382,436-446) */
int mf_axpby_n(const float* const* xs, const float* coefs, int32_t nin, float* y, int64_t n, void* stream);
/* Device-side update of a multistep scheduler (PNDM, UniPC): ONE launch per denoise step does what mf_cfg_combine followed by the
 * scheduler's mf_axpby_n calls does, bit for bit (same roundings, same order of terms, same FMA contraction).  The step's work is a
 * row in DEVICE memory (so a captured hipGraph or a step program serves every step; the host copies the next row in, as it does
 * for coef4).  The row's ops act on a per-element register file:
 *   register 0               e = eu + g*(ec - eu), the guided noise prediction
 *   register 1               the latents: the value on entry; the last value written is stored back (the new latents)
 *   registers 2 .. 2+nslots-1  state[s][0..n) for s = register - 2: history kept by the caller between steps
 *   registers above          temporaries of the step
 * op: dst = sum_k coef[k] * reg[src[k]] (k < nterms <= MF_SCHED_MAX_TERMS: coef[0]*x0, then fmaf(coef[k], x_k, acc)), or
 * nterms == 0: dst = reg[src[0]] (a move).  `load` / `store`: bit r = register r is read from / written back to memory (bits 1 and
 * 2 .. 2+nslots-1 only).  Every element reads what it loads before it stores anything, so the update is in place.  The row comes from
 * reflecting_reality_amd/schedulers.py (device_plan: a trace of the scheduler's own step()), which reads no slot it has not written.
 * state: nslots * n floats; n % 4 == 0; latents, state, eps_u, eps_c 16-byte aligned. */
#define MF_SCHED_MAX_OPS 8
#define MF_SCHED_MAX_TERMS 6
#define MF_SCHED_MAX_REGS 16
typedef struct mf_sched_op {
    int32_t dst;
    int32_t nterms;
    int32_t src[MF_SCHED_MAX_TERMS];
    float coef[MF_SCHED_MAX_TERMS];
} mf_sched_op;
typedef struct mf_sched_row {
    int32_t nops;
    int32_t nslots;
    uint32_t load;
    uint32_t store;
    mf_sched_op ops[MF_SCHED_MAX_OPS];
} mf_sched_row;
int mf_sizeof_sched_row(void);
/* g < 0 means no classifier-free guidance, the convention of mf_cfg_ddim_step_dev: register 0 is eps_u as loaded, eps_c is never read
 * and may be NULL.  With g >= 0 a NULL eps_c is MF_EINVAL (the message says so); nothing is launched. */
int mf_sched_step_dev(const float* eps_u, const float* eps_c, float g, float* latents, float* state, const mf_sched_row* row, int64_t n,
                      void* stream);
/* mf_sched_step_dev with one more source of values, for samplers that add fresh noise at every step (DPM-Solver++ SDE): before the ops
 * run, register `noise_reg` (2 <= noise_reg < MF_SCHED_MAX_REGS is checked; that it is a temporary of the row, noise_reg >= 2 + nslots,
 * is the caller's duty — the row lives in device memory and the entry does not read it; schedulers.device_plan reports the register
 * as plan.noise_reg) holds standard normals DRAWN IN THE KERNEL from the library's stream ("random numbers" below) — nothing is loaded
 * for it.  latents is [samples][per_sample] with samples = n / per_sample, the rows [first_sample, first_sample + samples) of a draw of
 * global_batch rows: element i of sample s is bit for bit what mf_philox_normal(scale = 1) writes for the same (seed, offset,
 * first_sample, global_batch), i.e. lane i % 4 of block offset + (first_sample + s) * (per_sample / 4) + i / 4 with the Box-Muller
 * pairing stated there.  One thread is one block: per_sample % 4 == 0 is required (MF_EINVAL otherwise).  seed / offset / rng_state
 * follow mf_philox_normal: a non-null rng_state (device uint64 {seed, offset}) overrides the host pair, and the kernel never writes
 * it; the caller follows the launch with mf_philox_advance(rng_state, mf_philox_normal_blocks(global_batch, per_sample)) on the same
 * stream, which therefore runs after the kernel has read the state.  g < 0 as for mf_sched_step_dev: no guidance, register 0 is eps_u,
 * eps_c may be NULL (and is MF_EINVAL when NULL with g >= 0). */
/* (appended; MF_ABI_VERSION stays 23: no existing entry or struct changed) */
int mf_sched_step_noise_dev(const float* eps_u, const float* eps_c, float g, float* latents, float* state, const mf_sched_row* row,
                            int64_t n, int32_t noise_reg, int64_t per_sample, int64_t first_sample, int64_t global_batch, int64_t seed,
                            int64_t offset, const uint64_t* rng_state, void* stream);
/* training loss (examples/brushnet/train_brushnet_mirror.py:1433-1449): per_sample[r] = mean_i (pred[r][i] -
 * target[r][i])^2 * (weights ? weights[r] : 1) and loss[0] = mean_r per_sample[r]; fp32 in, double accumulation */
int mf_mse_loss(const float* pred, const float* target, const float* weights, float* per_sample, float* loss,
                int32_t rows, int64_t n, void* stream);
/* DiagonalGaussianDistribution.sample * scaling (vae.py:769-791, pipeline_brushnet.py:1188):
 * moments NHWC [b][hw][ld] (mean = ch 0..c-1, logvar = ch c..2c-1) -> z NCHW fp32 [b][c][hw] */
int mf_vae_sample(const void* moments, int32_t m_dtype, int64_t ld, const float* noise, float* z, int32_t c,
                  int32_t batch, int32_t hw, float scaling, void* stream);
/* nearest-neighbour resize of NCHW fp32 planes (F.interpolate default, pipeline_brushnet.py:1189-1200) */
int mf_nearest_resize(const float* src, float* dst, int32_t planes, int32_t h_in, int32_t w_in, int32_t h_out,
                      int32_t w_out, void* stream);

/* ---- image front-end on the device (image_processor.py:446-610, pipeline_brushnet.py:1139,1196-1215,
 * examples/brushnet/dataset/dataset.py:98-145); fp32 NCHW planes, no host synchronisation ------------------- */
/* out2[0] = min, out2[1] = max of x[0..n) (only where mask[i] > 0 when mask is given); ws: mf_minmax_ws_floats() floats */
int64_t mf_minmax_ws_floats(void);
int mf_minmax(const float* x, const float* mask, int64_t n, float* out2, float* ws, void* stream);
/* VaeImageProcessor.preprocess's normalisation: y = 2x - 1 if minmax[0] >= 0 (device value from mf_minmax) else y = x */
int mf_image_normalize(const float* x, float* y, int64_t n, const float* minmax, void* stream);
/* out[b][0][p] = (sum_c mask[b][c][p] < 0) ? 1 : 0: 1 = keep, 0 = hole (pipeline_brushnet.py:1139) */
int mf_mask_keep(const float* mask, float* out, int32_t batch, int32_t channels, int64_t hw, void* stream);
/* The 'ip_adapter' normals transform (dataset.py:173-180): out3 = the mean of normals[p][0..2] (HWC fp32, `pixels` = H * W) over the
 * pixels with mask[p] > 0, divided by its L2 norm (ABI 23). */
int mf_masked_mean_normal(const float* normals, const float* mask, float* out3, int64_t pixels, void* stream);
/* torch.cat along channels of up to 8 NCHW sources into out [batch][sum channels][hw]; source i has batches[i] images and
 * is repeated (image b % batches[i]) when that is smaller than batch */
int mf_concat_channels(const float* const* srcs, const int32_t* channels, const int32_t* batches, int32_t nsrc, float* out,
                       int32_t batch, int64_t hw, void* stream);
/* VaeImageProcessor.postprocess: clamp(x / 2 + 0.5, 0, 1) (denormalize) to fp32 NCHW (out_f32) and / or round(. * 255) to
 * uint8 NHWC (out_u8, what PIL.Image.fromarray takes); either output may be NULL */
int mf_postprocess(const float* x, float* out_f32, void* out_u8, int32_t batch, int32_t channels, int64_t hw, int32_t denormalize,
                   void* stream);
/* apply_transforms_depth(normalization_method="max_scene_depth"): scene = (mask ? max over mask > 0 of depth : max_scene_depth
 * given) + (mask ? delta : 0); out = clip(depth, 0, scene) / scene, mapped to [-1, 1] when signed_range;
 * ws: mf_minmax_ws_floats() + 2 floats */
int mf_depth_normalize(const float* depth, const float* mask, float* out, int64_t n, float max_scene_depth, float delta,
                       int32_t signed_range, float* ws, void* stream);

/* apply_transforms_depth(normalization_method="percentile") (dataset.py:115-127): the order statistics np.percentile
 * interpolates between, by a two-level radix select (no sort; integer atomics, order-independent).  mf_select_ranks: the nr <= 4
 * order statistics x_(ranks[i]) (0-based ranks in DEVICE memory) -> vals[i] (device); ws: mf_select_ws_bytes() bytes.
 * mf_depth_percentile_normalize: ranks4 = {floor, ceil of 0.02 (n - 1); floor, ceil of 0.98 (n - 1)}, t_lo / t_hi the
 * fractional parts; d2 / d98 interpolated like numpy's 'linear' method, out = (clip(d, d2, d98) - d2) / (d98 - d2), mapped to
 * [-1, 1] when signed_range; vals4: 4 floats of device scratch. */
int64_t mf_select_ws_bytes(void);
int mf_select_ranks(const float* x, int64_t n, const int64_t* ranks, int32_t nr, float* vals, void* ws, void* stream);
int mf_depth_percentile_normalize(const float* depth, float* out, int64_t n, const int64_t* ranks4, float t_lo, float t_hi,
                                  int32_t signed_range, float* vals4, void* ws, void* stream);
/* torchvision Resize(interpolation=BICUBIC, antialias=False) + CenterCrop (+ Normalize) of dataset.py:150-164,184-192 on fp32 planes:
 * PyTorch's plain bicubic kernel (align_corners = False, A = -0.75, no antialiasing: torchvision < 0.17's default for tensors)
 * evaluated inside the crop window only:
 * dst[p][y][x] = a * bicubic(src[p] resized to h_res x w_res)[y + crop_top][x + crop_left] + b */
int mf_bicubic_resize_crop(const float* src, float* dst, int32_t planes, int32_t h_in, int32_t w_in, int32_t h_res, int32_t w_res,
                           int32_t crop_top, int32_t crop_left, int32_t h_out, int32_t w_out, float a, float b, void* stream);
/* The same with PyTorch's ANTIALIASED bicubic (F.interpolate(mode="bicubic", align_corners=False, antialias=True): ATen's
 * _upsample_bicubic2d_aa, Keys kernel a = -0.5 stretched by max(scale, 1), weights normalised per output pixel, width pass then
 * height pass) — what torchvision 0.18 (the reference's pinned version) runs for transforms.Resize(BICUBIC) on a tensor at every
 * scale (dataset.py:150-164,183-192: antialias defaults to True there). */
int mf_bicubic_aa_resize_crop(const float* src, float* dst, int32_t planes, int32_t h_in, int32_t w_in, int32_t h_res, int32_t w_res,
                              int32_t crop_top, int32_t crop_left, int32_t h_out, int32_t w_out, float a, float b, void* stream);
/* y[c][p] = a * x[p][c] + b: HWC -> CHW with Normalize([0.5], [0.5]) (apply_transforms_normals, dataset.py:184-192) */
int mf_hwc_to_chw_affine(const float* x, float* y, int64_t hw, int32_t channels, float a, float b, void* stream);
/* uint8 NHWC pixels (what a host holds after decoding an image file) -> fp32 NCHW planes in [0, 1]:
 * dst[b][c][p] = (float)src[b][p][c % channels_in] / 255.0f, a true fp32 division — bit for bit what
 * numpy.asarray(img).astype(np.float32) / 255.0 gives (VaeImageProcessor.preprocess for a PIL image, image_processor.py:471-480).
 * channels_out == channels_in, or channels_in == 1 with channels_out > 1: the grey plane is replicated (a mask the reference turns
 * into three equal channels with .convert("RGB")). */
int mf_u8_to_planes(const void* src_u8_nhwc, float* dst_nchw, int32_t batch, int32_t channels_in, int32_t channels_out, int64_t hw,
                    void* stream);

/* ---- the training batch on the device (csrc/train_batch.hip; examples/brushnet/dataset/dataset.py:61-96, 216-221 and
 * examples/brushnet/train_brushnet_mirror.py:1351-1449 minus the networks).  Appended to ABI 23; not part of step programs. ---------
 * mf_train_example_u8: one read of a decoded sample's bytes — image uint8 [B][H][W][3], mask uint8 [B][H][W] — gives the three fp32
 * NCHW tensors the dataset hands to the collate function:
 *   pixel_values[b][c][y][x]              = f(image[b][y][xs][c])
 *   conditioning_pixel_values[b][c][y][x] = f(mask[b][y][xs] == 255 ? 0 : image[b][y][xs][c])    (get_masked_image, invert=True)
 *   masks[b][0][y][x]                     = (float)mask[b][y][xs] / 255.0f
 * xs = flips && flips[b] ? W - 1 - x : x (np.fliplr; flips: int32 [B] in DEVICE memory, or NULL).  f(p) = ((float)p / 255.0f - 0.5f)
 * / 0.5f when normalize (Resize + CenterCrop are the identity at H == W == resolution), (float)p / 255.0f when not (the [0, 1] planes
 * mf_bicubic_aa_resize_crop takes with a = 2, b = -1).  The division is a true fp32 division, as in mf_u8_to_planes. */
int mf_train_example_u8(const void* image_u8, const void* mask_u8, const int32_t* flips, float* pixel_values,
                        float* conditioning_pixel_values, float* masks, int32_t batch, int32_t height, int32_t width, int32_t normalize,
                        void* stream);
/* HDF5Dataset.get_masked_image on uint8 pixels [pixels][channels] and a uint8 mask [pixels]: out = image with the pixels zeroed where
 * mask == 255 (invert = 1, the dataset's default) or where mask == 0 (invert = 0).  out may be image. */
int mf_masked_image_u8(const void* image_u8, const void* mask_u8, void* out_u8, int64_t pixels, int32_t channels, int32_t invert,
                       void* stream);
/* np.fliplr of fp32 [rows][width][channels] (channels 1 or 3: a depth or a normals map): dst[r][x][c] = src[r][width - 1 - x][c] */
int mf_fliplr(const float* src, float* dst, int64_t rows, int32_t width, int32_t channels, void* stream);
/* One launch from the VAE moments to everything the model call and the loss read.
 * moments / posterior_noise: HOST arrays of nsrc (2 .. 4) DEVICE pointers — image, conditioning image, depth, normals (entries 2 and
 * 3 may be null: that source is absent).  Moments are in mf_vae_sample's layout, NHWC [batch][h * w][ld] of m_dtype (MF_F32 / MF_BF16 /
 * MF_F16), mean = ch 0..c-1, logvar = ch c..2c-1, ld >= 2c; each posterior noise is fp32 [batch][c][h * w].
 * noise fp32 [batch][c][h * w]; timesteps int64 [batch] in DEVICE memory, clamped to [0, T) before the gather; sqrt_alpha,
 * sqrt_one_minus_alpha and (optional) loss_weight: fp32 device tables of T entries.  masks [batch][1][plane_h][plane_w], optional
 * depths [batch][1][..][..] and normals [batch][3][..][..]: full-resolution fp32 planes, resized with mf_nearest_resize's rule.
 * Writes, fp32 NCHW: latents = (mean + std * posterior noise) * scaling of source 0 (mf_vae_sample's arithmetic); noisy_latents =
 * sqrt_alpha[t] latents + sqrt_one_minus_alpha[t] noise (mf_axpby_n's arithmetic); target = noise (prediction_type 0, epsilon) or
 * sqrt_alpha[t] noise - sqrt_one_minus_alpha[t] latents (1, v); conditioning_latents [batch][ctot][h][w] = source 1's latents (c
 * channels), the mask (1), the depth plane (1) or source 2's latents (c), the normals planes (3) or source 3's latents (c), in that
 * order; timesteps_f32 [batch]; loss_weights [batch] = loss_weight[t] (both NULL or both given).  A source and its plane exclude
 * each other. */
int mf_train_batch_assemble(const void* const* moments, const float* const* posterior_noise, int32_t nsrc, int32_t m_dtype, int64_t ld,
                            int32_t c, int32_t batch, int32_t h, int32_t w, float scaling, const float* noise, const int64_t* timesteps,
                            const float* sqrt_alpha, const float* sqrt_one_minus_alpha, const float* loss_weight, int32_t T,
                            const float* masks, const float* depths, const float* normals, int32_t plane_h, int32_t plane_w,
                            int32_t prediction_type, float* latents, float* noisy_latents, float* target, float* conditioning_latents,
                            float* timesteps_f32, float* loss_weights, void* stream);

/* ---- tiled VAE encode / decode (csrc/vae_tile.hip; models/autoencoders/autoencoder_kl.py:311-423).  Appended to ABI 23; not part
 * of step programs. -----------------------------------------------------------------------------------------------------------------
 * mf_crop_pack_nhwc: mf_pack_nhwc with a window.  src is NCHW fp32 [batch][c][h][w]; its window [y0, y0 + th) x [x0, x0 + tw) goes to
 * NHWC [batch][th][tw][c_pad] of dst_dtype (MF_F32 / MF_BF16 / MF_F16), channels c .. c_pad - 1 zero, written at sample `batch_offset`
 * of dst = [dst_batch][th][tw][c_pad]: one launch takes one tile (x[:, :, i : i + tile, j : j + tile]) into its slot range of a
 * stacked group buffer.  The window must lie inside the source and the samples inside the buffer. */
int mf_crop_pack_nhwc(const float* src, int32_t batch, int32_t c, int32_t h, int32_t w, int32_t y0, int32_t x0, int32_t th, int32_t tw,
                      void* dst, int32_t dst_dtype, int32_t c_pad, int32_t dst_batch, int32_t batch_offset, void* stream);
/* mf_vae_tile_blend: blend_v, blend_h, the crop and the two torch.cat of tiled_decode / tiled_encode (autoencoder_kl.py:311-321,
 * 357-369, 407-419) for ONE tile; launch once per tile in raster order on one stream.  tile: fp32 NHWC [batch][th][tw][ld] (ld % 4 == 0,
 * 16-byte aligned), blended IN PLACE; above: the finished tile of the previous row, [batch][above_h][above_w][ld] with above_w == tw,
 * or NULL in row 0; left: the finished previous tile of this row, [batch][left_h][left_w][ld] with left_h == th, or NULL in column 0.
 * With ev = min(above_h, th, blend_extent) and eh = min(left_w, tw, blend_extent), every pixel is finished in the reference's order:
 *   y < ev:  t[y][x] = above[above_h - ev + y][x] * (float)(1.0 - (double)y / ev) + t[y][x] * (float)((double)y / ev)
 *   x < eh:  t[y][x] = left[y][left_w - eh + x]   * (float)(1.0 - (double)x / eh) + t[y][x] * (float)((double)x / eh)
 * each product and each sum rounded to fp32 on its own (ATen's arithmetic for those lines; no FMA), over all ld floats of the pixel.
 * The strips are written back into `tile` (the tiles below and to the right read them, the parts outside the crop included) and the
 * crop [:min(th, row_limit), :min(tw, row_limit)] goes to `out` at (out_y, out_x): NCHW fp32 [batch][c][out_h][out_w] (out_nhwc = 0,
 * the first c channels: the decoder's image) or NHWC fp32 [batch][out_h][out_w][ld] (out_nhwc = 1, 16-byte aligned: the encoder's
 * moments).  A neighbour whose shared dimension differs, or a crop that leaves the output, is refused. */
int mf_vae_tile_blend(float* tile, const float* above, const float* left, int32_t batch, int32_t th, int32_t tw, int32_t above_h,
                      int32_t above_w, int32_t left_h, int32_t left_w, int64_t ld, int32_t c, int32_t blend_extent, int32_t row_limit,
                      float* out, int32_t out_nhwc, int32_t out_h, int32_t out_w, int32_t out_y, int32_t out_x, void* stream);

/* ---- image scoring on the device (metrics/metrics.py:51-67,108-165: torchmetrics' peak_signal_noise_ratio and
 * structural_similarity_index_measure with their defaults, on the images taken as floats 0 .. 255) --------------------------------
 * One row per image, written on the device; every image of a batch is scored on its own.  PSNR and the SSIM mean are finished from
 * the row in float64 by whoever reads it:
 *   psnr = 10 log10(R^2 / (sq_err / (h w c)))   R = target_max - target_min (or the given data_range); sq_err == 0: inf
 *   ssim = ssim_sum / count                     count = (h - 10)(w - 10) c positions of the 11 x 11 Gaussian window (sigma 1.5) */
typedef struct mf_metrics_row {
    int64_t sq_err;      /* sum over every element of (pred - target)^2 after the region step: exact */
    int64_t count;
    double ssim_sum;     /* sum of the per-position SSIM values (fp32 each, added in float64 in a fixed order) */
    int32_t pred_min, pred_max, target_min, target_max;      /* after the region step */
} mf_metrics_row;
int mf_sizeof_metrics_row(void);
/* bytes of device scratch mf_image_metrics needs (8-byte aligned); -1 for dimensions it refuses */
int64_t mf_image_metrics_ws_bytes(int32_t batch, int32_t h, int32_t w, int32_t channels);
/* pred / target: uint8 [batch][h][w][channels], channels 1 .. 4, h and w >= 11; mask: uint8 [batch][h][w], or NULL with region 0.
 * region (dataset.py:62-68, applied to BOTH images before anything else): 0 none; 1 "mask": pixels with mask == 255 become 0 in every
 * channel; 2 "mirror": pixels with mask == 0 become 0.  data_range > 0: used for PSNR (by the caller) and for SSIM's c1 / c2, and the
 * statistics ride in the SSIM pass (2 launches); <= 0: SSIM takes max(range(pred), range(target)) of each image from the data (4
 * launches).  No host synchronisation, no floating-point atomics: the same inputs give the same bytes on every run. */
int mf_image_metrics(const void* pred_u8_nhwc, const void* target_u8_nhwc, const void* mask_u8, int32_t region, int32_t batch,
                     int32_t h, int32_t w, int32_t channels, float data_range, mf_metrics_row* rows_out, void* ws, void* stream);

/* ---- CLIP prompt fidelity on the device (metrics/metrics.py:156-157 calculate_clip_similarity: torchmetrics' clip_score on
 * openai/clip-vit-large-patch14, i.e. transformers' CLIPProcessor + CLIPModel).  Additive entries: the ABI version stays. ------------
 * mf_clip_preprocess: uint8 [batch][h][w][3] images -> the A operand of the patch-embedding GEMM, bit for bit what CLIPImageProcessor
 * (PIL backend) computes:
 *   1. resize so that the shortest edge is `size`, the other int(size * long / short): PIL's Image.resize(BICUBIC) on 8-bit pixels, the
 *      horizontal pass first, then the vertical one, a uint8 image between them; a pass whose size does not change is skipped.  htab /
 *      vtab are that pass' table in device memory, int32 [n_out][2] (first source index, tap count) followed by int32 [n_out][hk or vk]
 *      coefficients in 22-bit fixed point (built in float64 on the host: frontend.clip_resize_table); NULL exactly when the pass is skipped.
 *      A sample is clip8((2^21 + sum src * k) >> 22): integer arithmetic only.
 *   2. centre crop to crop x crop (crop <= size): top = (h1 - crop) / 2, left = (w1 - crop) / 2
 *   3. (u8 * (1 / 255) - mean[c]) / std[c] in fp32, three roundings, then one rounding to out_dtype
 *   4. patches_out [batch][(crop / patch)^2][k8]: column c * patch^2 + row * patch + col (patch_embedding.weight.reshape(C, -1)'s order),
 *      k8 = 3 patch^2 rounded up to 8, the pad columns written as zero; 16-byte aligned.
 * crop_u8_out (may be NULL): the cropped uint8 image [batch][crop][crop][3].  ws: mf_clip_preprocess_ws_bytes() bytes, 16-byte aligned
 * (-1 for sizes it refuses).  One or two launches.
 * mf_clip_vision_embed: out[b][0][:] = class_embedding + pos_table[0]; out[b][1 + i][:] = patches[b][i][:] + pos_table[1 + i], summed
 * in fp32 and rounded once (mf_embed_tokens' contract); patches [batch][tokens - 1][hidden], hidden % 8 == 0, 16-byte accesses.
 * mf_clip_score: out[b] = 100 <i, t> / (|i| |t|) for fp32 image_feats / text_feats [batch][dim]; one wave per row, fp32 sums in a fixed
 * order, one launch; norms_out [batch][2] receives |i| and |t|.  No epsilon: a zero vector gives NaN, as in the reference. */
int64_t mf_clip_preprocess_ws_bytes(int32_t batch, int32_t h, int32_t w, int32_t size, int32_t crop);
int mf_clip_preprocess(const void* images_u8_nhwc, int32_t batch, int32_t h, int32_t w, int32_t channels, int32_t size, int32_t crop,
                       int32_t patch, const int32_t* htab, int32_t hk, const int32_t* vtab, int32_t vk, float mean0, float mean1,
                       float mean2, float std0, float std1, float std2, void* patches_out, int32_t out_dtype, int32_t k8,
                       void* crop_u8_out, void* ws, void* stream);
int mf_clip_vision_embed(const void* patches, const void* class_embedding, const void* pos_table, int32_t in_dtype, void* out,
                         int32_t out_dtype, int32_t batch, int32_t tokens, int32_t hidden, void* stream);
int mf_clip_score(const float* image_feats, const float* text_feats, int32_t batch, int32_t dim, float* out, float* norms_out,
                  void* stream);

/* ---- LPIPS (csrc/lpips.hip): the reference's third image-quality number (metrics/metrics.py:51-67, :150-151, :202-204: torchmetrics'
 * learned_perceptual_image_patch_similarity(net_type="squeeze", normalize=False)).  The convolutions of squeezenet1_1.features are
 * mf_gemm_conv calls; these entries are the arithmetic around them.  fp32, bf16 or fp16 activations, NHWC, 16-byte accesses.
 * mf_lpips_prepare: uint8 NHWC pred / gt [batch][h][w][3] (mask [batch][h][w], region as in mf_image_metrics: the blackening happens
 *   before anything else) -> out [2 * batch][h][w][8], the pred images first: per channel x / 127.5 - 1 (unit_range 0) or x / 255
 *   (unit_range 1), then (v - shift[c]) / scale[c] of the LPIPS scaling layer, every step one fp32 rounding, then one rounding to
 *   out_dtype; channels 3 .. 7 are written as zero (the first conv is an 8-channel-segment implicit GEMM with K = 72).
 * mf_relu: x = max(x, 0) in place over rows x channels elements, row r at x + r * ld (channels % 8 == 0, ld % 8 == 0).
 * mf_maxpool3s2_ceil: MaxPool2d(3, 2, ceil_mode=True) of x [batch][h][w][channels] into out [batch][ho][wo][channels], ho =
 *   ceil((h - 3) / 2) + 1; a window that hangs over the edge takes the max of what exists; h, w >= 3, channels % 8 == 0.
 * mf_lpips_layer: feat [2 * batch][pixels][channels] (image b against image batch + b), weight fp32 [channels]: per pair the sum over
 *   the pixels of sum_c weight[c] (a_c / n(a) - b_c / n(b))^2, n(x) = sqrt(1e-8 + sum_c x_c^2), in fp32 per pixel; a fixed number of
 *   per-block partial sums per pair go to slot `layer` (0 .. 6) of ws.  channels 8 .. 512, a multiple of 8.  Equal halves give 0 exactly.
 * mf_lpips_finish: the partials of all seven slots, each summed in a fixed order -> rows_out fp32 [batch][7] (sums: the caller divides
 *   by the pixel counts).  No floating-point atomics anywhere: the same inputs give the same bits.
 * ws: mf_lpips_ws_bytes(batch) bytes, 8-byte aligned (-1 for a batch it refuses); every slot must have been written by a
 * mf_lpips_layer call before mf_lpips_finish reads it.  One launch each. */
int64_t mf_lpips_ws_bytes(int32_t batch);
int mf_lpips_prepare(const void* pred_u8_nhwc, const void* gt_u8_nhwc, const void* mask_u8, int32_t region, int32_t batch, int32_t h,
                     int32_t w, int32_t channels, int32_t unit_range, void* out, int32_t out_dtype, void* stream);
int mf_relu(void* x, int32_t dtype, int64_t rows, int32_t channels, int64_t ld, void* stream);
int mf_maxpool3s2_ceil(const void* x, void* out, int32_t dtype, int32_t batch, int32_t h, int32_t w, int32_t channels, void* stream);
int mf_lpips_layer(const void* feat, int32_t dtype, const float* weight, int32_t batch, int64_t pixels, int32_t channels, int32_t layer,
                   void* ws, void* stream);
int mf_lpips_finish(const void* ws, int32_t batch, float* rows_out, void* stream);

/* ============================================================================================
 * Training: the backward pass and the optimizer of examples/brushnet/train_brushnet_mirror.py:1459-1466
 * (accelerator.backward -> ATen autograd in the reference; clip_grad_norm_ :1463; torch.optim.AdamW :1188-1200).
 * All tensors fp32.  Data gradients of convolutions / linears need no entry of their own: they are mf_gemm_conv on the
 * transposed (tap-flipped) weight that mf_transpose lays out; strided / upsampling convs add mf_zero_insert2x /
 * mf_sumpool2x2.  Every reduction has a fixed order: gradients are bit-reproducible.
 * ========================================================================================== */

/* Weight gradient of mf_gemm_conv's convolution (same geometry fields): dw[n][(ky*kw + kx)*(c0+c1) + c] (+)= sum over
 * output pixels m of dy[m][n] * A[pixel(m, ky, kx)][c].  dtype MF_F32 (fp32 MFMA), MF_F16X3 (split precision), MF_BF16X1 (fp32
 * operands rounded to bf16 while staged) or MF_BF16 (bf16 operands in memory); dw is fp32 in every one.
 * Replaces autograd's conv2d / linear weight gradients (torch/nn/grad.py conv2d_weight; linear: dy^T x). */
typedef struct mf_wgrad_desc {
    /* MF_F32 / MF_F16X3 / MF_BF16X1: fp32 a0 / a1 / dy (rounded or split while staged).  MF_BF16: a0 / a1 / dy are bf16 tensors
     * (declared float* for the layout's sake; strides in elements; channel counts multiples of 8) — the pre-rounded operand copies of
     * the bf16x1 training mode: half the operand bytes, no conversion in the staging loop, the same products as MF_BF16X1. */
    int32_t dtype;
    const float* a0; const float* a1;   /* the forward input, NHWC, one or two channel segments */
    int32_t c0, c1;
    int64_t lda0, lda1;
    int32_t batch, h_in, w_in, h_out, w_out, kh, kw, stride, pad_t, pad_l, upsample;
    const float* dy; int64_t lddy;      /* gradient of the conv output, [batch*h_out*w_out][n] */
    int32_t n;
    float* dw; int64_t lddw;            /* [n][kh*kw*(c0+c1)] */
    int32_t accumulate;                 /* 1: dw += ... */
    int32_t splitm;                     /* slabs over the pixel dimension: 0 = heuristic */
    float* ws; int64_t ws_floats;       /* splitm * n * kh*kw*(c0+c1) floats (mf_conv_wgrad_ws_floats) */
} mf_wgrad_desc;
int mf_sizeof_wgrad_desc(void);
int64_t mf_conv_wgrad_ws_floats(const mf_wgrad_desc* d);
int mf_conv_wgrad(const mf_wgrad_desc* d, void* stream);
/* What mf_conv_wgrad would do with a descriptor, decided on the host: mf_conv_wgrad is this plan followed by its launches.
 * mf_conv_wgrad_plan makes every check and every choice of the call (same return code, same mf_last_error text), launches nothing,
 * needs no GPU and reads nothing behind the descriptor's pointers (their null-ness and alignment count).  It answers for the current
 * value of mf_debug_set_wgrad_dma's switch. */
typedef struct mf_wgrad_plan {
    int32_t form;               /* 0 fp32, 1 128-wide register-staged, 2 160-wide, 3 128-wide LDS-DMA */
    int32_t tile_w;             /* the tile is tile_w (n) x tile_w (channels of one tap): 128 or 160 */
    int32_t tiles;              /* output tiles: ceil(n / tile_w) * ceil((c0 + c1) / tile_w) * kh * kw */
    int32_t splitm;             /* slabs over the pixel dimension, after "no empty slabs" */
    int32_t m_per_split;        /* pixels per slab, a multiple of 32 */
    int32_t reduce_launch;      /* 1: the slabs go to the workspace and a slab-sum launch follows; 0: the kernel completes dw itself */
    int32_t slabs_xcd;          /* the first slabs_xcd slabs (splitm rounded down to a multiple of 8) are pinned to XCDs */
    int32_t blocks;             /* blocks of the main launch: tiles * splitm (form 0 launches them as a tiles x splitm grid) */
    int32_t threads;            /* threads per block */
    int32_t lds_bytes;          /* dynamic LDS bytes of the main launch */
} mf_wgrad_plan;
int mf_conv_wgrad_plan(const mf_wgrad_desc* d, mf_wgrad_plan* out);
int mf_sizeof_wgrad_plan(void);
/* Developer / test switch: 0 routes bf16-input weight gradients to the register-staged kernel instead of the LDS-DMA one (the two are
 * bit-identical; tests compare them).  On by default.  Process-wide, not thread-safe against concurrent mf_conv_wgrad calls. */
void mf_debug_set_wgrad_dma(int on);

/* base[offs[i] .. offs[i] + lens[i]) = 0 for i < count, one launch (offs / lens: DEVICE arrays of int64, element units).  The training
 * step clears only the small accumulated parameters of the gradient arena this way; conv / linear weight gradients are written by their
 * first mf_conv_wgrad of the step (accumulate = 0) — optimizer.zero_grad() of train_brushnet_mirror.py:1466 without the 2.5 GB memset. */
int mf_zero_ranges(float* base, const int64_t* offs, const int64_t* lens, int32_t count, void* stream);

/* fp32 weight [rows][k] (row stride ldw) -> mf_gemm_desc's w_split layout for MF_F16X3 / MF_BF16X3: out = 16-bit
 * [rows][2 * kp], kp = round_up(k, 32), per 32 k the 32 high halves then the 32 low halves (hi = RNE(w), lo = RNE(w - hi)),
 * zero padded.  The device form of what the inference weights get once on the host: training re-splits the weights the
 * optimizer just changed (models.py / autograd.py), the frozen network's once.  An |w| > 65504 under MF_F16X3 raises the
 * flag mf_split_overflow() reports. */
int mf_split_pack(const float* w, int64_t ldw, void* out, int64_t rows, int32_t k, int32_t dtype, void* stream);

/* y[z][c][r] = x[z][r][c] for nz matrices: element strides ldx / ldy between rows, zsx / zsy between matrices (signed:
 * a negative zsy with y pointing at the last matrix writes the batch in reverse — the tap flip of a dgrad weight) */
int mf_transpose(const float* x, float* y, int32_t nz, int32_t rows, int32_t cols, int64_t ldx, int64_t ldy, int64_t zsx,
                 int64_t zsy, void* stream);
/* The same with a bf16 (nearest-even) result, strides in elements: the transposed, tap-flipped weight of the data-gradient GEMM in the
 * bf16x1 training mode is rounded while it is laid out (one launch instead of mf_transpose + mf_cast_bf16). */
int mf_transpose_bf16(const float* x, void* y, int32_t nz, int32_t rows, int32_t cols, int64_t ldx, int64_t ldy, int64_t zsx,
                      int64_t zsy, void* stream);

/* out[s][j] (+)= sum over the rows of segment s (rows_per_seg consecutive rows) of x[row][j], j < n: bias gradients
 * (one segment), the time-embedding gradient of a resnet (one segment per image), dgamma / dbeta partials */
/* mf_transpose on bf16 in and out (16-byte accesses both ways): cols, ldx, ldy, zsx, zsy multiples of 8, ldy >= rows rounded up to 8
 * (pad columns are written as zeros).  Q^T / K^T / V^T of the MF_BF16X1 attention. */
int mf_transpose_bf16_bf16(const void* x, void* y, int32_t nz, int32_t rows, int32_t cols, int64_t ldx, int64_t ldy, int64_t zsx,
                           int64_t zsy, void* stream);

int64_t mf_colsum_ws_floats(int32_t segs, int64_t rows_per_seg, int32_t n);
int mf_colsum(const float* x, int64_t ldx, float* out, int64_t ldo, int32_t segs, int64_t rows_per_seg, int32_t n,
              int32_t accumulate, float* ws, void* stream);

/* mf_cast_bf16 of a contiguous [segs * rows_per_seg][n] gradient (n % 8 == 0) AND its column sums from the same read: seg_out[s][j]
 * (+)= the sum over segment s (nullable: the time-embedding gradient of a resnet, resnet.py:369-381), tot_out[j] (+)= the sum over all
 * rows (nullable: the bias gradient).  Replaces mf_cast_bf16 + up to two mf_colsum passes in the bf16x1 training mode. */
int64_t mf_cast_bf16_colsum_ws_floats(int32_t segs, int64_t rows_per_seg, int32_t n);
int mf_cast_bf16_colsum(const float* x, void* out16, int32_t segs, int64_t rows_per_seg, int32_t n, float* seg_out, int64_t ldo,
                        int32_t seg_accumulate, float* tot_out, int32_t tot_accumulate, float* ws, void* stream);

/* Backward of mf_groupnorm (GroupNorm + optional SiLU over one or two NHWC segments; native_group_norm_backward +
 * silu_backward in the reference's autograd): dx per segment, per-image dgamma / dbeta partials [batch][c0+c1]
 * (nullable; sum them with mf_colsum). */
typedef struct mf_groupnorm_bwd_desc {
    const float* x0; const float* x1; int32_t c0, c1;
    const float* dy;
    const float* gamma; const float* beta;
    float* dx0; float* dx1;
    float* dgamma_part; float* dbeta_part;
    int32_t batch, hw, groups, silu;
    float eps;
    float* ws;      /* mf_groupnorm_bwd_ws_floats() floats, 16-byte aligned; null = the one-block-per-group kernel only */
    float* dgamma_acc; float* dbeta_acc;   /* [c0 + c1], nullable, INSTEAD of the partials: the gradients summed over the batch
                                            * are ADDED here (needs mf_groupnorm_bwd_streams(...) != 0 and ws) */
    const float* add0; const float* add1;  /* nullable, laid out like dx0 / dx1: dx = gradient + add (the gradient a residual
                                            * connection already left for the same tensor: no separate accumulation pass) */
    const float* stats_in;                 /* nullable [batch][groups][2]: the (mean, rstd) mf_groupnorm wrote to stats_out for the same
                                            * input — the streaming form then skips its statistics pass (one read of x less) */
} mf_groupnorm_bwd_desc;
int mf_sizeof_groupnorm_bwd_desc(void);
int mf_groupnorm_bwd_streams(int32_t batch, int32_t hw, int32_t c0, int32_t c1);   /* 1: this shape runs the streaming form */
int64_t mf_groupnorm_bwd_ws_floats(int32_t batch, int32_t hw, int32_t channels, int32_t groups);
int mf_groupnorm_bwd(const mf_groupnorm_bwd_desc* d, void* stream);

/* LayerNorm backward over [rows][c] (c <= 2048): dx, and per-block dgamma / dbeta partials
 * [mf_layernorm_bwd_parts(rows)][c] (nullable) */
int64_t mf_layernorm_bwd_parts(int64_t rows);
int mf_layernorm_bwd(const float* x, const float* dy, const float* gamma, float* dx, float* dgamma_part, float* dbeta_part,
                     int64_t rows, int32_t c, float eps, const float* add /* nullable [rows][c]: dx = gradient + add */, void* stream);
/* ds = scale * p * (dp - sum_j dp*p) per row of [rows][ld] (valid length cols, pad written 0): softmax backward */
int mf_softmax_bwd(const float* p, const float* dp, float* ds, int64_t rows, int32_t cols, int32_t ld, float scale, void* stream);
int mf_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* h = [a | g] ([rows][2c]), out = a * gelu_erf(g): dh from dout ([rows][c]) */
int mf_geglu_bwd(const float* h, const float* dout, float* dh, int64_t rows, int32_t c, void* stream);
/* mf_geglu_bwd on a bf16 pre-activation h16 [rows][2c] (the MF_BF16X1 mode keeps FeedForward's hidden tensor in bf16, as the reference's
 * autocast does: attention.py:617-675 under train_brushnet_mirror.py:902-907,1127-1131): dh16 bf16 [rows][2c]; bias_grad (nullable, fp32 [2c],
 * ADDED to) receives the column sums of dh16 — ff.net.0.proj's bias gradient — from the same pass (ws: mf_geglu_bwd_bf16_ws_floats). */
int64_t mf_geglu_bwd_bf16_ws_floats(int64_t rows, int32_t c);
int mf_geglu_bwd_bf16(const void* h16, const float* dout, void* dh16, int64_t rows, int32_t c, float* bias_grad, float* ws, void* stream);
/* y[b][2h][2w][c]: x at the even positions, zeros elsewhere (a stride-2 conv's data gradient as a stride-1 conv) */
int mf_zero_insert2x(const float* x, float* y, int32_t batch, int32_t h, int32_t w, int32_t c, void* stream);
/* y[b][h][w][c] = sum of the 2x2 block of x[b][2h][2w][c]: backward of the nearest-2x upsample (upsampling.py:170-178) */
int mf_sumpool2x2(const float* x, float* y, int32_t batch, int32_t h, int32_t w, int32_t c, void* stream);
/* gradient of mf_mse_loss's loss[0] with respect to pred */
int mf_mse_grad(const float* pred, const float* target, const float* weights, float* dpred, int32_t rows, int64_t n, void* stream);

/* sum of squares of a flat gradient arena into out[0] (double, device), two fixed-order stages */
int64_t mf_sumsq_ws_doubles(void);
int mf_sumsq(const float* x, int64_t n, double* out, int32_t accumulate, double* ws, void* stream);
/* torch.nn.utils.clip_grad_norm_ (train_brushnet_mirror.py:1463) for an arena that holds gradients x S (S = 1 / unscale, the
 * loss scale of the split-precision backward; unscale = 1 without one): norm = sqrt(sumsq) * unscale -> norm_out[0]
 * (nullable); coef[0] = min(1, max_norm / (norm + 1e-6)) * unscale stays on the device (mf_adamw multiplies the stored
 * gradients with it: no host synchronisation in the step) */
int mf_clip_coef(const double* sumsq, float max_norm, float unscale, float* coef, float* norm_out, void* stream);
/* torch.optim.AdamW (train_brushnet_mirror.py:1188-1200; no amsgrad) over flat arenas of n fp32: the gradient is read as
 * g * grad_scale[0] (grad_scale nullable) */
int mf_adamw(float* w, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
             float weight_decay, int32_t step, const float* grad_scale, void* stream);

/* ---- step programs: a whole forward pass behind ONE entry (mf_brushnet_forward / mf_unet_forward /
 * mf_denoise_step_fused) -----------------------------------------------------------------------------------------------------
 * The sequencing of a pass — which of the entries above, on which buffers, with which tiles — is written down ONCE by the Python
 * side (reflecting_reality_amd/program.py: one eager pass of BrushNetModel.forward, models/brushnet.py:693-936;
 * UNet2DConditionModel.forward, models/unets/unet_2d_condition.py:1037-1311; or the loop body of
 * pipelines/brushnet/pipeline_brushnet.py:1250-1332) into a program file; a host with no Python loads the file, gives every buffer
 * memory, and replays it.  A program is specialised like a hipGraph (shapes, precision, tiles, scalar arguments are the recorded
 * ones) and, like one, is replayed on any stream and may itself be captured into a hipGraph by the host.
 *
 * File: a header of header_bytes (everything mf_program_load parses: magic "MFPROG1", ABI version, buffer table, calls) followed
 * by the bytes of the constant and io buffers at the file offsets mf_program_buffer_info reports.  Buffer kinds:
 *   MF_PROGRAM_CONST      weights in their device layouts, prompt K / V^T, tables, scratch: upload the file's bytes once
 *   MF_PROGRAM_WORKSPACE  intermediates: any device memory of `bytes` (contents undefined between runs, data_offset -1)
 *   MF_PROGRAM_IO         named inputs / outputs ("latents", "coef4", ...): the host's own buffers; the file holds the recorded
 *                         pass's values, so that replaying the file as it is reproduces the recorded pass bit for bit
 * Every buffer must be bound (16-byte aligned device memory of at least `bytes`) before mf_program_run; the library keeps the
 * pointers, never the memory.
 *
 * Streams: a program recorded inside a hipGraph capture (the denoise step: BrushNet on a side stream under the UNet's encoder,
 * pipeline.py::_denoise_graph) carries that capture's forks and joins.  Stream 0 is the `stream` argument of mf_program_run; the
 * others, and the events between them, are created by the first run on the device current then and destroyed by
 * mf_program_destroy — the only device objects this library ever owns.  Every side stream forks from stream 0 and has joined it
 * again when the run's last call is enqueued, so runs on one stream are ordered like single launches and the whole run can be
 * captured (hipStreamBeginCapture on `stream`). */
#define MF_PROGRAM_CONST 0
#define MF_PROGRAM_WORKSPACE 1
#define MF_PROGRAM_IO 2
typedef struct mf_program mf_program;
/* blob: the first header_bytes of the file (bytes 24..31 of the file, little endian); the library copies what it needs */
int mf_program_load(const void* blob, int64_t bytes, mf_program** out);
void mf_program_destroy(mf_program* p);
int32_t mf_program_num_buffers(const mf_program* p);
int mf_program_buffer_info(const mf_program* p, int32_t index, int32_t* kind, int64_t* bytes, int64_t* data_offset, const char** name);
int32_t mf_program_find_buffer(const mf_program* p, const char* name);      /* -1: no buffer of that name */
int mf_program_bind(mf_program* p, int32_t index, void* device_ptr);
int32_t mf_program_num_calls(const mf_program* p);
/* the free-form description the exporter stored (JSON: what was recorded, shapes, precision, steps of the tables); never NULL */
const char* mf_program_meta(const mf_program* p);
int mf_program_run(mf_program* p, void* stream);
/* The loop body of pipeline_brushnet.py:1250-1332 — latent doubling, BrushNet, UNet with the 28 injected residuals, classifier-free
 * guidance, DDIM update — as one call: binds the io buffers "latents" (NCHW fp32, updated IN PLACE), "coef4" (the step's
 * {sqrt_at, sqrt_1m_at, sqrt_ap, dir_coef}, mf_cfg_ddim_step_dev), "temb_unet" / "temb_brushnet" (the step's rows of the two
 * time-embedding tables) and runs the program.  A NULL argument keeps the buffer's current binding.  A step exported under a
 * multistep scheduler (PNDM, UniPC) has no "coef4"; it comes in one of two forms (export_denoise_step(..., scheduler=)):
 *   "device": the update is inside (mf_sched_step_dev): io buffers "sched_row" (the step's row of the named constant
 *             "table.sched_row", copied in like coef4) and "sched_state" (the scheduler's history, nslots * latents; it persists
 *             between runs, so bind it once and leave it alone).  mf_denoise_step_fused(step, NULL, NULL, NULL, NULL, stream) then
 *             runs a whole PNDM / UniPC / DPM-Solver++ step.  Under the SDE type of DPM-Solver++ the update is mf_sched_step_noise_dev
 *             followed by mf_philox_advance: the generator's device state {seed, offset} is one more io buffer, "philox_state"
 *             (16 bytes; bind it once and leave it alone, or write a pair into it to restart the noise), and the program's meta
 *             carries "philox": {per_sample, first_sample, global_batch, blocks_per_step, noise_reg}.
 *   "host":   it ends with the guided noise prediction e = eu + g (ec - eu) in the io buffer "eps" (pipeline_brushnet.py:1310-1312)
 *             and the host's scheduler steps from it. */
int mf_denoise_step_fused(mf_program* step, void* latents, const void* coef4, const void* temb_unet, const void* temb_brushnet, void* stream);
/* UNet2DConditionModel.forward (unet_2d_condition.py:1037-1311) with BrushNet's residuals injected (:1172-1177, 1218, 1262-1284):
 * io buffers "sample", "temb", "residual.<i>" (i < n_residuals, the order of brushnet.py:896-936: down, mid, up), "eps" (the noise
 * prediction).  The prompt enters through the program's constants (the cross-attention K / V^T bound when it was recorded). */
int mf_unet_forward(mf_program* unet, const void* sample, const void* temb, const void* const* residuals_in, int32_t n_residuals,
                    void* eps_out, void* stream);
/* BrushNetModel.forward (brushnet.py:693-936): io buffers "sample", "temb", "cond" (the 5-channel conditioning latents of
 * pipeline_brushnet.py:1186-1215) and "residual.<i>" (written). */
int mf_brushnet_forward(mf_program* brushnet, const void* sample, const void* temb, const void* cond, void* const* residuals_out,
                        int32_t n_residuals, void* stream);
/* AutoencoderKL.decode (models/autoencoders/autoencoder_kl.py:294-318, vae.py:285-351; pipeline_brushnet.py:1342 hands it latents /
 * scaling_factor): io buffers "z" (NCHW fp32 latents) and "image" (NCHW fp32, written). */
int mf_vae_decode(mf_program* vae_decoder, const void* z, void* image_out, void* stream);
/* AutoencoderKL.encode up to the posterior's moments (autoencoder_kl.py:256-291, vae.py:137-167 + quant_conv): io buffers "image"
 * (NCHW fp32) and "moments" (NHWC fp32 [b][h/8][w/8][2 * latent_channels]: mean | logvar, what mf_vae_sample reads; written). */
int mf_vae_encode_moments(mf_program* vae_encoder, const void* image, void* moments_out, void* stream);
/* The two ends of a call around the denoise loop, so that a host runs pipeline_brushnet.py:848-1363 from programs alone
 * (pipe.export_call writes the five files and a manifest; examples/c_host/inpaint_host.c runs them).  Each of the three entries below
 * refuses a program whose meta names another entry, binds the io buffers it is given (NULL keeps a binding) and runs the program.
 *
 * mf_encode_prompt: CLIPTextModel under encode_prompt (pipeline_brushnet.py:271-450, clip_skip included): io buffers "input_ids"
 * (int32 [2B][77]: the negative prompts' rows, then the positive ones') and "prompt_embeds" ([2B][77][C] in the model's storage dtype,
 * written — the very buffer the prompt-binding program reads: bind one allocation to both).  Token ids are CLAMPED into the vocabulary
 * (mf_embed_tokens's rule); checking them is the host's job. */
int mf_encode_prompt(mf_program* text_encoder, const int32_t* input_ids, void* prompt_embeds, void* stream);
/* pipeline_brushnet.py:1116-1215: io buffers "image_u8" / "mask_u8" (uint8 [B][H][W][3]), "depth" (fp32 [B][1][H][W] in [-1, 1]; only
 * a program exported with depth conditioning has it: pass NULL otherwise), "cond_noise" (the VAE posterior noise, fp32 NCHW at latent
 * resolution: B images when both guidance halves share one draw, else 2B — the program's meta says which) and "cond" (the denoise
 * step's conditioning buffer, written). */
int mf_build_conditioning(mf_program* conditioning, const void* image_u8, const void* mask_u8, const float* depth, const float* cond_noise,
                          void* cond, void* stream);
/* pipeline_brushnet.py:1342 and VaeImageProcessor.postprocess: latents / scaling_factor, AutoencoderKL.decode, mf_postprocess: io
 * buffers "latents" (NCHW fp32, the denoise step's) and "image_u8" (uint8 [B][H][W][3], written). */
int mf_decode_image(mf_program* decoder, const void* latents, void* image_u8, void* stream);
/* the device copies / fills a recorded pass contains (torch made them between the launches): hipMemcpy2DAsync / hipMemsetAsync */
int mf_memcpy2d(void* dst, int64_t dpitch, const void* src, int64_t spitch, int64_t width_bytes, int64_t height, void* stream);
int mf_memset(void* dst, int32_t value, int64_t bytes, void* stream);

/* ---- random numbers: one counter-based stream, the same from Python and from C (csrc/rng.hip, csrc/philox.h; appended, ABI stays 23) -----------
 * GENERATOR  Philox4x32-10 with the standard constants: multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85,
 *            10 rounds.  Key = (seed low 32 bits, seed high 32 bits) of a 64-bit seed; counter = (block low 32, block high 32, 0, 0)
 *            of a 64-bit block index.  A generator is the pair (seed, offset), offset counted in blocks; one block yields four uint32
 *            values x0..x3, the lanes.  Nothing else enters: not the grid, the device or the number of ranks.  (seed and offset
 *            travel as int64_t and are read as the same 64 bits unsigned: seed 2^63 + 1 is passed as -(2^63 - 1).)
 * BITS       Element i of a draw that starts at offset o is lane i % 4 of block o + i / 4; n elements advance the offset by
 *            ceil(n / 4).
 * NORMALS    Lanes (0, 1) give one Box-Muller pair, lanes (2, 3) the next.  u = ((xa >> 9) + 0.5f) * 2^-23 and
 *            phi = ((xb >> 9) + 0.5f) * 2^-23, both exact in fp32, u in (0, 1); s = sqrtf(-2.0f * logf(u)); the pair is
 *            (s * cospif(2 * phi), s * sinpif(2 * phi)), then times `scale`, each product rounded once.  The accurate math functions,
 *            fp32 out; the largest magnitude is sqrt(-2 ln 2^-24) = 5.768 (times scale).  A tensor [B, ...] is drawn PER SAMPLE: with
 *            `per` elements to a sample, sample s starts at block o + s * ceil(per / 4), and the draw advances the offset by
 *            B * ceil(per / 4).  So a rank that owns the samples [first, first + b) of a global batch G draws exactly those rows
 *            (first_sample = first, samples = b, global_batch = G), and every rank advances by G * ceil(per / 4).
 * INTEGERS   below T, 0 < T <= 2^31: element i takes its lane x as for bits and yields (uint64(x) * T) >> 32, as int64.  There is no
 *            rejection step: a value's probability differs from 1 / T by at most 2^-32, a relative bias of at most T / 2^32.
 *            [first, first + n) of a draw of `total` elements is a rank's slice; the draw advances by ceil(total / 4).
 * STATE      Every draw takes (seed, offset) as host values and an optional `state` in device memory, uint64 {seed, offset}; a
 *            non-null state overrides the host values (a captured graph reads it at every replay).  A draw never writes the state
 *            (all its blocks read it): mf_philox_advance, one tiny launch on the same stream, follows the draws.
 * Normals are device-only (the host's libm would not match the device bit for bit); bits are also computed on the host. */
/* blocks a [samples, per_sample] normal draw / an n-element integer or bits draw consumes; -1 (mf_last_error) for a negative count */
int64_t mf_philox_normal_blocks(int64_t samples, int64_t per_sample);
int64_t mf_philox_int_blocks(int64_t n);
/* the raw bits on the host, from the very block function the kernels run (no GPU, no HIP call) */
int mf_philox_bits_host(uint32_t* out, int64_t n, int64_t seed, int64_t offset);
int mf_philox_bits(uint32_t* out, int64_t n, int64_t seed, int64_t offset, const uint64_t* state, void* stream);
/* out: fp32 [samples][per_sample], the rows [first_sample, first_sample + samples) of a draw of global_batch rows */
int mf_philox_normal(float* out, int64_t samples, int64_t per_sample, float scale, int64_t first_sample, int64_t global_batch,
                     int64_t seed, int64_t offset, const uint64_t* state, void* stream);
/* out: int64 [n], the elements [first, first + n) of a draw of `total` integers below T */
int mf_philox_randint(int64_t* out, int64_t n, int64_t T, int64_t first, int64_t total, int64_t seed, int64_t offset,
                      const uint64_t* state, void* stream);
/* state[1] += blocks, on the stream (after the draws that read the state) */
int mf_philox_advance(uint64_t* state, int64_t blocks, void* stream);
/* Everything mf_train_batch_assemble reads as random input, in ONE launch: the posterior noises of the present sources
 * (posterior_noise: a host array of nsrc device pointers in the order image, conditioning image, depth, normals; entries 2 and 3 may be
 * NULL), then `noise` — each fp32 [samples][per_sample], per_sample = c * h * w — then `timesteps` (int64 [samples], below T).  The
 * offsets are consecutive, as if mf_philox_normal had been called once per present source and once for the noise, then
 * mf_philox_randint(first = first_sample, total = global_batch): the launch consumes
 * (present sources + 1) * mf_philox_normal_blocks(global_batch, per_sample) + mf_philox_int_blocks(global_batch) blocks. */
int mf_train_batch_draw(float* const* posterior_noise, int32_t nsrc, float* noise, int64_t* timesteps, int64_t samples,
                        int64_t per_sample, int64_t T, int64_t first_sample, int64_t global_batch, int64_t seed, int64_t offset,
                        const uint64_t* state, void* stream);

/* ---- LoRA adapters merged on the device (csrc/lora.hip; appended, ABI stays 23) -------------------------------------------------------
 * models/lora.py:324,410 (`_fuse_lora` of LoRACompatibleConv / LoRACompatibleLinear) for a TABLE of weights in one grouped launch.  For
 * every target t, with base_t and out_t row-major fp32 [rows][cols] in the reference's own weight layout (cols = Cin * kh * kw: a conv
 * LoRA needs no layout knowledge, down is [rank][Cin * kh * kw] and up is the 1 x 1 conv), and its terms first_term .. first_term + nterms:
 *     out[i][k] = base[i][k] + sum_terms coef[term] * ( sum_{j < rank} up[i][j] * down[j][k] )        up [rows][rank], down [rank][cols]
 * ARITHMETIC  Each output element is computed by exactly one thread: per term s = 0, then s = fmaf(up[i][j], down[j][k], s) for ascending
 *             j; the element starts as base[i][k] and takes fmaf(coef[term], s, element) per term, in table order.  fp32 throughout, no
 *             atomics, and the result does not depend on the grid: the same inputs give the same bits on every run.  (A term with
 *             coef 0 and finite factors leaves the element's value unchanged.)
 * TABLES      The target table, the term table and coef (one float per term) are read by the kernel from DEVICE memory (targets_dev,
 *             terms_dev, coef_dev); they are built once per adapter set, outside any capture, and a new scale or adapter weight
 *             rewrites coef alone before the next launch.  `targets` / `terms` are the HOST copies of the same two tables: the entry
 *             validates them and sizes the grid from them.  Targets use the term table in order without gaps (first_term is the running
 *             sum of nterms), and first_tile is the running sum of mf_lora_tiles(rows, cols).
 * REFUSED     (-EINVAL, text in mf_last_error) a null table or pointer, rows, cols or rank < 1, out overlapping base (the base is kept
 *             so that un-merging is exact: it is never subtracted back), a term or tile index out of sequence.  Outputs of different
 *             targets must not overlap each other either (not checked).
 * 16-byte accesses along cols are used where cols % 4 == 0 and the addresses allow; other targets (conv_in: cols = 36 is fine, 9 is
 * not) take scalar accesses.  All pointers need 4-byte alignment. */
typedef struct mf_lora_target {
    const float* base;       /* [rows][cols] */
    float* out;              /* [rows][cols], no overlap with base */
    int32_t rows, cols;
    int32_t first_term, nterms;
    int64_t first_tile;      /* sum of mf_lora_tiles over the targets before this one */
} mf_lora_target;
typedef struct mf_lora_term {
    const float* up;         /* [rows][rank] */
    const float* down;       /* [rank][cols] */
    int32_t rank;
    int32_t reserved;        /* 0 */
} mf_lora_term;
int mf_sizeof_lora_target(void);
int mf_sizeof_lora_term(void);
/* work items (thread blocks' tiles) of one target; -1 (mf_last_error) for rows or cols < 1 */
int64_t mf_lora_tiles(int32_t rows, int32_t cols);
int mf_lora_merge(const mf_lora_target* targets, const mf_lora_term* terms, const mf_lora_target* targets_dev, const mf_lora_term* terms_dev,
                  const float* coef_dev, int32_t ntargets, int32_t nterms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MFHIP_H */
