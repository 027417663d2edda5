/* A whole inpainting call with no Python in the process: token ids, pixels, mask and depth in, a uint8 image out.  Runs the directory
 *   pipe.export_call("call_dir", prompt=..., image=..., mask=..., depth=..., conditioning_noise=..., ...)     (pipeline.py, program.py)
 * writes: five step programs and manifest.txt (manifest_reader.h).  The reference's pipelines/brushnet/pipeline_brushnet.py:848-1363 as
 * five entries of include/mfhip.h:
 *   mf_encode_prompt       encode_prompt.mfprog   ids [2B][77] int32 (negative rows, then positive) -> prompt embeddings
 *   mf_program_run         bind_prompt.mfprog     prompt embeddings -> the cross-attention K / V^T the step reads as constants
 *   mf_build_conditioning  conditioning.mfprog    uint8 image + mask, depth, VAE posterior noise -> the step's "cond"
 *   mf_denoise_step_fused  step.mfprog            once per timestep (DDIM, PNDM or UniPC: the update is inside); row i of every
 *                                                 "table.X" goes into the io buffer "X" first, as in denoise_host.c
 *   mf_decode_image        decode.mfprog          latents -> uint8 [B][H][W][3]
 * Programs hand each other device buffers by name: "prompt_embeds" (encode -> bind), every constant bind and step both name (the
 * K / V^T), "cond" (conditioning -> step), "latents" (step -> decode) are ONE allocation each.
 *
 *   gcc -O2 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/c_host/inpaint_host.c \
 *       -Lreflecting-reality_amd/lib -lmfhip -L/opt/rocm/lib -lamdhip64 -o inpaint_host
 *   LD_LIBRARY_PATH=reflecting-reality_amd/lib:/opt/rocm/lib ./inpaint_host call_dir --ids ids.bin --image image.bin --mask mask.bin
 *       [--depth depth.bin] (--noise noise.bin --latents latents.bin | --seed N) --out image_out.bin [--latents-out latents_out.bin] [--graph]
 *
 * Raw files, each exactly the size of its io buffer: ids int32; image / mask uint8 HWC; depth fp32 in [-1, 1]; noise fp32 (the VAE
 * posterior noise, B or 2B images as exported: manifest key cond_noise_batch); latents fp32 (the initial noise).  Tokenising, decoding
 * image files stay the caller's; so do the random numbers, unless --seed N draws them here: the library's own stream (mfhip.h, "random
 * numbers") from generator (N, 0), in the order pipe(generator=PhiloxGenerator(N)) draws — the posterior noise (cond_noise_batch samples,
 * mf_philox_normal straight into "cond_noise"), then the latents (batch samples, scale init_noise_sigma, straight into "latents") at the
 * offset the first draw ends on — so the image is that call's, bit for bit.  Everything that can be checked on the host — the manifest, the five
 * headers, every input's size — is checked BEFORE the device is touched; after that every mf_* and hip* status is checked and the
 * first failure ends the process with a non-zero status.  --graph: the step is captured into a hipGraph once and replayed. */
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "manifest_reader.h"
#include "mfhip.h"

#define HIP_OK(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return 1;                                                                             \
        }                                                                                         \
    } while (0)
#define MF_OKAY(call)                                                                 \
    do {                                                                              \
        if ((call) != MF_OK) {                                                        \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #call, mf_last_error()); \
            return 1;                                                                 \
        }                                                                             \
    } while (0)
#define TRY(call)                  \
    do {                           \
        if ((call) != 0) return 1; \
    } while (0)

typedef struct host_prog {
    const char* what;
    char path[1024];
    FILE* f;
    mf_program* p;
    int32_t nbuf;
    void** dev;      /* device memory of every buffer (shared ones point into another program's) */
    char* owned;     /* 1: this program allocated dev[i] */
} host_prog;

/* host only: open the file, parse its header, check the entry it was exported for */
static int prog_open(host_prog* h, const mf_manifest* m, const char* dir, const char* what, const char* entry) {
    char key[64];
    unsigned char head[40];
    int64_t head_len;
    void* blob;
    const char* name;
    snprintf(key, sizeof(key), "files.%s", what);
    name = mf_manifest_get(m, key);
    if (!name) { fprintf(stderr, "manifest: no key %s\n", key); return 1; }
    h->what = what;
    snprintf(h->path, sizeof(h->path), "%s/%s", dir, name);
    h->f = fopen(h->path, "rb");
    if (!h->f) { fprintf(stderr, "%s: the manifest names this file (%s) but it cannot be opened\n", h->path, key); return 1; }
    if (fread(head, 1, 40, h->f) != 40) { fprintf(stderr, "%s: short file\n", h->path); return 1; }
    memcpy(&head_len, head + 24, 8);
    if (head_len < 40 || head_len > ((int64_t)1 << 30)) { fprintf(stderr, "%s: not a step program\n", h->path); return 1; }
    blob = malloc((size_t)head_len);
    if (!blob || fseek(h->f, 0, SEEK_SET) != 0 || fread(blob, 1, (size_t)head_len, h->f) != (size_t)head_len) {
        fprintf(stderr, "%s: short header\n", h->path);
        return 1;
    }
    MF_OKAY(mf_program_load(blob, head_len, &h->p));
    free(blob);
    if (entry) {
        char want[96];
        snprintf(want, sizeof(want), "\"entry\": \"%s\"", entry);
        if (!strstr(mf_program_meta(h->p), want)) { fprintf(stderr, "%s: not exported for %s\n", h->path, entry); return 1; }
    }
    h->nbuf = mf_program_num_buffers(h->p);
    h->dev = (void**)calloc((size_t)h->nbuf + 1, sizeof(void*));
    h->owned = (char*)calloc((size_t)h->nbuf + 1, 1);
    return (h->dev && h->owned) ? 0 : 1;
}

static int64_t io_bytes(const host_prog* h, const char* name) {
    const int32_t i = mf_program_find_buffer(h->p, name);
    int32_t kind = -1;
    int64_t bytes = 0;
    if (i < 0 || mf_program_buffer_info(h->p, i, &kind, &bytes, NULL, NULL) != MF_OK || kind != MF_PROGRAM_IO) return -1;
    return bytes;
}

static void* io_ptr(const host_prog* h, const char* name) {
    const int32_t i = mf_program_find_buffer(h->p, name);
    return i < 0 ? NULL : h->dev[i];
}

/* host only: a whole input file, which must have exactly the io buffer's size */
static int read_input(const char* path, const host_prog* h, const char* buffer, void** out, int64_t* bytes_out) {
    const int64_t want = io_bytes(h, buffer);
    FILE* f;
    long have;
    if (want <= 0) { fprintf(stderr, "%s: the program has no io buffer \"%s\"\n", h->path, buffer); return 1; }
    if (!path) { fprintf(stderr, "the %s program takes \"%s\" (%lld bytes): no file was given for it\n", h->what, buffer, (long long)want); return 1; }
    f = fopen(path, "rb");
    if (!f) { perror(path); return 1; }
    if (fseek(f, 0, SEEK_END) != 0 || (have = ftell(f)) < 0 || fseek(f, 0, SEEK_SET) != 0) { perror(path); return 1; }
    if ((int64_t)have != want) {
        fprintf(stderr, "%s: %ld bytes, but \"%s\" of the %s program holds %lld (a program is specialised on its shapes)\n", path, have, buffer,
                h->what, (long long)want);
        return 1;
    }
    *out = malloc((size_t)want);
    if (!*out || fread(*out, 1, (size_t)want, f) != (size_t)want) { fprintf(stderr, "%s: cannot read\n", path); return 1; }
    fclose(f);
    *bytes_out = want;
    return 0;
}

/* device memory for every buffer: `share`'s allocation for a constant or io buffer both programs name (`only`: just that name), else
 * memory of its own with the file's bytes uploaded */
static int prog_place(host_prog* h, const host_prog* share, const char* only) {
    int32_t i;
    for (i = 0; i < h->nbuf; ++i) {
        int32_t kind;
        int64_t bytes, off;
        const char* name;
        MF_OKAY(mf_program_buffer_info(h->p, i, &kind, &bytes, &off, &name));
        if (share && kind != MF_PROGRAM_WORKSPACE && (!only || !strcmp(only, name))) {
            const int32_t j = mf_program_find_buffer(share->p, name);
            if (j >= 0) {
                int64_t there = 0;
                MF_OKAY(mf_program_buffer_info(share->p, j, NULL, &there, NULL, NULL));
                if (there < bytes) { fprintf(stderr, "buffer %s: %lld bytes in %s, %lld in %s\n", name, (long long)there, share->what, (long long)bytes, h->what); return 1; }
                h->dev[i] = share->dev[j];
                MF_OKAY(mf_program_bind(h->p, i, h->dev[i]));
                continue;
            }
        }
        HIP_OK(hipMalloc(&h->dev[i], (size_t)(bytes > 0 ? bytes : 16)));
        h->owned[i] = 1;
        if (off >= 0 && bytes > 0) {
            void* host = malloc((size_t)bytes);
            if (!host || fseek(h->f, (long)off, SEEK_SET) != 0 || fread(host, 1, (size_t)bytes, h->f) != (size_t)bytes) {
                fprintf(stderr, "%s: short data for buffer %s\n", h->path, name);
                return 1;
            }
            HIP_OK(hipMemcpy(h->dev[i], host, (size_t)bytes, hipMemcpyHostToDevice));
            free(host);
        }
        MF_OKAY(mf_program_bind(h->p, i, h->dev[i]));
    }
    fclose(h->f);
    h->f = NULL;
    return 0;
}

static int prog_close(host_prog* h) {
    int32_t i;
    for (i = 0; i < h->nbuf; ++i)
        if (h->owned[i]) HIP_OK(hipFree(h->dev[i]));
    mf_program_destroy(h->p);
    free(h->dev);
    free(h->owned);
    return 0;
}

int main(int argc, char** argv) {
    const char *ids_path = NULL, *image_path = NULL, *mask_path = NULL, *depth_path = NULL, *noise_path = NULL, *lat_path = NULL, *out_path = NULL,
               *lat_out_path = NULL, *seed_s = NULL;
    int use_graph = 0, a;
    if (argc < 2) {
        fprintf(stderr, "usage: %s call_dir --ids F --image F --mask F [--depth F] (--noise F --latents F | --seed N) --out F [--latents-out F] [--graph]\n", argv[0]);
        return 2;
    }
    for (a = 2; a < argc; ++a) {
        const char** dst = !strcmp(argv[a], "--ids") ? &ids_path : !strcmp(argv[a], "--image") ? &image_path : !strcmp(argv[a], "--mask") ? &mask_path
                         : !strcmp(argv[a], "--depth") ? &depth_path : !strcmp(argv[a], "--noise") ? &noise_path : !strcmp(argv[a], "--latents") ? &lat_path
                         : !strcmp(argv[a], "--out") ? &out_path : !strcmp(argv[a], "--latents-out") ? &lat_out_path
                         : !strcmp(argv[a], "--seed") ? &seed_s : NULL;
        if (!strcmp(argv[a], "--graph")) use_graph = 1;
        else if (dst && a + 1 < argc) *dst = argv[++a];
        else { fprintf(stderr, "unknown or incomplete argument %s\n", argv[a]); return 2; }
    }
    if (!out_path) { fprintf(stderr, "--out image_out.bin is needed\n"); return 2; }
    if (seed_s && (noise_path || lat_path)) { fprintf(stderr, "--seed draws the noise and the latents: give it OR --noise / --latents\n"); return 2; }
    char* seed_end = NULL;
    const int64_t seed = seed_s ? (int64_t)strtoull(seed_s, &seed_end, 0) : 0;        /* any 64 bits: the library reads them unsigned */
    if (seed_s && (seed_end == seed_s || *seed_end)) { fprintf(stderr, "--seed %s is not an integer\n", seed_s); return 2; }

    /* ---- host only: manifest, headers, inputs ---------------------------------------------------------------------------------- */
    static mf_manifest man;
    char err[1280], mpath[1024];
    long long abi = -1, steps_m = -1, has_depth = 0;
    snprintf(mpath, sizeof(mpath), "%s/manifest.txt", argv[1]);
    if (mf_manifest_read(mpath, &man, err, sizeof(err)) != 0) { fprintf(stderr, "%s\n", err); return 1; }
    if (mf_manifest_int(&man, "abi_version", &abi) != 0 || abi != mf_abi_version()) {
        fprintf(stderr, "%s: exported against ABI %lld, this library is ABI %d\n", mpath, abi, mf_abi_version());
        return 1;
    }
    if (mf_manifest_int(&man, "steps", &steps_m) != 0 || steps_m < 1 || mf_manifest_int(&man, "depth", &has_depth) != 0) {
        fprintf(stderr, "%s: keys steps / depth missing or malformed\n", mpath);
        return 1;
    }
    const char* sigma_s = mf_manifest_get(&man, "init_noise_sigma");
    const float sigma = sigma_s ? (float)atof(sigma_s) : 1.0f;
    static host_prog step, bind, enc, cond, dec;
    TRY(prog_open(&step, &man, argv[1], "step", "mf_denoise_step_fused"));
    TRY(prog_open(&bind, &man, argv[1], "bind_prompt", NULL));
    TRY(prog_open(&enc, &man, argv[1], "encode_prompt", "mf_encode_prompt"));
    TRY(prog_open(&cond, &man, argv[1], "conditioning", "mf_build_conditioning"));
    TRY(prog_open(&dec, &man, argv[1], "decode", "mf_decode_image"));
    if (io_bytes(&step, "latents") <= 0 || io_bytes(&step, "cond") <= 0 || (io_bytes(&step, "coef4") <= 0 && io_bytes(&step, "sched_row") <= 0)) {
        fprintf(stderr, "%s: not a denoise step with its scheduler update inside (io buffers latents, cond, coef4 or sched_row)\n", step.path);
        return 1;
    }
    if (io_bytes(&step, "cond") != io_bytes(&cond, "cond") || io_bytes(&step, "latents") != io_bytes(&dec, "latents") ||
        io_bytes(&enc, "prompt_embeds") != io_bytes(&bind, "prompt_embeds")) {
        fprintf(stderr, "%s: the programs disagree on the size of a buffer they share (cond, latents or prompt_embeds)\n", argv[1]);
        return 1;
    }
    void *h_ids, *h_image, *h_mask, *h_depth = NULL, *h_noise, *h_lat;
    int64_t n_ids, n_image, n_mask, n_depth = 0, n_noise, n_lat, n_out = io_bytes(&dec, "image_u8");
    TRY(read_input(ids_path, &enc, "input_ids", &h_ids, &n_ids));
    TRY(read_input(image_path, &cond, "image_u8", &h_image, &n_image));
    TRY(read_input(mask_path, &cond, "mask_u8", &h_mask, &n_mask));
    if (has_depth) TRY(read_input(depth_path, &cond, "depth", &h_depth, &n_depth));
    else if (depth_path) { fprintf(stderr, "--depth given, but the call was exported without depth conditioning\n"); return 1; }
    long long nb = 0, noise_b = 0;
    if (seed_s) {
        /* the draws are per sample: the sample counts come from the manifest, the sample sizes from the io buffers */
        h_noise = NULL;
        n_noise = io_bytes(&cond, "cond_noise");
        n_lat = io_bytes(&step, "latents");
        if (mf_manifest_int(&man, "batch", &nb) != 0 || mf_manifest_int(&man, "cond_noise_batch", &noise_b) != 0 || nb < 1 || noise_b < 1 ||
            n_noise <= 0 || n_noise % (4 * noise_b) || n_lat % (4 * nb)) {
            fprintf(stderr, "%s: keys batch / cond_noise_batch missing, or they do not divide the cond_noise / latents buffers\n", mpath);
            return 1;
        }
        h_lat = malloc((size_t)n_lat);               /* the final latents come back through it (--latents-out) */
        if (!h_lat) return 1;
    } else {
        TRY(read_input(noise_path, &cond, "cond_noise", &h_noise, &n_noise));
        TRY(read_input(lat_path, &step, "latents", &h_lat, &n_lat));
    }
    if (n_out <= 0) { fprintf(stderr, "%s: no io buffer image_u8\n", dec.path); return 1; }
    if (!seed_s && sigma != 1.0f) {                      /* prepare_latents (pipeline_brushnet.py:777-791): latents * scheduler.init_noise_sigma */
        int64_t i;
        for (i = 0; i < n_lat / 4; ++i) ((float*)h_lat)[i] *= sigma;
    }

    /* ---- the device ------------------------------------------------------------------------------------------------------------ */
    HIP_OK(hipSetDevice(0));
    TRY(prog_place(&step, NULL, NULL));
    TRY(prog_place(&bind, &step, NULL));
    TRY(prog_place(&enc, &bind, "prompt_embeds"));
    TRY(prog_place(&cond, &step, "cond"));
    TRY(prog_place(&dec, &step, "latents"));
    /* every "table.X" of the step with an io buffer "X": row i goes into X before step i */
    int ntab = 0, steps = -1;
    int32_t i;
    void** tab_dst = (void**)calloc((size_t)step.nbuf + 1, sizeof(void*));
    const char** tab_src = (const char**)calloc((size_t)step.nbuf + 1, sizeof(char*));
    int64_t* tab_row = (int64_t*)calloc((size_t)step.nbuf + 1, sizeof(int64_t));
    if (!tab_dst || !tab_src || !tab_row) return 1;
    for (i = 0; i < step.nbuf; ++i) {
        int32_t kind;
        int64_t bytes, off, row_bytes;
        const char* name;
        MF_OKAY(mf_program_buffer_info(step.p, i, &kind, &bytes, &off, &name));
        if (strncmp(name, "table.", 6) != 0) continue;
        row_bytes = io_bytes(&step, name + 6);
        if (row_bytes <= 0 || bytes % row_bytes) { fprintf(stderr, "table %s: no io buffer %s whose size divides it\n", name, name + 6); return 1; }
        if (steps >= 0 && bytes / row_bytes != steps) { fprintf(stderr, "table %s has %lld rows, another table %d\n", name, (long long)(bytes / row_bytes), steps); return 1; }
        steps = (int)(bytes / row_bytes);
        tab_dst[ntab] = io_ptr(&step, name + 6); tab_src[ntab] = (const char*)step.dev[i]; tab_row[ntab] = row_bytes; ++ntab;
    }
    if (steps < 1 || steps != (int)steps_m) { fprintf(stderr, "the step's tables hold %d rows, the manifest says %lld steps\n", steps, steps_m); return 1; }

    hipStream_t stream;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    HIP_OK(hipMemcpyAsync(io_ptr(&enc, "input_ids"), h_ids, (size_t)n_ids, hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(io_ptr(&cond, "image_u8"), h_image, (size_t)n_image, hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(io_ptr(&cond, "mask_u8"), h_mask, (size_t)n_mask, hipMemcpyHostToDevice, stream));
    if (has_depth) HIP_OK(hipMemcpyAsync(io_ptr(&cond, "depth"), h_depth, (size_t)n_depth, hipMemcpyHostToDevice, stream));
    if (seed_s) MF_OKAY(mf_philox_normal((float*)io_ptr(&cond, "cond_noise"), noise_b, n_noise / (4 * noise_b), 1.0f, 0, noise_b, seed, 0, NULL, stream));
    else HIP_OK(hipMemcpyAsync(io_ptr(&cond, "cond_noise"), h_noise, (size_t)n_noise, hipMemcpyHostToDevice, stream));
    /* NULL arguments: the bindings made by prog_place stay */
    MF_OKAY(mf_encode_prompt(enc.p, NULL, NULL, stream));
    MF_OKAY(mf_program_run(bind.p, stream));
    MF_OKAY(mf_build_conditioning(cond.p, NULL, NULL, NULL, NULL, NULL, stream));
    hipGraphExec_t exec = NULL;
    if (use_graph) {
        /* one eager run first (keeps the capture free of first-use work: the program's own streams and events are made by it); the
         * latents it steps are overwritten below, a PNDM / UniPC history is never read by step 0 */
        hipGraph_t graph;
        for (a = 0; a < ntab; ++a) HIP_OK(hipMemcpyAsync(tab_dst[a], tab_src[a], (size_t)tab_row[a], hipMemcpyDeviceToDevice, stream));
        MF_OKAY(mf_program_run(step.p, stream));
        HIP_OK(hipStreamSynchronize(stream));
        HIP_OK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        MF_OKAY(mf_program_run(step.p, stream));
        HIP_OK(hipStreamEndCapture(stream, &graph));
        HIP_OK(hipGraphInstantiateWithFlags(&exec, graph, hipGraphInstantiateFlagAutoFreeOnLaunch));
    }
    if (seed_s)
        MF_OKAY(mf_philox_normal((float*)io_ptr(&step, "latents"), nb, n_lat / (4 * nb), sigma, 0, nb, seed,
                                 mf_philox_normal_blocks(noise_b, n_noise / (4 * noise_b)), NULL, stream));
    else HIP_OK(hipMemcpyAsync(io_ptr(&step, "latents"), h_lat, (size_t)n_lat, hipMemcpyHostToDevice, stream));
    int s;
    for (s = 0; s < steps; ++s) {
        for (a = 0; a < ntab; ++a)
            HIP_OK(hipMemcpyAsync(tab_dst[a], tab_src[a] + (size_t)s * tab_row[a], (size_t)tab_row[a], hipMemcpyDeviceToDevice, stream));
        if (exec) HIP_OK(hipGraphLaunch(exec, stream));
        else MF_OKAY(mf_denoise_step_fused(step.p, NULL, NULL, NULL, NULL, stream));
    }
    MF_OKAY(mf_decode_image(dec.p, NULL, NULL, stream));
    unsigned char* image = (unsigned char*)malloc((size_t)n_out);
    if (!image) return 1;
    HIP_OK(hipMemcpyAsync(image, io_ptr(&dec, "image_u8"), (size_t)n_out, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(h_lat, io_ptr(&step, "latents"), (size_t)n_lat, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    clock_gettime(CLOCK_MONOTONIC, &t1);
    printf("inpainted: %d steps (%s), %lld image bytes, %.3f ms from the first upload to the image on the host\n", steps,
           exec ? "hipGraph replay of the step" : "mf_denoise_step_fused", (long long)n_out,
           (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6);
    FILE* g = fopen(out_path, "wb");
    if (!g || fwrite(image, 1, (size_t)n_out, g) != (size_t)n_out || fclose(g) != 0) { perror(out_path); return 1; }
    if (lat_out_path) {
        g = fopen(lat_out_path, "wb");
        if (!g || fwrite(h_lat, 1, (size_t)n_lat, g) != (size_t)n_lat || fclose(g) != 0) { perror(lat_out_path); return 1; }
    }
    if (exec) HIP_OK(hipGraphExecDestroy(exec));
    HIP_OK(hipStreamDestroy(stream));
    TRY(prog_close(&dec)); TRY(prog_close(&cond)); TRY(prog_close(&enc)); TRY(prog_close(&bind)); TRY(prog_close(&step));
    free(image); free(h_ids); free(h_image); free(h_mask); free(h_depth); free(h_noise); free(h_lat);
    free(tab_dst); free(tab_src); free(tab_row);
    return 0;
}
