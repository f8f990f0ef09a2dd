// capi_image.cpp -- C ABI of the image stage: the two rasterisers, the Gabor bank and the DoG prefilter
#include <cstring>
#include <new>

#include "mh_capi.h"

static size_t render_vt_bytes(int Nv) { return (((size_t)(Nv > 0 ? Nv : 1) * 16) + 255) / 256 * 256; }

static size_t render_q_bytes(int Nf) { return (((size_t)(Nf > 0 ? Nf : 1) * 4) + 255) / 256 * 256; }

// scratch: [camera | queue counter] 512 B | vertices | z/primitive keys | queue of large triangles
extern "C" size_t mh_render_scratch_bytes(int Nv, int Nf, int H, int W) {
    if (Nv < 0 || Nf < 0 || H < 1 || W < 1) return 0;
    return 512 + render_vt_bytes(Nv) + (size_t)H * W * sizeof(unsigned long long) + render_q_bytes(Nf);
}

extern "C" int mh_render_depth(mh_ctx *ctx, const float *cam_host, const float *verts, int Nv, const int32_t *faces,
                               int Nf, int H, int W, float pixel_center, void *scratch, size_t scratch_bytes,
                               float *out, int channels, void *stream) {
    if (!ctx) return fail(MH_ERR_ARG, "mh_render_depth: no context");
    if (!cam_host || !out || !scratch || H < 1 || W < 1 || Nv < 0 || Nf < 0 || channels < 1 ||
        ((Nv > 0 && Nf > 0) && (!verts || !faces)) || !(pixel_center >= 0.0f && pixel_center < 1.0f))
        return fail(MH_ERR_ARG, "mh_render_depth: bad arguments");
    if (scratch_bytes < mh_render_scratch_bytes(Nv, Nf, H, W))
        return fail(MH_ERR_ARG, "mh_render_depth: scratch too small (%zu < %zu)", scratch_bytes,
                    mh_render_scratch_bytes(Nv, Nf, H, W));
    MH_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)scratch;
    float *cam = (float *)base;
    MH_HIP(hipMemcpyAsync(cam, cam_host, MH_CAM_STRIDE * sizeof(float), hipMemcpyHostToDevice, st));
    unsigned int *qcount = (unsigned int *)(base + 256);
    MhRVert *vt = (MhRVert *)(base + 512);
    unsigned long long *zbuf = (unsigned long long *)(base + 512 + render_vt_bytes(Nv));
    int32_t *queue = (int32_t *)((char *)zbuf + (size_t)H * W * sizeof(unsigned long long));
    const int off = (int)(pixel_center * 256.0f + 0.5f);
    return launched(mh_launch_render_depth(cam, verts, Nv, faces, Nf, H, W, off, 1 << ctx->raster_subpixel_bits, vt, zbuf,
                                           queue, qcount, out, channels, st),
                    "mh_render_depth");
}

extern "C" size_t mh_render_strands_scratch_bytes(int Nv, int Nf, int Nseg, int H, int W) {
    if (Nv < 0 || Nf < 0 || Nseg < 0 || H < 1 || W < 1) return 0;
    return mh_render_scratch_bytes(Nv, Nf, H, W) + 64 + (size_t)2 * Nseg * 32;
}

extern "C" int mh_render_strands(mh_ctx *ctx, const float *cam_host, const float *verts, int Nv, const int32_t *faces,
                                 int Nf, const float *line_pts, const float *line_tan, int Nseg, int H, int W,
                                 float pixel_center, int line_width, int color_option, int depth_option, float clear,
                                 void *scratch, size_t scratch_bytes, float *out, void *stream) {
    if (!ctx) return fail(MH_ERR_ARG, "mh_render_strands: no context");
    if (!cam_host || !out || !scratch || H < 1 || W < 1 || Nv < 0 || Nf < 0 || Nseg < 0 || line_width < 1 ||
        line_width > 64 || color_option > 3 || depth_option < 0 || depth_option > 2 ||
        ((Nv > 0 && Nf > 0) && (!verts || !faces)) || (Nseg > 0 && color_option >= 0 && (!line_pts || !line_tan)) ||
        !(pixel_center >= 0.0f && pixel_center < 1.0f))
        return fail(MH_ERR_ARG, "mh_render_strands: bad arguments");
    if (scratch_bytes < mh_render_strands_scratch_bytes(Nv, Nf, Nseg, H, W))
        return fail(MH_ERR_ARG, "mh_render_strands: scratch too small (%zu < %zu)", scratch_bytes,
                    mh_render_strands_scratch_bytes(Nv, Nf, Nseg, H, W));
    MH_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)scratch;
    float *cam = (float *)base;
    MH_HIP(hipMemcpyAsync(cam, cam_host, MH_CAM_STRIDE * sizeof(float), hipMemcpyHostToDevice, st));
    unsigned int *qcount = (unsigned int *)(base + 256);
    MhRVert *vt = (MhRVert *)(base + 512);
    unsigned long long *zbuf = (unsigned long long *)(base + 512 + render_vt_bytes(Nv));
    int32_t *queue = (int32_t *)((char *)zbuf + (size_t)H * W * sizeof(unsigned long long));
    MhRLVert *lv = (MhRLVert *)(base + ((mh_render_scratch_bytes(Nv, Nf, H, W) + 63) / 64) * 64);
    const int off = (int)(pixel_center * 256.0f + 0.5f);
    return launched(mh_launch_render_strands(cam, verts, Nv, faces, Nf, line_pts, line_tan, Nseg, H, W, off,
                                             1 << ctx->raster_subpixel_bits, line_width, ctx->line_rule, color_option, depth_option, clear, vt, lv, zbuf, queue, qcount,
                                             out, st),
                    "mh_render_strands");
}

static int gabor_alloc(mh_ctx *ctx) {
    if (ctx->gabor) return MH_OK;
    MH_HIP(hipSetDevice(ctx->device));
    MH_HIP(hipMalloc(&ctx->gabor, 290 * 192 * sizeof(float)));   // 289 taps + one zero pad tap (MFMA K = 290)
    MH_HIP(hipMalloc(&ctx->gabor_max, mh_gabor_state_bytes()));
    MH_HIP(hipMalloc(&ctx->gabor_q, mh_gabor_bankq_bytes()));
    return MH_OK;
}

extern "C" int mh_gabor_set_bank(mh_ctx *ctx, const float *bank_host) {
    if (!ctx || !bank_host) return fail(MH_ERR_ARG, "mh_gabor_set_bank: bad arguments");
    int rc = gabor_alloc(ctx);
    if (rc) return rc;
    // kernel-major [180][289] -> tap-major [289][192], zero padded
    float *tmp = new (std::nothrow) float[290 * 192]();
    if (!tmp) return fail(MH_ERR_NOMEM, "mh_gabor_set_bank: out of host memory");
    for (int k = 0; k < 180; ++k)
        for (int t = 0; t < 289; ++t) tmp[t * 192 + k] = bank_host[k * 289 + t];
    hipError_t e = hipMemcpy(ctx->gabor, tmp, 290 * 192 * sizeof(float), hipMemcpyHostToDevice);
    delete[] tmp;
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mh_gabor_set_bank: %s", hipGetErrorString(e));
    rc = launched(mh_launch_gabor_relayout(ctx->gabor, ctx->gabor_q, nullptr), "mh_gabor_set_bank(relayout)");
    if (rc) return rc;
    MH_HIP(hipStreamSynchronize(nullptr));      // (installation is rare; later launches may come on any stream)
    return MH_OK;
}

extern "C" int mh_gabor_bank(mh_ctx *ctx, const float *image, int H, int W, int32_t *orient_index, float *conf,
                             float *variance, void *stream) {
    if (!ctx || !image || !orient_index || !conf || !variance || H < 1 || W < 1)
        return fail(MH_ERR_ARG, "mh_gabor_bank: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (!ctx->gabor) {
        int rc = gabor_alloc(ctx);
        if (rc) return rc;
        rc = launched(mh_launch_gabor_build(ctx->gabor, st), "mh_gabor_bank(build)");
        if (rc) return rc;
        rc = launched(mh_launch_gabor_relayout(ctx->gabor, ctx->gabor_q, st), "mh_gabor_bank(relayout)");
        if (rc) return rc;
    }
    return launched(mh_launch_gabor_bank(ctx->gabor, ctx->gabor_q, image, H, W, orient_index, conf, variance, ctx->gabor_max,
                                         ctx->gabor_variant, nullptr, nullptr, st),
                    "mh_gabor_bank");
}

// The DoG weights (two symmetric halves, float64, computed by the caller the way scipy.ndimage does) live in a small device
// struct; it is re-uploaded only when they change (in practice once: the reference always calls (0.4, 10)).
static int dog_weights(mh_ctx *ctx, const double *w_lo, int r_lo, const double *w_hi, int r_hi, hipStream_t st) {
    if (!w_lo || !w_hi || r_lo < 0 || r_hi < 0)
        return fail(MH_ERR_ARG, "mh_dog: weights missing");
    if (r_lo > MH_DG_MAXR || r_hi > MH_DG_MAXR)
        return fail(MH_ERR_ARG, "mh_dog: kernel radius %d exceeds the built-in limit of %d (sigma <= %.1f at truncate 4); the "
                                "reference uses sigma 0.4 and 10 (radius 2 and 40)", r_lo > r_hi ? r_lo : r_hi, MH_DG_MAXR,
                    (MH_DG_MAXR + 0.49) / 4.0);
    MhDogWeights h;
    memset(&h, 0, sizeof h);
    memcpy(h.w[0], w_lo, sizeof(double) * (r_lo + 1));
    memcpy(h.w[1], w_hi, sizeof(double) * (r_hi + 1));
    h.r[0] = r_lo;
    h.r[1] = r_hi;
    MH_HIP(hipSetDevice(ctx->device));
    if (!ctx->dog_w) {
        MH_HIP(hipMalloc(&ctx->dog_w, sizeof(MhDogWeights)));
        ctx->dog_w_host = new MhDogWeights;
        memset(ctx->dog_w_host, 0xff, sizeof(MhDogWeights));
    }
    if (memcmp(ctx->dog_w_host, &h, sizeof h) != 0) {
        // (other streams may still be reading the old weights: wait for the device before replacing them)
        MH_HIP(hipDeviceSynchronize());
        *ctx->dog_w_host = h;
        MH_HIP(hipMemcpy(ctx->dog_w, ctx->dog_w_host, sizeof h, hipMemcpyHostToDevice));
    }
    (void)st;
    return MH_OK;
}

extern "C" size_t mh_dog_scratch_bytes(int H, int W) { return (size_t)2 * H * W * sizeof(double); }

extern "C" int mh_dog(mh_ctx *ctx, const void *image, int in_kind, int H, int W, const double *w_lo, int r_lo,
                      const double *w_hi, int r_hi, void *scratch, double *out64, float *out32, void *stream) {
    if (!ctx || !image || !scratch || (!out64 && !out32) || H < 1 || W < 1 || (in_kind != 0 && in_kind != 1))
        return fail(MH_ERR_ARG, "mh_dog: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dog_weights(ctx, w_lo, r_lo, w_hi, r_hi, st)) return rc;
    return launched(mh_launch_dog(image, in_kind, H, W, ctx->dog_w, (double *)scratch, out64, out32, st), "mh_dog");
}

// One view of the Gabor stage, device to device: gray uint8 image -> DoG (float64, cast to float32) -> bank -> confidence
// -> the two 8-bit file codes.  scratch: mh_gabor_view_scratch_bytes(H, W) = two float64 planes + the float32 DoG image +
// the image-maximum slot (in the caller's scratch, so views on different streams do not share it).
extern "C" size_t mh_gabor_view_scratch_bytes(int H, int W) { return (size_t)H * W * (16 + 4) + mh_gabor_state_bytes(); }

extern "C" int mh_gabor_view(mh_ctx *ctx, const uint8_t *gray, int H, int W, const double *w_lo, int r_lo, const double *w_hi,
                             int r_hi, void *scratch, int32_t *orient_index, float *conf, float *variance, uint8_t *k8,
                             uint8_t *c8, void *stream) {
    if (!ctx || !gray || !scratch || !orient_index || !variance || H < 1 || W < 1)
        return fail(MH_ERR_ARG, "mh_gabor_view: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dog_weights(ctx, w_lo, r_lo, w_hi, r_hi, st)) return rc;
    if (!ctx->gabor) {
        int rc = gabor_alloc(ctx);
        if (rc) return rc;
        rc = launched(mh_launch_gabor_build(ctx->gabor, st), "mh_gabor_view(build)");
        if (rc) return rc;
        rc = launched(mh_launch_gabor_relayout(ctx->gabor, ctx->gabor_q, st), "mh_gabor_view(relayout)");
        if (rc) return rc;
    }
    char *base = (char *)scratch;
    double *planes = (double *)base;
    float *dog32 = (float *)(base + (size_t)H * W * 16);
    unsigned int *maxbits = (unsigned int *)(base + (size_t)H * W * 20);
    if (int rc = launched(mh_launch_dog(gray, 0, H, W, ctx->dog_w, planes, nullptr, dog32, st), "mh_gabor_view(dog)")) return rc;
    return launched(mh_launch_gabor_bank(ctx->gabor, ctx->gabor_q, dog32, H, W, orient_index, conf, variance, maxbits,
                                         ctx->gabor_variant, k8, c8, st),
                    "mh_gabor_view");
}
