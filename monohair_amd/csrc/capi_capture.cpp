// capi_capture.cpp -- C ABI of the hair capture (csrc/haircapture.hip; no counterpart in the reference)
#include <cstring>

#include "mh_capi.h"

// scratch of mh_capture_view: the shared front (mh_capi.h) | zmin | cnt | c2 | s2
struct CaptureScratch : ViewScratch {
    float *zmin;
    int32_t *cnt;
    long long *c2, *s2;
    CaptureScratch(int n_points, int H, int W, void *base) : ViewScratch(n_points, base) {
        const size_t npix = (size_t)H * W;
        zmin = take<float>(npix * 4), cnt = take<int32_t>(npix * 4);
        c2 = take<long long>(npix * 8), s2 = take<long long>(npix * 8);
    }
};

extern "C" size_t mh_capture_scratch_bytes(int n_points, int H, int W) {
    if (n_points < 0 || !image_fits_int32(H, W)) return 0;
    return CaptureScratch(n_points, H, W, nullptr).bytes;
}

extern "C" int mh_capture_project(mh_ctx *ctx, const float *cam_host, const float *points, int n_points, int H, int W,
                                  float *vert, uint8_t *valid, void *stream) {
    if (n_points == 0) return MH_OK;
    if (!ctx || !cam_host || !points || !vert || !valid || n_points < 0 || !image_fits_int32(H, W))
        return fail(MH_ERR_ARG, "mh_capture_project: bad arguments");
    MhCapCam cam;
    memcpy(cam.c, cam_host, sizeof(cam.c));
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_capture_project(cam, points, n_points, H, W, vert, valid, (hipStream_t)stream),
                    "mh_capture_project");
}

extern "C" int mh_capture_zmin(mh_ctx *ctx, const float *vert, const uint8_t *valid, const long long *offsets, int n_strands,
                               int n_points, int H, int W, int radius, const float *depth0, float *zmin, int32_t *dropped,
                               void *stream) {
    if (!ctx || !zmin || !dropped || !strands_ok(vert, valid, offsets, n_strands, n_points) || !image_fits_int32(H, W) ||
        radius < 0 || radius > MH_MAX_RADIUS)
        return fail(MH_ERR_ARG, "mh_capture_zmin: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_capture_zmin(vert, valid, (const int64_t *)offsets, n_strands, n_points, H, W, radius, depth0,
                                           zmin, dropped, (hipStream_t)stream),
                    "mh_capture_zmin");
}

extern "C" int mh_capture_accumulate(mh_ctx *ctx, const float *vert, const uint8_t *valid, const long long *offsets,
                                     int n_strands, int n_points, int H, int W, int radius, float tol, const float *depth0,
                                     const float *zmin, int32_t *cnt, long long *c2, long long *s2, void *stream) {
    if (!ctx || !zmin || !cnt || !c2 || !s2 || !strands_ok(vert, valid, offsets, n_strands, n_points) ||
        !image_fits_int32(H, W) || radius < 0 || radius > MH_MAX_RADIUS || !(tol >= 0.0f))
        return fail(MH_ERR_ARG, "mh_capture_accumulate: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_capture_accum(vert, valid, (const int64_t *)offsets, n_strands, n_points, H, W, radius, tol,
                                            depth0, zmin, cnt, c2, s2, (hipStream_t)stream),
                    "mh_capture_accumulate");
}

extern "C" int mh_capture_resolve(mh_ctx *ctx, const float *zmin, const int32_t *cnt, const long long *c2,
                                  const long long *s2, const float *depth0, const float *table_host, int n_full, int H, int W,
                                  float *depth, uint8_t *ori_u8, uint8_t *conf_u8, uint8_t *mask_u8, void *stream) {
    if (!ctx || !zmin || !cnt || !c2 || !s2 || !table_host || !depth || !ori_u8 || !conf_u8 || !mask_u8 || n_full < 1 ||
        !image_fits_int32(H, W))
        return fail(MH_ERR_ARG, "mh_capture_resolve: bad arguments");
    MhCapTable tab;
    memcpy(tab.t, table_host, sizeof(tab.t));
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_capture_resolve(zmin, cnt, c2, s2, depth0, tab, n_full, H, W, depth, ori_u8, conf_u8, mask_u8,
                                              (hipStream_t)stream),
                    "mh_capture_resolve");
}

extern "C" int mh_capture_view(mh_ctx *ctx, const float *cam_host, const float *points, const long long *offsets,
                               int n_strands, int n_points, int H, int W, int radius, float tol, int n_full,
                               const float *depth0, const float *table_host, void *scratch, size_t scratch_bytes,
                               float *depth, uint8_t *ori_u8, uint8_t *conf_u8, uint8_t *mask_u8, void *stream) {
    if (!ctx || !scratch || n_points < 0 || !image_fits_int32(H, W) || (n_points > 0 && !points))
        return fail(MH_ERR_ARG, "mh_capture_view: bad arguments");
    const size_t need = mh_capture_scratch_bytes(n_points, H, W);
    if (scratch_bytes < need) return fail(MH_ERR_ARG, "mh_capture_view: scratch too small (%zu < %zu)", scratch_bytes, need);
    const CaptureScratch s(n_points, H, W, scratch);
    int rc = mh_capture_project(ctx, cam_host, points, n_points, H, W, s.vert, s.valid, stream);
    if (rc == MH_OK)
        rc = mh_capture_zmin(ctx, s.vert, s.valid, offsets, n_strands, n_points, H, W, radius, depth0, s.zmin, s.dropped,
                             stream);
    if (rc == MH_OK)
        rc = mh_capture_accumulate(ctx, s.vert, s.valid, offsets, n_strands, n_points, H, W, radius, tol, depth0, s.zmin,
                                   s.cnt, s.c2, s.s2, stream);
    if (rc == MH_OK)
        rc = mh_capture_resolve(ctx, s.zmin, s.cnt, s.c2, s.s2, depth0, table_host, n_full, H, W, depth, ori_u8, conf_u8,
                                mask_u8, stream);
    return rc;
}

// ---- the photograph rule

#define MH_PHOTO_MAX_WIDTH 16

static bool photo_grid_ok(int H, int W, int ss) {
    return H >= 1 && W >= 1 && (ss == 1 || ss == 2 || ss == 4 || ss == 8) && (long long)H * ss * W * ss < (1ll << 31);
}

static bool photo_code_ok(int code) { return code >= 0 && code <= 255; }

// scratch of mh_photo_view: the shared front (mh_capi.h) | shade | keys
struct PhotoScratch : ViewScratch {
    uint8_t *shade;
    unsigned long long *keys;
    PhotoScratch(int n_points, int H, int W, int ss, void *base) : ViewScratch(n_points, base) {
        shade = take<uint8_t>(n), keys = take<unsigned long long>((size_t)H * ss * W * ss * 8);
    }
};

extern "C" size_t mh_photo_scratch_bytes(int n_points, int H, int W, int supersample) {
    if (n_points < 0 || !photo_grid_ok(H, W, supersample)) return 0;
    return PhotoScratch(n_points, H, W, supersample, nullptr).bytes;
}

extern "C" int mh_photo_shade(mh_ctx *ctx, const float *points, const uint8_t *valid, const long long *offsets, int n_strands,
                              int n_points, const float *albedo, const double *light_host, double ambient, uint8_t *shade,
                              void *stream) {
    if (n_points == 0 && n_strands >= 0) return MH_OK;      // (local: an empty set is accepted before any other argument is read)
    if (!ctx || !strands_ok(points, valid, offsets, n_strands, n_points) || !albedo || !light_host || !shade ||
        !(ambient >= 0.0 && ambient <= 1.0))
        return fail(MH_ERR_ARG, "mh_photo_shade: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_photo_shade(points, valid, (const int64_t *)offsets, n_strands, n_points, albedo, light_host[0],
                                          light_host[1], light_host[2], ambient, shade, (hipStream_t)stream),
                    "mh_photo_shade");
}

extern "C" int mh_photo_front(mh_ctx *ctx, const float *vert, const uint8_t *valid, const long long *offsets, int n_strands,
                              int n_points, const uint8_t *shade, int H, int W, int supersample, int width,
                              const float *depth0, unsigned long long *keys, int32_t *dropped, void *stream) {
    if (!ctx || !keys || !dropped || !strands_ok(vert, valid, offsets, n_strands, n_points) || (n_points > 0 && !shade) ||
        !photo_grid_ok(H, W, supersample) || width < 0 || width > MH_PHOTO_MAX_WIDTH)
        return fail(MH_ERR_ARG, "mh_photo_front: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_photo_front(vert, valid, (const int64_t *)offsets, n_strands, n_points, shade, H, W, supersample,
                                          width, depth0, keys, dropped, (hipStream_t)stream),
                    "mh_photo_front");
}

extern "C" int mh_photo_resolve(mh_ctx *ctx, const unsigned long long *keys, const float *depth0, int H, int W,
                                int supersample, int bust_code, int background_code, uint8_t *gray_u8, int32_t *cover,
                                void *stream) {
    if (!ctx || !keys || !gray_u8 || !photo_grid_ok(H, W, supersample) || !photo_code_ok(bust_code) ||
        !photo_code_ok(background_code))
        return fail(MH_ERR_ARG, "mh_photo_resolve: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_photo_resolve(keys, depth0, H, W, supersample, bust_code, background_code, gray_u8, cover,
                                            (hipStream_t)stream),
                    "mh_photo_resolve");
}

extern "C" int mh_photo_view(mh_ctx *ctx, const float *cam_host, const float *points, const long long *offsets, int n_strands,
                             int n_points, const float *albedo, const double *light_host, double ambient, int H, int W,
                             int supersample, int width, const float *depth0, int bust_code, int background_code,
                             void *scratch, size_t scratch_bytes, uint8_t *gray_u8, int32_t *cover, void *stream) {
    if (!ctx || !scratch || n_points < 0 || !photo_grid_ok(H, W, supersample) || (n_points > 0 && !points))
        return fail(MH_ERR_ARG, "mh_photo_view: bad arguments");
    const size_t need = mh_photo_scratch_bytes(n_points, H, W, supersample);
    if (scratch_bytes < need) return fail(MH_ERR_ARG, "mh_photo_view: scratch too small (%zu < %zu)", scratch_bytes, need);
    const PhotoScratch s(n_points, H, W, supersample, scratch);
    int rc = mh_capture_project(ctx, cam_host, points, n_points, H, W, s.vert, s.valid, stream);
    if (rc == MH_OK)
        rc = mh_photo_shade(ctx, points, s.valid, offsets, n_strands, n_points, albedo, light_host, ambient, s.shade, stream);
    if (rc == MH_OK)
        rc = mh_photo_front(ctx, s.vert, s.valid, offsets, n_strands, n_points, s.shade, H, W, supersample, width, depth0,
                            s.keys, s.dropped, stream);
    if (rc == MH_OK)
        rc = mh_photo_resolve(ctx, s.keys, depth0, H, W, supersample, bust_code, background_code, gray_u8, cover, stream);
    return rc;
}
