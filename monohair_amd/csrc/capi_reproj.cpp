// capi_reproj.cpp -- C ABI of the capture agreement (csrc/hairreproj.hip; no counterpart in the reference)
#include <cstring>

#include "mh_capi.h"

#define MH_SUP_MAX_RADIUS 16

static size_t sup_align(size_t b) { return (b + 255) / 256 * 256; }

static bool sup_image_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31); }

// scratch of mh_support_view: dropped 256 B | vert | valid | zmin
extern "C" size_t mh_support_scratch_bytes(int n_points, int H, int W) {
    if (n_points < 0 || !sup_image_ok(H, W)) return 0;
    const size_t n = (size_t)(n_points > 0 ? n_points : 1), npix = (size_t)H * W;
    return 256 + sup_align(n * 12) + sup_align(n) + sup_align(npix * 4);
}

extern "C" int mh_support_accumulate(mh_ctx *ctx, const float *vert, const uint8_t *valid, const long long *offsets,
                                     int n_strands, int n_points, int H, int W, float tol, const float *depth0,
                                     const float *zmin, const uint8_t *ori_u8, const uint8_t *conf_u8, const uint8_t *mask_u8,
                                     int conf_min_code, const float *table_host, const double *bounds_host, int n_bounds,
                                     long long *strand_counts, long long *view_counts, void *stream) {
    if (!ctx || !zmin || !ori_u8 || !conf_u8 || !mask_u8 || !table_host || !bounds_host || !view_counts || n_strands < 0 ||
        n_points < 0 || (n_points > 0 && (!vert || !valid || !offsets || n_strands < 1 || !strand_counts)) ||
        !sup_image_ok(H, W) || !(tol >= 0.0f) || n_bounds < 1 || n_bounds > MH_SUP_MAX_BOUNDS || conf_min_code < 0 ||
        conf_min_code > 256)
        return fail(MH_ERR_ARG, "mh_support_accumulate: bad arguments");
    MhCapTable tab;
    memcpy(tab.t, table_host, sizeof(tab.t));
    MhSupBounds bd;
    memset(&bd, 0, sizeof(bd));
    memcpy(bd.b, bounds_host, sizeof(double) * n_bounds);
    bd.n = n_bounds;
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_support_accum(vert, valid, (const int64_t *)offsets, n_strands, n_points, H, W, tol, depth0,
                                            zmin, ori_u8, conf_u8, mask_u8, conf_min_code, tab, bd,
                                            (unsigned long long *)strand_counts, (unsigned long long *)view_counts,
                                            (hipStream_t)stream),
                    "mh_support_accumulate");
}

extern "C" int mh_support_silhouette(mh_ctx *ctx, const float *zmin, const uint8_t *mask_u8, int H, int W,
                                     long long *silhouette, void *stream) {
    if (!ctx || !zmin || !mask_u8 || !silhouette || !sup_image_ok(H, W))
        return fail(MH_ERR_ARG, "mh_support_silhouette: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_support_silhouette(zmin, mask_u8, H, W, (unsigned long long *)silhouette, (hipStream_t)stream),
                    "mh_support_silhouette");
}

extern "C" int mh_support_view(mh_ctx *ctx, const float *cam_host, const float *points, const long long *offsets,
                               int n_strands, int n_points, int H, int W, int radius, float tol, const float *depth0,
                               const uint8_t *ori_u8, const uint8_t *conf_u8, const uint8_t *mask_u8, int conf_min_code,
                               const float *table_host, const double *bounds_host, int n_bounds, void *scratch,
                               size_t scratch_bytes, long long *strand_counts, long long *view_counts, long long *silhouette,
                               void *stream) {
    if (!ctx || !scratch || n_points < 0 || !sup_image_ok(H, W) || (n_points > 0 && !points) || radius < 0 ||
        radius > MH_SUP_MAX_RADIUS)
        return fail(MH_ERR_ARG, "mh_support_view: bad arguments");
    const size_t need = mh_support_scratch_bytes(n_points, H, W);
    if (scratch_bytes < need) return fail(MH_ERR_ARG, "mh_support_view: scratch too small (%zu < %zu)", scratch_bytes, need);
    const size_t n = (size_t)(n_points > 0 ? n_points : 1);
    char *base = (char *)scratch;
    int32_t *dropped = (int32_t *)base;
    float *vert = (float *)(base += 256);
    uint8_t *valid = (uint8_t *)(base += sup_align(n * 12));
    float *zmin = (float *)(base += sup_align(n));
    int rc = mh_capture_project(ctx, cam_host, points, n_points, H, W, vert, valid, stream);
    if (rc == MH_OK)
        rc = mh_capture_zmin(ctx, vert, valid, offsets, n_strands, n_points, H, W, radius, depth0, zmin, dropped, stream);
    if (rc == MH_OK)
        rc = mh_support_accumulate(ctx, vert, valid, offsets, n_strands, n_points, H, W, tol, depth0, zmin, ori_u8, conf_u8,
                                   mask_u8, conf_min_code, table_host, bounds_host, n_bounds, strand_counts, view_counts,
                                   stream);
    if (rc == MH_OK) rc = mh_support_silhouette(ctx, zmin, mask_u8, H, W, silhouette, stream);
    return rc;
}
