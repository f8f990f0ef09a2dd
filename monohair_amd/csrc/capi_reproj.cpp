// capi_reproj.cpp -- C ABI of the capture agreement (csrc/hairreproj.hip; no counterpart in the reference)
#include <cstring>

#include "mh_capi.h"

// scratch of mh_support_view: the shared front (mh_capi.h) | zmin
struct SupportScratch : ViewScratch {
    float *zmin;
    SupportScratch(int n, int H, int W, void *base) : ViewScratch(n, base) { zmin = take<float>((size_t)H * W * 4); }
};

extern "C" size_t mh_support_scratch_bytes(int n_points, int H, int W) {
    if (n_points < 0 || !image_fits_int32(H, W)) return 0;
    return SupportScratch(n_points, H, W, nullptr).bytes;
}

extern "C" int mh_support_accumulate(mh_ctx *ctx, const float *vert, const uint8_t *valid, const long long *offsets,
                                     int n_strands, int n_points, int H, int W, float tol, const float *depth0,
                                     const float *zmin, const uint8_t *ori_u8, const uint8_t *conf_u8, const uint8_t *mask_u8,
                                     int conf_min_code, const float *table_host, const double *bounds_host, int n_bounds,
                                     long long *strand_counts, long long *view_counts, void *stream) {
    if (!ctx || !zmin || !ori_u8 || !conf_u8 || !mask_u8 || !table_host || !bounds_host || !view_counts ||
        !strands_ok(vert, valid, offsets, n_strands, n_points) || (n_points > 0 && !strand_counts) ||
        !image_fits_int32(H, W) || !(tol >= 0.0f) || n_bounds < 1 || n_bounds > MH_SUP_MAX_BOUNDS || conf_min_code < 0 ||
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
    if (!ctx || !zmin || !mask_u8 || !silhouette || !image_fits_int32(H, W))
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
    if (!ctx || !scratch || n_points < 0 || !image_fits_int32(H, W) || (n_points > 0 && !points) || radius < 0 ||
        radius > MH_MAX_RADIUS)
        return fail(MH_ERR_ARG, "mh_support_view: bad arguments");
    const size_t need = mh_support_scratch_bytes(n_points, H, W);
    if (scratch_bytes < need) return fail(MH_ERR_ARG, "mh_support_view: scratch too small (%zu < %zu)", scratch_bytes, need);
    const SupportScratch s(n_points, H, W, scratch);
    int rc = mh_capture_project(ctx, cam_host, points, n_points, H, W, s.vert, s.valid, stream);
    if (rc == MH_OK)
        rc = mh_capture_zmin(ctx, s.vert, s.valid, offsets, n_strands, n_points, H, W, radius, depth0, s.zmin, s.dropped,
                             stream);
    if (rc == MH_OK)
        rc = mh_support_accumulate(ctx, s.vert, s.valid, offsets, n_strands, n_points, H, W, tol, depth0, s.zmin, ori_u8,
                                   conf_u8, mask_u8, conf_min_code, table_host, bounds_host, n_bounds, strand_counts,
                                   view_counts, stream);
    if (rc == MH_OK) rc = mh_support_silhouette(ctx, s.zmin, mask_u8, H, W, silhouette, stream);
    return rc;
}
