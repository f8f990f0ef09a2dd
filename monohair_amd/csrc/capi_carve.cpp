// capi_carve.cpp -- C ABI of the silhouette carve (csrc/haircarve.hip; include/mh_pmvo.h, "Silhouette carve"): the hull of the
// hair masks as vote counts, as flags and as a mesh; no counterpart in the reference
#include "mh_capi.h"

// a grid whose cells AND corners an int32 can index
static bool carve_mesh_dims_ok(const int32_t *dims) {
    if (!vol_dims_ok(dims)) return false;
    const long long xy = ((long long)dims[0] + 1) * ((long long)dims[1] + 1);      // (below 2^62: no overflow)
    return xy < (1ll << 31) && xy * ((long long)dims[2] + 1) < (1ll << 31);
}

static bool carve_views_set(const mh_ctx *ctx) { return ctx && ctx->mask && ctx->cams && ctx->V >= 1; }

extern "C" int mh_carve_votes(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size, const int32_t *dims,
                              int32_t *counts, void *stream) {
    if (!carve_views_set(ctx)) return fail(MH_ERR_STATE, "mh_carve_votes: views not set");
    MhVolGrid gr;
    if (!bust || !counts || !vol_grid(&gr, voxel_min, voxel_size, dims)) return fail(MH_ERR_ARG, "mh_carve_votes: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_carve_votes(ctx->views(), bust, gr, counts, (hipStream_t)stream), "mh_carve_votes");
}

extern "C" int mh_carve_inside(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size, const int32_t *dims,
                               int min_free, int max_miss, uint8_t *flags, void *stream) {
    if (!carve_views_set(ctx)) return fail(MH_ERR_STATE, "mh_carve_inside: views not set");
    MhVolGrid gr;
    if (!bust || !flags || min_free < 1 || max_miss < 0 || !vol_grid(&gr, voxel_min, voxel_size, dims))
        return fail(MH_ERR_ARG, "mh_carve_inside: bad arguments (min_free >= 1, max_miss >= 0)");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_carve_inside(ctx->views(), bust, gr, min_free, max_miss, ctx->carve_early_exit, flags,
                                           (hipStream_t)stream),
                    "mh_carve_inside");
}

extern "C" size_t mh_carve_mesh_scratch_bytes(const int32_t *dims) {
    return carve_mesh_dims_ok(dims) ? mh_carve_mesh_scratch_bytes_impl(dims[0], dims[1], dims[2]) : 0;
}

extern "C" int mh_carve_mesh_count(mh_ctx *ctx, const uint8_t *flags, const int32_t *dims, long long *counts, void *scratch,
                                   size_t scratch_bytes, void *stream) {
    if (!carve_mesh_dims_ok(dims))
        return fail(MH_ERR_ARG, "mh_carve_mesh_count: dims must have X*Y*Z and (X+1)*(Y+1)*(Z+1) below 2^31");
    if (!ctx || !flags || !counts || !scratch || scratch_bytes < mh_carve_mesh_scratch_bytes(dims))
        return fail(MH_ERR_ARG, "mh_carve_mesh_count: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_carve_mesh_count(flags, dims[0], dims[1], dims[2], scratch, counts, (hipStream_t)stream),
                    "mh_carve_mesh_count");
}

extern "C" int mh_carve_mesh(mh_ctx *ctx, const uint8_t *flags, const double *voxel_min, double voxel_size, const int32_t *dims,
                             long long n_vertices, long long n_triangles, float *vertices, int32_t *faces, void *scratch,
                             size_t scratch_bytes, void *stream) {
    if (!carve_mesh_dims_ok(dims))
        return fail(MH_ERR_ARG, "mh_carve_mesh: dims must have X*Y*Z and (X+1)*(Y+1)*(Z+1) below 2^31");
    MhVolGrid gr;
    if (!ctx || !flags || !vol_grid(&gr, voxel_min, voxel_size, dims) || n_vertices < 0 || n_triangles < 0 ||
        (n_vertices > 0 && !vertices) || (n_triangles > 0 && !faces) || !scratch ||
        scratch_bytes < mh_carve_mesh_scratch_bytes(dims))
        return fail(MH_ERR_ARG, "mh_carve_mesh: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_carve_mesh(flags, gr, scratch, n_vertices, n_triangles, vertices, faces, (hipStream_t)stream),
                    "mh_carve_mesh");
}
