// capi_stereo.cpp -- C ABI of the photo-consistent carve (csrc/hairstereo.hip; include/mh_pmvo.h, "Photo-consistent carve"): census
// codes of the gray photographs, the winner keys per (view, cell), the agreement counts, the refined flags and the stereo depth
// planes; no counterpart in the reference
#include "mh_capi.h"

#define MH_STEREO_MAXK 8
#define MH_STEREO_MAXCELL 256

static bool stereo_views_set(const mh_ctx *ctx) { return ctx && ctx->mask && ctx->cams && ctx->V >= 1; }
static bool stereo_cell_ok(int cell) { return cell >= 1 && cell <= MH_STEREO_MAXCELL; }
static bool stereo_bounds_ok(int cell, int max_cost, float m255) {
    return stereo_cell_ok(cell) && max_cost >= 0 && std::isfinite(m255) && m255 >= 0.0f;
}

extern "C" int mh_stereo_census(mh_ctx *ctx, const uint8_t *gray, int n_views, int height, int width, int cell, int radius,
                                uint8_t *reduced, unsigned long long *census, void *stream) {
    if (!ctx || !gray || !reduced || !census || n_views < 1 || !image_fits_int32(height, width) ||
        (long long)n_views * height * width >= (1ll << 31) || !stereo_cell_ok(cell) || radius < 1 || radius > 3)
        return fail(MH_ERR_ARG, "mh_stereo_census: bad arguments (1 <= cell <= 256, radius in {1, 2, 3}, V*H*W < 2^31)");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_stereo_census(gray, n_views, height, width, cell, radius, reduced, census, (hipStream_t)stream),
                    "mh_stereo_census");
}

extern "C" int mh_stereo_winners(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size,
                                 const int32_t *dims, const int32_t *candidates, int n_candidates,
                                 const unsigned long long *census, const int32_t *neighbours, int n_neighbours, int cell,
                                 int radius, int keep, unsigned long long *keys, void *stream) {
    if (!stereo_views_set(ctx)) return fail(MH_ERR_STATE, "mh_stereo_winners: views not set");
    MhVolGrid gr;
    if (!bust || !census || !neighbours || !keys || n_candidates < 0 || (n_candidates > 0 && !candidates) ||
        n_neighbours < 1 || n_neighbours > MH_STEREO_MAXK || keep < 1 || keep > n_neighbours || !stereo_cell_ok(cell) ||
        radius < 1 || radius > 3 || !vol_grid(&gr, voxel_min, voxel_size, dims))
        return fail(MH_ERR_ARG, "mh_stereo_winners: bad arguments (1 <= keep <= n_neighbours <= 8, 1 <= cell <= 256, radius "
                                "in {1, 2, 3})");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_stereo_winners(ctx->views(), bust, gr, candidates, n_candidates, census, neighbours, n_neighbours,
                                             cell, radius, keep, keys, (hipStream_t)stream),
                    "mh_stereo_winners");
}

extern "C" int mh_stereo_agree(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size, const int32_t *dims,
                               const uint8_t *flags, const unsigned long long *keys, int cell, int max_cost, float m255,
                               int32_t *agree, void *stream) {
    if (!stereo_views_set(ctx)) return fail(MH_ERR_STATE, "mh_stereo_agree: views not set");
    MhVolGrid gr;
    if (!bust || !flags || !keys || !agree || !stereo_bounds_ok(cell, max_cost, m255) ||
        !vol_grid(&gr, voxel_min, voxel_size, dims))
        return fail(MH_ERR_ARG, "mh_stereo_agree: bad arguments (1 <= cell <= 256, max_cost >= 0, m255 finite and >= 0)");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_stereo_agree(ctx->views(), bust, gr, flags, keys, cell, max_cost, m255, agree,
                                           (hipStream_t)stream),
                    "mh_stereo_agree");
}

extern "C" int mh_stereo_refine(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size, const int32_t *dims,
                                const uint8_t *flags, const unsigned long long *keys, const int32_t *agree, int cell,
                                int max_cost, float m255, int min_agree, int min_through, uint8_t *refined, float *depth,
                                void *stream) {
    if (!stereo_views_set(ctx)) return fail(MH_ERR_STATE, "mh_stereo_refine: views not set");
    MhVolGrid gr;
    if (!bust || !flags || !keys || !agree || !refined || !depth || !stereo_bounds_ok(cell, max_cost, m255) || min_agree < 1 ||
        min_through < 1 || !vol_grid(&gr, voxel_min, voxel_size, dims))
        return fail(MH_ERR_ARG, "mh_stereo_refine: bad arguments (1 <= cell <= 256, max_cost >= 0, m255 finite and >= 0, "
                                "min_agree >= 1, min_through >= 1)");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_stereo_refine(ctx->views(), bust, gr, flags, keys, agree, cell, max_cost, m255, min_agree,
                                            min_through, refined, depth, (hipStream_t)stream),
                    "mh_stereo_refine");
}
