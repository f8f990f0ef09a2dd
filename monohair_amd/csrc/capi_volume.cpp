// capi_volume.cpp -- C ABI of the strand volume, the volume scores (csrc/hairvolume.hip) and the inner fill (csrc/hairfill.hip);
// none has a counterpart in the reference
#include <cmath>

#include "mh_capi.h"

extern "C" int mh_strand_volume_accumulate(mh_ctx *ctx, const float *points, const long long *offsets, int n_strands,
                                           int n_points, const double *bust_to_origin, const double *voxel_min,
                                           double voxel_size, const int32_t *dims, int sub, long long *acc, uint8_t *occ,
                                           long long *counters, void *stream) {
    if (!ctx || !bust_to_origin || !voxel_min || !vol_dims_ok(dims) || !acc || !occ || !counters ||
        !strands_ok(points, nullptr, offsets, n_strands, n_points, /*has_valid=*/false) || sub < 1 || sub > 16 ||
        !(voxel_size > 0.0 && std::isfinite(voxel_size)))
        return fail(MH_ERR_ARG, "mh_strand_volume_accumulate: bad arguments");
    MhVolGrid gr;      // (what is left for vol_grid to refuse here is a value that is not finite)
    if (!vol_grid(&gr, voxel_min, voxel_size, dims, bust_to_origin))
        return fail(MH_ERR_ARG, "mh_strand_volume_accumulate: bust_to_origin and voxel_min must be finite");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_strand_volume_accum(points, (const int64_t *)offsets, n_strands, n_points, gr, sub,
                                                  (unsigned long long *)acc, occ, (unsigned long long *)counters,
                                                  (hipStream_t)stream),
                    "mh_strand_volume_accumulate");
}

extern "C" int mh_strand_volume_resolve(mh_ctx *ctx, const long long *acc, const int32_t *index, int n_voxels,
                                        const int32_t *dims, long long *voxels, float *ori, int32_t *cnt, double *coh,
                                        long long *sums, int32_t *refused, void *stream) {
    if (!ctx || !acc || !vol_dims_ok(dims) || !refused || n_voxels < 0 ||
        (n_voxels > 0 && (!index || !voxels || !ori || !cnt || !coh)))
        return fail(MH_ERR_ARG, "mh_strand_volume_resolve: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_strand_volume_resolve(acc, index, n_voxels, dims[1], dims[2], voxels, ori, cnt, coh, sums,
                                                    refused, (hipStream_t)stream),
                    "mh_strand_volume_resolve");
}

extern "C" int mh_volume_index(mh_ctx *ctx, const long long *voxels, int n_voxels, const int32_t *dims, int32_t *index,
                               int32_t *status, void *stream) {
    if (!ctx || !vol_dims_ok(dims) || !index || !status || n_voxels < 0 || (n_voxels > 0 && !voxels))
        return fail(MH_ERR_ARG, "mh_volume_index: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_volume_index(voxels, n_voxels, dims[0], dims[1], dims[2], index, status, (hipStream_t)stream),
                    "mh_volume_index");
}

extern "C" int mh_volume_match(mh_ctx *ctx, const long long *q_voxels, const float *q_ori, int nq, const int32_t *t_index,
                               const float *t_ori, const int32_t *dims, const int32_t *reach, const double *cos2, int n_pairs,
                               uint8_t *out_flags, void *stream) {
    if (nq == 0) return MH_OK;
    if (!ctx || !q_voxels || !q_ori || nq < 0 || !t_index || !vol_dims_ok(dims) || !reach || !cos2 || n_pairs < 1 ||
        n_pairs > MH_VOL_MAXK || !out_flags)
        return fail(MH_ERR_ARG, "mh_volume_match: bad arguments");
    MhVolPairs pr;
    pr.K = n_pairs;
    for (int k = 0; k < MH_VOL_MAXK; ++k) {
        pr.reach[k] = k < n_pairs ? reach[k] : 0;
        pr.cos2[k] = k < n_pairs ? cos2[k] : 0.0;
        if (k < n_pairs && (reach[k] < 0 || reach[k] > MH_VOL_MAXREACH || std::isnan(cos2[k])))
            return fail(MH_ERR_ARG, "mh_volume_match: pair %d: reach %d (0..%d), cos2 %g", k, reach[k], MH_VOL_MAXREACH,
                        cos2[k]);
    }
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_volume_match(q_voxels, q_ori, nq, t_index, t_ori, dims[0], dims[1], dims[2], pr, out_flags,
                                           (hipStream_t)stream),
                    "mh_volume_match");
}

// ---- the inner fill (csrc/hairfill.hip; include/mh_pmvo.h, "Inner fill")
extern "C" int mh_inner_votes(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size, const int32_t *dims,
                              int32_t *counts, void *stream) {
    if (!ctx || !ctx->rec || !ctx->mask || !ctx->cams || ctx->V < 1) return fail(MH_ERR_STATE, "mh_inner_votes: views not set");
    MhVolGrid gr;
    if (!bust || !counts || !vol_grid(&gr, voxel_min, voxel_size, dims)) return fail(MH_ERR_ARG, "mh_inner_votes: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_inner_votes(ctx->views(), bust, gr, counts, (hipStream_t)stream), "mh_inner_votes");
}

extern "C" int mh_inner_domain(mh_ctx *ctx, const int32_t *counts, const int32_t *ext_index, const int32_t *dims, int max_bad,
                               uint8_t *flags, void *stream) {
    if (!ctx || !counts || !vol_dims_ok(dims) || !flags || max_bad < 0) return fail(MH_ERR_ARG, "mh_inner_domain: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_inner_domain(counts, ext_index, (size_t)dims[0] * dims[1] * dims[2], max_bad, flags,
                                           (hipStream_t)stream),
                    "mh_inner_domain");
}

extern "C" int mh_inner_diffuse(mh_ctx *ctx, const long long *ext_voxels, const float *ext_ori, int n_ext,
                                const long long *dom_voxels, int n_dom, const int32_t *dims, int sweeps, int32_t *map,
                                double *ext_tensor, uint8_t *ext_source, int32_t *cell, double *tensor, double *tensor_b,
                                uint8_t *known, uint8_t *known_b, int32_t *depth, int32_t *status, void *stream) {
    if (!ctx || !vol_dims_ok(dims) || !map || !status || n_ext < 0 || n_dom < 0 || sweeps < 0 || sweeps > MH_FILL_MAXSWEEPS ||
        (n_ext > 0 && (!ext_voxels || !ext_ori || !ext_tensor || !ext_source)) ||
        (n_dom > 0 && (!dom_voxels || !cell || !tensor || !tensor_b || !known || !known_b || !depth)))
        return fail(MH_ERR_ARG, "mh_inner_diffuse: bad arguments (0 <= sweeps <= %d)", MH_FILL_MAXSWEEPS);
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_inner_diffuse(ext_voxels, ext_ori, n_ext, dom_voxels, n_dom, dims[0], dims[1], dims[2], sweeps, map,
                                            ext_tensor, ext_source, cell, tensor, tensor_b, known, known_b, depth, status,
                                            (hipStream_t)stream),
                    "mh_inner_diffuse");
}

extern "C" int mh_inner_resolve(mh_ctx *ctx, const long long *dom_voxels, int n_dom, const double *tensor, const uint8_t *known,
                                const double *voxel_min, double voxel_size, const int32_t *dims, double min_coh, float *world,
                                float *ori, double *coh, uint8_t *emit, void *stream) {
    if (n_dom == 0) return MH_OK;
    MhVolGrid gr;
    if (!ctx || n_dom < 0 || !dom_voxels || !tensor || !known || !vol_grid(&gr, voxel_min, voxel_size, dims) ||
        std::isnan(min_coh) || !world || !ori || !coh || !emit)
        return fail(MH_ERR_ARG, "mh_inner_resolve: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_inner_resolve(dom_voxels, n_dom, tensor, known, gr, min_coh, world, ori, coh, emit,
                                            (hipStream_t)stream),
                    "mh_inner_resolve");
}
