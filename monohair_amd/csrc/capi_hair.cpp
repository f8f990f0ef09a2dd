// capi_hair.cpp -- C ABI of the hair stage: trace, compact, connect, smooth, scalp, mesh sampling, diffusion, metrics
#include "mh_capi.h"

// ---- strand tracing on the fitted volume (HairGrow.py:59-299) ------------------------------------------------
extern "C" int mh_volume_pack(mh_ctx *ctx, const float *occ, const float *ori, int W, int H, int Z, void *vox,
                              void *stream) {
    if (!ctx || !occ || !ori || !vox || W < 1 || H < 1 || Z < 1) return fail(MH_ERR_ARG, "mh_volume_pack: bad arguments");
    return launched(mh_launch_pack_volume(occ, ori, (size_t)W * H * Z, (float4 *)vox, (hipStream_t)stream),
                    "mh_volume_pack");
}

extern "C" int mh_trace_seeds(mh_ctx *ctx, const void *vox, int W, int H, int Z, const float *seeds, int n,
                              float thr_dot, float *out, int32_t *first, int32_t *len, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !vox || !seeds || !out || !first || !len || n < 0) return fail(MH_ERR_ARG, "mh_trace_seeds: bad arguments");
    return launched(mh_launch_trace_seeds((const float4 *)vox, W, H, Z, seeds, n, thr_dot, out, first, len,
                                          (hipStream_t)stream),
                    "mh_trace_seeds");
}

extern "C" int mh_trace_scalp(mh_ctx *ctx, const void *vox, int W, int H, int Z, const float *seeds,
                              const float *normals, int n, float thr_dot, float *out, int32_t *len, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !vox || !seeds || !normals || !out || !len || n < 0)
        return fail(MH_ERR_ARG, "mh_trace_scalp: bad arguments");
    return launched(mh_launch_trace_scalp((const float4 *)vox, W, H, Z, seeds, normals, n, thr_dot, out, len,
                                          (hipStream_t)stream),
                    "mh_trace_scalp");
}

extern "C" int mh_strands_compact(mh_ctx *ctx, const float *rows, const int32_t *first, const int32_t *len,
                                  const long long *offsets, int n, int stride, float *packed, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !rows || !len || !offsets || !packed || n < 0 || stride < 1)
        return fail(MH_ERR_ARG, "mh_strands_compact: bad arguments");
    return launched(mh_launch_strands_compact(rows, first, len, (const int64_t *)offsets, n, stride, packed,
                                              (hipStream_t)stream),
                    "mh_strands_compact");
}

// ---- segment connection and smoothing (HairGrow.py:303-590, Utils/Utils.py:1148-1198), float64 ----------------------
extern "C" int mh_end_knn64(mh_ctx *ctx, const double *q, const int32_t *qcell, int nq, const double *data,
                            const int32_t *order, const int32_t *cstart, int gx, int gy, int gz, double bound,
                            int skip_self, int32_t *out_idx, double *out_dist, int32_t *out_cnt, void *stream) {
    if (nq == 0) return MH_OK;
    if (!ctx || !q || !qcell || !data || !order || !cstart || !out_idx || !out_dist || !out_cnt || nq < 0 ||
        !cells_fit_int32(gx, gy, gz) || !(bound > 0.0))
        return fail(MH_ERR_ARG, "mh_end_knn64: bad arguments");
    return launched(mh_launch_end_knn64(q, qcell, nq, data, order, cstart, gx, gy, gz, bound * bound, skip_self, out_idx,
                                        out_dist, out_cnt, (hipStream_t)stream),
                    "mh_end_knn64");
}

extern "C" int mh_connect_candidates(mh_ctx *ctx, const double *pts, const long long *offsets, int n,
                                     const int32_t *const *nei_idx, const double *const *nei_dist,
                                     const int32_t *const *nei_cnt, double dot_threshold, int32_t *best,
                                     int32_t *best_type, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !pts || !offsets || !nei_idx || !nei_dist || !nei_cnt || !best || !best_type || n < 0 ||
        n > (1 << 29))
        return fail(MH_ERR_ARG, "mh_connect_candidates: bad arguments");
    for (int t = 0; t < 4; ++t)
        if (!nei_idx[t] || !nei_dist[t] || !nei_cnt[t]) return fail(MH_ERR_ARG, "mh_connect_candidates: list %d is NULL", t);
    return launched(mh_launch_connect_cand(pts, (const int64_t *)offsets, n, nei_idx, nei_dist, nei_cnt, dot_threshold,
                                           best, best_type, (hipStream_t)stream),
                    "mh_connect_candidates");
}

extern "C" int mh_chain_count(mh_ctx *ctx, const long long *offsets, int n, const int32_t *best, const int32_t *best_type,
                              long long *total, long long *root_len, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !offsets || !best || !best_type || !total || !root_len || n < 0)
        return fail(MH_ERR_ARG, "mh_chain_count: bad arguments");
    return launched(mh_launch_chain_count((const int64_t *)offsets, n, best, best_type, (int64_t *)total,
                                          (int64_t *)root_len, (hipStream_t)stream),
                    "mh_chain_count");
}

extern "C" int mh_chain_emit(mh_ctx *ctx, const double *pts, const long long *offsets, int n, const int32_t *best,
                             const int32_t *best_type, const long long *root_len, const long long *out_offsets,
                             double *out, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !pts || !offsets || !best || !best_type || !root_len || !out_offsets || !out || n < 0)
        return fail(MH_ERR_ARG, "mh_chain_emit: bad arguments");
    return launched(mh_launch_chain_emit(pts, (const int64_t *)offsets, n, best, best_type, (const int64_t *)root_len,
                                         (const int64_t *)out_offsets, out, (hipStream_t)stream),
                    "mh_chain_emit");
}

extern "C" int mh_occ_check(mh_ctx *ctx, const double *pts, const long long *offsets, int n, const float *occ,
                            long long occ_stride, int W, int H, int Z, double vmin_x, double vmin_y, double vmin_z,
                            double voxel_size, int32_t *status, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !pts || !offsets || !occ || !status || n < 0 || occ_stride < 1 || W < 1 || H < 1 || Z < 1)
        return fail(MH_ERR_ARG, "mh_occ_check: bad arguments");
    return launched(mh_launch_occ_check(pts, (const int64_t *)offsets, n, occ, occ_stride, W, H, Z, vmin_x, vmin_y, vmin_z,
                                        voxel_size, status, (hipStream_t)stream),
                    "mh_occ_check");
}

extern "C" int mh_smooth_strands(mh_ctx *ctx, double *pts, const long long *offsets, int n, double lap_constraint,
                                 double pos_constraint, double *work, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !pts || !offsets || !work || n < 0) return fail(MH_ERR_ARG, "mh_smooth_strands: bad arguments");
    return launched(mh_launch_smooth(pts, (const int64_t *)offsets, n, lap_constraint, pos_constraint, work,
                                     (hipStream_t)stream),
                    "mh_smooth_strands");
}

// ---- scalp attachment (HairGrow.py:606-812): one pass of connect_to_scalp's while loop ---------------------------------
static bool scalp_grid_ok(const float *grid, const int32_t *dims) {
    return grid && dims && grid[3] > 0.0f && cells_fit_int32(dims[0], dims[1], dims[2]);
}

extern "C" int mh_scalp_ball_count(mh_ctx *ctx, const float *pts, const long long *offsets, const int32_t *active,
                                   int n_active, const float *core, int n_core, const int32_t *order,
                                   const int32_t *cell_start, const float *grid, const int32_t *dims, double thr_dist,
                                   long long *count, void *stream) {
    if (n_active == 0) return MH_OK;
    if (!ctx || !pts || !offsets || !active || !core || !order || !cell_start || !count || n_active < 0 || n_core < 1 ||
        !scalp_grid_ok(grid, dims) || !(thr_dist > 0.0) || !((double)grid[3] > thr_dist))
        return fail(MH_ERR_ARG, "mh_scalp_ball_count: bad arguments");
    return launched(mh_launch_scalp_ball_count(pts, (const int64_t *)offsets, active, n_active, core, order, cell_start,
                                               grid, dims, thr_dist, (int64_t *)count, (hipStream_t)stream),
                    "mh_scalp_ball_count");
}

extern "C" int mh_scalp_choose(mh_ctx *ctx, const float *pts, const long long *offsets, const int32_t *active, int n_active,
                               const float *core, const int32_t *core_strand, const int32_t *core_rank, int n_core,
                               const int32_t *order, const int32_t *cell_start, const float *grid, const int32_t *dims,
                               double thr_dist, double thr_dot, const double *out_ratio, const long long *ball_offsets,
                               unsigned long long *ball_scratch, uint8_t *flip, int32_t *best_strand, int32_t *best_index,
                               void *stream) {
    if (n_active == 0) return MH_OK;
    if (!ctx || !pts || !offsets || !active || !core || !core_strand || !core_rank || !order || !cell_start ||
        !out_ratio || !ball_offsets || !ball_scratch || !flip || !best_strand || !best_index || n_active < 0 ||
        n_core < 1 || !scalp_grid_ok(grid, dims) || !(thr_dist > 0.0) || !((double)grid[3] > thr_dist))
        return fail(MH_ERR_ARG, "mh_scalp_choose: bad arguments");
    return launched(mh_launch_scalp_choose(pts, (const int64_t *)offsets, active, n_active, core, core_strand, core_rank,
                                           order, cell_start, grid, dims, thr_dist, thr_dot, out_ratio,
                                           (const int64_t *)ball_offsets, ball_scratch, flip, best_strand, best_index,
                                           (hipStream_t)stream),
                    "mh_scalp_choose");
}

extern "C" int mh_scalp_emit(mh_ctx *ctx, const float *pts, const long long *offsets, int n, const uint8_t *flip,
                             const int32_t *best_strand, const int32_t *best_index, const long long *new_offsets,
                             const float *vox, int W, int H, int Z, double out_ratio_threshold, float *new_pts,
                             uint8_t *flags, double *out_ratio, float *similar, int32_t *counters, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !pts || !offsets || !flip || !best_strand || !best_index || !new_offsets || !vox || !new_pts || !flags ||
        !out_ratio || !similar || !counters || n < 0 || W < 1 || H < 1 || Z < 1)
        return fail(MH_ERR_ARG, "mh_scalp_emit: bad arguments");
    return launched(mh_launch_scalp_emit(pts, (const int64_t *)offsets, n, flip, best_strand, best_index,
                                         (const int64_t *)new_offsets, (const float4 *)vox, W, H, Z, out_ratio_threshold,
                                         new_pts, flags, out_ratio, similar, counters, (hipStream_t)stream),
                    "mh_scalp_emit");
}

// ---- scalp sampling (HairGrow.py:880-897) ---------------------------------------------------------------------------
extern "C" int mh_tri_area64(mh_ctx *ctx, const double *vertices, int nv, const int32_t *faces, int nf, double *area,
                             void *stream) {
    if (nf == 0) return MH_OK;
    if (!ctx || !vertices || !faces || !area || nv < 1 || nf < 0) return fail(MH_ERR_ARG, "mh_tri_area64: bad arguments");
    return launched(mh_launch_tri_area64(vertices, faces, nf, area, (hipStream_t)stream), "mh_tri_area64");
}

extern "C" int mh_mesh_sample(mh_ctx *ctx, const double *vertices, const double *normals, int nv, const int32_t *faces,
                              int nf, const long long *bounds, const double *uniforms, int n, const double *bust_to_origin,
                              float *out_points, float *out_normals, int32_t *out_triangle, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !vertices || !normals || !faces || !bounds || !uniforms || !bust_to_origin || !out_points || !out_normals ||
        nv < 1 || nf < 1 || n < 0)
        return fail(MH_ERR_ARG, "mh_mesh_sample: bad arguments");
    // points_to_voxel's voxel_min is a float32 tensor that promotes against the float64 points; its voxel size is 0.005 / 2
    const double vmin[3] = {(double)-0.32f, (double)-0.32f, (double)-0.24f};
    return launched(mh_launch_mesh_sample(vertices, normals, faces, nf, (const int64_t *)bounds, uniforms, n, bust_to_origin,
                                          vmin, 0.005 / 2, out_points, out_normals, out_triangle, (hipStream_t)stream),
                    "mh_mesh_sample");
}

// ---- scalp diffusion (Utils/PMVO_utils.py:467-593) ------------------------------------------------------------------
extern "C" int mh_diffuse_walk(mh_ctx *ctx, const float *occ, const float *ori, int W, int H, int Z, const float *points,
                               const float *normals, int n, int32_t *status, int32_t *steps, float *end_points,
                               float *first_normals, float *last_normals, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !occ || !ori || !points || !normals || !status || !steps || !end_points || !first_normals ||
        !last_normals || n < 0 || !cells_fit_int32(W, H, Z))
        return fail(MH_ERR_ARG, "mh_diffuse_walk: bad arguments");
    return launched(mh_launch_diffuse_walk(occ, ori, W, H, Z, points, normals, n, status, steps, end_points, first_normals,
                                           last_normals, (hipStream_t)stream),
                    "mh_diffuse_walk");
}

extern "C" int mh_diffuse_arc(mh_ctx *ctx, const float *points, const float *end_points, const float *first_normals,
                              const float *last_normals, const int32_t *steps, const long long *row_offsets, int n, int rows,
                              int W, int H, int Z, double *sample, double *tangent, double *unit, int32_t *voxel,
                              unsigned long long *keys, void *stream) {
    if (rows == 0) return MH_OK;
    if (!ctx || !points || !end_points || !first_normals || !last_normals || !steps || !row_offsets || !sample ||
        !tangent || !unit || !voxel || !keys || n < 1 || rows < 0 || !cells_fit_int32(W, H, Z))
        return fail(MH_ERR_ARG, "mh_diffuse_arc: bad arguments");
    return launched(mh_launch_diffuse_arc(points, end_points, first_normals, last_normals, steps,
                                          (const int64_t *)row_offsets, n, rows, W, H, Z, sample, tangent, unit, voxel, keys,
                                          (hipStream_t)stream),
                    "mh_diffuse_arc");
}

extern "C" int mh_diffuse_splat(mh_ctx *ctx, const int32_t *seg_start, const unsigned long long *head_keys,
                                const int32_t *meta, const int32_t *order, const double *unit, int rows, int W, int H, int Z,
                                float *occ, float *ori, void *stream) {
    if (rows == 0) return MH_OK;
    if (!ctx || !seg_start || !head_keys || !meta || !order || !unit || !occ || !ori || rows < 0 ||
        !cells_fit_int32(W, H, Z))
        return fail(MH_ERR_ARG, "mh_diffuse_splat: bad arguments");
    return launched(mh_launch_diffuse_splat(seg_start, head_keys, meta, order, unit, rows, W, H, Z, occ, ori,
                                            (hipStream_t)stream),
                    "mh_diffuse_splat");
}

// ---- strand metrics (csrc/hairmetrics.hip; no counterpart in the reference) -----------------------------------------
extern "C" int mh_strand_arclen(mh_ctx *ctx, const float *points, const long long *offsets, int n_strands, double step,
                                double *cum_length, long long *n_samples, void *stream) {
    if (n_strands == 0) return MH_OK;
    if (!ctx || !points || !offsets || !cum_length || !n_samples || n_strands < 0 || !(step > 0.0))
        return fail(MH_ERR_ARG, "mh_strand_arclen: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_strand_arclen(points, (const int64_t *)offsets, n_strands, step, cum_length,
                                            (int64_t *)n_samples, (hipStream_t)stream),
                    "mh_strand_arclen");
}

extern "C" int mh_strand_resample(mh_ctx *ctx, const float *points, const long long *offsets, const double *cum_length,
                                  const long long *sample_offsets, int n_strands, int n_samples, double step,
                                  float *out_points, void *stream) {
    if (n_samples == 0) return MH_OK;
    if (!ctx || !points || !offsets || !cum_length || !sample_offsets || !out_points || n_strands < 1 || n_samples < 0 ||
        !(step > 0.0))
        return fail(MH_ERR_ARG, "mh_strand_resample: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_strand_resample(points, (const int64_t *)offsets, cum_length, (const int64_t *)sample_offsets,
                                              n_strands, n_samples, step, out_points, (hipStream_t)stream),
                    "mh_strand_resample");
}

extern "C" int mh_strand_tangents(mh_ctx *ctx, const float *points, const long long *offsets, int n_strands, int n_points,
                                  double *tangents, uint8_t *valid, void *stream) {
    if (n_points == 0) return MH_OK;
    if (!ctx || !points || !offsets || !tangents || !valid || n_strands < 1 || n_points < 0)
        return fail(MH_ERR_ARG, "mh_strand_tangents: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_strand_tangents(points, (const int64_t *)offsets, n_strands, n_points, tangents, valid,
                                              (hipStream_t)stream),
                    "mh_strand_tangents");
}

extern "C" int mh_strand_match(mh_ctx *ctx, const float *q_points, const double *q_tangents, const uint8_t *q_valid,
                               const int32_t *q_order, int nq, const float *t_points_sorted,
                               const double *t_tangents_sorted, int nt, const int32_t *cell_start, const float *g,
                               const int32_t *d, const double *r2, const double *cos_bound, int n_pairs, uint8_t *out_flags,
                               void *stream) {
    if (nq == 0) return MH_OK;
    if (!ctx || !q_points || !q_tangents || !q_valid || !q_order || !t_points_sorted || !t_tangents_sorted || !cell_start ||
        !g || !d || !r2 || !cos_bound || !out_flags || nq < 0 || nt < 1 || n_pairs < 1 || n_pairs > MH_MATCH_MAXK ||
        !(g[3] > 0.0f) || !cells_fit_int32(d[0], d[1], d[2]))
        return fail(MH_ERR_ARG, "mh_strand_match: bad arguments");
    MhMatchPairs pr = {};
    pr.K = n_pairs;
    for (int k = 0; k < n_pairs; ++k) pr.r2[k] = r2[k], pr.c[k] = cos_bound[k];
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_strand_match(q_points, q_tangents, q_valid, q_order, nq, t_points_sorted, t_tangents_sorted,
                                           cell_start, g[0], g[1], g[2], g[3], d[0], d[1], d[2], pr, out_flags,
                                           (hipStream_t)stream),
                    "mh_strand_match");
}

extern "C" int mh_flag_counts(mh_ctx *ctx, const uint8_t *flags, const uint8_t *valid, int n, unsigned long long *out9,
                              void *stream) {
    if (!ctx || !out9 || n < 0 || (n > 0 && (!flags || !valid))) return fail(MH_ERR_ARG, "mh_flag_counts: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_flag_counts(flags, valid, n, out9, (hipStream_t)stream), "mh_flag_counts");
}
