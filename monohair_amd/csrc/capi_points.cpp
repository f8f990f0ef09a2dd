// capi_points.cpp -- C ABI of the point-set utilities: grid, k-NN, sort, voxel groups, selection (csrc/knn.hip, sortgroup.hip)
#include "mh_capi.h"

extern "C" int mh_knn_grid(mh_ctx *ctx, const float *grid_origin_h /*host: ox,oy,oz,h*/, const int32_t *grid_dims /*host*/,
                           const float *pts_sorted, const int32_t *order, const int32_t *cell_start,
                           const void *queries, int query_f64, int Q, int k, int first_ring, const int32_t *query_order,
                           const unsigned char *valid, int32_t *out_idx, int32_t *status, void *stream) {
    if (Q == 0) return MH_OK;
    if (!ctx || !grid_origin_h || !grid_dims || !pts_sorted || !order || !cell_start || !queries || !out_idx ||
        !status || Q < 0)
        return fail(MH_ERR_ARG, "mh_knn_grid: bad arguments");
    return launched(mh_launch_knn(grid_origin_h[0], grid_origin_h[1], grid_origin_h[2], grid_origin_h[3], grid_dims[0],
                                  grid_dims[1], grid_dims[2], pts_sorted, order, cell_start, queries, query_f64 ? 1 : 0, Q,
                                  k, first_ring, query_order, valid, out_idx, status, (hipStream_t)stream),
                    "mh_knn_grid");
}

extern "C" int mh_nearest_distance(mh_ctx *ctx, const float *points, int N, const double *ref_points, int M,
                                   double *out_dist, double max_dist, double z_limit, unsigned char *out_mask,
                                   void *stream) {
    if (N == 0) return MH_OK;
    if (!ctx || !points || !ref_points || (!out_dist && !out_mask) || N < 0 || M < 1)
        return fail(MH_ERR_ARG, "mh_nearest_distance: bad arguments");
    return launched(mh_launch_nearest_dist(points, N, ref_points, M, out_dist, max_dist, z_limit, out_mask,
                                           (hipStream_t)stream),
                    "mh_nearest_distance");
}

extern "C" size_t mh_grid_scratch_bytes(int M) { return M < 0 ? 0 : mh_grid_scratch_bytes_impl(M); }
extern "C" size_t mh_sort_scratch_bytes(int n) { return n < 0 ? 0 : mh_sort_scratch_bytes_impl(n); }

extern "C" int mh_grid_build(mh_ctx *ctx, const float *g, const int32_t *d, const float *points, int M, void *scratch,
                             size_t scratch_bytes, float *pts_sorted, int32_t *order, int32_t *cell_start,
                             int32_t *n_occupied, void *stream) {
    if (M == 0) return MH_OK;
    if (!ctx || !g || !d || !points || !scratch || !order || M < 0 || !(g[3] > 0.0f) || !cells_fit_int32(d[0], d[1], d[2]))
        return fail(MH_ERR_ARG, "mh_grid_build: bad arguments");
    if (scratch_bytes < mh_grid_scratch_bytes_impl(M)) return fail(MH_ERR_ARG, "mh_grid_build: scratch too small");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_grid_build(points, M, g[0], g[1], g[2], g[3], d[0], d[1], d[2], scratch, scratch_bytes,
                                         pts_sorted, order, cell_start, n_occupied, (hipStream_t)stream),
                    "mh_grid_build");
}

extern "C" int mh_sort_keys(mh_ctx *ctx, const unsigned long long *keys, int n, int end_bit, void *scratch,
                            size_t scratch_bytes, unsigned long long *keys_out, int32_t *order, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !keys || !scratch || !keys_out || !order || n < 0 || end_bit < 1 || end_bit > 64)
        return fail(MH_ERR_ARG, "mh_sort_keys: bad arguments");
    if (scratch_bytes < mh_sort_scratch_bytes_impl(n)) return fail(MH_ERR_ARG, "mh_sort_keys: scratch too small");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_sort_keys(keys, n, end_bit, scratch, scratch_bytes, keys_out, order, (hipStream_t)stream),
                    "mh_sort_keys");
}

extern "C" size_t mh_voxel_group_scratch_bytes(int n) { return n < 0 ? 0 : mh_voxel_group_scratch_bytes_impl(n); }

extern "C" int mh_voxel_group(mh_ctx *ctx, const void *points, int points_f64, const float *ori, int n,
                              const double *voxel_min, double voxel_size, const int32_t *dims, void *scratch,
                              size_t scratch_bytes, unsigned long long *keys_sorted, int32_t *order, float *ori_sorted,
                              void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !points || !voxel_min || !dims || !scratch || !keys_sorted || !order || n < 0 || !(voxel_size > 0.0) ||
        dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || (ori == nullptr) != (ori_sorted == nullptr))
        return fail(MH_ERR_ARG, "mh_voxel_group: bad arguments");
    if (scratch_bytes < mh_voxel_group_scratch_bytes_impl(n)) return fail(MH_ERR_ARG, "mh_voxel_group: scratch too small");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_voxel_group(points, points_f64, ori, n, voxel_min, voxel_size, dims, scratch, scratch_bytes,
                                          keys_sorted, order, ori_sorted, (hipStream_t)stream),
                    "mh_voxel_group");
}

// ---- device-side selection between the stages of refine (csrc/sortgroup.hip): no host round trip ------------------
extern "C" size_t mh_select_scratch_bytes(int n) { return n < 0 ? 0 : mh_select_scratch_bytes_impl(n); }

extern "C" int mh_select_rows(mh_ctx *ctx, const uint8_t *flags, const uint8_t *veto, int invert, int n, const float *a,
                              const float *b, float *a_out, float *b_out, int32_t *index_out, const int32_t *base,
                              int32_t *count, void *scratch, size_t scratch_bytes, void *stream) {
    if (!ctx || !count || !scratch || n < 0 ||
        (n > 0 && (!flags || (a == nullptr) != (a_out == nullptr) || (b == nullptr) != (b_out == nullptr))))
        return fail(MH_ERR_ARG, "mh_select_rows: bad arguments");
    if (scratch_bytes < mh_select_scratch_bytes_impl(n)) return fail(MH_ERR_ARG, "mh_select_rows: scratch too small");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_select_rows(flags, veto, invert, n, a, b, a_out, b_out, index_out, base, count, scratch,
                                          (hipStream_t)stream),
                    "mh_select_rows");
}

extern "C" int mh_segment_heads(mh_ctx *ctx, const unsigned long long *keys_sorted, int n, int32_t *seg_start,
                                unsigned long long *head_keys, int32_t *meta, void *scratch, size_t scratch_bytes,
                                void *stream) {
    if (!ctx || !seg_start || !meta || !scratch || n < 0 || (n > 0 && !keys_sorted))
        return fail(MH_ERR_ARG, "mh_segment_heads: bad arguments");
    if (scratch_bytes < mh_select_scratch_bytes_impl(n)) return fail(MH_ERR_ARG, "mh_segment_heads: scratch too small");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_segment_heads(keys_sorted, n, seg_start, head_keys, meta, scratch, (hipStream_t)stream),
                    "mh_segment_heads");
}

extern "C" int mh_flag_less(mh_ctx *ctx, const float *x, float threshold, int n, uint8_t *out, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !x || !out || n < 0) return fail(MH_ERR_ARG, "mh_flag_less: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_flag_less(x, threshold, n, out, (hipStream_t)stream), "mh_flag_less");
}

extern "C" int mh_points_bbox(mh_ctx *ctx, const float *points, int M, float *out6, void *stream) {
    if (!ctx || !out6 || M < 0 || (M > 0 && !points)) return fail(MH_ERR_ARG, "mh_points_bbox: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_points_bbox(points, M, out6, (hipStream_t)stream), "mh_points_bbox");
}

extern "C" int mh_buffers_differ(mh_ctx *ctx, const void *a, const void *b, size_t bytes, int32_t *flag, void *stream) {
    if (!ctx || !flag || (bytes && (!a || !b)) || (bytes & 3)) return fail(MH_ERR_ARG, "mh_buffers_differ: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    return launched(mh_launch_words_differ(a, b, bytes / 4, flag, (hipStream_t)stream), "mh_buffers_differ");
}
