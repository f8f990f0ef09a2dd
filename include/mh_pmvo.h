/*
 * mh_pmvo.h -- C ABI of libmhpmvo.so: MonoHair's PMVO hot path as hand-written HIP kernels for
 * MI355X (gfx950).  This is the drop-in boundary: the reference has no FFI of its own (the path is
 * plain PyTorch, /root/reference/PMVO.py), so each entry point below names the reference function(s)
 * whose tensor-op sequence it replaces; the Python mirror of the reference classes
 * (monohair_amd/pmvo.py, gabor.py, pmvo_utils.py) binds them with ctypes -- see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer that is not marked "host" is a DEVICE pointer owned by the caller (e.g. a torch
 *     tensor's data_ptr()); nothing is retained after the call returns except inside mh_ctx;
 *   - all calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return value: 0 on success, negative mh_status on failure; mh_last_error() returns a
 *     thread-local description.  No exceptions cross the ABI.  No global state.
 *   - layouts are the reference's (row-major, fp32): vis[V,N], ori[V,N,2], conf[V,N], mask[V,N],
 *     ori_patch[V,N,P,2], conf_patch[V,N,P], with P = patch*patch taps in row-offset-major order.
 */
#ifndef MH_PMVO_H
#define MH_PMVO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mh_ctx mh_ctx;

enum mh_status {
    MH_OK = 0,
    MH_ERR_ARG = -1,     /* bad argument */
    MH_ERR_HIP = -2,     /* a HIP runtime call failed */
    MH_ERR_STATE = -3,   /* call order violated (e.g. views not set) */
    MH_ERR_NOMEM = -4
};

#define MH_CAM_STRIDE 48 /* floats per camera record: pose[16] | proj[16] | inv(pose[:3,:3])[9] | pad */
#define MH_TOPK 20       /* PMVO.py:341 */

const char *mh_last_error(void);
int mh_version(void);

/* ---- context: owns the packed per-view maps, the camera table and the depth-offset table -------- */
int mh_ctx_create(int device_id, mh_ctx **out);
void mh_ctx_destroy(mh_ctx *ctx);

/* Allocate packed storage for V views of H x W pixels (20 B / pixel: {ori_row, ori_col, conf, depth}
 * + mask).  Replaces the per-view H2D copies of PMVO.__init__ (PMVO.py:21-28). */
int mh_ctx_alloc_views(mh_ctx *ctx, int V, int H, int W);

/* Pack one view.  depth/mask are the reference's [H,W,C] arrays of which channel 0 is used
 * (PMVO.py:485,523): pass the channel count as the pixel stride.  cam_host: MH_CAM_STRIDE floats (host). */
int mh_ctx_set_view(mh_ctx *ctx, int view, const float *cam_host, const float *depth, int depth_stride,
                    const float *ori /*[H,W,2]*/, const float *conf /*[H,W]*/, const float *mask,
                    int mask_stride, void *stream);

/* Same, from the 8-bit image files the maps are stored in (Utils/PMVO_utils.py:255-313: best_ori/ gray u8,
 * conf/ gray u8, hair_mask/ channel 0 u8) without the float64 host decode: lut_host is 256 x {ori_row, ori_col,
 * conf, mask} floats -- the loader's value for each pixel code -- and the decode is a table lookup in the pack
 * kernel (bit-identical to uploading the decoded float maps).  ori_u8/conf_u8/mask_u8: device [H,W] planes. */
int mh_ctx_set_view_u8(mh_ctx *ctx, int view, const float *cam_host, const float *depth, int depth_stride,
                       const unsigned char *ori_u8, const unsigned char *conf_u8, const unsigned char *mask_u8,
                       const float *lut_host /*[256][4]*/, void *stream);

/* The S depth offsets of PMVO.sample_next_3d_pos (PMVO.py:274-278), host pointer, S <= 256 (MH_ERR_ARG beyond).  The search
 * entry points below add a limit of their own on S: nrank * S <= 1024 items per point. */
int mh_ctx_set_depth_offsets(mh_ctx *ctx, const float *offsets_host, int S);

/* Host -> device copy of a points chunk on `stream` (PMVO.py:40, `torch.from_numpy(points).type(torch.float).to(device)`):
 * a plain hipMemcpyAsync.  `host` should be page-locked for the copy to be asynchronous; the caller keeps it unchanged until the
 * copy has completed (an event of its own).  Exists because the tensor library's own non-blocking copy from a pinned source
 * also records an allocator-tracking event per call: 70 -> 55 us of host time per forward() on the 8-bit loop, where the host
 * has 0.24 ms per iteration to enqueue the next one. */
int mh_upload_async(mh_ctx *ctx, const void *host, void *device, size_t bytes, void *stream);
/* The same copy when `pinned_host` IS page-locked, device-visible memory (hipHostMalloc / a pin_memory tensor): up to 1 MiB
 * (4-byte aligned) it is issued as a KERNEL on `stream` that reads the host buffer over the link, larger copies as
 * hipMemcpyAsync.  Round 6: the 60 KB chunk of an iteration through hipMemcpyAsync stalls ONE call for 6-7 ms every so often
 * (the runtime reclaiming the copy commands that piled up while the host ran ahead: 7 ms of idle GPU when its queue is
 * shallow -- the "one timed round in ten is 20 % slower" of rounds 3-5); the kernel form has no such call, and the iteration
 * is 0.8 % (fp32 maps) / 4 % (8-bit maps) faster with it because the copy no longer waits for a copy engine.  MH_UPLOAD_KERNEL=0
 * in the environment selects hipMemcpyAsync for every size (A/B). */
int mh_upload_pinned(mh_ctx *ctx, const void *pinned_host, void *device, size_t bytes, void *stream);

/* ---- K3+K4+K5: PMVO.Compute_Visible_and_Ori (PMVO.py:346-376) with project_points (:378-397),
 * the gathers (:482-523) and compute_visible (:525-529).  Any output may be NULL.
 * pixf[V,N,2] = unrounded (row, col) of each point in each view (what Camera.uv2pixel returns,
 * Camera_utils.py:60-71); the search kernel reuses it. */
int mh_project_gather(mh_ctx *ctx, const float *points /*[N,3]*/, int N, int patch, float *vis, float *ori,
                      float *conf, float *mask, float *ori_patch, float *conf_patch, float *pixf, void *stream);

/* ---- K6: PMVO.Find_max_conf_from_visible_view (PMVO.py:339-343).  out_idx/out_val are [MH_TOPK,N].
 * Equal values come back in the order torch.topk gives them on the CPU (std::nth_element + std::sort of libstdc++ on
 * (value, view) pairs, restated step for step for one wave per point in csrc/mh_topk_wave.h) -- confidences from 8-bit
 * maps saturate, ties are the rule, and the base views decide which candidates are tried.
 * mh_ctx_set_option("topk_order", 1) selects the simpler rule of round 1 instead (value descending, then view index
 * ascending), 2 the literal one-lane-per-point form (csrc/mh_topk_order.h; slow, cross-check).  Needs V >= MH_TOPK
 * (the reference raises below 20 views). */
int mh_topk_views(mh_ctx *ctx, const float *vis, const float *conf, int N, int32_t *out_idx, float *out_val,
                  void *stream);

/* bytes of scratch mh_search_forward / mh_refine_loss need for N points and this patch size */
size_t mh_search_scratch_bytes(mh_ctx *ctx, int N, int patch);
/* byte offset, inside that scratch, of the [V,N] uint8 array of tap-list lengths the preparation kernels leave there
 * (0 for views that do not see the point): what the search orders its workgroups by, and what a caller can read to
 * count the (candidate, view, tap) evaluations a launch actually executes */
size_t mh_search_counts_offset(mh_ctx *ctx, int N, int patch);

/* ---- K7-K10 fused: the body of PMVO.forward (PMVO.py:50-78): for base-view ranks 0,rank_step,...
 * sample_next_3d_pos (:263-335), compute_reproject_ori (:219-241), compute_prj_loss (:151-209) and the
 * best-so-far update (:57-70); line_ori = normalize(best_sample - point).
 * Inputs are the tensors mh_project_gather produced for the same points.  Optional outputs may be NULL.
 *
 * THE N POINTS OF A CALL ARE ONE BATCH OF THE REFERENCE (PMVO.py:572-574 hands forward() 5000 points at a time), and a
 * point's answer depends on its batch as it does there: the points that share a (rank, base view) select how the sgemms
 * of sample_next_3d_pos round (Utils/Camera_utils.py:50-53,103; option "reproject_rule"), and the last N*S mod 32 samples of
 * the batch are the trailing columns of ATen's sums over the views (option "sum_block") -- see mh_ctx_set_option.  Base view
 * indices of ranks whose base_val is <= 0 may be anything (they are clamped; PMVO.py:64 never takes those ranks).
 * The scratch is opaque and must come from this library's own preparation calls: the search relies on the tap records being
 * unit vectors (|cos| <= 1 + 2^-14 in its integer-key body).
 *
 * The ranks and samples a call takes: nrank >= 1, rank_step >= 1, (nrank - 1) * rank_step < MH_TOPK, and -- one workgroup
 * holds the nrank * S (rank, sample) items of a point -- nrank <= 16 and nrank * S <= 1024 (the reference's 10 ranks leave
 * S <= 102; 16 ranks S <= 64; S = 256 four ranks).  mh_search_forward, mh_search_prepared and mh_forward refuse anything
 * else with MH_ERR_ARG and a text that names the limit, before they launch anything: no output is written.  (Order of the
 * checks: state -- views, depth offsets -- first; in mh_search_forward / mh_search_prepared then the pointers, then these
 * limits; mh_forward, once the depth offsets are set, reports these limits before its front end's pointer and patch checks.) */
int mh_search_forward(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold, int nrank,
                      int rank_step, const float *vis, const float *ori, const float *pixf,
                      const float *ori_patch, const float *conf_patch, const int32_t *base_idx,
                      const float *base_val, void *scratch, size_t scratch_bytes, float *line_ori,
                      float *min_loss, uint8_t *high_conf, float *best_sample, int32_t *best_rank,
                      int32_t *best_s, void *stream);

/* ---- The same path without materialising the patch tensors (what PMVO.forward uses): mh_forward_prepare is
 * the projection / visibility / centre-sample part of Compute_Visible_and_Ori (PMVO.py:346-376) fused with the
 * tap-list preparation, straight from the packed maps (patches of views that fail the depth test are not even
 * gathered); mh_topk_views then ranks the base views; mh_search_prepared runs the fused loss search on the
 * prepared scratch (its tail is work space: the search takes the points in descending order of work, which it
 * derives there).  Results are identical to mh_project_gather + mh_search_forward.  mask may be NULL. */
int mh_forward_prepare(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold, float *vis,
                       float *ori, float *conf, float *mask, void *scratch, size_t scratch_bytes, void *stream);
int mh_search_prepared(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold, int nrank,
                       int rank_step, const float *ori, const int32_t *base_idx, const float *base_val,
                       void *scratch, float *line_ori, float *min_loss, uint8_t *high_conf, float *best_sample,
                       int32_t *best_rank, int32_t *best_s, void *stream);
/* PMVO.forward (PMVO.py:39-78) in ONE call: mh_forward_prepare + mh_topk_views + mh_search_prepared on the same stream
 * (base_idx [20,N] int32 and base_val [20,N] receive the ranking).  What monohair_amd.pmvo.PMVO.forward calls: on 8-bit
 * maps an iteration is 0.24 ms of GPU work, so every host-side call per iteration counts.  With the default kernels the
 * ranking kernel also writes the work classes of the search's launch order and counts the batch's points per (rank, base
 * view) (fewer launches than the three calls; same results -- the order only decides WHEN a point is processed). */
int mh_forward(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold, int nrank, int rank_step,
               float *vis, float *ori, float *conf, float *mask, void *scratch, size_t scratch_bytes, int32_t *base_idx,
               float *base_val, float *line_ori, float *min_loss, uint8_t *high_conf, float *best_sample,
               int32_t *best_rank, int32_t *best_s, void *stream);

/* ---- compute_reproject_ori + compute_prj_loss with ONE given candidate per point: the core of
 * PMVO.refine (PMVO.py:86-90), next = point + ori*step_mul/step_div
 * (0.005 and 4 in the reference, applied in that order).  loss[N] (raw num/den, PMVO.py:199-204). */
int mh_refine_loss(mh_ctx *ctx, const float *points, const float *dir /*[N,3]*/, float step_mul, float step_div,
                   int N, int patch, float conf_threshold, const float *vis, const float *ori_patch,
                   const float *conf_patch, float *loss, uint8_t *high_conf, void *stream);

/* The same loss evaluated straight from the resident maps (no patch tensors): what refine's smoothing loop needs per
 * chunk (PMVO.py:619-623 calls PMVO.refine, i.e. Compute_Visible_and_Ori + this loss).  Bit-identical to
 * mh_project_gather + mh_refine_loss.
 *
 * batch / row0 / total: where these N points sit in the reference's batches.  The loss is a sum over views of a [V, n]
 * tensor per batch of n points (PMVO.py:198-204) and ATen adds the trailing n mod 32 columns of such a sum in another
 * order than the rest (csrc/mh_device.h: mh_row_sum_views), so the last bits of a point's loss depend on where it sits
 * in its batch.  The points are rows row0 .. row0+N-1 of `total` points that the reference processes `batch` at a time
 * (PMVO.py:602-606: 5000); batch = 0: these N points are one batch.  mh_ctx_set_option("sum_block", 0) turns the rule off. */
int mh_refine_loss_maps(mh_ctx *ctx, const float *points, const float *dir, float step_mul, float step_div, int N,
                        int patch, float conf_threshold, float *loss, uint8_t *high_conf, int batch, long long row0,
                        long long total, void *stream);

/* The tail of one chunk of refine's smoothing loop (PMVO.py:91-92, 631-642), in place on slices of the global arrays:
 * update = head_filter && !head_top ? -1 : loss_u;  ori <- center where |cos(center, ori)| < replace_threshold;
 * loss_out = update == -1 ? 0.5 : update.  ori may be NULL (loss only: the single-rank loop applies the replacement with
 * mh_replace_dissimilar inside its dependent chain and evaluates the losses of many chunks in one launch beside it). */
int mh_refine_combine(mh_ctx *ctx, const float *center, const float *loss_u, const unsigned char *head_filter,
                      const unsigned char *head_top, float replace_threshold, float *ori /*[N,3] in/out*/,
                      float *loss_out, int N, void *stream);

/* ---- the intermediate methods of the reference's class PMVO as stand-alone calls (the fused path above does not need
 * them; they keep the class's method surface): project_points (PMVO.py:378-397) for resident view `view`: row_col
 * int32 [N,2] rounded+clamped, z_half = -z/2, out_of_image flags, unrounded (row, col); any output may be NULL. */
int mh_project_points(mh_ctx *ctx, int view, const float *points, int N, int32_t *row_col, float *z_half,
                      unsigned char *out_of_image, float *pixel_unrounded, void *stream);
/* get_depth / get_ori / get_conf / get_mask / get_ori_patch / get_c_patch (PMVO.py:482-523): the resident records
 * {ori_row, ori_col, conf, depth} [N, size*size, 4] and mask [N, size*size] of view `view` at row_col (int64 [N,2]),
 * taps clamped to the image one by one, row offset outer. */
int mh_gather_pixels(mh_ctx *ctx, int view, const long long *row_col, int N, int size, float *records, float *mask,
                     void *stream);
/* compute_visible (PMVO.py:525-529), elementwise. */
int mh_compute_visible(mh_ctx *ctx, const float *depth, const float *z, size_t n, float *out, void *stream);
/* sample_next_3d_pos (PMVO.py:263-335): samples [N,S,3] for base_view [N]; ori = the [V,N,2] centre orientations of
 * Compute_Visible_and_Ori; offsets [S] on the device. */
int mh_sample_next(mh_ctx *ctx, const float *points, const int32_t *base_view, const float *ori, const float *offsets,
                   int N, int S, float *samples, void *stream);
/* compute_reproject_ori / compute_points_prj_ori (PMVO.py:219-260): D [V,N,S,2] = pixel(sample) - pixel(point). */
int mh_reproject_ori(mh_ctx *ctx, const float *points, const float *samples, int N, int S, float *D, void *stream);
/* compute_prj_loss (PMVO.py:151-209) on materialised tensors: loss [N], index int64 [N], high_conf [N];
 * all_loss [N,S] (the per-sample losses after the positive / low-confidence rules) may be NULL.  S <= 8187: a workgroup keeps
 * two floats of LDS per sample next to 36 bytes of its own, 64 KiB in all (MH_ERR_ARG beyond). */
int mh_prj_loss(mh_ctx *ctx, const float *D, const float *ori_patch, const float *conf_patch, const float *vis, int V,
                int N, int S, int P, float conf_threshold, float *loss, long long *index, unsigned char *high_conf,
                float *all_loss, void *stream);

/* ---- K13: per-view visibility / mask / confidence votes of PMVO.filter_points (PMVO.py:402-459),
 * PMVO.compute_unvisible_points (:461-480) and PMVO.filter_head_points (:110-137).
 * surface_index/filter_index/unvisible_index/head_filter: uint8 [N]; any may be NULL.
 * batch / row0 / total: as for mh_refine_loss_maps (the votes are sums over views of [V, n] tensors; mask values in
 * (0, 0.2] stay fractional, PMVO.py:427, so the order of the sum can matter). */
int mh_filter_points(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold,
                     float visible_threshold, uint8_t *surface_index, uint8_t *filter_index,
                     uint8_t *unvisible_index, uint8_t *head_filter, int batch, long long row0, long long total,
                     void *stream);

/* The same votes with the rows taken in the order `order` (int32 [N], a permutation of 0..N-1 on the device, or NULL): the
 * results are those of mh_filter_points, row for row -- a row's votes do not depend on when it is processed -- but a wave of
 * the large-launch kernel then holds 64 spatial neighbours instead of 64 consecutive candidates.  The candidates' own order
 * (a raster over the volume) sweeps every image once per slab: 10 GB of line fetches per pass for isolated 20-byte gathers;
 * in cell order (mh_grid_build's `order` on any grid of a few millimetres: the drivers use cells of 5 mm, or the grid the
 * neighbour search built anyway) the launch over 465 k candidates takes 0.97 instead of 2.15 ms. */
int mh_filter_points_ordered(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold,
                             float visible_threshold, uint8_t *surface_index, uint8_t *filter_index,
                             uint8_t *unvisible_index, uint8_t *head_filter, int batch, long long row0, long long total,
                             const int32_t *order, void *stream);

/* ---- K11: compute_points_similarity (Utils/PMVO_utils.py:366-382): medoid orientation of each group.
 * Dense form: ori[G,K,3] -> out[G,3], out_index[G].  Segmented form (voxel fit, PMVO.py:717-726):
 * ori[M,3] sorted by group, seg_start[G+1] (device), max_group = largest group size (groups beyond 4096 members take a staged path). */
/* Indexed form: group g = rows index[g*K .. g*K+K) of ori_rows[M,3] (the neighbour lists of refine, PMVO.py:612-618,
 * without materialising ori[index]). */
int mh_medoid_indexed(mh_ctx *ctx, const float *ori_rows, const int32_t *index, int G, int K, float *out,
                      int32_t *out_index, void *stream);
int mh_medoid_dense(mh_ctx *ctx, const float *ori, int G, int K, float *out, int32_t *out_index, void *stream);
int mh_medoid_segmented(mh_ctx *ctx, const float *ori, const int32_t *seg_start, int G, int max_group,
                        float *out, int32_t *out_index, void *stream);

/* refine's in-place replacement rule (PMVO.py:631-636): ori[n] <- center[n] where |cos(center[n], ori[n])| < threshold
 * (0.95 in the reference), cos evaluated as torch.cosine_similarity does on [N,3] fp32 tensors. */
int mh_replace_dissimilar(mh_ctx *ctx, const float *center, float *ori /*in/out [N,3]*/, float threshold, int N,
                          void *stream);

/* Exact k nearest neighbours on a uniform grid: the `points_tree.query(sub_points, 100)` of refine (PMVO.py:612,671).
 * pts_sorted[M,3]: the data points sorted by cell (x fastest), order[M]: their original indices, cell_start[ncell+1];
 * grid_origin_h (host): {ox, oy, oz, cell size}, grid_dims (host): {dx, dy, dz}.  out_idx[Q,k] sorted by (fp64 distance,
 * index); status[Q] != 0 marks queries the kernel could not finish (candidate buffer / ring limit): redo on the host. */
int mh_knn_grid(mh_ctx *ctx, const float *grid_origin_h, const int32_t *grid_dims, const float *pts_sorted,
                const int32_t *order, const int32_t *cell_start, const void *queries /*[Q,3] float32, or float64 if
                query_f64*/, int query_f64, int Q, int k, int first_ring /*cells around the query's cell looked at first
                (>= 1)*/, const int32_t *query_order /*optional [Q]: order in which the queries are taken (locality)*/,
                const unsigned char *valid /*optional [M], by original index: only these points count as neighbours*/,
                int32_t *out_idx, int32_t *status, void *stream);

/* Distance (float64) from each of N float32 points to the nearest of M float64 reference points, exhaustive: the
 * `scalp_tree.query(points, k=1)` of PMVO.filter_head_points (PMVO.py:100-101) -- d = sqrt(min_j ((dx*dx + dy*dy) + dz*dz))
 * evaluated in float64 as scipy's KDTree does.  out_mask (optional, uint8 [N]) = dist < max_dist && z < z_limit in
 * float64: the `head_top_index` of PMVO.py:102-106 (4 cm from the scalp, 1 cm below its top).  out_dist may be NULL. */
int mh_nearest_distance(mh_ctx *ctx, const float *points, int N, const double *ref_points, int M, double *out_dist,
                        double max_dist, double z_limit, unsigned char *out_mask, void *stream);

/* The grid mh_knn_grid searches: points sorted by cell (x fastest) with their original indices and the first sorted
 * position of every cell.  grid_origin_h (host): {ox, oy, oz, cell size}, grid_dims (host): {dx, dy, dz}.  Any of
 * pts_sorted / cell_start [dx*dy*dz + 1] / n_occupied (device int32: number of non-empty cells) may be NULL; order[M]
 * is always written.  (Replaces the torch sort / searchsorted / unique pipeline of the first implementation.) */
/* Bounding box of M float32 points: out6 (device) = {min x, min y, min z, max x, max y, max z} (M == 0: +inf / -inf).  What
 * the grid is laid over (scipy's KDTree needs no such thing: PMVO.py:605). */
int mh_points_bbox(mh_ctx *ctx, const float *points, int M, float *out6, void *stream);
size_t mh_grid_scratch_bytes(int M);
int mh_grid_build(mh_ctx *ctx, const float *grid_origin_h, const int32_t *grid_dims, const float *points, int M,
                  void *scratch, size_t scratch_bytes, float *pts_sorted, int32_t *order, int32_t *cell_start,
                  int32_t *n_occupied, void *stream);

/* Stable ascending sort of n 64-bit keys on their low end_bit bits -> keys_out[n], order[n] (original positions):
 * the grouping of points by voxel of the volume fit, PMVO.py:705-715 (a dict of lists in point order). */
size_t mh_sort_scratch_bytes(int n);
int mh_sort_keys(mh_ctx *ctx, const unsigned long long *keys, int n, int end_bit, void *scratch, size_t scratch_bytes,
                 unsigned long long *keys_out, int32_t *order, void *stream);

/* The grouping step of the volume fit in one call (PMVO.py:697-715 + Utils/PMVO_utils.py:386-404 p2v): voxel keys
 * (x*gy + y)*gz + z of the points evaluated in float64 exactly as numpy does (y, z negated, (p - min) / size, round half
 * to even, x86 int32 cast, clip), stable sort -> keys_sorted[n], order[n]; ori_sorted[n,3] (optional, with ori) = the
 * orientation rows in that order with the sign canonicalisation of :697-698 applied (y > 0 -> negated).  points are
 * float32 or float64 (points_f64); voxel_min (3 doubles) and dims (3 int32) are host arrays.  Nothing is modified in
 * place (the reference's p2v flips its input array). */
size_t mh_voxel_group_scratch_bytes(int n);
int mh_voxel_group(mh_ctx *ctx, const void *points, int points_f64, const float *ori, int n, const double *voxel_min,
                   double voxel_size, const int32_t *dims, void *scratch, size_t scratch_bytes,
                   unsigned long long *keys_sorted, int32_t *order, float *ori_sorted, void *stream);

/* ---- Selection on the device between the stages of refine: the `points[index]` / `ori[index]` of the loss threshold
 * (PMVO.py:651-653), the `centres[keep]` of the shell points (:680-686), their np.concatenate (:690-693) and the run
 * boundaries of the sorted voxel keys (:705-715) -- stable stream compaction, no host round trip.
 * mh_select_rows: element i is selected when (flags[i] && !(veto && veto[i])) != invert.  Selected rows of a / b ([n,3]
 * float32, optional) are written to a_out / b_out starting at row *base (device int32, optional: 0), in their original
 * order; index_out (optional) receives the selected i; *count (device int32) = *base + number selected -- hand it as
 * `base` to a second call to append.  scratch: mh_select_scratch_bytes(n).
 * mh_segment_heads: keys_sorted[n] ascending -> seg_start[G+1] (first position of every run of equal keys, seg_start[G]
 * = n; capacity n+1), head_keys[G] (optional, capacity n), meta (device int32[2]) = {G, largest run}.
 * mh_flag_less: out[i] = x[i] < threshold (float32 comparison; NaN -> 0). */
size_t mh_select_scratch_bytes(int n);
int mh_select_rows(mh_ctx *ctx, const unsigned char *flags, const unsigned char *veto, int invert, int n, const float *a,
                   const float *b, float *a_out, float *b_out, int32_t *index_out, const int32_t *base, int32_t *count,
                   void *scratch, size_t scratch_bytes, void *stream);
int mh_segment_heads(mh_ctx *ctx, const unsigned long long *keys_sorted, int n, int32_t *seg_start,
                     unsigned long long *head_keys, int32_t *meta, void *scratch, size_t scratch_bytes, void *stream);
int mh_flag_less(mh_ctx *ctx, const float *x, float threshold, int n, unsigned char *out, void *stream);
/* flag[0] (device int32) = 1 when two device buffers of `bytes` (a multiple of 4) differ in any bit, else 0: how refine
 * recognises the points a neighbour table was prepared for while optimize ran (monohair_amd/pmvo.py: RefinePrefetch). */
int mh_buffers_differ(mh_ctx *ctx, const void *a, const void *b, size_t bytes, int32_t *flag, void *stream);

/* ---- depth-map producer (the step before the path): Utils/Render_utils.py:310-347 render_bust_hair_depth with
 * the BustObj shader (:146-188) and Renderer.draw/ReadBuffer (:239-262) -- triangles drawn with a LESS depth test,
 * value (-z_camera / 2) * 255, background 255, top-left image origin.  verts[Nv,3] (world, bust offset applied),
 * faces[Nf,3] int32 (several meshes: concatenate them, earlier primitives win depth ties as in GL draw order).
 * pixel_center: 0.5 = OpenGL's sample position, 0.0 = the integer positions PMVO.project_points rounds to.
 * out[H,W,channels] float32 (channels = 3 gives the reference's .npy layout).  scratch: mh_render_scratch_bytes. */
size_t mh_render_scratch_bytes(int Nv, int Nf, int H, int W);
int mh_render_depth(mh_ctx *ctx, const float *cam_host, const float *verts, int Nv, const int32_t *faces, int Nf,
                    int H, int W, float pixel_center, void *scratch, size_t scratch_bytes, float *out, int channels,
                    void *stream);

/* ---- the caller on the other side of the path: Utils/Render_utils.py:269-307 render_data -- the
 * strand segments traced from the exterior volume drawn as GL_LINES of width 3 (StrandsObj, :8-127) over the bust mesh
 * (BustObj, :130-203) with a shared depth test, one of four fragment colourings; the images DeepMVSHair reads
 * (infer_inner.py:60-73).  line_pts / line_tan [2*Nseg,3]: the reference's `Lines` / `tangent` vertex buffers (two
 * vertices per segment).  color_option 0 depth/2, 1 direction, 2 undirected direction (2 theta), 3 white, < 0: strands
 * not drawn; depth_option (mesh fragments) 0 depth/2, 1 black, 2 white; clear: background value of all three channels.
 * out [H,W,3] float32 in the shader's range, top-left origin.  A specified rasteriser (header of csrc/raster.hip) that
 * follows the GL specification's rules; pinned against a real OpenGL implementation (Google SwiftShader,
 * tests/golden/gl_raster.npz) up to what GL leaves to the implementation (sub-pixel snapping, interpolation rounding). */
size_t mh_render_strands_scratch_bytes(int Nv, int Nf, int Nseg, int H, int W);
int mh_render_strands(mh_ctx *ctx, const float *cam_host, const float *verts, int Nv, const int32_t *faces, int Nf,
                      const float *line_pts, const float *line_tan, int Nseg, int H, int W, float pixel_center,
                      int line_width, int color_option, int depth_option, float clear, void *scratch,
                      size_t scratch_bytes, float *out, void *stream);

/* ---- K1+K2: calOrientationGabor.forward with iter=1 (preprocess_capture_data/GaborFilter.py:29-145):
 * 180 real Gabor kernels 17x17 (sigma 1.8/2.4, lambda 4), |response| argmax -> orientation index,
 * response-curve variance -> confidence normalised by the image maximum.
 * image[H,W] (DoG-filtered gray) -> orient_index[H,W] (int32, degrees), conf[H,W], variance[H,W] (un-normalised). */
int mh_gabor_bank(mh_ctx *ctx, const float *image, int H, int W, int32_t *orient_index, float *conf,
                  float *variance, void *stream);
/* Optional: install the 180 x 17 x 17 kernels (host pointer, kernel-major like gabor_fn's output) instead of
 * the bank the library builds on the device; lets the host reproduce the reference's CPU transcendental
 * functions bit for bit. */
int mh_gabor_set_bank(mh_ctx *ctx, const float *bank_host);
/* The difference-of-Gaussians prefilter of the stage (GaborFilter.py:190-192: skimage.filters.difference_of_gaussians(img,
 * 0.4, 10) = img_as_float, two scipy.ndimage.gaussian_filter passes with mode='nearest', their difference) in float64 with
 * scipy's operation order -- two launches.  image: uint8 [H,W] (in_kind 0; codes are multiplied by the double 1/255) or
 * float64 [H,W] (in_kind 1), device.  w_lo / w_hi: HOST pointers to the symmetric halves w[0..r] (w[r] = centre) of the two
 * normalised 1-D Gaussians as scipy builds them (radius = int(4 sigma + 0.5) <= 48).  scratch: mh_dog_scratch_bytes(H, W)
 * device bytes.  out64 and/or out32 (device, [H,W]; either may be NULL): lo - hi and its float32 cast. */
size_t mh_dog_scratch_bytes(int H, int W);
int mh_dog(mh_ctx *ctx, const void *image, int in_kind, int H, int W, const double *w_lo, int r_lo, const double *w_hi,
           int r_hi, void *scratch, double *out64, float *out32, void *stream);
/* One view of the Gabor stage, device to device (calculate_orientation, GaborFilter.py:164-224, without the file IO):
 * gray uint8 [H,W] -> DoG -> bank -> orient_index / conf / variance as mh_gabor_bank, plus (k8, c8 non-NULL) the two 8-bit
 * codes the reference writes to best_ori/<view> and conf/<view> (orientation in degrees; floor(conf*255+0.5)) -- what the
 * PMVO loaders read back (mh_ctx_set_view_u8).  conf may be NULL.  scratch: mh_gabor_view_scratch_bytes(H, W). */
size_t mh_gabor_view_scratch_bytes(int H, int W);
int mh_gabor_view(mh_ctx *ctx, const uint8_t *gray, int H, int W, const double *w_lo, int r_lo, const double *w_hi, int r_hi,
                  void *scratch, int32_t *orient_index, float *conf, float *variance, uint8_t *k8, uint8_t *c8, void *stream);

/* ---- strand tracing on the fitted volume (HairGrow.py).
 * mh_volume_pack: occ[Z,H,W] + ori[Z,H,W,3] (the .mat readers' layout, Utils/PMVO_utils.py:86-113) -> 16-byte voxels
 *   {ori_x, -ori_y, -ori_z, occ} (HairGrowing.__init__, HairGrow.py:41-55); vox: W*H*Z*16 bytes.
 * mh_trace_seeds: HairGrowing.trace (:59-149) for n already-jittered seeds, WITHOUT the flag gate: strand i occupies
 *   out[i][first[i] .. first[i]+len[i]) of a 513-point row.
 * mh_trace_scalp: HairGrowing.traceFromScalp (:154-223): rows of 257 points, len 0 where the reference returns None.  Such
 *   a rejected walk -- one still inside the head after 25 steps -- leaves the points it took in its own row, the seed and
 *   exactly 25 steps in slots 0 .. 25 (no caller reads a row past its len, and every caller allocates whole rows); nothing
 *   else of the row, and no other row, is written.
 * mh_strands_accept: the sequential flag gate of GenerateGuideStrandFromScalp (:226-265) / randomlyGenerateSegments
 *   (:269-299) replayed over the finished traces -- HOST pointers, runs on the calling thread. */
int mh_volume_pack(mh_ctx *ctx, const float *occ, const float *ori, int W, int H, int Z, void *vox, void *stream);
int mh_trace_seeds(mh_ctx *ctx, const void *vox, int W, int H, int Z, const float *seeds, int n, float thr_dot,
                   float *out, int32_t *first, int32_t *len, void *stream);
int mh_trace_scalp(mh_ctx *ctx, const void *vox, int W, int H, int Z, const float *seeds, const float *normals, int n,
                   float thr_dot, float *out, int32_t *len, void *stream);
int mh_strands_accept(int W, int H, int Z, float *flag, const float *pts, const int32_t *first, const int32_t *len,
                      int stride, const float *seeds, int n, int mode, uint8_t *accepted);
/* Packs the fixed-stride rows of mh_trace_seeds / mh_trace_scalp (device) into one point list, strand after strand:
 * packed[offsets[i] .. offsets[i]+len[i]) = rows[i][first[i] .. ) (first may be NULL = 0); offsets = exclusive prefix sum
 * of len (device, int64).  mh_strands_accept reads the packed list with stride 0 and first = offsets. */
int mh_strands_compact(mh_ctx *ctx, const float *rows, const int32_t *first, const int32_t *len, const long long *offsets,
                       int n, int stride, float *packed, void *stream);
/* Segment connection (HairGrowing.find_connect_info, HairGrow.py:434-590 with connect_segments :303-420) and the Laplacian
 * smoothing of Utils/Utils.py:1148-1198, all float64.  Strands are one point list pts [P,3] with offsets [n+1] (int64),
 * every pointer on the device.
 * mh_end_knn64: KDTree(data).query(q, k=50, distance_upper_bound=bound) per query, pruned to d^2 < bound^2 and sorted by
 *   (distance, index); with skip_self the query's own index is dropped afterwards.  data is binned on a uniform grid of
 *   gx*gy*gz cells no smaller than `bound` (order = data indices sorted by cell, cstart [cells+1]); qcell [nq,3] = each
 *   query's cell by the same formula.  Rows of 50: out_idx / out_dist (the distance itself) [nq,50], out_cnt [nq].
 * mh_connect_candidates: find_best_connect_strands for both ends of every segment.  nei_* (host arrays of 4 device
 *   pointers): the lists root->roots, root->tips, tip->roots, tip->tips of mh_end_knn64.  best[2i+e] = the segment joined
 *   at end e (0 root, 1 tip) of segment i or -1; best_type = 0 if it is joined at its root, 1 at its tip.
 * mh_chain_count / mh_chain_emit: connect_segments (add_mid, weight 0) for every segment: total points and points of the
 *   root-side pieces, then (out_offsets = exclusive scan of total) the connected strands.
 * mh_occ_check: attempt 0 of the occupancy loop (:514-544): status 1 accepted, 0 rejected (the caller draws and retries),
 *   2 outside the reference's fixed 256x256x192 box, 3 an index the reference's torch indexing refuses.  occ [Z,H,W]
 *   float32 with element stride occ_stride; vmin = float64 of the float32 voxel_min.
 * mh_smooth_strands: smnooth_strand (fix_tips False), one lane per strand: pts holds b = strand * pos_constraint on entry
 *   (formed in the strand's own dtype, as the reference's numpy does) and the solution on return; work: 3*P doubles. */
int mh_end_knn64(mh_ctx *ctx, const double *q, const int32_t *qcell, int nq, const double *data, const int32_t *order,
                 const int32_t *cstart, int gx, int gy, int gz, double bound, int skip_self, int32_t *out_idx,
                 double *out_dist, int32_t *out_cnt, void *stream);
int mh_connect_candidates(mh_ctx *ctx, const double *pts, const long long *offsets, int n, const int32_t *const *nei_idx,
                          const double *const *nei_dist, const int32_t *const *nei_cnt, double dot_threshold,
                          int32_t *best, int32_t *best_type, void *stream);
int mh_chain_count(mh_ctx *ctx, const long long *offsets, int n, const int32_t *best, const int32_t *best_type,
                   long long *total, long long *root_len, void *stream);
int mh_chain_emit(mh_ctx *ctx, const double *pts, const long long *offsets, int n, const int32_t *best,
                  const int32_t *best_type, const long long *root_len, const long long *out_offsets, double *out,
                  void *stream);
int mh_occ_check(mh_ctx *ctx, const double *pts, const long long *offsets, int n, const float *occ, long long occ_stride,
                 int W, int H, int Z, double vmin_x, double vmin_y, double vmin_z, double voxel_size, int32_t *status,
                 void *stream);
int mh_smooth_strands(mh_ctx *ctx, double *pts, const long long *offsets, int n, double lap_constraint,
                      double pos_constraint, double *work, void *stream);
/* Scalp attachment (HairGrowing.connect_to_scalp, HairGrow.py:606-784 with compute_strands_similar :788-812, connect_strands
 * :384-416 and random_move_strands, Utils/PMVO_utils.py:618-658): ONE pass of its while loop; thresholds and termination
 * stay with the caller.  Strands are one float32 point list pts [P,3] in voxel units with offsets [n+1] (int64); flags [n]:
 * bit 0 rooted, bit 1 out.  The core points core [n_core,3] are the points of the strands rooted when the pass starts, in
 * strand order, with core_strand [n_core] (the strand of each) and core_rank [n_core]: rank[KDTree(core).indices[j]] = j,
 * the order in which query_ball_point returns its members.  order / cell_start: mh_grid_build's binning of core on the
 * grid (host arrays grid = {origin xyz, cell size > thr_dist}, dims).  active [n_active]: the strands neither rooted nor
 * out.  Every other pointer is on the device.
 * mh_scalp_ball_count: count[a] = members of query_ball_point(strand[0], thr_dist) (float64, bound included).
 * mh_scalp_choose: ball_offsets = exclusive scan of count [n_active+1], ball_scratch one 64-bit word per member.  Per
 *   active strand i: flip[i] = 1 if the flip test reverses it, best_strand[i] / best_index[i] = the neighbour and the point
 *   index it joins (-1: none).  The caller presets the three arrays for the strands that are not active (0, -1, 0).
 * mh_scalp_emit: new_offsets = exclusive scan of the new lengths (len + best_index + 1 where joined).  Writes every strand
 *   to new_pts (reversed where flip is set, the join in front); a joined strand goes through random_move_strands' test on
 *   vox [Z,H,W,4] = {orientation with y/z negated, occupancy} (mh_volume_pack): flags, out_ratio [n] (float64) and similar
 *   [n] are updated for it, counters[0..2] += newly rooted, newly out, strands torch's indexing would refuse. */
int mh_scalp_ball_count(mh_ctx *ctx, const float *pts, const long long *offsets, const int32_t *active, int n_active,
                        const float *core, int n_core, const int32_t *order, const int32_t *cell_start, const float *grid,
                        const int32_t *dims, double thr_dist, long long *count, void *stream);
int mh_scalp_choose(mh_ctx *ctx, const float *pts, const long long *offsets, const int32_t *active, int n_active,
                    const float *core, const int32_t *core_strand, const int32_t *core_rank, int n_core,
                    const int32_t *order, const int32_t *cell_start, const float *grid, const int32_t *dims,
                    double thr_dist, double thr_dot, const double *out_ratio, const long long *ball_offsets,
                    unsigned long long *ball_scratch, uint8_t *flip, int32_t *best_strand, int32_t *best_index,
                    void *stream);
int mh_scalp_emit(mh_ctx *ctx, const float *pts, const long long *offsets, int n, const uint8_t *flip,
                  const int32_t *best_strand, const int32_t *best_index, const long long *new_offsets, const float *vox,
                  int W, int H, int Z, double out_ratio_threshold, float *new_pts, uint8_t *flags, double *out_ratio,
                  float *similar, int32_t *counters, void *stream);

/* Scalp sampling (HairGrow.py:880-897: Open3D's sample_points_uniformly with interpolated vertex normals, then the step
 * to voxel space), float64.  vertices / normals [nv,3] float64, faces [nf,3] int32 with every index in [0, nv): the caller
 * checks them, the kernels do not.
 * mh_tri_area64: area[t] = 0.5 * |(b-a) x (c-a)|.
 * mh_mesh_sample: bounds [nf] (int64, non-decreasing, bounds[nf-1] = n): sample i lies in the first triangle t with
 *   bounds[t] > i -- Open3D's allocation, bounds[t] = round(n * cdf[t]).  uniforms [n,2] in [0,1).  With r1 = sqrt(u0),
 *   r2 = u1 the weights (1-r1, r1(1-r2), r1 r2) on (a, b, c) give the point and the normal.  out_points = ((p +
 *   bust_to_origin) * (1,-1,-1) - vmin) / 0.0025 with vmin the float32 (-0.32, -0.32, -0.24) widened; out_normals = the
 *   normal over its 2-norm, y/z negated; both cast to float32 [n,3].  bust_to_origin: HOST [3].  out_triangle (optional,
 *   int32 [n]): t. */
int mh_tri_area64(mh_ctx *ctx, const double *vertices, int nv, const int32_t *faces, int nf, double *area, void *stream);
int mh_mesh_sample(mh_ctx *ctx, const double *vertices, const double *normals, int nv, const int32_t *faces, int nf,
                   const long long *bounds, const double *uniforms, int n, const double *bust_to_origin, float *out_points,
                   float *out_normals, int32_t *out_triangle, void *stream);

/* Scalp diffusion (the reference's diffusion_scalp, Utils/PMVO_utils.py:467-593): the volumes HairGrow.py reads when
 * `scalp_diffusion` is set.  occ [Z,H,W] and ori [3][Z,H,W] (planar) are the float32 volumes as the .mat files hold them
 * (no y/z flip); points / normals [n,3] are float32 world-space scalp samples.  voxel_min and the voxel size are the
 * reference's constants (-0.32, -0.32, -0.24 as float32; 0.005 / 2).
 * mh_diffuse_walk: per sample the walk along its normal (:494-536) -> status (0 accepted, 1 the sample lies in hair, 2 ten
 *   steps without an end, 3 nine restarts without an end, 4 the walk left the volume -- the reference's indexing raises or
 *   wraps there), steps, end_points [n,3] (point_set[-1]), first_normals / last_normals [n,3] (normal_set[0] / [-1]).
 * mh_diffuse_arc: row_offsets [n+1] (int64) = exclusive scan of steps + 1 over the accepted samples, rows = its last entry.
 *   Per row the float64 Hermite sample (:545-547, scipy's power-form evaluation), its forward-difference tangent (:548), the
 *   unit tangent (:560), the voxel (x, y, z) of the sample (:561; -1 where it leaves the volume) and the sort key (the
 *   linear voxel z*H*W + y*W + x, or W*H*Z for a row outside).
 * mh_diffuse_splat: the rows grouped by voxel with a STABLE sort (mh_sort_keys on the keys -> order; mh_segment_heads on the
 *   sorted keys -> seg_start, head_keys, meta).  Per touched voxel the unit tangents are added in row order into a float32
 *   accumulator through a float64 sum (:563-567) and combined in place: ori += (1 - occ) * acc / max(count, 1e-6), occ +=
 *   (1 - occ) (:568-592).  Untouched voxels are not written. */
int mh_diffuse_walk(mh_ctx *ctx, const float *occ, const float *ori, int W, int H, int Z, const float *points,
                    const float *normals, int n, int32_t *status, int32_t *steps, float *end_points, float *first_normals,
                    float *last_normals, void *stream);
int mh_diffuse_arc(mh_ctx *ctx, const float *points, const float *end_points, const float *first_normals,
                   const float *last_normals, const int32_t *steps, const long long *row_offsets, int n, int rows, int W,
                   int H, int Z, double *sample, double *tangent, double *unit, int32_t *voxel, unsigned long long *keys,
                   void *stream);
int mh_diffuse_splat(mh_ctx *ctx, const int32_t *seg_start, const unsigned long long *head_keys, const int32_t *meta,
                     const int32_t *order, const double *unit, int rows, int W, int H, int Z, float *occ, float *ori,
                     void *stream);

/* Strand metrics (monohair_amd.hairmetrics; no counterpart in the reference): point-wise precision / recall of one strand
 * set against another under joint distance-and-direction bounds.  points [n,3] float32, offsets [n_strands+1] (int64, the
 * exclusive scan of the per-strand point counts).  float64 arithmetic on the float32 coordinates, + - * / sqrt in the order
 * written here, nothing fused.
 * mh_strand_arclen: cum_length[i] (float64 [n]) = length of the strand up to point i, L_i = L_{i-1} + sqrt((dx*dx + dy*dy) +
 *   dz*dz); n_samples[s] (int64) = floor(L_last / step) + 1, 1 for a strand of one point or of length 0, 0 for an empty one.
 * mh_strand_resample: sample_offsets [n_strands+1] = exclusive scan of n_samples, n_samples = its last entry.  Sample j of a
 *   strand sits at arc = j * step on the first segment i with L_{i+1} > arc (when none is, on the last segment of non-zero
 *   length): u = (arc - L_i) / (L_{i+1} - L_i), q = p_i + u * (p_{i+1} - p_i), rounded to float32.
 * mh_strand_tangents: d = p[min(i+1, last)] - p[max(i-1, first)], tangents[i] (float64 [n,3]) = d / |d|, valid[i] = 1; 0 and
 *   valid[i] = 0 where the strand has one point or |d| = 0.
 * mh_strand_match: out_flags[q] bit k is set iff q_valid[q] and some target has (dx*dx + dy*dy) + dz*dz <= r2[k] and
 *   |(tx*ux + ty*uy) + tz*uz| >= cos_bound[k] (r2, cos_bound: HOST float64 [n_pairs], n_pairs <= 8).  The targets are the VALID
 *   targets only, binned by mh_grid_build on a grid (grid_origin_h, grid_dims: HOST) whose cell exceeds the largest radius
 *   by a slack that covers float32 rounding: t_points_sorted is its pts_sorted, t_tangents_sorted the tangents gathered by its
 *   order, cell_start its cell_start.  q_order [nq]: a permutation of the queries, mh_grid_build's order of the queries on the
 *   same grid (it only decides which queries share a wave).  nt >= 1: with no targets every flag is 0 and nothing is to launch.
 * mh_flag_counts: out9 (uint64 [9]) = per bit k < 8 the number of flag bytes that have it, then the number of non-zero bytes
 *   of valid. */
int mh_strand_arclen(mh_ctx *ctx, const float *points, const long long *offsets, int n_strands, double step,
                     double *cum_length, long long *n_samples, void *stream);
int mh_strand_resample(mh_ctx *ctx, const float *points, const long long *offsets, const double *cum_length,
                       const long long *sample_offsets, int n_strands, int n_samples, double step, float *out_points,
                       void *stream);
int mh_strand_tangents(mh_ctx *ctx, const float *points, const long long *offsets, int n_strands, int n_points,
                       double *tangents, uint8_t *valid, void *stream);
int mh_strand_match(mh_ctx *ctx, const float *q_points, const double *q_tangents, const uint8_t *q_valid,
                    const int32_t *q_order, int nq, const float *t_points_sorted, const double *t_tangents_sorted, int nt,
                    const int32_t *cell_start, const float *grid_origin_h, const int32_t *grid_dims, const double *r2,
                    const double *cos_bound, int n_pairs, uint8_t *out_flags, void *stream);
int mh_flag_counts(mh_ctx *ctx, const uint8_t *flags, const uint8_t *valid, int n, unsigned long long *out9, void *stream);

/* Hair capture (monohair_amd.synth_hair; no counterpart in the reference): a strand set rendered into the four per-view maps
 * PMVO reads -- depth, orientation code, confidence code, hair mask -- so that a capture exists for which the ground-truth
 * strands are known.  points [n_points,3] float32 world points, offsets [n_strands+1] (int64, the exclusive scan of the
 * per-strand point counts).  The rule, per view:
 *
 * Vertex.  (u, v, z) = Camera.projection and (row, col) = the unrounded pixel, by the float32 arithmetic PMVO itself projects
 *   with (mh_project_points: csrc/mh_device.h mh_cam_project, mh_ndc_to_pixel); z255 = (-z / 2) * 255 in float32.  A vertex is
 *   valid iff z < -0.1 (the camera's near plane) and |row| < 2^20 and |col| < 2^20 (NaN fails).  Everything below is float64
 *   arithmetic on these float32 values, + - * / sqrt in the order written, nothing fused.
 * Segment (a, b) = consecutive points of one strand, both valid; any other pair makes nothing.  dr = row_b - row_a, dc = col_b -
 *   col_a, dz = z255_b - z255_a; n = max(1, ceil(max(|dr|, |dc|))); a segment with n > 8192 is dropped and counted.  len =
 *   sqrt(dr*dr + dc*dc).  If len > 0: ur = dr/len, uc = dc/len, c2 = uc*uc - ur*ur, s2 = -2*(uc*ur) -- the double angle of the
 *   line whose (row, col) direction is (-sin phi, cos phi) -- and qc = rint(4096*c2), qs = rint(4096*s2), half to even, as
 *   integers; otherwise qc = qs = 0.
 * Sample j = 0 .. n-1: t = (j + 0.5)/n; centre pixel = (rint(row_a + t*dr), rint(col_a + t*dc)), half to even; zf =
 *   float32(z255_a + t*dz).  A sample whose zf is not finite makes nothing (only |z| beyond 2^121 does that).  Otherwise it
 *   makes one fragment of depth zf on every pixel of the (2*radius+1)^2 square around the centre that lies inside the image
 *   (pixels outside are dropped, not clamped).  With an occluder plane depth0 (float32 [H,W], PMVO's depth convention,
 *   background 255) a fragment with zf > depth0[p] is discarded; equal depth stays.
 * Pass A: zmin[p] = the smallest zf of the fragments of pixel p, float32 (+inf where there is none).
 * Pass B: a fragment counts iff zf <= zmin[p] + tol (a float32 addition); per pixel cnt += 1 (int32), C2 += qc, S2 += qs
 *   (int64).  Integer sums: the result does not depend on the order of arrival.
 * Resolve, per pixel: mask code 255 if cnt > 0 else 0.  Orientation code: the first k in 0..179 that maximises
 *   C2*T[k][0] + S2*T[k][1] in float64 (the two products rounded, then their sum), T[k] = the float32 pair (cos 2 theta_k,
 *   sin 2 theta_k), theta_k = k degrees, widened; 0 where cnt = 0 or C2 = S2 = 0.  Confidence code: min(255, floor((255*coh)*dens
 *   + 0.5)) with coh = sqrt(C2*C2 + S2*S2) / (4096*cnt) and dens = min(1, cnt / n_full); 0 where cnt = 0.  Depth: zmin[p] where
 *   cnt > 0, else depth0[p], else 255.
 * Orientation code k names the line whose (row, col) direction is (-sin theta_k, cos theta_k): the loaders' decode of it
 * (Utils/PMVO_utils.py:265-272) is parallel to the segment.  Defaults of the callers: radius 1, tol 0.25 (about 2 mm of hair
 * layer in depth-map units), n_full = 2*radius + 1 (one strand's worth of samples).
 *
 * mh_capture_project: vert [n_points,3] = (row, col, z255), valid [n_points].  cam_host: MH_CAM_STRIDE floats (host).
 * mh_capture_zmin: pass A -> zmin [H,W], dropped (device int32: the segments with n > 8192).  depth0 may be NULL.
 * mh_capture_accumulate: pass B on the zmin of pass A -> cnt [H,W] int32, c2 / s2 [H,W] int64 (all three are zeroed first).
 * mh_capture_resolve: table_host = T, 180 x 2 float32 (HOST) -> depth [H,W] float32, ori_u8 / conf_u8 / mask_u8 [H,W].
 * mh_capture_view: the four steps for one view on a scratch of mh_capture_scratch_bytes(n_points, H, W) bytes: what
 *   PMVO.from_u8 takes for that view.  0 <= radius <= 16, tol >= 0, n_full >= 1, H*W < 2^31. */
size_t mh_capture_scratch_bytes(int n_points, int H, int W);
int mh_capture_project(mh_ctx *ctx, const float *cam_host, const float *points, int n_points, int H, int W, float *vert,
                       uint8_t *valid, void *stream);
int mh_capture_zmin(mh_ctx *ctx, const float *vert, const uint8_t *valid, const long long *offsets, int n_strands,
                    int n_points, int H, int W, int radius, const float *depth0, float *zmin, int32_t *dropped, void *stream);
int mh_capture_accumulate(mh_ctx *ctx, const float *vert, const uint8_t *valid, const long long *offsets, int n_strands,
                          int n_points, int H, int W, int radius, float tol, const float *depth0, const float *zmin,
                          int32_t *cnt, long long *c2, long long *s2, void *stream);
int mh_capture_resolve(mh_ctx *ctx, const float *zmin, const int32_t *cnt, const long long *c2, const long long *s2,
                       const float *depth0, const float *table_host, int n_full, int H, int W, float *depth, uint8_t *ori_u8,
                       uint8_t *conf_u8, uint8_t *mask_u8, void *stream);
int mh_capture_view(mh_ctx *ctx, const float *cam_host, const float *points, const long long *offsets, int n_strands,
                    int n_points, int H, int W, int radius, float tol, int n_full, const float *depth0,
                    const float *table_host, void *scratch, size_t scratch_bytes, float *depth, uint8_t *ori_u8,
                    uint8_t *conf_u8, uint8_t *mask_u8, void *stream);

/* Hair photograph (monohair_amd.synth_hair.photo_planes; no counterpart in the reference): the same strand set rendered as
 * the 8-bit gray images a capture consists of -- thin, shaded, mutually occluding strands, anti-aliased by supersampling -- so
 * that capture_images/ holds pictures and the Gabor stage (mh_gabor_view) makes best_ori/ and conf/ from them.  Per view there
 * is a supersampling factor S in {1, 2, 4, 8} and a sub-pixel half-width w, 0 <= w <= 16; S*H * S*W < 2^31.  The rule:
 *
 * Vertex.  mh_capture_project unchanged: (row, col, z255, valid).  Everything below is float64 arithmetic on float32 values,
 *   + - * / sqrt in the order written, nothing fused; every per-pixel quantity is an integer.
 * Sub-pixel grid.  S*H x S*W sub-pixels; row' = S*row + (S-1)/2, col' = S*col + (S-1)/2.  Sub-pixel (r', c') belongs to pixel
 *   (r' div S, c' div S): pixel p owns the sub-pixel centres in [p - 1/2, p + 1/2), the positions PMVO rounds to p (but for
 *   the ties: at S > 1 a sample centred exactly on k + 1/2 goes to pixel k + 1, PMVO's half-to-even rounding gives it to the
 *   even one of k and k + 1; at S = 1 the two agree everywhere).
 * Segment (a, b) = consecutive points of one strand, both valid; any other pair makes nothing.  It is walked as the capture
 *   rule walks it, in sub-pixel units: dr = row'_b - row'_a, dc = col'_b - col'_a, dz = z255_b - z255_a; n = max(1,
 *   ceil(max(|dr|, |dc|))); a segment with n > 8192 is dropped and counted.  Sample j = 0 .. n-1: t = (j + 0.5)/n; centre
 *   sub-pixel = (rint(row'_a + t*dr), rint(col'_a + t*dc)), half to even; zf = float32(z255_a + t*dz); a sample whose zf is
 *   not finite makes nothing.  Otherwise it makes one fragment (zf, q) on every sub-pixel of the (2w+1)^2 square around the
 *   centre that lies inside the grid.  With an occluder plane depth0 (float32 [H,W], at image resolution) a fragment with
 *   zf > depth0[owning pixel] is discarded; equal depth stays.
 * Shade of a segment, one integer q in 0..255 (the Kajiya-Kay diffuse term): T = P_b - P_a from the float32 world points
 *   widened to float64; tt = (Tx*Tx + Ty*Ty) + Tz*Tz, tl = (Tx*Lx + Ty*Ly) + Tz*Lz; sin = sqrt(max(0, 1 - (tl*tl)/tt)) if
 *   tt > 0, else 0; v = (255*albedo[s]) * (ambient + (1 - ambient)*sin); q = min(255, rint(v)), half to even, if v > 0, else 0
 *   (NaN included).  L is a unit 3-vector per view (float64, host; the callers' default is the view's direction towards the
 *   camera, a head light), albedo a float32 table with one entry per strand (the host decides its bits, as with T above),
 *   0 <= ambient <= 1.  shade[i] is the q of segment (i, i+1), 0 where the pair makes no segment.
 * Front pass.  Each sub-pixel holds one unsigned 64-bit key, (bits(zf) << 32) | q; zf > 0 for valid vertices, so the bits
 *   order as the values do.  The plane starts as all ones and takes the minimum over the fragments: the nearest strand wins,
 *   and at exactly equal depth the darker shade wins.  An integer minimum: the result does not depend on the order of arrival.
 * Resolve, per pixel: sum over its S^2 sub-pixels of the key's q where a fragment arrived, else bust_code where depth0 is given
 *   and depth0[p] < 255, else background_code (both 0..255).  gray = (2*sum + S^2) div (2*S^2) as uint8 (the mean, half up);
 *   cover = the number of sub-pixels where a fragment arrived, int32.
 *
 * mh_photo_shade: valid = mh_capture_project's -> shade [n_points] uint8.  light_host: 3 doubles (HOST).
 * mh_photo_front: keys [S*H, S*W] (filled first), dropped (device int32: the segments with n > 8192).  depth0 may be NULL.
 * mh_photo_resolve: gray_u8 [H,W], cover [H,W] int32 (may be NULL).
 * mh_photo_view: mh_capture_project and the three steps for one view on a scratch of mh_photo_scratch_bytes(n_points, H, W,
 *   supersample) bytes, whose first int32 is left holding the dropped count. */
size_t mh_photo_scratch_bytes(int n_points, int H, int W, int supersample);
int mh_photo_shade(mh_ctx *ctx, const float *points, const uint8_t *valid, const long long *offsets, int n_strands,
                   int n_points, const float *albedo, const double *light_host, double ambient, uint8_t *shade, void *stream);
int mh_photo_front(mh_ctx *ctx, const float *vert, const uint8_t *valid, const long long *offsets, int n_strands, int n_points,
                   const uint8_t *shade, int H, int W, int supersample, int width, const float *depth0,
                   unsigned long long *keys, int32_t *dropped, void *stream);
int mh_photo_resolve(mh_ctx *ctx, const unsigned long long *keys, const float *depth0, int H, int W, int supersample,
                     int bust_code, int background_code, uint8_t *gray_u8, int32_t *cover, void *stream);
int mh_photo_view(mh_ctx *ctx, const float *cam_host, const float *points, const long long *offsets, int n_strands,
                  int n_points, const float *albedo, const double *light_host, double ambient, int H, int W, int supersample,
                  int width, const float *depth0, int bust_code, int background_code, void *scratch, size_t scratch_bytes,
                  uint8_t *gray_u8, int32_t *cover, void *stream);

/* Capture agreement (monohair_amd.hairreproj; no counterpart in the reference): a strand set scored against the observed 2D
 * maps of the capture it was reconstructed from -- do the strands run where the cameras saw hair, and along the orientation
 * they saw? -- a measurement that needs no ground truth.  Per view the inputs are the camera record, the observed planes
 * ori_u8 / conf_u8 / mask_u8 (uint8 [H,W] file codes, what mh_ctx_set_view_u8 takes), an optional occluder plane depth0
 * (float32 [H,W], PMVO's depth convention, background 255) and the strand set: points [n_points,3] float32 WORLD points,
 * offsets [n_strands+1] (int64).  The rule, per view:
 *
 * Vertex, segment, sample.  Exactly those of "Hair capture": mh_capture_project's (row, col, z255, valid); a segment = two
 *   consecutive valid points of one strand, n = max(1, ceil(max(|dr|, |dc|))), dropped and counted when n > 8192; qc =
 *   rint(4096*c2), qs = rint(4096*s2) and 0 when len = 0; sample j at t = (j + 0.5)/n with the half-to-even centre pixel p and
 *   zf = float32(z255_a + t*dz).
 * Front plane.  zmin = pass A of the capture rule (mh_capture_zmin) at a footprint `radius`, with depth0.
 * Classes of a sample, judged at its centre pixel p alone.  A sample whose centre lies outside the image, or whose zf is not
 *   finite, belongs to no class.
 *     visible    zf <= depth0[p] (when depth0 is given) and zf <= zmin[p] + tol (a float32 addition)
 *     on hair    visible and mask_u8[p] >= 52: PMVO's m > 0.2 on the loaders' decode (codes 50 and 51 decode to 50/255 and
 *                51/255, which are not above 0.2: they are not hair)
 *     confident  on hair and conf_u8[p] >= conf_min_code and ori_u8[p] < 180
 *     agrees at bound k (k < n_bounds <= 8)  confident, the segment's len > 0, and qc*T[c][0] + qs*T[c][1] >= bound[k] in
 *                float64 with c = ori_u8[p] (the two products rounded, then their sum); T = the float32 table of the capture
 *                rule's resolve step, widened (HOST); bound[k] HOST float64 (the callers set 4096*cos(2*angle_k))
 * Counters.  A row of 4 + n_bounds int64: {visible, on hair, confident, dropped segments, agrees[0], .. agrees[n_bounds-1]}:
 *   the numbers of samples of each class, and of segments with n > 8192.  strand_counts [n_strands, 4 + n_bounds] holds one row
 *   per strand, summed over its segments; it is ADDED to, never zeroed by a call, so one buffer collects all views.  view_counts
 *   [4 + n_bounds] is the same row summed over all strands of this call (zeroed first).  Integer sums: the result does not
 *   depend on the order of arrival.
 * Silhouette, three int64 pixel counts from zmin and mask_u8 (zeroed first): {predicted and observed, predicted only, observed
 *   only}; predicted = zmin[p] finite, observed = mask_u8[p] >= 52.
 *
 * mh_support_accumulate: vert / valid = mh_capture_project's, zmin = mh_capture_zmin's.  table_host: 180 x 2 float32 (HOST),
 *   bounds_host: n_bounds float64 (HOST), 0 <= conf_min_code <= 256 (256: no pixel is confident).  depth0 may be NULL;
 *   strand_counts may be NULL when n_points = 0.  No launch is made for fewer than two points.
 * mh_support_silhouette: silhouette [3].
 * mh_support_view: mh_capture_project, mh_capture_zmin and the two steps for one view on a scratch of
 *   mh_support_scratch_bytes(n_points, H, W) bytes, whose first int32 is left holding pass A's dropped count.
 *   0 <= radius <= 16, tol >= 0, H*W < 2^31, 1 <= n_bounds <= 8. */
size_t mh_support_scratch_bytes(int n_points, int H, int W);
int mh_support_accumulate(mh_ctx *ctx, const float *vert, const uint8_t *valid, const long long *offsets, int n_strands,
                          int n_points, int H, int W, float tol, const float *depth0, const float *zmin,
                          const uint8_t *ori_u8, const uint8_t *conf_u8, const uint8_t *mask_u8, int conf_min_code,
                          const float *table_host, const double *bounds_host, int n_bounds, long long *strand_counts,
                          long long *view_counts, void *stream);
int mh_support_silhouette(mh_ctx *ctx, const float *zmin, const uint8_t *mask_u8, int H, int W, long long *silhouette,
                          void *stream);
int mh_support_view(mh_ctx *ctx, const float *cam_host, const float *points, const long long *offsets, int n_strands,
                    int n_points, int H, int W, int radius, float tol, const float *depth0, const uint8_t *ori_u8,
                    const uint8_t *conf_u8, const uint8_t *mask_u8, int conf_min_code, const float *table_host,
                    const double *bounds_host, int n_bounds, void *scratch, size_t scratch_bytes, long long *strand_counts,
                    long long *view_counts, long long *silhouette, void *stream);

/* Strand volume (monohair_amd.hairvolume; no counterpart in the reference): a strand set turned into the volume the fit of
 * refine would ideally produce -- the occupied voxels with one direction each, in PMVO's own voxel conventions -- so that the
 * strand stage can be run on a perfect volume and a fitted volume can be scored.  points [n_points,3] float32 in `.hair`
 * coordinates (world minus bust_to_origin), offsets [n_strands+1] (int64, the exclusive scan of the per-strand point counts);
 * bust_to_origin [3], voxel_min [3] and voxel_size are HOST float64 (finite, voxel_size > 0), dims = (X, Y, Z) HOST int32 with
 * X*Y*Z < 2^31; 1 <= sub <= 16 samples per voxel of travel.  Everything is float64 arithmetic on the float32 values, + - * /
 * sqrt in the order written, nothing fused.  The rule:
 *
 * Vertex.  w = p + bust_to_origin; voxel coordinate g = ((w.x - vmin.x)/vs, ((-w.y) - vmin.y)/vs, ((-w.z) - vmin.z)/vs): p2v
 *   before rounding (Utils/PMVO_utils.py:386-404).  A vertex is valid iff all three are finite.
 * Segment (a, b) = consecutive points of one strand, both valid; any other pair makes nothing.  d = g_b - g_a; n = max(1,
 *   ceil(sub * max(|d.x|, |d.y|, |d.z|))); a segment with n > 8192 is dropped and counted (dropped_segments).  Direction, in
 *   WORLD space as the fit stores it: e = w_b - w_a, len = sqrt((e.x*e.x + e.y*e.y) + e.z*e.z), u = e / len, q = rint(4096 * u)
 *   per component, half to even, as integers; q = 0 when len is 0 (or not finite).
 * Sample j = 0 .. n-1: t = (j + 0.5)/n; voxel = rint(g_a + t*d) per component, half to even.  A sample whose voxel lies outside
 *   [0,X) x [0,Y) x [0,Z) is dropped and counted (outside_samples), not clamped.  Each kept sample adds to its voxel cnt += 1 and
 *   the six products qx*qx, qy*qy, qz*qz, qx*qy, qx*qz, qy*qz (int64).  Integer sums: the result does not depend on the order
 *   of arrival.
 * Resolve, per voxel with cnt > 0.  A voxel with cnt > 2^29 is refused (|q| <= 4096: up to there every sum stays within 2^53
 *   and converts to float64 exactly).  M = the symmetric 3x3 of the six sums as float64; trace = (Mxx + Myy) + Mzz.  If trace
 *   = 0: ori = 0, coh = 0 (occupied, no direction).  Otherwise v = the column of M with the largest diagonal entry, the first
 *   on ties; 24 times y = M v, each row as (a*v.x + b*v.y) + c*v.z, then v = y / sqrt((y.x*y.x + y.y*y.y) + y.z*y.z); then
 *   coh = ((v.x*y.x + v.y*y.y) + v.z*y.z) / trace with y = M v once more; if v.y > 0, v = -v (the fit's canonical sign,
 *   PMVO.py:702-703); ori = float32(v).
 *
 * mh_strand_volume_accumulate: acc [X*Y*Z][8] int64 = per voxel (x*Y + y)*Z + z {cnt, xx, yy, zz, xy, xz, yz, unused} and occ
 *   [X*Y*Z] uint8 = 1 where cnt > 0 (both are zeroed first); counters (device int64 [2]) = {dropped_segments, outside_samples}.
 * mh_strand_volume_resolve: index [n_voxels] int32 = the occupied voxels ascending (mh_select_rows on occ) -> voxels [n_voxels,3]
 *   int64 (x, y, z), the order mh_voxel_group's fit returns; ori [n_voxels,3] float32, cnt [n_voxels] int32, coh [n_voxels]
 *   float64, sums [n_voxels,6] int64 (optional: the six sums); refused (device int32) = the voxels over the cnt bound, whose
 *   outputs are zero.
 *
 * Volume scores: one sparse volume against another on the same grid.  A query voxel with float32 direction a has bit k set iff
 * some target voxel lies within Chebyshev distance reach[k] of it (|dx|, |dy|, |dz| <= reach[k]; neighbours outside the grid
 * do not exist) whose float32 direction b passes: cos2[k] < 0 (no direction test), or, in float64, dot = (a.x*b.x + a.y*b.y) +
 * a.z*b.z, na = (a.x*a.x + a.y*a.y) + a.z*a.z, nb likewise, na > 0 and nb > 0 and dot*dot >= cos2[k] * (na*nb).  reach (int32,
 * 0..4) and cos2 (float64) are HOST arrays of n_pairs <= 8.  Precision = matched predicted voxels / predicted voxels, recall
 * the same query the other way round; the flags are counted by mh_flag_counts.
 * mh_volume_index: voxels [n_voxels,3] int64 -> index [X*Y*Z] int32 = the row of the voxel at (x*Y + y)*Z + z, -1 where there
 *   is none; status (device int32 [2]) = {voxels outside the grid, voxels listed more than once}: either makes the list
 *   unusable (the caller raises).
 * mh_volume_match: out_flags [nq] uint8 for the queries (q_voxels, q_ori) against the targets (t_index, t_ori [n_targets,3]). */
int mh_strand_volume_accumulate(mh_ctx *ctx, const float *points, const long long *offsets, int n_strands, int n_points,
                                const double *bust_to_origin, const double *voxel_min, double voxel_size, const int32_t *dims,
                                int sub, long long *acc, uint8_t *occ, long long *counters, void *stream);
int mh_strand_volume_resolve(mh_ctx *ctx, const long long *acc, const int32_t *index, int n_voxels, const int32_t *dims,
                             long long *voxels, float *ori, int32_t *cnt, double *coh, long long *sums, int32_t *refused,
                             void *stream);
int mh_volume_index(mh_ctx *ctx, const long long *voxels, int n_voxels, const int32_t *dims, int32_t *index, int32_t *status,
                    void *stream);
int mh_volume_match(mh_ctx *ctx, const long long *q_voxels, const float *q_ori, int nq, const int32_t *t_index,
                    const float *t_ori, const int32_t *dims, const int32_t *reach, const double *cos2, int n_pairs,
                    uint8_t *out_flags, void *stream);

/* Inner fill (monohair_amd.hairfill; no counterpart in the reference, whose interior is the output of a network): the voxels
 * that lie inside the hair, outside the head and are seen by almost no view, and the exterior volume's orientations carried
 * inward to them -- the rows of `ours/raw.npy` the second pass merges (PMVO.py:733-751).  voxel_min [3] and voxel_size are HOST
 * float64 (finite, voxel_size > 0), dims = (X, Y, Z) HOST int32 with X*Y*Z < 2^31.  The votes compare float32 values as the vote
 * kernels do; everything else is float64 arithmetic on float32 inputs, + - * / sqrt in the order written, nothing fused.  The
 * rule has three parts.
 *
 * 1. Domain votes, for the centre of every voxel (x, y, z) of the grid.  Its world point is the inverse of p2v: w = (vmin.x +
 *   x*vs, -(vmin.y + y*vs), -(vmin.z + z*vs)) in float64, each component rounded once to float32.  For every view of the context
 *   (fp32 planes or 8-bit codes) w is projected and its pixel p rounded and clamped by the rule of the vote kernels
 *   (PMVO.project_points, PMVO.py:378-397: Camera.projection, ndc -> pixel, round half to even, the bounds tests on the
 *   integers); z' = -z_camera / 2 and z255 = z' * 255 in float32 as the votes form them.  A view ABSTAINS if the pixel is out of
 *   the image (out_index) or the point is not in front of the camera (not z' > 0; a NaN point abstains everywhere).  Otherwise
 *     visible = not (z255 - depth[p] > 0.9)        the float32 comparison of compute_unvisible_points, PMVO.py:470
 *     front   = z255 <= bust[p]                    bust: float32 [V,H,W], the depth plane of the bust ALONE in PMVO's depth
 *                                                  convention, 255 where there is none; equality counts as in front
 *     hair    = mask[p] > 0.2                      as the votes read the mask
 *   and the voxel's four int32 counts are n_in (views that do not abstain), n_vis (visible), n_front (front) and n_bad (front
 *   and not hair).  The voxel is in the DOMAIN iff n_in >= 1, n_vis <= 2 (the reference's "seen by at most two views"), n_front
 *   >= 1 (a voxel behind the bust's front surface in every view is inside the head), n_bad <= max_bad (0: no free line of sight
 *   ends on a pixel that is not hair) and it is not a voxel of the exterior volume.  This is a visual-hull test, not an inside
 *   test of the bust: it wrongly excludes hair in a concavity of the hull such as the one between neck and shoulder, where some
 *   view sees past the hair onto a pixel that is not hair.  The domain list is the flagged voxels ascending by (x*Y + y)*Z + z
 *   (mh_select_rows on the flags).
 * 2. Orientation sweeps.  An exterior voxel with float32 direction a has the tensor of the six products qx*qx, qy*qy, qz*qz,
 *   qx*qy, qx*qz, qy*qz of q = rint(4096 * a) per component, half to even, as integers (exact in float64).  A voxel whose
 *   direction is not finite, whose q is 0, or with a |q| component above 2^26 (the products would not be exact) is no SOURCE: it
 *   counts as absent.  A dense int32 map over the grid holds for every cell a domain row, an exterior row or nothing; the two
 *   lists must be unique, inside the grid and disjoint (status counts the offenders: the caller raises).  Per domain row there
 *   are six float64 T and a byte `known`, all zero at the start, each twice (ping-pong).  Sweep k = 1 .. sweeps updates every
 *   domain row from the buffers of sweep k-1: over the neighbours in the fixed order (x-1), (x+1), (y-1), (y+1), (z-1), (z+1),
 *   those outside the grid not existing, S = the sum in that order (from 0) of the tensors of the neighbours that are exterior
 *   sources or known domain rows, c = their number.  If c > 0: T = S / c per component, known = 1, and depth = k if the row was
 *   unknown; otherwise the row is carried over unchanged.  One lane per row, no atomics: a permuted domain list gives the
 *   permuted result.
 * 3. Resolve.  Each known row is resolved by the Resolve rule of "Strand volume" on M = T (the same device function,
 *   csrc/mh_volume.h): trace, the first-largest-diagonal column, 24 power steps, coh = v.(M v) / trace, v.y > 0 -> -v, ori =
 *   float32(v); rows that are unknown or have trace = 0 get ori = 0 and coh = 0.  A row is EMITTED iff it is known, trace > 0
 *   and coh >= min_coh (HOST float64, not NaN).  An output row is [w (float32), ori, 1.0], the seven columns of raw.npy, in
 *   domain order.
 *
 * mh_inner_votes: bust [V,H,W] float32 on the device, the views of ctx -> counts [X*Y*Z][4] int32 = {n_in, n_vis, n_front,
 *   n_bad} per voxel (x*Y + y)*Z + z.
 * mh_inner_domain: counts and ext_index [X*Y*Z] (mh_volume_index of the exterior voxels, or NULL: no exterior) -> flags
 *   [X*Y*Z] uint8.
 * mh_inner_diffuse: ext_voxels [n_ext,3] / dom_voxels [n_dom,3] int64, ext_ori [n_ext,3] float32, 0 <= sweeps <= 1024 -> map
 *   [X*Y*Z] int32 (domain row d: d + 1, exterior row e: -(e + 1), 0: none), ext_tensor [n_ext,6] float64, ext_source [n_ext]
 *   uint8, cell [n_dom] int32 (the row's (x*Y + y)*Z + z, -1 outside the grid), tensor [n_dom,6] float64 and known [n_dom] uint8
 *   = the state after the last sweep (tensor_b / known_b: the other half of the ping-pong, same sizes), depth [n_dom] int32 (0:
 *   never reached), status (device int32 [2]) = {voxels outside the grid, voxels whose cell was already taken}.
 * mh_inner_resolve: -> world [n_dom,3] and ori [n_dom,3] float32, coh [n_dom] float64, emit [n_dom] uint8; the emitted rows
 *   are compacted by mh_select_rows(emit, a = world, b = ori). */
int mh_inner_votes(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size, const int32_t *dims,
                   int32_t *counts, void *stream);
int mh_inner_domain(mh_ctx *ctx, const int32_t *counts, const int32_t *ext_index, const int32_t *dims, int max_bad,
                    uint8_t *flags, void *stream);
int mh_inner_diffuse(mh_ctx *ctx, const long long *ext_voxels, const float *ext_ori, int n_ext, const long long *dom_voxels,
                     int n_dom, const int32_t *dims, int sweeps, int32_t *map, double *ext_tensor, uint8_t *ext_source,
                     int32_t *cell, double *tensor, double *tensor_b, uint8_t *known, uint8_t *known_b, int32_t *depth,
                     int32_t *status, void *stream);
int mh_inner_resolve(mh_ctx *ctx, const long long *dom_voxels, int n_dom, const double *tensor, const uint8_t *known,
                     const double *voxel_min, double voxel_size, const int32_t *dims, double min_coh, float *world, float *ori,
                     double *coh, uint8_t *emit, void *stream);

/* Silhouette carve (monohair_amd.haircarve; no counterpart in the reference, whose coarse surface `ours/colmap_points.obj` and
 * depth maps `render_depth/` come from instant-ngp): the visual hull of the hair masks outside the head, as vote counts, as
 * flags and as a closed triangle mesh.  The conventions are those of "Inner fill": voxel_min [3] and voxel_size are HOST
 * float64 (finite, voxel_size > 0), dims = (X, Y, Z) HOST int32 with X*Y*Z < 2^31; the votes compare float32 values as the vote
 * kernels do; positions are float64 arithmetic rounded once to float32, nothing fused.  The rule has two parts.
 *
 * 1. Votes, for the centre of every voxel (x, y, z) of the grid: the float32 world point w of "Inner fill" part 1 (the same
 *   device function, csrc/mh_volume.h).  For every view of the context (fp32 planes or 8-bit codes) w is projected, its pixel p
 *   rounded and clamped, and z' and z255 formed exactly as there, and the view ABSTAINS exactly as there: the pixel is out of
 *   the image, or not z' > 0 (a NaN point abstains everywhere).  Otherwise
 *     free = z255 <= bust[p]                       bust: float32 [V,H,W], the depth plane of the bust ALONE, 255 where there is
 *                                                  none: the bust's front face does not hide the voxel; equality counts as free
 *     hair = mask[p] > 0.2                         as the votes read the mask
 *   and the voxel's three int32 counts are n_in (views that do not abstain), n_free (free) and n_miss (free and not hair): on
 *   any context the columns n_in, n_front and n_bad of mh_inner_votes.  Only the cameras and the mask planes of the context are
 *   read (never depth, orientation or confidence).  The voxel is INSIDE iff n_free >= min_free and n_miss <= max_miss (HOST
 *   ints, min_free >= 1, max_miss >= 0; the defaults of the Python layer are 2 and 0).  A voxel that the bust hides in every
 *   view is inside the head: n_free = 0, never INSIDE.
 * 2. The hull as a mesh, of uint8 flags [X*Y*Z] (non-zero = INSIDE) at (x*Y + y)*Z + z, whatever made them.  Walk the INSIDE
 *   voxels ascending by (x*Y + y)*Z + z and, for each, the six directions in the order -x, +x, -y, +y, -z, +z.  A face is
 *   EXPOSED iff the neighbour in that direction lies outside the grid or is not INSIDE.  Voxel (x, y, z) has the eight grid
 *   corners (x + di, y + dj, z + dk), di, dj, dk in {0, 1}; the four corners c0..c3 of a face, as (di dj dk):
 *     -x: 000 001 011 010      +x: 100 110 111 101
 *     -y: 000 100 101 001      +y: 010 011 111 110
 *     -z: 000 010 110 100      +z: 001 101 111 011
 *   Each exposed face gives the triangles (c0, c1, c2) and (c0, c2, c3), in that order.  In voxel coordinates every face is
 *   counter-clockwise seen from outside (right-handed normal = the direction); world y and z are the negated voxel axes, a
 *   rotation by half a turn about x, so the same holds in world coordinates: the signed volume of the mesh is the number of
 *   INSIDE voxels times voxel_size^3.  The VERTICES are the distinct grid corners (i, j, k), 0 <= i <= X, 0 <= j <= Y, 0 <= k <=
 *   Z, that some exposed face uses, ascending by (i*(Y+1) + j)*(Z+1) + k; corner (i, j, k) lies at
 *     (vmin.x + (i - 0.5)*vs, -(vmin.y + (j - 0.5)*vs), -(vmin.z + (k - 0.5)*vs))
 *   in float64 ((i - 0.5) is exact, then one product, one sum, the negation), each component rounded once to float32: a voxel's
 *   cell is centred on its centre of part 1.  Faces index the vertices from 0 as int32; (X+1)*(Y+1)*(Z+1) < 2^31 is required
 *   and refused otherwise.  The output order is fixed by this rule: every position is a count of what precedes it (counting
 *   passes and scans, no atomics).
 *
 * mh_carve_votes: bust [V,H,W] float32 on the device, the views of ctx -> counts [X*Y*Z][3] int32 = {n_in, n_free, n_miss}.
 * mh_carve_inside: -> flags [X*Y*Z] uint8, the decision of part 1.  A voxel leaves its view loop once n_miss > max_miss (the
 *   decision is then taken: n_miss only grows).
 * mh_carve_mesh_scratch_bytes: the bytes of `scratch` for these dims (host), 0 for dims that are refused.
 * mh_carve_mesh_count: flags -> counts (device int64 [2]) = {n_vertices, n_triangles}.
 * mh_carve_mesh: -> vertices [n_vertices,3] float32, faces [n_triangles,3] int32, for the counts of mh_carve_mesh_count on the
 *   same flags (HOST values).  It repeats the counting passes, so the scratch carries nothing from call to call; a row at or
 *   beyond the stated sizes is not written.  Nothing but the two outputs and `scratch` is written. */
int mh_carve_votes(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size, const int32_t *dims,
                   int32_t *counts, void *stream);
int mh_carve_inside(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size, const int32_t *dims,
                    int min_free, int max_miss, uint8_t *flags, void *stream);
size_t mh_carve_mesh_scratch_bytes(const int32_t *dims);
int mh_carve_mesh_count(mh_ctx *ctx, const uint8_t *flags, const int32_t *dims, long long *counts, void *scratch,
                        size_t scratch_bytes, void *stream);
int mh_carve_mesh(mh_ctx *ctx, const uint8_t *flags, const double *voxel_min, double voxel_size, const int32_t *dims,
                  long long n_vertices, long long n_triangles, float *vertices, int32_t *faces, void *scratch,
                  size_t scratch_bytes, void *stream);

/* Photo-consistent carve (monohair_amd.hairstereo; no counterpart in the reference): a second carve pass over candidate
 * voxels, by the agreement of the capture's gray photographs across neighbouring views.  The conventions are those of
 * "Silhouette carve" and "Inner fill": voxel_min [3] and voxel_size are HOST float64 (finite, voxel_size > 0), dims = (X, Y, Z)
 * HOST int32 with X*Y*Z < 2^31, a voxel's linear index is (x*Y + y)*Z + z, its centre w and the projection of w are those of
 * "Inner fill" part 1 (the same device functions, csrc/mh_volume.h and csrc/mh_front.h), and the float32 comparisons are those
 * of the vote kernels.  Only the cameras and the mask planes of the context are read.  Everything after the projection is
 * integer arithmetic, so the result does not depend on any order of evaluation.  Host ints: cell (1 <= cell <= 256), radius in
 * {1, 2, 3}, K = n_neighbours (1 <= K <= 8), keep (1 <= keep <= K), max_cost >= 0, min_agree >= 1, min_through >= 1; host
 * float32 m255 (finite, >= 0), a margin on the scale of the depth planes (z255).  The rule has five parts.
 *
 * 1. Reduced images and census codes, of gray: uint8 [V,H,W].  Hc = ceil(H / cell), Wc = ceil(W / cell); block (i, j) holds the
 *   pixels (row, col) of the image with row / cell == i and col / cell == j (integer division), n of them (fewer than cell^2 at
 *   the lower and right borders), and g[v,i,j] = (2*sum + n) / (2*n) in integers, sum being the sum of the block's pixels: the
 *   mean rounded half up, a uint8.  With B = (2*radius + 1)^2 - 1, bit b of census[v,i,j] (a uint64, bits B and above zero)
 *   is g[v, clamp(i + dy, 0, Hc - 1), clamp(j + dx, 0, Wc - 1)] < g[v,i,j], the offsets (dy, dx) running row-major from
 *   (-radius, -radius) to (radius, radius) with the centre left out: b = 0 is (-radius, -radius), b = B - 1 is (radius, radius).
 * 2. Per (voxel w, view v) terms.  The view abstains, and otherwise free, hair, the rounded and clamped pixel (row, col) and
 *   z255 are formed, exactly as in "Silhouette carve" part 1.  The view TAKES PART in w iff it does not abstain and w is both
 *   free and hair there.  The voxel's cell in the view is (row / cell, col / cell).
 * 3. Cost and winners.  neighbours: int32 [V,K]; row r lists the neighbour views of view r, an entry outside [0, V) (-1 by
 *   convention) is none; a row never names r itself (an entry that does is none as well; the Python layer refuses such a
 *   table).  For a candidate voxel w and a view r that takes part in w, h_n = popcount(census[r, cell of w in r] ^ census[n,
 *   cell of w in n]) for every entry n of row r that takes part in w (an n listed twice counts twice).  With fewer than keep
 *   such n the pair (w, r) has no cost.  Otherwise S = the sum of the keep smallest h_n and cost = (1024 * S) / (B * keep) in
 *   integers (at most 1024).  The WINNER of (r, cell) is the minimum, over the candidates w that have a cost in r and lie in
 *   that cell, of the uint64 key (cost << 32) | linear index of w: the lowest cost, among equal costs the lowest index.  A
 *   cell without such a candidate holds all ones.
 * 4. Agreement.  A cell's key is VALID iff it is not all ones, its cost (key >> 32) is <= max_cost and its index (the low 32
 *   bits) is below X*Y*Z; w* is then the voxel of that index and z255_r(w*) its z255 in view r, projected again by the same
 *   function.  agree[w] of a candidate w is the number of views r that take part in w, whose cell of w holds a valid key, and
 *   in which |z255_r(w) - z255_r(w*)| <= m255 (the float32 difference, its absolute value, the float32 comparison).  A winner
 *   agrees with itself.  agree of a voxel that is no candidate is 0.
 * 5. Refinement.  through[w] of a candidate w is the number of views r that do not abstain and in which w is free (hair or
 *   not), whose cell of w holds a valid key with agree[w*] >= min_agree, and in which z255_r(w) + m255 < z255_r(w*) (the
 *   float32 sum, the float32 comparison): w lies in front of a confirmed winner by more than the margin.  refined[w] = 1 iff w
 *   is a candidate and through[w] < min_through, else 0.  The stereo depth of (r, cell) is z255_r(w*) of a valid key with
 *   agree[w*] >= min_agree, else 255.
 *
 * mh_stereo_census: gray [n_views, height, width] uint8 on the device (any context: nothing of it is read) -> reduced
 *   [n_views, Hc, Wc] uint8 = g and census [n_views, Hc, Wc] uint64.
 * mh_stereo_winners: the views of ctx are V x H x W; bust [V,H,W] float32 as for the carve; candidates [n_candidates] int32, the
 *   linear indices of the candidate voxels in any order, each at most once (an index outside the grid is skipped; the Python
 *   layer compacts the flags with mh_select_rows); census [V,Hc,Wc] of part 1 for the same cell and radius; neighbours [V,K]
 *   int32 on the device -> keys [V,Hc,Wc] uint64, every cell written (all ones first, then a 64-bit atomic minimum per
 *   (candidate, view) with a cost: the one place the rule's minimum needs an atomic).  n_candidates = 0 gives all ones.
 * mh_stereo_agree: flags [X*Y*Z] uint8 (non-zero = candidate), keys of mh_stereo_winners -> agree [X*Y*Z] int32.
 * mh_stereo_refine: -> refined [X*Y*Z] uint8 and depth [V,Hc,Wc] float32.  agree is read at the index of a valid key only.
 * Nothing but the stated outputs is written; no entry point synchronises with the host. */
int mh_stereo_census(mh_ctx *ctx, const uint8_t *gray, int n_views, int height, int width, int cell, int radius,
                     uint8_t *reduced, unsigned long long *census, void *stream);
int mh_stereo_winners(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size, const int32_t *dims,
                      const int32_t *candidates, int n_candidates, const unsigned long long *census,
                      const int32_t *neighbours, int n_neighbours, int cell, int radius, int keep, unsigned long long *keys,
                      void *stream);
int mh_stereo_agree(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size, const int32_t *dims,
                    const uint8_t *flags, const unsigned long long *keys, int cell, int max_cost, float m255, int32_t *agree,
                    void *stream);
int mh_stereo_refine(mh_ctx *ctx, const float *bust, const double *voxel_min, double voxel_size, const int32_t *dims,
                     const uint8_t *flags, const unsigned long long *keys, const int32_t *agree, int cell, int max_cost,
                     float m255, int min_agree, int min_through, uint8_t *refined, float *depth, void *stream);

/* ---- the one exchange of the data path, RCCL over xGMI.  The reference has no multi-GPU path
 * (options.py:112 asserts a single GPU); the voxel fit of refine (PMVO.py:695-726) is sharded here by x-slabs of
 * the volume, every rank fitting the voxels of its slab into a zero-initialised dense [X,Y,Z,C] fp32 volume (C = 4:
 * occupancy + orientation), and rank `root` assembles the shared volume:
 *   mode 0: slab gather -- ownership is disjoint, so every peer ncclSend's its slab straight to the root, which
 *           ncclRecv's it in place ((nranks-1)/nranks of the volume crosses xGMI, one slab per link);
 *   mode 1: dense ncclReduce(sum) of the whole volume (x + 0 is exact: the same result; kept for comparison).
 * slab_host (host, nranks+1 ints): rank r owns x in [slab_host[r], slab_host[r+1]).  `comm` is an ncclComm_t:
 * mh_comm_init makes one from a 128-byte ncclUniqueId that rank 0 obtains with mh_comm_unique_id and hands to the
 * other ranks by any means (torch.distributed broadcast, a file, MPI); any ncclComm_t of the caller works as well.
 * librccl.so.1 is bound at run time; a process that never calls these does not load it. */
int mh_comm_unique_id(void *id_out_host /*128 bytes*/);
int mh_comm_init(mh_ctx *ctx, const void *id_host /*128 bytes*/, int nranks, int rank, void **comm_out);
int mh_comm_destroy(void *comm);
int mh_volume_reduce(mh_ctx *ctx, void *comm, int rank, int nranks, int root, float *volume /*[X,Y,Z,C] in place*/,
                     int X, int Y, int Z, int C, const int32_t *slab_host, int mode, void *stream);
/* The slab gather with slab-sized buffers on the peers (what monohair_amd.dist.voxel_fit_reduced uses): `slab` is this
 * rank's own x-slab [slab_host[rank+1]-slab_host[rank], Y, Z, C] (device, contiguous; may be NULL when the slab is empty),
 * `volume` the dense [X,Y,Z,C] volume on the root only (NULL elsewhere).  The root's own slab is copied into place on the
 * stream unless slab == volume + slab_host[root]*Y*Z*C.  Wire traffic = mode 0 above; a peer holds 1/nranks of the volume.
 * The environment variable MH_RCCL_LIB=<path> binds another library for these entry points (e.g. tests/fake_rccl.cpp, a
 * stand-in built against rccl.h that lets several ranks share one GPU: how the nranks > 1 branches are tested on a
 * one-GPU box); an unloadable path is an error. */
int mh_volume_gather(mh_ctx *ctx, void *comm, int rank, int nranks, int root, const float *slab, float *volume, int X,
                     int Y, int Z, int C, const int32_t *slab_host, void *stream);

/* ---- host-side IO of the volume files: scipy.io.savemat of PMVO.py:753-764 writes dense float64 arrays that are zero
 * except at the occupied voxels.  Creates `path` = prefix (the MAT-v5 header + array tags, built by the caller) + a
 * zero-filled payload of payload_bytes, then stores values[i] at payload element elem_index[i] (float64 elements; later
 * entries win on duplicates).  The file is sparse on disk; the scatter runs on `threads` host threads split by
 * destination range.  Host pointers only; no GPU involved. */
int mh_mat_write_sparse(const char *path, const void *prefix, size_t prefix_bytes, size_t payload_bytes,
                        const long long *elem_index, const double *values, size_t n, int threads);
/* The same file in steps (open -> touch -> store -> close): `touch` makes the pages of the given elements resident without
 * changing them, so a background thread can take the page faults of the zero-filled mapping (16-19 ms for the two volume files
 * of a pass) early -- with every candidate point's voxel, a superset of what can become occupied -- while the GPU still works;
 * `store` writes the occupied elements (later entries win).  The finished file is byte for byte what mh_mat_write_sparse and
 * scipy's dense savemat write (PMVO.py:753-764). */
int mh_mat_sparse_open(const char *path, const void *prefix, size_t prefix_bytes, size_t payload_bytes, void **handle);
int mh_mat_sparse_touch(void *handle, const long long *elem_index, size_t n);
int mh_mat_sparse_store(void *handle, const long long *elem_index, const double *values, size_t n);
/* store from the voxel list of the fit: vox [G,3] (x,y,z) -> element y + Y*(x + X*z) (+ c*X*Y*Z for channel c of Ori);
 * ori == NULL writes 1.0 (Occ), else ori [G,3] float32 (ori_is_f64 = 0) or float64; later rows win */
int mh_mat_sparse_store_voxels(void *handle, const long long *vox, const void *ori, int ori_is_f64, size_t G, int X, int Y,
                               int Z);
int mh_mat_sparse_close(void *handle);

/* Supported options of a context (mh_ctx_set_option): how results are rounded and which shipped form computes them.
 * Anything else is an argument error; the A/B forms and cross-check kernels the tests and bench.py switch between are NOT
 * here but in include/mh_pmvo_lab.h (mh_ctx_set_lab_option).
 *   "reproject_rule": how the sgemms of PMVO.sample_next_3d_pos (Camera.projection / Camera.reprojection of the points that
 *       share a base view, PMVO.py:289,318 -> Utils/Camera_utils.py:50-53,103) round.  0 (default): by the number M of points
 *       of the batch that share the (rank, base view), as MKL does in the reference -- M == 1: single-column projection;
 *       S*M >= "reproject_fma_min_cols" or S*M <= 3: k-ordered fma chain; otherwise separately rounded products.  1: the
 *       mid-size forms for every point (rounds 1-4; independent of the batch).  2: the chain forms for every point.
 *   "reproject_fma_min_cols": the column count from which MKL's sgemm switches to its threaded (fma chain) kernel ON THE
 *       HOST THE REFERENCE RUNS ON -- it moves with that host's thread count: 8 threads 28445 (default: MKL 2024.2, AVX-512,
 *       where the goldens were generated), 4 threads 14223, 2 threads 21334, 1 thread never (2147483647).
 *       `python tools/probe_mkl_forms.py --emit-options` prints the value for a host; PMVO.py takes it as
 *       --PMVO.reference_host=<json>; pinned end to end at 1 / 2 / 4 / 8 threads (tests/golden/pmvo_threads.npz).
 *   "sum_block": 32 (default) ATen's sum(dim=0) adds the trailing (columns mod 32) of a [V, N*S] / [V, N] sum in its
 *       row_sum order (forward: the last samples of the last point of a batch; refine / filter votes: the last points of a
 *       batch), and the [V, 1] sums of a batch of ONE point in its inner-sum order; 0: cascade order everywhere (rounds 1-4).
 *   "topk_order": see mh_topk_views (0 = torch.topk's order among equal confidences, default; 1 = view order).
 *   "gabor_variant": 3 (default) mh_gabor_mfma2_kernel (FP32 MFMA); 0 the direct v_pk_fma kernel.  Same results.
 *   "tap_plane_max_mb" (default 4096; environment MH_TAP_PLANE_MAX_MB at context creation): contexts with fp32 views keep
 *       every pixel once more as a ready-made patch tap (unit orientation, clamped confidence: 16 B per pixel, +1.2 %
 *       iterations/s) only if that plane is at most this large and leaves a quarter of the free device memory: 60 x 1080p
 *       (1 991 MB) gets it, 120 x 4K (15 925 MB) does not unless the budget is raised.  Takes effect before the first view.
 *   "line_rule" (mh_render_strands): 0 = OpenGL's diamond-exit rule (default), 1 = the pixel that holds a segment's end
 *       point is drawn too (what Google SwiftShader does; changes the image: used to compare with that GL).
 *   "raster_subpixel_bits" (mh_render_depth, mh_render_strands): window positions are snapped to 2^-bits pixel, 4..8,
 *       default 8; OpenGL requires at least 4, which is what SwiftShader uses (changes the image at silhouettes). */
int mh_ctx_set_option(mh_ctx *ctx, const char *key, int value);

#ifdef __cplusplus
}
#endif
#endif /* MH_PMVO_H */
