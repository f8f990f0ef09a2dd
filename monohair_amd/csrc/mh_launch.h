// mh_launch.h -- everything that crosses between capi*.cpp (the C ABI) and the kernel files: the plain structs that go by
// value or by layout, the sizes both sides must agree on, and ONE prototype per launcher / preload / size function.
// Internal (not installed).  Every .hip file sees it through mh_device.h before it defines its launchers, so a definition
// that disagrees with its declaration does not compile.  No __device__ code here: capi*.cpp include this file alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/mh_pmvo.h"   // MH_CAM_STRIDE, MH_TOPK

struct MhViews {
    int V, H, W;
    const float4 *rec;   // [V][H][W] {ori_row, ori_col, conf, depth}
    const float *mask;   // [V][H][W]
    const float *cams;   // [V][MH_CAM_STRIDE]
    const float4 *tap;   // [V][H][W] {unit ori_row, unit ori_col, clamped conf, 0}: what a patch tap of the search is, per pixel,
                         // made once at upload by the same mh_unit2 / mh_clampf the front end would apply per iteration
                         // (nullptr: not resident -- views uploaded as 8-bit codes use the code tables instead)
    int batch_rule;      // 1: option reproject_rule 0 -- the projections follow the batch (a batch of ONE point projects
                         // through the single-column form, see mh_cam_project_b); 0: one form for everything
};

// The points per (rank, base view) of a batch (mh_device.h: MhRule) are counted in MH_GROUP_COPIES partial arrays (a workgroup
// of the counting kernel adds to copy blockIdx % COPIES): up to 670 points of a 5000-point chunk share one (rank, base view),
// and that many atomics on ONE address drain in ~9 us.  The C API hands the array out of the search scratch.
#define MH_GROUP_COPIES 16
// One workgroup of the search holds one point: its nrank * S (rank, sample) items share LDS arrays of these sizes.  The entry
// points of capi.cpp refuse more items or ranks (MH_ERR_ARG) before their first launch; mh_launch_search answers -1.
#define MH_MAX_ITEMS 1024
#define MH_MAX_RANKS 16
#define MH_GROUP_RANKS MH_MAX_RANKS
// mh_prj_loss_kernel keeps 2 * S floats of dynamic LDS next to MH_PRJ_LOSS_STATIC_LDS bytes of static LDS (s_npos, s_bl[4],
// s_bi[4]); without a raised dynamic-LDS attribute a workgroup's static + dynamic LDS may not exceed 64 KiB
#define MH_PRJ_LOSS_STATIC_LDS 36
#define MH_PRJ_LOSS_MAX_S ((65536 - MH_PRJ_LOSS_STATIC_LDS) / 8)   // 8187

#define MH_DG_MAXR 48                 // radius limit: sigma <= 11.9 at truncate 4 (the reference uses 0.4 and 10: 2 and 40)
struct MhDogWeights {                 // device-resident; w[s][j + r[s]] for j = -r[s] .. 0 (the symmetric half incl. the centre)
    double w[2][MH_DG_MAXR + 1];
    int r[2];
};

#define MH_MATCH_MAXK 8               // threshold pairs of one mh_strand_match launch: one bit each of the flag byte
struct MhMatchPairs {                 // pair k: squared distance bound and cosine of the angle bound, both inclusive
    double r2[MH_MATCH_MAXK], c[MH_MATCH_MAXK];
    int K;
};

#define MH_CAP_MAXN 8192              // hair capture: a segment of more samples than this is dropped and counted
struct MhCapCam {                     // one camera record, by value (a kernel argument)
    float c[MH_CAM_STRIDE];
};
struct MhCapTable {                   // float32 (cos 2 theta_k, sin 2 theta_k) of the 180 orientation codes, by value
    float t[180][2];
};
#define MH_SUP_COLS 4                 // capture agreement: visible, on hair, confident, dropped segments; then one per bound
#define MH_SUP_MAX_BOUNDS 8
struct MhSupBounds {                  // the agreement bounds 4096 cos(2 angle_k) of the host, by value
    double b[MH_SUP_MAX_BOUNDS];
    int n;
};

#define MH_VOL_MAXN 8192              // strand volume: a segment of more samples than this is dropped and counted
#define MH_VOL_MAXCNT (1ll << 29)     // ... and a voxel of more samples than this is refused: |q| <= 4096, so every sum stays
                                      // within 2^29 * 2^24 = 2^53 and converts to float64 exactly
struct MhVolGrid {                    // the voxel grid of PMVO's volume, by value (all host values)
    double bust[3], vmin[3], vs;
    int X, Y, Z;
};
#define MH_VOL_MAXK 8                 // threshold pairs of one mh_volume_match launch: one bit each of the flag byte
#define MH_VOL_MAXREACH 4
struct MhVolPairs {                   // pair k: Chebyshev radius in voxels, squared-cosine bound (< 0: no direction test)
    double cos2[MH_VOL_MAXK];
    int reach[MH_VOL_MAXK];
    int K;
};
#define MH_FILL_MAXQ 67108864.0       // inner fill: |q| = |rint(4096 a)| up to 2^26 has exact products in int64 and float64
#define MH_FILL_MAXSWEEPS 1024

struct MhRVert;   // raster.hip: a transformed mesh vertex (16 B)
struct MhRLVert;   // raster.hip: a transformed strand vertex (32 B)

// What one launch of the search does, decoded once from the lab option "search_variant" (include/mh_pmvo_lab.h) by capi.cpp.
struct MhSearchPlan {
    bool portable;      // mh_search_kernel<4,256>, the cross-check of the shipped kernel (1256; also what a launch without
                        // list lengths gets); nothing below applies to it
    bool select_body;   // mh_search3_kernel with the compare-and-select tap body instead of the key body (100.., "search_body",
                        // contexts of 8-bit views)
    enum Order {
        ORDER_NATURAL,         // points in their natural order (7)
        ORDER_BY_WORK,         // descending order of work: mh_search_work_kernel + mh_search_order_kernel (0)
        ORDER_CLASSES_READY    // the same order; the work classes are in order[0..N) already -- the fused forward lets the
                               // ranking kernel write them
    } order;
    enum Part {         // the launch split for measurements (bench.py times the two parts with HIP events)
        PART_ALL,
        PART_PRE_ONLY,      // what precedes the search (group sizes, work classes, launch order), then stop (9)
        PART_KERNEL_ONLY    // mh_search3_kernel alone on what PART_PRE_ONLY left in the scratch (10)
    } part;
};

// The patch sides the kernels templated on PATCH are built for: odd sides 1..11 (the reference's configurations use 5, 7 and
// 9).  launch(std::integral_constant<int, PATCH>) launches the instantiation(s) of a launcher; the answer is what they left in
// hipGetLastError, or -1 -- nothing launched -- for any other side (the C API turns that into MH_ERR_ARG).
template <int... PS, typename F>
static inline int mh_dispatch_patch_among(int patch, F &&launch) {
    const bool launched = ((patch == PS && (launch(std::integral_constant<int, PS>{}), true)) || ...);
    return launched ? (int)hipGetLastError() : -1;
}
template <typename F>
static inline int mh_dispatch_patch(int patch, F &&launch) {
    return mh_dispatch_patch_among<1, 3, 5, 7, 9, 11>(patch, launch);
}

extern "C" {
// ---- pmvo_project.hip
int mh_launch_pack_view(float4 *rec, float *maskp, const float *depth, int dstride, const float *ori, const float *conf,
                        const float *mask, int mstride, size_t npix, float4 *tapp, hipStream_t st);
int mh_launch_pack_view_u8(float4 *rec, float *maskp, const float *depth, int dstride, const uint8_t *ori,
                           const uint8_t *conf, const uint8_t *mask, const float4 *lut, size_t npix, uint16_t *oc,
                           float4 *tapp, hipStream_t st);
size_t mh_code_tabs_bytes();
int mh_launch_code_tabs(const float4 *lut, void *tabs, hipStream_t st);
int mh_launch_project_gather(MhViews vw, const float *pts, int N, int patch, float *vis, float *ori, float *conf,
                             float *mask, float *ori_patch, float *conf_patch, float *pixf, hipStream_t st);
int mh_launch_topk_work(const float *vis, const float *conf, int V, int N, int32_t *out_idx, float *out_val, int order,
                        const uint8_t *cnt, int32_t *cls, int P1, int nrank, int rank_step, int S,
                        int32_t *gcnt /* [nrank][V], zeroed: the batch's group sizes (or nullptr) */,
                        int tail_n0 /* first point with trailing columns of the batch's sums (N: none) */, hipStream_t st);
int mh_launch_topk(const float *vis, const float *conf, int V, int N, int32_t *out_idx, float *out_val, int order,
                   hipStream_t st);
int mh_launch_prep_taps(const float *ori_patch, const float *conf_patch, const float *vis, const float *pixf, int VN, int P,
                        float thr, float4 *taps, uint8_t *cnt, hipStream_t st);
int mh_launch_project_taps(MhViews vw, const float *pts, int N, int patch, float thr, float *vis, float *ori, float *conf,
                           float *mask, float4 *taps, uint8_t *cnt, int tile, const uint16_t *oc, const void *tabs_v,
                           int32_t *zero, int nzero /* ints the first workgroup clears (group sizes of the batch) */,
                           hipStream_t st);
int mh_preload_pmvo_project();

// ---- pmvo_search.hip (mh_debug_key_stats: include/mh_pmvo_lab.h)
int mh_launch_search(MhViews vw, const float *offs, int S, int nrank, int rank_step, const float *pts, int N, int P1,
                     float thr, const float *ori_c, const int32_t *base_idx, const float *base_val, const float4 *taps,
                     int32_t *order /* 2N ints of work space */, const uint8_t *cnt /* [V,N] list lengths */,
                     float *line_ori, float *min_loss, uint8_t *high_conf, float *best_sample, int32_t *best_rank,
                     int32_t *best_s, MhSearchPlan plan, int rule_mode, int fma_min_cols, int sum_block,
                     int32_t *gcnt /* MH_GROUP_COPIES * MH_GROUP_RANKS * V ints of work space */,
                     int groups_ready /* gcnt holds the batch's group sizes already (the fused forward) */, hipStream_t st);
int mh_preload_pmvo_search();

// ---- pmvo_refine.hip (the losses of PMVO.refine and of its smoothing loop)
int mh_launch_refine_loss_maps(MhViews vw, const float *pts, const float *dir, float mul, float dv, int N, int patch,
                               float thr, float *loss, uint8_t *hc, int batch, long long row0, long long total,
                               int sum_block, hipStream_t st);
int mh_launch_refine_combine(const float *center, const float *loss_u, const uint8_t *head, const uint8_t *head_top,
                             float thr, float *ori, float *loss_out, int N, hipStream_t st);
int mh_launch_refine_loss(MhViews vw, const float *pts, const float *dir, float mul, float dv, int N, int P, float thr,
                          const float *vis, const float *ori_patch, const float *conf_patch, float *loss, uint8_t *hc,
                          int sum_block, hipStream_t st);
int mh_preload_pmvo_refine();

// ---- pmvo_filter.hip
int mh_launch_filter_points(MhViews vw, const float *pts, int N, int patch, float thr, float vis_thr,
                            uint8_t *surface_index, uint8_t *filter_index, uint8_t *unvisible_index, uint8_t *head_filter,
                            int batch, long long row0, long long total, int sum_block, int rows_kernel,
                            const int32_t *order, hipStream_t st);
int mh_preload_pmvo_filter();

// ---- pmvo_pieces.hip
int mh_launch_project_points(const float *cam, const float *pts, int N, int H, int W, int32_t *rc, float *zp, uint8_t *oob,
                             float *pixf, int batch_rule, hipStream_t st);
int mh_launch_gather(MhViews vw, int v, const long long *uv, int N, int size, float4 *rec_out, float *mask_out,
                     hipStream_t st);
int mh_launch_compute_visible(const float *depth, const float *z, size_t n, float *out, hipStream_t st);
int mh_launch_sample_next(MhViews vw, const float *pts, const int32_t *base_view, const float *ori, const float *offs,
                          int N, int S, float *out, int rule_mode, int fma_min_cols,
                          int32_t *gcnt /* MH_GROUP_COPIES * MH_GROUP_RANKS * V ints of work space (rule_mode 0) */,
                          hipStream_t st);
int mh_launch_reproject(MhViews vw, const float *pts, const float *samples, int N, int S, float *D, hipStream_t st);
int mh_launch_prj_loss(const float *D, const float *ori_patch, const float *conf_patch, const float *vis, int V, int N,
                       int S, int P, float thr, float *loss, long long *index, uint8_t *hc, float *all_loss, int sum_block,
                       hipStream_t st);
int mh_preload_pmvo_pieces();

// ---- consensus.hip
int mh_launch_replace_dissimilar(const float *center, float *ori, float thr, int N, hipStream_t st);
int mh_launch_medoid_dense(const float *ori, const int32_t *index, int G, int K, float *out, int32_t *out_index,
                           hipStream_t st);
int mh_launch_medoid_segmented(const float *ori, const int32_t *seg_start, int G, int max_group, float *out,
                               int32_t *out_index, hipStream_t st);
int mh_preload_consensus();

// ---- gabor.hip
int mh_launch_gabor_build(float *bankT, hipStream_t st);
size_t mh_gabor_state_bytes();
size_t mh_gabor_bankq_bytes();
int mh_launch_gabor_relayout(const float *bankT, float *bankQ, hipStream_t st);
int mh_launch_gabor_bank(const float *bankT, const float *bankQ, const float *img, int H, int W, int32_t *orient,
                         float *conf, float *var, unsigned int *maxbits, int variant, uint8_t *k8, uint8_t *c8,
                         hipStream_t st);
int mh_preload_gabor();

// ---- dog.hip
int mh_launch_dog(const void *img, int in_kind, int H, int W, const void *weights /* device MhDogWeights */,
                  double *scratch, double *out64, float *out32, hipStream_t st);
int mh_preload_dog();

// ---- knn.hip
int mh_launch_knn(float ox, float oy, float oz, float h, int dx, int dy, int dz, const float *pts, const int32_t *order,
                  const int32_t *cell_start, const void *queries, int q64, int Q, int k, int ring0, const int32_t *qperm,
                  const uint8_t *valid, int32_t *out_idx, int32_t *status, hipStream_t st);
int mh_launch_nearest_dist(const float *pts, int N, const double *ref, int M, double *out, double max_dist,
                           double z_limit, uint8_t *mask, hipStream_t st);
int mh_preload_knn();

// ---- sortgroup.hip
size_t mh_grid_scratch_bytes_impl(int M);
size_t mh_sort_scratch_bytes_impl(int n);
int mh_launch_grid_build(const float *pts, int M, float ox, float oy, float oz, float h, int dx, int dy, int dz,
                         void *scratch, size_t scratch_bytes, float *pts_sorted, int32_t *order, int32_t *cell_start,
                         int32_t *n_occupied, hipStream_t st);
int mh_launch_sort_keys(const unsigned long long *keys, int n, int end_bit, void *scratch, size_t scratch_bytes,
                        unsigned long long *keys_out, int32_t *order, hipStream_t st);
size_t mh_voxel_group_scratch_bytes_impl(int n);
int mh_launch_voxel_group(const void *pts, int pts_f64, const float *ori, int n, const double *vmin, double vs,
                          const int32_t *dims, void *scratch, size_t scratch_bytes, unsigned long long *keys_out,
                          int32_t *order, float *ori_sorted, hipStream_t st);
int mh_launch_words_differ(const void *a, const void *b, size_t nwords, int32_t *flag, hipStream_t st);
int mh_launch_points_bbox(const float *pts, int M, float *out6, hipStream_t st);
int mh_launch_copy_words(const void *src, void *dst, size_t nwords, hipStream_t st);
size_t mh_select_scratch_bytes_impl(int n);
int mh_launch_select_rows(const uint8_t *flags, const uint8_t *veto, int invert, int n, const float *a, const float *b,
                          float *a_out, float *b_out, int32_t *idx_out, const int32_t *base, int32_t *count, void *scratch,
                          hipStream_t st);
int mh_launch_segment_heads(const unsigned long long *keys, int n, int32_t *seg_start, unsigned long long *head_keys,
                            int32_t *meta, void *scratch, hipStream_t st);
int mh_launch_flag_less(const float *x, float thr, int n, uint8_t *out, hipStream_t st);
int mh_preload_sortgroup();

// ---- raster.hip
int mh_launch_render_depth(const float *cam, const float *verts, int Nv, const int32_t *faces, int Nf, int H, int W,
                           int off, int snap, MhRVert *vt, unsigned long long *zbuf, int32_t *queue, unsigned int *qcount,
                           float *out, int channels, hipStream_t st);
int mh_launch_render_strands(const float *cam, const float *verts, int Nv, const int32_t *faces, int Nf, const float *lpts,
                             const float *ltan, int Ns, int H, int W, int off, int snap, int width, int rule,
                             int color_option, int depth_option, float clear, MhRVert *vt, MhRLVert *lv,
                             unsigned long long *zbuf, int32_t *queue, unsigned int *qcount, float *out, hipStream_t st);
int mh_preload_raster();

// ---- hairgrow.hip
int mh_launch_pack_volume(const float *occ, const float *ori, size_t nvox, float4 *vox, hipStream_t st);
int mh_launch_trace_seeds(const float4 *vox, int W, int H, int Z, const float *seeds, int n, float thr, float *out,
                          int32_t *first, int32_t *len, hipStream_t st);
int mh_launch_trace_scalp(const float4 *vox, int W, int H, int Z, const float *seeds, const float *normals, int n,
                          float thr, float *out, int32_t *len, hipStream_t st);
int mh_launch_strands_compact(const float *rows, const int32_t *first, const int32_t *len, const int64_t *offs, int n,
                              int stride, float *packed, hipStream_t st);
int mh_preload_hairgrow();

// ---- hairconnect.hip (its code object loads with its first launch: no preload)
int mh_launch_end_knn64(const double *q, const int32_t *qcell, int nq, const double *data, const int32_t *order,
                        const int32_t *cstart, int gx, int gy, int gz, double bound2, int skip_self, int32_t *out_idx,
                        double *out_dist, int32_t *out_cnt, hipStream_t st);
int mh_launch_connect_cand(const double *P, const int64_t *offs, int N, const int32_t *const *idx,
                           const double *const *dist, const int32_t *const *cnt, double thr, int32_t *out_nb,
                           int32_t *out_ty, hipStream_t st);
int mh_launch_chain_count(const int64_t *offs, int N, const int32_t *nb, const int32_t *ty, int64_t *total,
                          int64_t *rootlen, hipStream_t st);
int mh_launch_chain_emit(const double *P, const int64_t *offs, int N, const int32_t *nb, const int32_t *ty,
                         const int64_t *rootlen, const int64_t *ooffs, double *out, hipStream_t st);
int mh_launch_occ_check(const double *S, const int64_t *offs, int N, const float *occ, int64_t ostride, int W, int H, int Z,
                        double vx, double vy, double vz, double vs, int32_t *status, hipStream_t st);
int mh_launch_smooth(double *S, const int64_t *offs, int N, double lap, double pos, double *work, hipStream_t st);

// ---- hairscalp.hip (loads with its first launch, like hairconnect.hip)
int mh_launch_scalp_ball_count(const float *P, const int64_t *offs, const int32_t *act, int nact, const float *core,
                               const int32_t *order, const int32_t *cstart, const float *grid, const int32_t *dims,
                               double thr_dist, int64_t *count, hipStream_t st);
int mh_launch_scalp_choose(const float *P, const int64_t *offs, const int32_t *act, int nact, const float *core,
                           const int32_t *csid, const int32_t *crank, const int32_t *order, const int32_t *cstart,
                           const float *grid, const int32_t *dims, double thr_dist, double thr_dot, const double *out_ratio,
                           const int64_t *boff, unsigned long long *bscr, uint8_t *flip, int32_t *best_sid,
                           int32_t *best_idx, hipStream_t st);
int mh_launch_scalp_emit(const float *P, const int64_t *offs, int n, const uint8_t *flip, const int32_t *best_sid,
                         const int32_t *best_idx, const int64_t *noffs, const float4 *vox, int W, int H, int Z,
                         double ratio_thr, float *Pn, uint8_t *flags, double *out_ratio, float *similar, int32_t *counters,
                         hipStream_t st);

// ---- meshsample.hip (loads with its first launch)
int mh_launch_tri_area64(const double *verts, const int32_t *faces, int nf, double *area, hipStream_t st);
int mh_launch_mesh_sample(const double *verts, const double *normals, const int32_t *faces, int nf, const int64_t *bounds,
                          const double *uniforms, int n, const double *bust /* host [3] */,
                          const double *vmin /* host [3] */, double vs, float *out_pts, float *out_nrm, int32_t *out_tri,
                          hipStream_t st);

// ---- hairdiffuse.hip (loads with its first launch)
int mh_launch_diffuse_walk(const float *occ, const float *ori, int W, int H, int Z, const float *pts, const float *nrm,
                           int n, int32_t *status, int32_t *steps, float *end_pt, float *first_n, float *last_n,
                           hipStream_t st);
int mh_launch_diffuse_arc(const float *pts, const float *end_pt, const float *first_n, const float *last_n,
                          const int32_t *steps, const int64_t *offs, int n, int rows, int W, int H, int Z, double *sample,
                          double *tangent, double *unit, int32_t *voxel, unsigned long long *keys, hipStream_t st);
int mh_launch_diffuse_splat(const int32_t *seg_start, const unsigned long long *head_keys, const int32_t *meta,
                            const int32_t *order, const double *unit, int rows, int W, int H, int Z, float *occ, float *ori,
                            hipStream_t st);

// ---- hairmetrics.hip (loads with its first launch)
int mh_launch_strand_arclen(const float *pts, const int64_t *offs, int S, double step, double *L, int64_t *m,
                            hipStream_t st);
int mh_launch_strand_resample(const float *pts, const int64_t *offs, const double *L, const int64_t *soffs, int S,
                              int total, double step, float *out, hipStream_t st);
int mh_launch_strand_tangents(const float *pts, const int64_t *offs, int S, int n, double *tan, uint8_t *valid,
                              hipStream_t st);
int mh_launch_strand_match(const float *q_pts, const double *q_tan, const uint8_t *q_valid, const int32_t *q_order, int nq,
                           const float *t_pts, const double *t_tan, const int32_t *cstart, float ox, float oy, float oz,
                           float h, int dx, int dy, int dz, MhMatchPairs pr, uint8_t *out, hipStream_t st);
int mh_launch_flag_counts(const uint8_t *flags, const uint8_t *valid, int n, unsigned long long *out9, hipStream_t st);

// ---- haircapture.hip (loads with its first launch)
int mh_launch_capture_project(MhCapCam cam, const float *pts, int n, int H, int W, float *vert, uint8_t *valid,
                              hipStream_t st);
int mh_launch_capture_zmin(const float *vert, const uint8_t *valid, const int64_t *offs, int S, int n_points, int H, int W,
                           int radius, const float *depth0, float *zmin, int32_t *dropped, hipStream_t st);
int mh_launch_capture_accum(const float *vert, const uint8_t *valid, const int64_t *offs, int S, int n_points, int H, int W,
                            int radius, float tol, const float *depth0, const float *zmin, int32_t *cnt, long long *C2,
                            long long *S2, hipStream_t st);
int mh_launch_capture_resolve(const float *zmin, const int32_t *cnt, const long long *C2, const long long *S2,
                              const float *depth0, MhCapTable tab, int n_full, int H, int W, float *depth, uint8_t *ori,
                              uint8_t *conf, uint8_t *mask, hipStream_t st);
int mh_launch_photo_shade(const float *pts, const uint8_t *valid, const int64_t *offs, int S, int n_points,
                          const float *albedo, double lx, double ly, double lz, double ambient, uint8_t *shade,
                          hipStream_t st);
int mh_launch_photo_front(const float *vert, const uint8_t *valid, const int64_t *offs, int S, int n_points,
                          const uint8_t *shade, int H, int W, int ss, int width, const float *depth0,
                          unsigned long long *keys, int32_t *dropped, hipStream_t st);
int mh_launch_photo_resolve(const unsigned long long *keys, const float *depth0, int H, int W, int ss, int bust_code,
                            int background_code, uint8_t *gray, int32_t *cover, hipStream_t st);

// ---- hairreproj.hip (loads with its first launch)
int mh_launch_support_accum(const float *vert, const uint8_t *valid, const int64_t *offs, int S, int n_points, int H, int W,
                            float tol, const float *depth0, const float *zmin, const uint8_t *ori, const uint8_t *conf,
                            const uint8_t *mask, int conf_min, MhCapTable tab, MhSupBounds bd,
                            unsigned long long *strand_counts, unsigned long long *view_counts, hipStream_t st);
int mh_launch_support_silhouette(const float *zmin, const uint8_t *mask, int H, int W, unsigned long long *out3,
                                 hipStream_t st);

// ---- hairvolume.hip (loads with its first launch)
int mh_launch_strand_volume_accum(const float *pts, const int64_t *offs, int S, int n_points, MhVolGrid gr, int sub,
                                  unsigned long long *acc, uint8_t *occ, unsigned long long *counters, hipStream_t st);
int mh_launch_strand_volume_resolve(const long long *acc, const int32_t *index, int G, int Y, int Z, long long *voxels,
                                    float *ori, int32_t *cnt, double *coh, long long *sums, int32_t *refused, hipStream_t st);
int mh_launch_volume_index(const long long *voxels, int G, int X, int Y, int Z, int32_t *index, int32_t *status,
                           hipStream_t st);
int mh_launch_volume_match(const long long *q_vox, const float *q_ori, int nq, const int32_t *t_index, const float *t_ori,
                           int X, int Y, int Z, MhVolPairs pr, uint8_t *out, hipStream_t st);
// hairfill.hip
int mh_launch_inner_votes(MhViews vw, const float *bust, MhVolGrid gr, int32_t *counts, hipStream_t st);
int mh_launch_inner_domain(const int32_t *counts, const int32_t *ext_index, size_t nvox, int max_bad, uint8_t *flags,
                           hipStream_t st);
int mh_launch_inner_diffuse(const long long *ext_voxels, const float *ext_ori, int n_ext, const long long *dom_voxels, int n_dom,
                            int X, int Y, int Z, int sweeps, int32_t *map, double *ext_tensor, uint8_t *ext_source,
                            int32_t *cell, double *t_a, double *t_b, uint8_t *known_a, uint8_t *known_b, int32_t *depth,
                            int32_t *status, hipStream_t st);
int mh_launch_inner_resolve(const long long *dom_voxels, int n_dom, const double *tensor, const uint8_t *known, MhVolGrid gr,
                            double min_coh, float *world, float *ori, double *coh, uint8_t *emit, hipStream_t st);
// haircarve.hip
int mh_launch_carve_votes(MhViews vw, const float *bust, MhVolGrid gr, int32_t *counts, hipStream_t st);
int mh_launch_carve_inside(MhViews vw, const float *bust, MhVolGrid gr, int min_free, int max_miss, int early_exit,
                           uint8_t *flags, hipStream_t st);
size_t mh_carve_mesh_scratch_bytes_impl(int X, int Y, int Z);
int mh_launch_carve_mesh_count(const uint8_t *flags, int X, int Y, int Z, void *scratch, long long *counts, hipStream_t st);
int mh_launch_carve_mesh(const uint8_t *flags, MhVolGrid gr, void *scratch, long long n_vertices, long long n_triangles,
                         float *vertices, int32_t *faces, hipStream_t st);
// hairstereo.hip
int mh_launch_stereo_census(const uint8_t *gray, int V, int H, int W, int cell, int radius, uint8_t *reduced,
                            unsigned long long *census, hipStream_t st);
int mh_launch_stereo_winners(MhViews vw, const float *bust, MhVolGrid gr, const int32_t *cand, int n_cand,
                             const unsigned long long *census, const int32_t *nb, int K, int cell, int radius, int keep,
                             unsigned long long *keys, hipStream_t st);
int mh_launch_stereo_agree(MhViews vw, const float *bust, MhVolGrid gr, const uint8_t *flags, const unsigned long long *keys,
                           int cell, int max_cost, float m255, int32_t *agree, hipStream_t st);
int mh_launch_stereo_refine(MhViews vw, const float *bust, MhVolGrid gr, const uint8_t *flags, const unsigned long long *keys,
                            const int32_t *agree, int cell, int max_cost, float m255, int min_agree, int min_through,
                            uint8_t *refined, float *depth, hipStream_t st);
}
