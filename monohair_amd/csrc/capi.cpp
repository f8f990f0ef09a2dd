// capi.cpp -- the C ABI of libmhpmvo.so (include/mh_pmvo.h): argument checking, the context that owns the packed maps, and
// the launch sequences of the PMVO entry points.  All arithmetic lives in the .hip kernels.  The other stages' entry points
// are in capi_points.cpp, capi_hair.cpp, capi_capture.cpp, capi_image.cpp and capi_comm.cpp; what needs no GPU is in capi_host.cpp.
#include <cstdlib>
#include <cstring>
#include <new>

#include "mh_capi.h"

int launched(int rc, const char *what) {
    if (rc == -1) return fail(MH_ERR_ARG, "%s: unsupported size/shape", what);
    if (rc != 0) return fail(MH_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)rc));
    return MH_OK;
}

extern "C" int mh_ctx_create(int device_id, mh_ctx **out) {
    if (!out) return fail(MH_ERR_ARG, "mh_ctx_create: out is NULL");
    int ndev = 0;
    MH_HIP(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(MH_ERR_ARG, "mh_ctx_create: no device %d", device_id);
    mh_ctx *c = new (std::nothrow) mh_ctx();
    if (!c) return fail(MH_ERR_NOMEM, "mh_ctx_create: out of host memory");
    c->device = device_id;
    if (const char *e = getenv("MH_TAP_PLANE_MAX_MB")) c->tap_plane_max_mb = atoll(e);
    // the code objects of the library go onto the device now (HIP would load each translation unit's on the first launch
    // of one of its kernels -- in the middle of the first pass's stages); a failure here only means they load lazily
    if (hipSetDevice(device_id) == hipSuccess) {
        int (*const preload[])() = {mh_preload_pmvo_project, mh_preload_pmvo_search, mh_preload_pmvo_refine,
                                    mh_preload_pmvo_filter,  mh_preload_consensus,   mh_preload_gabor,
                                    mh_preload_hairgrow,     mh_preload_knn,         mh_preload_raster,
                                    mh_preload_sortgroup,    mh_preload_pmvo_pieces, mh_preload_dog};
        for (auto f : preload) (void)f();
        (void)hipGetLastError();
    }
    *out = c;
    return MH_OK;
}

static void free_views(mh_ctx *c) {
    if (c->rec) (void)hipFree(c->rec);
    if (c->mask) (void)hipFree(c->mask);
    if (c->cams) (void)hipFree(c->cams);
    if (c->oc) (void)hipFree(c->oc);
    c->oc = nullptr;
    if (c->tapp) (void)hipFree(c->tapp);
    c->tapp = nullptr;
    c->tapp_failed = false;
    c->tap_view.clear();
    c->code_view.clear();
    c->lut_set = c->lut_mixed = false;
    c->rec = nullptr;
    c->mask = nullptr;
    c->cams = nullptr;
    c->V = c->H = c->W = 0;
}

extern "C" void mh_ctx_destroy(mh_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    free_views(ctx);
    if (ctx->offs) (void)hipFree(ctx->offs);
    if (ctx->gabor) (void)hipFree(ctx->gabor);
    if (ctx->gabor_max) (void)hipFree(ctx->gabor_max);
    if (ctx->gabor_q) (void)hipFree(ctx->gabor_q);
    if (ctx->dog_w) (void)hipFree(ctx->dog_w);
    delete ctx->dog_w_host;
    if (ctx->lut) (void)hipFree(ctx->lut);
    if (ctx->code_tabs) (void)hipFree(ctx->code_tabs);
    delete ctx;
}

extern "C" int mh_ctx_alloc_views(mh_ctx *ctx, int V, int H, int W) {
    if (!ctx || V < 1 || H < 1 || W < 1) return fail(MH_ERR_ARG, "mh_ctx_alloc_views: bad arguments");
    MH_HIP(hipSetDevice(ctx->device));
    free_views(ctx);
    const size_t npix = (size_t)V * H * W;
    if (hipMalloc(&ctx->rec, npix * sizeof(float4)) != hipSuccess ||
        hipMalloc(&ctx->mask, npix * sizeof(float)) != hipSuccess ||
        hipMalloc(&ctx->cams, (size_t)V * MH_CAM_STRIDE * sizeof(float)) != hipSuccess) {
        free_views(ctx);
        return fail(MH_ERR_NOMEM, "mh_ctx_alloc_views: hipMalloc of %zu bytes failed", npix * 20);
    }
    ctx->V = V;
    ctx->H = H;
    ctx->W = W;
    ctx->code_view.assign(V, 0);
    ctx->tap_view.assign(V, 0);
    return MH_OK;
}

extern "C" int mh_ctx_set_view(mh_ctx *ctx, int view, const float *cam_host, const float *depth, int depth_stride,
                               const float *ori, const float *conf, const float *mask, int mask_stride,
                               void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_ctx_set_view: views not allocated");
    if (view < 0 || view >= ctx->V || !cam_host || !depth || !ori || !conf || !mask || depth_stride < 1 ||
        mask_stride < 1)
        return fail(MH_ERR_ARG, "mh_ctx_set_view: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)ctx->H * ctx->W;
    // pageable host -> device copy of 192 bytes: synchronous w.r.t. the host buffer, ordered on `st`
    MH_HIP(hipMemcpyAsync(ctx->cams + (size_t)view * MH_CAM_STRIDE, cam_host, MH_CAM_STRIDE * sizeof(float),
                          hipMemcpyHostToDevice, st));
    if ((int)ctx->code_view.size() == ctx->V) ctx->code_view[view] = 0;      // this view has no resident codes (any more)
    // the plane of ready-made taps (MhViews::tap): optional, like the code plane of the 8-bit views
    if (!ctx->tapp && !ctx->tapp_failed && ctx->use_tap_plane) {
        MH_HIP(hipSetDevice(ctx->device));
        const size_t bytes = (size_t)ctx->V * npix * sizeof(float4);
        size_t free_b = 0, total_b = 0;
        const bool fits = bytes <= (size_t)(ctx->tap_plane_max_mb > 0 ? ctx->tap_plane_max_mb : 0) * 1048576ull &&
                          hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes <= free_b - free_b / 4;
        if (!fits || hipMalloc(&ctx->tapp, bytes) != hipSuccess) {
            ctx->tapp = nullptr;
            ctx->tapp_failed = true;     // not retried per view: the front end normalises per iteration instead
            (void)hipGetLastError();
        }
    }
    const int rc = launched(mh_launch_pack_view(ctx->rec + (size_t)view * npix, ctx->mask + (size_t)view * npix, depth,
                                                depth_stride, ori, conf, mask, mask_stride, npix,
                                                ctx->tapp ? ctx->tapp + (size_t)view * npix : nullptr, st),
                            "mh_ctx_set_view");
    // (the view's slice of the plane counts as current only once its pack launch has been accepted)
    if (ctx->tapp && (int)ctx->tap_view.size() == ctx->V) ctx->tap_view[view] = rc == MH_OK ? 1 : 0;
    return rc;
}

extern "C" int mh_ctx_set_view_u8(mh_ctx *ctx, int view, const float *cam_host, const float *depth, int depth_stride,
                                  const unsigned char *ori_u8, const unsigned char *conf_u8,
                                  const unsigned char *mask_u8, const float *lut_host, void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_ctx_set_view_u8: views not allocated");
    if (view < 0 || view >= ctx->V || !cam_host || !depth || !ori_u8 || !conf_u8 || !mask_u8 || !lut_host ||
        depth_stride < 1)
        return fail(MH_ERR_ARG, "mh_ctx_set_view_u8: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)ctx->H * ctx->W;
    MH_HIP(hipSetDevice(ctx->device));
    if (!ctx->lut) MH_HIP(hipMalloc(&ctx->lut, 256 * sizeof(float4)));
    if (!ctx->code_tabs) MH_HIP(hipMalloc(&ctx->code_tabs, mh_code_tabs_bytes()));
    if (!ctx->oc && !ctx->oc_failed) {   // (2 B per pixel next to the 20 B of records; without it the tap gathers use the records)
        if (hipMalloc(&ctx->oc, (size_t)ctx->V * npix * sizeof(uint16_t)) != hipSuccess) {
            ctx->oc = nullptr;
            ctx->oc_failed = true;       // not retried per view
            (void)hipGetLastError();     // the fallback is intended: do not leave the error for the next launch check
        }
    }
    // one table per context: views decoded through DIFFERENT tables cannot share the code tables of the tap gather
    if (ctx->lut_set && memcmp(ctx->lut_host, lut_host, sizeof ctx->lut_host) != 0) ctx->lut_mixed = true;
    if (!ctx->lut_set || ctx->lut_mixed) {
        if (ctx->lut_set) MH_HIP(hipDeviceSynchronize());     // (a pack kernel of another stream may still read the old table)
        memcpy(ctx->lut_host, lut_host, sizeof ctx->lut_host);
        ctx->lut_set = true;
        MH_HIP(hipMemcpyAsync(ctx->lut, ctx->lut_host, 256 * sizeof(float4), hipMemcpyHostToDevice, st));
        if (int rc = launched(mh_launch_code_tabs(ctx->lut, ctx->code_tabs, st), "mh_ctx_set_view_u8(tables)")) return rc;
    }
    MH_HIP(hipMemcpyAsync(ctx->cams + (size_t)view * MH_CAM_STRIDE, cam_host, MH_CAM_STRIDE * sizeof(float),
                          hipMemcpyHostToDevice, st));
    if ((int)ctx->code_view.size() == ctx->V) ctx->code_view[view] = ctx->oc ? 1 : 0;
    const int rc = launched(mh_launch_pack_view_u8(ctx->rec + (size_t)view * npix, ctx->mask + (size_t)view * npix, depth,
                                                   depth_stride, ori_u8, conf_u8, mask_u8, ctx->lut, npix,
                                                   ctx->oc ? ctx->oc + (size_t)view * npix : nullptr,
                                                   ctx->tapp ? ctx->tapp + (size_t)view * npix : nullptr, st),
                            "mh_ctx_set_view_u8");
    // (only when an fp32 view allocated the plane; current only once the pack launch has been accepted)
    if (ctx->tapp && (int)ctx->tap_view.size() == ctx->V) ctx->tap_view[view] = rc == MH_OK ? 1 : 0;
    return rc;
}

extern "C" int mh_ctx_set_depth_offsets(mh_ctx *ctx, const float *offsets_host, int S) {
    if (!ctx || !offsets_host || S < 1) return fail(MH_ERR_ARG, "mh_ctx_set_depth_offsets: bad arguments");
    if (S > 256) return fail(MH_ERR_ARG, "mh_ctx_set_depth_offsets: S = %d exceeds the limit of 256 samples", S);
    MH_HIP(hipSetDevice(ctx->device));
    if (ctx->offs) (void)hipFree(ctx->offs);
    ctx->offs = nullptr;
    MH_HIP(hipMalloc(&ctx->offs, S * sizeof(float)));
    MH_HIP(hipMemcpy(ctx->offs, offsets_host, S * sizeof(float), hipMemcpyHostToDevice));
    ctx->S = S;
    return MH_OK;
}

extern "C" int mh_upload_async(mh_ctx *ctx, const void *host, void *device, size_t bytes, void *stream) {
    if (!ctx || (bytes && (!host || !device))) return fail(MH_ERR_ARG, "mh_upload_async: bad arguments");
    if (!bytes) return MH_OK;
    MH_HIP(hipMemcpyAsync(device, host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return MH_OK;
}

// the same copy for a PAGE-LOCKED source: up to 1 MiB as a kernel that reads the host buffer over the link (see the header)
extern "C" int mh_upload_pinned(mh_ctx *ctx, const void *pinned_host, void *device, size_t bytes, void *stream) {
    if (!ctx || (bytes && (!pinned_host || !device))) return fail(MH_ERR_ARG, "mh_upload_pinned: bad arguments");
    if (!bytes) return MH_OK;
    static const bool by_copy_engine = getenv("MH_UPLOAD_KERNEL") && atoi(getenv("MH_UPLOAD_KERNEL")) == 0;
    if (!by_copy_engine && !(bytes & 3) && !((uintptr_t)pinned_host & 3) && !((uintptr_t)device & 3) && bytes <= (1u << 20)) {
        MH_HIP(hipSetDevice(ctx->device));
        return launched(mh_launch_copy_words(pinned_host, device, bytes / 4, (hipStream_t)stream), "mh_upload_pinned");
    }
    MH_HIP(hipMemcpyAsync(device, pinned_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return MH_OK;
}

// The lab switches (include/mh_pmvo_lab.h): A/B forms and cross-check kernels; same results, not part of the supported surface
// flag: stored as 0 / 1; must: the key takes 0..hi only, and this is what the error text says
static const struct { const char *key; int mh_ctx::*field; bool flag; int hi; const char *must; } lab_options[] = {
    {"search_variant", &mh_ctx::search_variant, false, 0, nullptr},
    {"search_body", &mh_ctx::search_body, false, 2, "must be 0 (by the maps), 1 (keys) or 2 (select)"},
    {"tap_plane", &mh_ctx::use_tap_plane, true, 0, nullptr},
    {"tap_codes", &mh_ctx::use_codes, true, 0, nullptr},
    {"taps_tile", &mh_ctx::taps_tile, false, 0, nullptr},
    {"filter_rows", &mh_ctx::filter_rows, true, 0, nullptr},
    {"carve_early_exit", &mh_ctx::carve_early_exit, true, 0, nullptr}};

extern "C" int mh_ctx_set_option(mh_ctx *ctx, const char *key, int value) {
    if (!ctx || !key) return fail(MH_ERR_ARG, "mh_ctx_set_option: bad arguments");
    // the values a key takes: lo, lo + step, ... up to hi
    static const struct { const char *key; int mh_ctx::*field; int lo, hi, step; const char *must; } ranged[] = {
        {"reproject_rule", &mh_ctx::reproject_rule, 0, 2, 1, "must be 0 (by group size), 1 (mid forms) or 2 (chain forms)"},
        {"reproject_fma_min_cols", &mh_ctx::reproject_fma_min_cols, 1, 0x7fffffff, 1, "must be >= 1"},
        {"sum_block", &mh_ctx::sum_block, 0, 32, 32, "must be 32 (ATen's outer sum) or 0"},
        {"gabor_variant", &mh_ctx::gabor_variant, 0, 3, 3, "must be 0 (valu) or 3 (mfma2)"},
        {"raster_subpixel_bits", &mh_ctx::raster_subpixel_bits, 4, 8, 1, "must be 4..8"}};
    for (const auto &o : ranged)
        if (!strcmp(key, o.key)) {
            if (value < o.lo || value > o.hi || (value - o.lo) % o.step)
                return fail(MH_ERR_ARG, "mh_ctx_set_option: %s %s", key, o.must);
            ctx->*o.field = value;
            return MH_OK;
        }
    if (!strcmp(key, "topk_order")) {
        if ((value & 255) > 1) return fail(MH_ERR_ARG, "mh_ctx_set_option: topk_order must be 0 (torch.topk's order) or 1");
        ctx->topk_order = value;
        return MH_OK;
    }
    if (!strcmp(key, "tap_plane_max_mb")) {      // takes effect for planes not yet allocated (before the first fp32 view)
        if (value < 0) return fail(MH_ERR_ARG, "mh_ctx_set_option: tap_plane_max_mb must be >= 0");
        ctx->tap_plane_max_mb = value;
        return MH_OK;
    }
    if (!strcmp(key, "line_rule")) {
        ctx->line_rule = value ? 1 : 0;
        return MH_OK;
    }
    for (const auto &o : lab_options)
        if (!strcmp(key, o.key))
            return fail(MH_ERR_ARG, "mh_ctx_set_option: %s is a lab switch, not a supported option: mh_ctx_set_lab_option "
                                    "(include/mh_pmvo_lab.h)", key);
    return fail(MH_ERR_ARG, "mh_ctx_set_option: unknown key %s", key);
}

extern "C" int mh_ctx_set_lab_option(mh_ctx *ctx, const char *key, int value) {
    if (!ctx || !key) return fail(MH_ERR_ARG, "mh_ctx_set_lab_option: bad arguments");
    for (const auto &o : lab_options)
        if (!strcmp(key, o.key)) {
            if (o.must && (value < 0 || value > o.hi)) return fail(MH_ERR_ARG, "mh_ctx_set_lab_option: %s %s", key, o.must);
            ctx->*o.field = o.flag ? (value ? 1 : 0) : value;
            return MH_OK;
        }
    return fail(MH_ERR_ARG, "mh_ctx_set_lab_option: unknown key %s", key);
}

extern "C" int mh_project_gather(mh_ctx *ctx, const float *points, int N, int patch, float *vis, float *ori,
                                 float *conf, float *mask, float *ori_patch, float *conf_patch, float *pixf,
                                 void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_project_gather: views not set");
    if (N == 0) return MH_OK;
    if (!points || N < 0 || patch < 1 || !(patch & 1)) return fail(MH_ERR_ARG, "mh_project_gather: bad arguments");
    return launched(mh_launch_project_gather(ctx->views(), points, N, patch, vis, ori, conf, mask, ori_patch,
                                             conf_patch, pixf, (hipStream_t)stream),
                    "mh_project_gather");
}

extern "C" int mh_topk_views(mh_ctx *ctx, const float *vis, const float *conf, int N, int32_t *out_idx,
                             float *out_val, void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_topk_views: views not set");
    if (N == 0) return MH_OK;
    if (!vis || !conf || !out_idx || !out_val || N < 0) return fail(MH_ERR_ARG, "mh_topk_views: bad arguments");
    if (ctx->V < MH_TOPK)
        return fail(MH_ERR_ARG, "mh_topk_views: %d views < %d (the reference's torch.topk raises too, PMVO.py:341)",
                    ctx->V, MH_TOPK);
    return launched(mh_launch_topk(vis, conf, ctx->V, N, out_idx, out_val, ctx->topk_order, (hipStream_t)stream),
                    "mh_topk_views");
}

// The search scratch of N points with a patch x patch window, in four regions:
//   taps    V*N lists of patch*patch + 1 tap records, + 16 records of slack: the search kernel prefetches tap records in
//           groups past the end of a list
//   order   2N ints: the launch order of the search (mh_search_order_kernel) and its staging area
//   counts  V*N bytes: the list lengths once more, compact, for the work estimate
//   groups  (256-byte aligned) the points per (rank, base view) of the batch: MH_GROUP_COPIES partial copies x
//           MH_GROUP_RANKS ranks x V ints -- csrc/mh_device.h: MhRule
struct SearchScratch {
    float4 *taps;
    int32_t *order, *groups;
    uint8_t *counts;
    size_t counts_offset, bytes;
    SearchScratch(int V, int N, int patch, void *base) {
        const size_t order_offset = ((size_t)V * (size_t)N * (size_t)(patch * patch + 1) + 16) * sizeof(float4);
        counts_offset = order_offset + 2 * (size_t)N * sizeof(int32_t);
        const size_t groups_offset = (counts_offset + (size_t)V * (size_t)N + 255) & ~(size_t)255;
        bytes = groups_offset + (size_t)MH_GROUP_COPIES * MH_GROUP_RANKS * V * sizeof(int32_t);
        const uintptr_t b = (uintptr_t)base;      // (an integer: the size queries pass no buffer)
        taps = (float4 *)b;
        order = (int32_t *)(b + order_offset);
        counts = (uint8_t *)(b + counts_offset);
        groups = (int32_t *)(b + groups_offset);
    }
};

extern "C" size_t mh_search_counts_offset(mh_ctx *ctx, int N, int patch) {
    if (!ctx || N < 0 || patch < 1) return 0;
    return SearchScratch(ctx->V, N, patch, nullptr).counts_offset;
}

extern "C" size_t mh_search_scratch_bytes(mh_ctx *ctx, int N, int patch) {
    if (!ctx || N < 0 || patch < 1) return 0;
    return SearchScratch(ctx->V, N, patch, nullptr).bytes;
}

// The ranks a search call takes -- ranks 0, rank_step, ... of the MH_TOPK ranked views -- and what one workgroup of the search
// holds (csrc/mh_launch.h): at most MH_MAX_RANKS ranks and MH_MAX_ITEMS = nrank * S items.  Checked by every entry point in
// front of its first launch (mh_launch_search would answer a bare -1 behind the front end).
static int search_limits(const mh_ctx *ctx, const char *what, int nrank, int rank_step) {
    if (nrank < 1 || rank_step < 1 || ((long long)nrank - 1) * rank_step >= MH_TOPK)
        return fail(MH_ERR_ARG, "%s: bad arguments: nrank = %d, rank_step = %d (nrank >= 1, rank_step >= 1 and "
                                "(nrank - 1) * rank_step < %d, the ranked views: MH_TOPK)", what, nrank, rank_step, MH_TOPK);
    if (nrank > MH_MAX_RANKS)
        return fail(MH_ERR_ARG, "%s: nrank = %d exceeds the limit of %d base-view ranks (MH_MAX_RANKS)", what, nrank,
                    MH_MAX_RANKS);
    if ((long long)nrank * ctx->S > MH_MAX_ITEMS)
        return fail(MH_ERR_ARG, "%s: nrank * S = %d * %d items exceed the limit of %d items per point (MH_MAX_ITEMS)", what,
                    nrank, ctx->S, MH_MAX_ITEMS);
    return MH_OK;
}

// What mh_search_forward puts in front of the search: the tap lists from gathered patches (mh_forward_prepare writes them
// from the maps instead)
struct SearchPrep {
    const float *vis, *pixf, *ori_patch, *conf_patch;
    size_t scratch_bytes;
};

// The one search launch behind mh_search_forward, mh_search_prepared and the fused tail of mh_forward.  `what`: the entry
// point named in the error texts; classes_ready / groups_ready: the ranking kernel of the fused forward has written the
// work classes / the group sizes.  mh_search_forward's prep launch (`prep`, its only user, hence the fixed text) sits in
// here, between the argument checks and the search_variant check, because that is where the error precedence has it.
static int search(mh_ctx *ctx, const char *what, const SearchPrep *prep, const float *points, int N, int patch,
                  float conf_threshold, int nrank, int rank_step, const float *ori, const int32_t *base_idx,
                  const float *base_val, void *scratch, float *line_ori, float *min_loss, uint8_t *high_conf,
                  float *best_sample, int32_t *best_rank, int32_t *best_s, bool classes_ready, int groups_ready,
                  void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "%s: views not set", what);
    if (!ctx->offs) return fail(MH_ERR_STATE, "%s: depth offsets not set", what);
    if (N == 0) return MH_OK;
    if (!points || !ori || !base_idx || !base_val || !scratch || !line_ori || !min_loss || !high_conf || N < 0 ||
        (prep && (!prep->vis || !prep->pixf || !prep->ori_patch || !prep->conf_patch)))
        return fail(MH_ERR_ARG, "%s: bad arguments", what);
    if (int rc = search_limits(ctx, what, nrank, rank_step)) return rc;
    if (prep && prep->scratch_bytes < mh_search_scratch_bytes(ctx, N, patch))
        return fail(MH_ERR_ARG, "%s: scratch too small (%zu < %zu)", what, prep->scratch_bytes,
                    mh_search_scratch_bytes(ctx, N, patch));
    if (ctx->V >= 4096) return fail(MH_ERR_ARG, "%s: V >= 4096 needs a fourth cascade level", what);
    const SearchScratch s(ctx->V, N, patch, scratch);
    const int P = patch * patch;
    if (prep)
        if (int rc = launched(mh_launch_prep_taps(prep->ori_patch, prep->conf_patch, prep->vis, prep->pixf, ctx->V * N, P,
                                                  conf_threshold, s.taps, s.counts, (hipStream_t)stream),
                              "mh_search_forward(prep)"))
            return rc;
    MhSearchPlan plan;
    if (!ctx->search_plan(&plan)) return fail(MH_ERR_ARG, "%s: unknown search_variant %d", what, ctx->search_variant);
    if (classes_ready) plan.order = MhSearchPlan::ORDER_CLASSES_READY;   // (the fused forward, which runs the default plan only)
    return launched(mh_launch_search(ctx->views(), ctx->offs, ctx->S, nrank, rank_step, points, N, P + 1, conf_threshold, ori,
                                     base_idx, base_val, s.taps, s.order, s.counts, line_ori, min_loss, high_conf,
                                     best_sample, best_rank, best_s, plan, ctx->reproject_rule, ctx->reproject_fma_min_cols,
                                     ctx->sum_block, s.groups, groups_ready, (hipStream_t)stream),
                    what);
}

extern "C" int mh_search_forward(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold, int nrank,
                                 int rank_step, const float *vis, const float *ori, const float *pixf,
                                 const float *ori_patch, const float *conf_patch, const int32_t *base_idx,
                                 const float *base_val, void *scratch, size_t scratch_bytes, float *line_ori,
                                 float *min_loss, uint8_t *high_conf, float *best_sample, int32_t *best_rank,
                                 int32_t *best_s, void *stream) {
    const SearchPrep prep = {vis, pixf, ori_patch, conf_patch, scratch_bytes};
    return search(ctx, "mh_search_forward", &prep, points, N, patch, conf_threshold, nrank, rank_step, ori, base_idx, base_val,
                  scratch, line_ori, min_loss, high_conf, best_sample, best_rank, best_s, false, 0, stream);
}

static int forward_prepare(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold, float *vis, float *ori,
                           float *conf, float *mask, void *scratch, size_t scratch_bytes, int zero_groups, void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_forward_prepare: views not set");
    if (N == 0) return MH_OK;
    if (!points || !vis || !ori || !conf || !scratch || N < 0 || patch < 1 || !(patch & 1))
        return fail(MH_ERR_ARG, "mh_forward_prepare: bad arguments");
    const SearchScratch s(ctx->V, N, patch, scratch);
    if (scratch_bytes < s.bytes) return fail(MH_ERR_ARG, "mh_forward_prepare: scratch too small");
    return launched(mh_launch_project_taps(ctx->views(), points, N, patch, conf_threshold, vis, ori, conf, mask, s.taps,
                                           s.counts, ctx->taps_tile, ctx->codes_ready() ? ctx->oc : nullptr, ctx->code_tabs,
                                           s.groups, zero_groups ? MH_GROUP_COPIES * MH_GROUP_RANKS * ctx->V : 0,
                                           (hipStream_t)stream),
                    "mh_forward_prepare");
}

extern "C" int mh_forward_prepare(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold,
                                  float *vis, float *ori, float *conf, float *mask, void *scratch,
                                  size_t scratch_bytes, void *stream) {
    return forward_prepare(ctx, points, N, patch, conf_threshold, vis, ori, conf, mask, scratch, scratch_bytes, 0, stream);
}

extern "C" int mh_search_prepared(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold, int nrank,
                                  int rank_step, const float *ori, const int32_t *base_idx, const float *base_val,
                                  void *scratch, float *line_ori, float *min_loss, uint8_t *high_conf,
                                  float *best_sample, int32_t *best_rank, int32_t *best_s, void *stream) {
    return search(ctx, "mh_search_prepared", nullptr, points, N, patch, conf_threshold, nrank, rank_step, ori, base_idx,
                  base_val, scratch, line_ori, min_loss, high_conf, best_sample, best_rank, best_s, false, 0, stream);
}

extern "C" int mh_forward(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold, int nrank, int rank_step,
                          float *vis, float *ori, float *conf, float *mask, void *scratch, size_t scratch_bytes,
                          int32_t *base_idx, float *base_val, float *line_ori, float *min_loss, uint8_t *high_conf,
                          float *best_sample, int32_t *best_rank, int32_t *best_s, void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_forward: views not set");
    // the rank arguments, in front of the front end's launch (the search checks them again, behind it)
    if (N > 0 && ctx->offs)
        if (int rc = search_limits(ctx, "mh_forward", nrank, rank_step)) return rc;
    // with the default kernels the ranking kernel also writes the work classes of the search's launch order (it has the
    // point's ranking in its lanes): one launch less per iteration than the three separate calls
    const bool fuse_cls = ctx->search_variant == 0 && (ctx->topk_order & 255) == 0 && N > 1 && base_idx && base_val && vis &&
                          conf && nrank >= 1 && rank_step >= 1 && ctx->V >= MH_TOPK && ctx->offs;
    // ... and counts the points per (rank, base view) of the batch (csrc/mh_device.h: MhRule) into the array the front end cleared
    const int fuse_groups = fuse_cls && ctx->reproject_rule == 0 && nrank <= 16;
    if (int rc = forward_prepare(ctx, points, N, patch, conf_threshold, vis, ori, conf, mask, scratch, scratch_bytes, fuse_groups,
                                 stream))
        return rc;
    if (!fuse_cls) {
        if (int rc = mh_topk_views(ctx, vis, conf, N, base_idx, base_val, stream)) return rc;
        return mh_search_prepared(ctx, points, N, patch, conf_threshold, nrank, rank_step, ori, base_idx, base_val, scratch,
                                  line_ori, min_loss, high_conf, best_sample, best_rank, best_s, stream);
    }
    const SearchScratch s(ctx->V, N, patch, scratch);
    // (the points that hold the trailing columns of the batch's [V, N*S] sums go first in the search's launch order)
    const long long cols = (long long)N * ctx->S;
    const int tail_n0 = ctx->sum_block > 0 ? (int)((cols - cols % ctx->sum_block) / ctx->S) : N;
    if (int rc = launched(mh_launch_topk_work(vis, conf, ctx->V, N, base_idx, base_val, ctx->topk_order, s.counts, s.order,
                                              patch * patch + 1, nrank, rank_step, ctx->S, fuse_groups ? s.groups : nullptr,
                                              tail_n0, (hipStream_t)stream),
                          "mh_forward (base-view ranking)"))
        return rc;
    return search(ctx, "mh_search_prepared", nullptr, points, N, patch, conf_threshold, nrank, rank_step, ori, base_idx, base_val,
                  scratch, line_ori, min_loss, high_conf, best_sample, best_rank, best_s, true /* work classes written */,
                  fuse_groups, stream);
}

extern "C" int mh_refine_loss(mh_ctx *ctx, const float *points, const float *dir, float step_mul, float step_div,
                              int N, int patch, float conf_threshold, const float *vis, const float *ori_patch,
                              const float *conf_patch, float *loss, uint8_t *high_conf, void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_refine_loss: views not set");
    if (N == 0) return MH_OK;
    if (!points || !dir || !vis || !ori_patch || !conf_patch || !loss || N < 0)
        return fail(MH_ERR_ARG, "mh_refine_loss: bad arguments");
    return launched(mh_launch_refine_loss(ctx->views(), points, dir, step_mul, step_div, N, patch * patch,
                                          conf_threshold, vis, ori_patch, conf_patch, loss, high_conf, ctx->sum_block,
                                          (hipStream_t)stream),
                    "mh_refine_loss");
}

static int filter_points_impl(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold,
                              float visible_threshold, uint8_t *surface_index, uint8_t *filter_index,
                              uint8_t *unvisible_index, uint8_t *head_filter, int batch, long long row0, long long total,
                              const int32_t *order, void *stream, const char *what) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "%s: views not set", what);
    if (N == 0) return MH_OK;
    if (!points || N < 0 || patch < 1 || !(patch & 1) || batch < 0 || row0 < 0 || (batch > 0 && total < row0 + N))
        return fail(MH_ERR_ARG, "%s: bad arguments", what);
    if (batch == 0) row0 = 0, total = N;
    return launched(mh_launch_filter_points(ctx->views(), points, N, patch, conf_threshold, visible_threshold,
                                            surface_index, filter_index, unvisible_index, head_filter, batch, row0, total,
                                            ctx->sum_block, ctx->filter_rows, order, (hipStream_t)stream),
                    what);
}

extern "C" int mh_filter_points(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold,
                                float visible_threshold, uint8_t *surface_index, uint8_t *filter_index,
                                uint8_t *unvisible_index, uint8_t *head_filter, int batch, long long row0,
                                long long total, void *stream) {
    return filter_points_impl(ctx, points, N, patch, conf_threshold, visible_threshold, surface_index, filter_index,
                              unvisible_index, head_filter, batch, row0, total, nullptr, stream, "mh_filter_points");
}

extern "C" int mh_filter_points_ordered(mh_ctx *ctx, const float *points, int N, int patch, float conf_threshold,
                                        float visible_threshold, uint8_t *surface_index, uint8_t *filter_index,
                                        uint8_t *unvisible_index, uint8_t *head_filter, int batch, long long row0,
                                        long long total, const int32_t *order, void *stream) {
    return filter_points_impl(ctx, points, N, patch, conf_threshold, visible_threshold, surface_index, filter_index,
                              unvisible_index, head_filter, batch, row0, total, order, stream, "mh_filter_points_ordered");
}

extern "C" int mh_medoid_dense(mh_ctx *ctx, const float *ori, int G, int K, float *out, int32_t *out_index,
                               void *stream) {
    if (!ctx || !ori || !out || G < 0 || K < 1) return fail(MH_ERR_ARG, "mh_medoid_dense: bad arguments");
    if (G == 0) return MH_OK;
    return launched(mh_launch_medoid_dense(ori, nullptr, G, K, out, out_index, (hipStream_t)stream), "mh_medoid_dense");
}

extern "C" int mh_medoid_indexed(mh_ctx *ctx, const float *ori_rows, const int32_t *index, int G, int K, float *out,
                                 int32_t *out_index, void *stream) {
    if (!ctx || !ori_rows || !index || !out || G < 0 || K < 1) return fail(MH_ERR_ARG, "mh_medoid_indexed: bad arguments");
    if (G == 0) return MH_OK;
    return launched(mh_launch_medoid_dense(ori_rows, index, G, K, out, out_index, (hipStream_t)stream),
                    "mh_medoid_indexed");
}

extern "C" int mh_refine_loss_maps(mh_ctx *ctx, const float *points, const float *dir, float step_mul, float step_div,
                                   int N, int patch, float conf_threshold, float *loss, uint8_t *high_conf,
                                   int batch, long long row0, long long total, void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_refine_loss_maps: views not set");
    if (N == 0) return MH_OK;
    if (!points || !dir || !loss || N < 0 || patch < 1 || !(patch & 1) || batch < 0 || row0 < 0 ||
        (batch > 0 && total < row0 + N))
        return fail(MH_ERR_ARG, "mh_refine_loss_maps: bad arguments");
    if (batch == 0) row0 = 0, total = N;
    if (patch > 11)
        return fail(MH_ERR_ARG, "mh_refine_loss_maps: patch side %d is not built in (odd sides 1..11 are; the reference's "
                                "configurations use 5, 7 and 9) -- use mh_project_gather + mh_refine_loss for larger patches",
                    patch);
    if (ctx->V > 512) return fail(MH_ERR_ARG, "mh_refine_loss_maps: %d views exceed the limit of 512", ctx->V);
    return launched(mh_launch_refine_loss_maps(ctx->views(), points, dir, step_mul, step_div, N, patch, conf_threshold,
                                               loss, high_conf, batch, row0, total, ctx->sum_block, (hipStream_t)stream),
                    "mh_refine_loss_maps");
}

extern "C" int mh_refine_combine(mh_ctx *ctx, const float *center, const float *loss_u, const uint8_t *head_filter,
                                 const uint8_t *head_top, float replace_threshold, float *ori, float *loss_out, int N,
                                 void *stream) {
    if (N == 0) return MH_OK;
    if (!ctx || !center || !loss_u || !head_filter || !head_top || !loss_out || N < 0)   // (ori may be NULL: loss only)
        return fail(MH_ERR_ARG, "mh_refine_combine: bad arguments");
    return launched(mh_launch_refine_combine(center, loss_u, head_filter, head_top, replace_threshold, ori, loss_out, N,
                                             (hipStream_t)stream),
                    "mh_refine_combine");
}

extern "C" int mh_medoid_segmented(mh_ctx *ctx, const float *ori, const int32_t *seg_start, int G, int max_group,
                                   float *out, int32_t *out_index, void *stream) {
    if (!ctx || !ori || !seg_start || !out || G < 0 || max_group < 1)
        return fail(MH_ERR_ARG, "mh_medoid_segmented: bad arguments");
    if (G == 0) return MH_OK;
    return launched(mh_launch_medoid_segmented(ori, seg_start, G, max_group, out, out_index, (hipStream_t)stream),
                    "mh_medoid_segmented");
}

extern "C" int mh_replace_dissimilar(mh_ctx *ctx, const float *center, float *ori, float threshold, int N,
                                     void *stream) {
    if (N == 0) return MH_OK;
    if (!ctx || !center || !ori || N < 0) return fail(MH_ERR_ARG, "mh_replace_dissimilar: bad arguments");
    return launched(mh_launch_replace_dissimilar(center, ori, threshold, N, (hipStream_t)stream),
                    "mh_replace_dissimilar");
}

// ---- the intermediate methods of the reference's class, as stand-alone calls (csrc/pmvo_pieces.hip) ---------------
extern "C" int mh_project_points(mh_ctx *ctx, int view, const float *points, int N, int32_t *row_col, float *z_half,
                                 uint8_t *out_of_image, float *pixel_unrounded, void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_project_points: views not set");
    if (N == 0) return MH_OK;
    if (!points || N < 0 || view < 0 || view >= ctx->V) return fail(MH_ERR_ARG, "mh_project_points: bad arguments");
    return launched(mh_launch_project_points(ctx->cams + (size_t)view * MH_CAM_STRIDE, points, N, ctx->H, ctx->W, row_col,
                                             z_half, out_of_image, pixel_unrounded, ctx->reproject_rule == 0 ? 1 : 0,
                                             (hipStream_t)stream),
                    "mh_project_points");
}

extern "C" int mh_gather_pixels(mh_ctx *ctx, int view, const long long *row_col, int N, int size, float *records,
                                float *mask, void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_gather_pixels: views not set");
    if (N == 0) return MH_OK;
    if (!row_col || N < 0 || view < 0 || view >= ctx->V || size < 1 || !(size & 1))
        return fail(MH_ERR_ARG, "mh_gather_pixels: bad arguments");
    return launched(mh_launch_gather(ctx->views(), view, row_col, N, size, (float4 *)records, mask, (hipStream_t)stream),
                    "mh_gather_pixels");
}

extern "C" int mh_compute_visible(mh_ctx *ctx, const float *depth, const float *z, size_t n, float *out, void *stream) {
    if (n == 0) return MH_OK;
    if (!ctx || !depth || !z || !out) return fail(MH_ERR_ARG, "mh_compute_visible: bad arguments");
    return launched(mh_launch_compute_visible(depth, z, n, out, (hipStream_t)stream), "mh_compute_visible");
}

extern "C" int mh_sample_next(mh_ctx *ctx, const float *points, const int32_t *base_view, const float *ori,
                              const float *offsets, int N, int S, float *samples, void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_sample_next: views not set");
    if (N == 0) return MH_OK;
    if (!points || !base_view || !ori || !offsets || !samples || N < 0 || S < 1)
        return fail(MH_ERR_ARG, "mh_sample_next: bad arguments");
    // (the V group sizes of this batch -- stream-ordered work space, so that calls on several streams do not share it)
    int32_t *gcnt = nullptr;
    if (ctx->reproject_rule == 0)
        MH_HIP(hipMallocAsync((void **)&gcnt, sizeof(int32_t) * (size_t)MH_GROUP_COPIES * MH_GROUP_RANKS * ctx->V,
                              (hipStream_t)stream));
    const int rc = launched(mh_launch_sample_next(ctx->views(), points, base_view, ori, offsets, N, S, samples,
                                                  ctx->reproject_rule, ctx->reproject_fma_min_cols, gcnt,
                                                  (hipStream_t)stream),
                            "mh_sample_next");
    if (gcnt) (void)hipFreeAsync(gcnt, (hipStream_t)stream);
    return rc;
}

extern "C" int mh_reproject_ori(mh_ctx *ctx, const float *points, const float *samples, int N, int S, float *D,
                                void *stream) {
    if (!ctx || !ctx->rec) return fail(MH_ERR_STATE, "mh_reproject_ori: views not set");
    if (N == 0) return MH_OK;
    if (!points || !samples || !D || N < 0 || S < 1) return fail(MH_ERR_ARG, "mh_reproject_ori: bad arguments");
    return launched(mh_launch_reproject(ctx->views(), points, samples, N, S, D, (hipStream_t)stream), "mh_reproject_ori");
}

extern "C" int mh_prj_loss(mh_ctx *ctx, const float *D, const float *ori_patch, const float *conf_patch,
                           const float *vis, int V, int N, int S, int P, float conf_threshold, float *loss,
                           long long *index, uint8_t *high_conf, float *all_loss, void *stream) {
    if (N == 0) return MH_OK;
    if (!ctx || !D || !ori_patch || !conf_patch || !vis || !loss || V < 1 || V >= 4096 || N < 0 || S < 1 || P < 1)
        return fail(MH_ERR_ARG, "mh_prj_loss: bad arguments");
    if (S > MH_PRJ_LOSS_MAX_S)
        return fail(MH_ERR_ARG, "mh_prj_loss: S = %d exceeds the limit of %d samples (two floats of LDS each, 64 KiB)", S,
                    MH_PRJ_LOSS_MAX_S);
    return launched(mh_launch_prj_loss(D, ori_patch, conf_patch, vis, V, N, S, P, conf_threshold, loss, index, high_conf,
                                       all_loss, ctx->sum_block, (hipStream_t)stream),
                    "mh_prj_loss");
}
