// mh_capi.h -- what the translation units of the C ABI (capi*.cpp) share: the context, the error helpers, the one grid
// rule, the strand tools' checks and scratch front.  Internal (not installed).  Nothing here is part of the exported
// surface: all of it has hidden visibility.
// capi_host.cpp, which must build without HIP, does not include this file; it defines fail().
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mh_pmvo.h"
#include "../../include/mh_pmvo_lab.h"
#include "mh_launch.h"

#pragma GCC visibility push(hidden)

struct mh_ctx {
    int device = 0;
    int V = 0, H = 0, W = 0;
    float4 *rec = nullptr;    // [V][H][W]
    float *mask = nullptr;    // [V][H][W]
    float *cams = nullptr;    // [V][MH_CAM_STRIDE]
    // every pixel as a ready-made patch tap {unit ori, clamped conf} (MhViews::tap; 16 B per pixel more, 2 GB at 60 x 1080p):
    // allocated with the first view that comes in as fp32 planes, used by the fused front end once every view has been
    // written since; contexts of 8-bit code views never allocate it (their front end reads the 2 B codes)
    float4 *tapp = nullptr;
    bool tapp_failed = false;
    int use_tap_plane = 1;             // option "tap_plane": 0 = normalise per iteration (A/B, cross-check)
    // the plane doubles the resident map memory for +1.2 % iterations/s: only below this size (option "tap_plane_max_mb",
    // environment MH_TAP_PLANE_MAX_MB at context creation; 60 x 1080p = 1 991 MB fits, 120 x 4K = 15 925 MB does not) and
    // only while it leaves a quarter of the device's free memory to the scratch buffers of the drivers
    long long tap_plane_max_mb = 4096;
    std::vector<unsigned char> tap_view;   // per view: its slice of tapp is current
    const float4 *tap_ready() const {
        if (!tapp || !use_tap_plane || (int)tap_view.size() != V) return nullptr;
        for (unsigned char c : tap_view)
            if (!c) return nullptr;
        return tapp;
    }
    float *offs = nullptr;    // [S]
    float *gabor = nullptr;   // tap-major Gabor bank [289][192]
    float *gabor_q = nullptr; // the same coefficients in the operand order of mh_gabor_mfma2_kernel [145][64][8]
    unsigned int *gabor_max = nullptr;
    void *dog_w = nullptr;    // device MhDogWeights of the difference-of-Gaussians prefilter (csrc/dog.hip)
    MhDogWeights *dog_w_host = nullptr;   // what dog_w holds
    float4 *lut = nullptr;    // [256] pixel-code table of the 8-bit map files
    // views uploaded as 8-bit file codes keep the codes resident as well (2 B per pixel: orientation | confidence << 8) for
    // the per-iteration tap gathers of mh_forward_prepare; used when EVERY view was uploaded that way with one table
    uint16_t *oc = nullptr;           // [V][H][W]
    bool oc_failed = false;           // the optional allocation of `oc` failed once: stay on the records
    void *code_tabs = nullptr;        // MhCodeTabs (csrc/pmvo_project.hip), derived from lut
    std::vector<unsigned char> code_view;   // per view: uploaded as codes
    float lut_host[1024];             // the table the resident records and code tables were made with
    bool lut_set = false, lut_mixed = false;
    int use_codes = 1;                // option "tap_codes": 0 = always gather the fp32 records (A/B, cross-check)
    bool codes_ready() const {
        if (!oc || !code_tabs || !use_codes || lut_mixed || (int)code_view.size() != V) return false;
        for (unsigned char c : code_view)
            if (!c) return false;
        return true;
    }
    bool views_8bit() const {   // every view came in as 8-bit file codes (whatever "tap_codes" says)
        if ((int)code_view.size() != V || V == 0) return false;
        for (unsigned char c : code_view)
            if (!c) return false;
        return true;
    }
    int S = 0;
    int search_variant = 0;
    int search_body = 0;      // tap body of mh_search3_kernel: 0 = by the maps (see mh_ctx_set_option), 1 = keys, 2 = select
    // The lab option "search_variant" (include/mh_pmvo_lab.h) in words; false: not a value of that option.
    bool search_plan(MhSearchPlan *plan) const {
        *plan = MhSearchPlan{false, false, MhSearchPlan::ORDER_BY_WORK, MhSearchPlan::PART_ALL};
        switch (search_variant) {
            case 0: case 100: break;
            case 7: case 107: plan->order = MhSearchPlan::ORDER_NATURAL; break;
            case 9: case 109: plan->part = MhSearchPlan::PART_PRE_ONLY; break;
            case 10: case 110: plan->part = MhSearchPlan::PART_KERNEL_ONLY; break;
            case 1256: plan->portable = true; break;
            default: return false;
        }
        const bool select_asked = search_variant == 100 || search_variant == 107 || search_variant == 109 || search_variant == 110;
        // The shipped search has two tap bodies with the same results (csrc/pmvo_search.hip): the key body (5.5 instructions per
        // evaluation, a fixed cost per view) and the compare-and-select body (7, none).  Lists of continuous maps hold ~45 taps,
        // lists of 8-bit maps ~2 after the exact duplicate removal: the kernel that carries both bodies runs short lists 5 %
        // slower than the select-only kernel (register allocation), so contexts whose views are all 8-bit codes get that one.
        plan->select_body = select_asked || search_body == 2 || (search_body == 0 && views_8bit());
        return true;
    }
    // The reference's batch composition in the arithmetic (csrc/mh_device.h: MhRule, MhBatch; oracle/pmvo_oracle.c):
    int reproject_rule = 0;   // 0: sample_next_3d_pos's sgemms round by the size of the (rank, base view) group as MKL does in
                              //    the reference; 1: the mid-size forms for every point; 2: the chain forms
    int reproject_fma_min_cols = 28445;   // columns (S x group) from which MKL's threaded sgemm (fma chain) takes over
    int sum_block = 32;       // ATen's outer sum adds the trailing (columns mod 32) of a batch in row_sum order; 0: never
    int topk_order = 0;       // 0: torch.topk's CPU tie order (mh_topk_wave.h); 1: value desc, view asc (round 1's rule)
    int carve_early_exit = 1; // lab "carve_early_exit": 1 = mh_carve_inside leaves a voxel's view loop once n_miss > max_miss, 0 = all views
    int filter_rows = 1;      // lab "filter_rows": 1 = votes of large launches with lane = point (mh_filter_rows_kernel), 0 = wave per point
    int taps_tile = 1;        // points per wave of mh_project_taps2_kernel: 16 / 32 (A/B), anything else = 64 (default)
    int line_rule = 0;        // strand renderer: 0 GL's diamond-exit, 1 every touched diamond (SwiftShader)
    int raster_subpixel_bits = 8;   // both rasterisers: window positions snapped to 2^-bits pixel (SwiftShader: 4)
    int gabor_variant = 3;    // 3: FP32-MFMA im2col contraction (default); 0: direct v_pk_fma form (cross-check).
                              // (1 and 2 named two forms removed in round 4.)
    MhViews views() const { return MhViews{V, H, W, rec, mask, cams, tap_ready(), reproject_rule == 0 ? 1 : 0}; }
};

int fail(int code, const char *fmt, ...);      // capi_host.cpp: sets mh_last_error()'s text, returns code
int launched(int rc, const char *what);        // capi.cpp: a launcher's return value as an MH_ code

#define MH_HIP(call)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) return fail(MH_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// a grid of x * y * z cells that an int32 can index: every dimension at least 1, fewer than 2^31 cells
inline bool cells_fit_int32(int x, int y, int z) {
    return x >= 1 && y >= 1 && z >= 1 && (long long)x * y < (1ll << 31) && (long long)x * y * z < (1ll << 31);
}

// ---- the voxel grid of the volume entry points (capi_volume.cpp, capi_carve.cpp)
inline bool vol_dims_ok(const int32_t *dims) { return dims && cells_fit_int32(dims[0], dims[1], dims[2]); }

// the one place that fills an MhVolGrid; bust_to_origin: null = no shift.  false: an argument is missing or not usable
inline bool vol_grid(MhVolGrid *gr, const double *voxel_min, double voxel_size, const int32_t *dims,
                     const double *bust_to_origin = nullptr) {
    if (!voxel_min || !vol_dims_ok(dims) || !(voxel_size > 0.0 && std::isfinite(voxel_size))) return false;
    for (int c = 0; c < 3; ++c) {
        gr->bust[c] = bust_to_origin ? bust_to_origin[c] : 0.0, gr->vmin[c] = voxel_min[c];
        if (!std::isfinite(gr->bust[c]) || !std::isfinite(voxel_min[c])) return false;
    }
    gr->vs = voxel_size;
    gr->X = dims[0], gr->Y = dims[1], gr->Z = dims[2];
    return true;
}

// ---- what the entry points of the strand tools share (capi_capture.cpp, capi_reproj.cpp, capi_volume.cpp)
#define MH_MAX_RADIUS 16      // the largest splat radius of the capture and of the capture agreement

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// an image of H * W pixels that an int32 can index
inline bool image_fits_int32(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31); }

// a strand set (points or projected vertices, valid, offsets): an empty one needs no pointer, any other needs all of them
// and a strand.  has_valid = false: the entry point takes no `valid` (mh_strand_volume_accumulate)
inline bool strands_ok(const float *points, const uint8_t *valid, const long long *offsets, int n_strands, int n_points,
                       bool has_valid = true) {
    return n_strands >= 0 && n_points >= 0 && (n_points == 0 || (points && (valid || !has_valid) && offsets && n_strands >= 1));
}

// The front of every per-view scratch (mh_capture_view, mh_photo_view, mh_support_view): dropped 256 B | vert | valid, then
// whatever the deriving layout take()s, every region on a 256 B boundary.  The size queries construct a layout on a null
// base and read `bytes`; the entry points construct the same layout on the caller's buffer.
struct ViewScratch {
    int32_t *dropped;
    float *vert;
    uint8_t *valid;
    size_t n, bytes = 0;      // n: the points the per-point regions are sized for (at least 1)
    ViewScratch(int n_points, void *base) : n((size_t)(n_points > 0 ? n_points : 1)), base_((uintptr_t)base) {
        dropped = take<int32_t>(256), vert = take<float>(n * 12), valid = take<uint8_t>(n);
    }
    template <typename T>
    T *take(size_t b) {      // the next region, of b bytes
        bytes += align256(b);
        return (T *)(base_ + bytes - align256(b));
    }
    uintptr_t base_;      // (an integer: the size queries pass no buffer)
};

#pragma GCC visibility pop
