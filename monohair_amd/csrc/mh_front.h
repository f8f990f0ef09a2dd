// mh_front.h -- the rules every PMVO front end applies to a (view, point) pair, each stated ONCE (gfx950 only): the centre
// sample, the clamped patch window, tap eligibility, the duplicate rule with the compaction of one wave's tap list, the list
// header and the per-(view, point) stores of the fused front ends.  Included by pmvo_project.hip, pmvo_filter.hip,
// pmvo_refine.hip and pmvo_pieces.hip; the search (pmvo_search.hip) reads what these write and includes none of it.
// Everything is __forceinline__: the kernels keep their own organisation (which lane is a point, a view or a tap) and call
// these for the arithmetic, so that the front ends cannot drift apart (docs/HISTORY.md, "front ends share their rules").
#pragma once
#include "mh_device.h"

// ---- the centre sample (PMVO.project_points, PMVO.py:378-397) -------------------------------------------------------------
// Camera.projection of the point, ndc -> unrounded pixel (rowf, colf), then torch.round (half to even) -> long with the bounds
// tests and the clamp on the integers (mh_round_clamp_pixel: PMVO.py:383-390): (r, c) is the clamped centre, oob the
// reference's out_index, z the camera-space depth.  single: the point is alone in its batch (mh_cam_project_b).
struct MhCentre {
    float rowf, colf, z;
    int r, c;
    bool oob;
};
__device__ __forceinline__ MhCentre mh_centre_sample(const float *__restrict__ cam, float X0, float X1, float X2, int H, int W,
                                                     bool single) {
    MhCentre s;
    float u, w;
    mh_cam_project_b(cam, X0, X1, X2, u, w, s.z, single);
    mh_ndc_to_pixel(u, w, (float)H, (float)W, s.rowf, s.colf);
    s.oob = mh_round_clamp_pixel(s.rowf, s.colf, H, W, s.r, s.c);
    return s;
}
// the point's depth on the scale of the depth maps (PMVO.py:355: z' = -z / 2, times 255)
__device__ __forceinline__ float mh_centre_depth(const MhCentre &s) { return (-s.z / 2.0f) * 255.0f; }
// soft visibility of the centre record q (PMVO.py:346-376): compute_visible of the depth test, -1 outside the image
__device__ __forceinline__ float mh_centre_visible(const MhCentre &s, const float4 &q) {
    const float vb = mh_soft_visible(q.w, mh_centre_depth(s));
    return s.oob ? -1.0f : vb;
}
// how far the point lies behind the surface the view sees at its centre: what the votes threshold (PMVO.py:409-413)
__device__ __forceinline__ float mh_centre_gap(const MhCentre &s, const float4 &q) { return mh_centre_depth(s) - q.w; }

// ---- the patch window (get_ori_patch / get_c_patch, PMVO.py:482-523) ------------------------------------------------------
// tap p of a side x side window, row offset outer: offsets (di, dj) from the centre
__device__ __forceinline__ void mh_tap_offset(int p, int side, int &di, int &dj) {
    di = p / side - side / 2;
    dj = p - (p / side) * side - side / 2;
}
// the pixel a tap reads: each coordinate clamped to the image on its own (a window over the border repeats the border pixels)
__device__ __forceinline__ size_t mh_tap_pixel(int r, int c, int di, int dj, int H, int W) {
    return (size_t)min(max(r + di, 0), H - 1) * W + min(max(c + dj, 0), W - 1);
}

// ---- tap eligibility (compute_prj_loss, PMVO.py:162,177-182) --------------------------------------------------------------
// which taps can ever replace the running minimum: tap 0 always; a later tap iff its confidence exceeds the threshold or no
// tap of the patch does (hc = patch max conf > thr).  *conf is read only where it decides: callers keep it in memory.
__device__ __forceinline__ bool mh_tap_eligible(int p, bool hc, const float *conf, float thr) {
    return (p == 0) || (hc ? (*conf > thr) : true);
}

// ---- the tap list of a (view, point) -------------------------------------------------------------------------------------
// float4 header {count(bits), vis, pix_row, pix_col} followed by `count` float4 taps {ox_hat, oy_hat, conf, 0}; stride
// (P + 1) float4.  cnt[vn]: the compact copy of the list lengths [V,N] the search's work estimate reads coalesced.  (cnt and
// vn apart, the byte's address formed after the header store: as one pointer argument it costs the fp32 front end 2 VGPRs.)
__device__ __forceinline__ void mh_list_header(float4 *out, uint8_t *cnt, size_t vn, int count, float vis, float rowf,
                                               float colf) {
    out[0] = make_float4(__int_as_float(count), vis, rowf, colf);
    cnt[vn] = (uint8_t)count;
}
// vis == -1: the search skips this view for this point -- header only
__device__ __forceinline__ void mh_list_empty(float4 *out, uint8_t *cnt, size_t vn, float vis) {
    mh_list_header(out, cnt, vn, 0, vis, 0.0f, 0.0f);
}

// bucket of a unit orientation in the 256-entry "first tap with this orientation" table
__device__ __forceinline__ unsigned mh_ori_bucket(unsigned ox, unsigned oy) {
    return ((ox * 0x9E3779B1u) ^ (oy * 0x85EBCA77u)) >> 24;
}

// The duplicate rule and the compaction, by ONE wave on its own LDS slices; returns the length of the list.  The caller stores
// the header (mh_list_header): its values come out of lanes the callers read after the passes, as they always did.
// In: conf[p] the clamped confidences of the P taps (LDS or global); first[256] filled with 0xffffffff; o[p] the unit
// orientations (normalised as torch.cosine_similarity does, PMVO.py:171) -- or, with RAW, raw[p] the orientations as the maps
// hold them, normalised into o[p] in pass 1.  What this wave wrote of them need not be fenced yet.  el[p] is the wave's flag
// slice, filled here.  P: PC when the caller knows it at compile time (the loops then resolve), else PC = 0 and P_rt.
//   pass 1: eligibility (mh_tap_eligible); every eligible tap bids for "first tap with this orientation" in the table, keyed
//           by a hash of the unit vector's bits;
//   pass 2: a tap whose unit orientation is bit-identical to an EARLIER eligible tap can never win the strict '<' of
//           PMVO.py:177 (its loss equals that tap's for every candidate), so it is dropped -- exact, and on 8-bit orientation
//           maps (<= 180 distinct angles) it removes most of a patch.  A hash collision only means that a duplicate survives
//           (harmless); nothing distinct is ever dropped because the bits are compared.  The survivors are stored in their
//           original order (strict '<' keeps first-index tie-breaking).
// (Formulations that cost registers, kept out: the confidence passed to mh_tap_eligible by value -- an unconditional load,
// +1 VGPR in mh_prep_taps_kernel; the header stored in here -- +2 VGPRs in mh_project_taps2_kernel; DESIGN.md §4.3a, docs/HISTORY.md.)
template <int PC, bool RAW>
__device__ __forceinline__ int mh_wave_tap_list(int P_rt, int lane, const float2 *raw, float2 *o, const float *conf,
                                                unsigned char *el, unsigned int *first, bool hc, float thr,
                                                float4 *__restrict__ out) {
    const int P = PC > 0 ? PC : P_rt;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int p = lane; p < P; p += MH_WAVE) {
        float2 u;
        if (RAW) {
            const float2 r = raw[p];
            mh_unit2(r.x, r.y, u.x, u.y);
            o[p] = u;
        }
        const bool e = mh_tap_eligible(p, hc, conf + p, thr);
        el[p] = e;
        if (e) {
            if (!RAW) u = o[p];
            atomicMin(&first[mh_ori_bucket(__float_as_uint(u.x), __float_as_uint(u.y))], (unsigned)p);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int base = 0;
    for (int p0 = 0; p0 < P; p0 += MH_WAVE) {
        const int p = p0 + lane;
        bool e = false;
        float2 u = make_float2(0.f, 0.f);
        float cc = 0.f;
        if (p < P) {
            e = el[p] != 0;
            u = o[p];
            cc = conf[p];
            if (e) {
                const unsigned ox = __float_as_uint(u.x), oy = __float_as_uint(u.y);
                const unsigned qf = first[mh_ori_bucket(ox, oy)];
                if (qf < (unsigned)p) {
                    const float2 w = o[qf];
                    if (__float_as_uint(w.x) == ox && __float_as_uint(w.y) == oy) e = false;
                }
            }
        }
        const unsigned long long m = __ballot(e);
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        if (e) out[1 + pos] = make_float4(u.x, u.y, cc, 0.0f);
        base += __popcll(m);
    }
    return base;
}

// ---- the per-(view, point) outputs of the fused front ends (what the base-view ranking and the sampler read) ---------------
// vis, the raw centre orientation, the clamped centre confidence, the mask value *mk (read only if it is wanted), and the
// empty list of a pair the search will skip
__device__ __forceinline__ void mh_store_centre(size_t vn, float visv, const float4 &q0, const float *mk, int P,
                                                float *__restrict__ vis, float *__restrict__ ori,
                                                float *__restrict__ conf, float *__restrict__ mask,
                                                float4 *__restrict__ taps, uint8_t *__restrict__ cnt) {
    vis[vn] = visv;
    reinterpret_cast<float2 *>(ori)[vn] = make_float2(q0.x, q0.y);
    conf[vn] = mh_clampf(q0.z, 1e-6f, 1.0f);
    if (mask) mask[vn] = *mk;
    if (visv == -1.0f) mh_list_empty(taps + vn * (P + 1), cnt, vn, visv);
}
