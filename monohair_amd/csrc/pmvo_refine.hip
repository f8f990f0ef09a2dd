// pmvo_refine.hip -- the losses of PMVO.refine (PMVO.py:86-92) and of refine's smoothing loop (PMVO.py:602-650), gfx950 only:
// the loss of ONE given direction per point from gathered patches (mh_refine_loss_kernel) or straight from the maps
// (mh_refine_loss_maps_kernel), and the combine step of the smoothing loop (mh_refine_combine_kernel).  They share nothing
// with the search (pmvo_search.hip) but mh_device.h; the maps kernel takes its centre sample, patch window and tap eligibility
// from mh_front.h.
#include "mh_front.h"

// ---------------------------------------------------------------------------------------------
// PMVO.refine's loss of ONE given direction per point (PMVO.py:86-90): next = p + dir*mul/div,
// compute_reproject_ori + compute_prj_loss with S = 1 (then `low_conf_index` is always true and the raw
// num/den is returned, PMVO.py:199-204).  One wave per point, lane = view; the per-view terms go through
// LDS so that lane 0 can add them in ATen's cascade order.  Patches are read raw ([V,N,P,..] layout).
// ---------------------------------------------------------------------------------------------
#define MH_REFINE_VMAX 512
__global__ __launch_bounds__(256) void mh_refine_loss_kernel(MhViews vw, const float *__restrict__ pts,
                                                             const float *__restrict__ dir, float mul, float dv,
                                                             int N, int P, float thr, const float *__restrict__ vis,
                                                             const float *__restrict__ ori_patch,
                                                             const float *__restrict__ conf_patch,
                                                             float *__restrict__ loss, uint8_t *__restrict__ hcout,
                                                             MhBatch bt) {
    __shared__ float s_num[4][MH_REFINE_VMAX], s_den[4][MH_REFINE_VMAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + wave;
    if (n >= N) return;
    const int V = vw.V;
    const float Hf = (float)vw.H, Wf = (float)vw.W;
    const float P0 = pts[3 * n], P1 = pts[3 * n + 1], P2 = pts[3 * n + 2];
    const float Q0 = P0 + dir[3 * n] * mul / dv, Q1 = P1 + dir[3 * n + 1] * mul / dv,
                Q2 = P2 + dir[3 * n + 2] * mul / dv;
    // a batch of ONE point: its [V,1] sums over the views are ATen's inner sums whenever the outer-sum rule is on (sum_block > 0)
    // and -- with the batch rule of the products (reproject_rule 0) -- its projections are single-column products
    const bool one_point = mh_batch_single(bt, n);
    const bool single = bt.single_ok && one_point;
    for (int v = lane; v < V; v += MH_WAVE) {
        const float *cam = vw.cams + v * MH_CAM_STRIDE;
        float r0, c0, r1, c1, dx, dy;
        mh_pixel_of_b(cam, P0, P1, P2, Hf, Wf, r0, c0, single);
        mh_pixel_of_b(cam, Q0, Q1, Q2, Hf, Wf, r1, c1, single);
        mh_unit2(r1 - r0, c1 - c0, dx, dy);
        const size_t vn = (size_t)v * N + n;
        const float *__restrict__ cp = conf_patch + vn * P;
        const float2 *__restrict__ op = reinterpret_cast<const float2 *>(ori_patch) + vn * P;
        float cmax = cp[0];
        for (int p = 1; p < P; ++p) cmax = (cp[p] > cmax) ? cp[p] : cmax;
        const bool hc = cmax > thr;
        float ml = 0.f, bc = 0.f;
        for (int p = 0; p < P; ++p) {
            float o0, o1;
            const float2 o = op[p];
            mh_unit2(o.x, o.y, o0, o1);
            const float cs = o0 * dx + o1 * dy;
            const float l = 1.0f - __builtin_fabsf(cs);
            const float c = cp[p];
            const bool upd = (p == 0) || ((l < ml) && (hc ? (c > thr) : true));
            ml = upd ? l : ml;
            bc = upd ? c : bc;
        }
        const float w = (vis[vn] == -1.0f ? 0.0f : 1.0f) * bc;
        s_num[wave][v] = ml * w;
        s_den[wave][v] = w;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        MhCascV nm = {0.f, 0.f, 0.f}, dn = {0.f, 0.f, 0.f};
        int cnt = 0;
        for (int v = 0; v < V; ++v) {
            if (v > 0 && (v & 15) == 0) {
                mh_cascv_flush(nm, v);
                mh_cascv_flush(dn, v);
            }
            const float w = s_den[wave][v];
            nm.a0 = nm.a0 + s_num[wave][v];
            dn.a0 = dn.a0 + w;
            cnt += (w > 0.0f) ? 1 : 0;
        }
        float d = mh_cascv_done(dn), m = mh_cascv_done(nm);
        if (one_point && bt.block > 0) {   // [V, 1]: ATen's sum over a contiguous innermost dimension
            m = mh_inner_sum_views(V, [&](int v) { return s_num[wave][v]; });
            d = mh_inner_sum_views(V, [&](int v) { return s_den[wave][v]; });
        } else if (mh_tail_row(bt, n)) {   // a trailing column of the batch's [V, N] sums (ATen's row_sum order)
            m = mh_row_sum_views(V, [&](int v) { return s_num[wave][v]; });
            d = mh_row_sum_views(V, [&](int v) { return s_den[wave][v]; });
        }
        loss[n] = m / d;
        if (hcout) hcout[n] = (d / (float)cnt > thr) ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// The same loss straight from the maps (refine's smoothing loop, PMVO.py:602-650, calls PMVO.refine once per 5000-point
// chunk): projection, visibility and the patch of every view that sees the point are evaluated in the kernel, the
// [V,N,P,..] patch tensors (365 MB per chunk at the headline size) are never written.  Per (view, point) the
// operations are those of mh_project_gather_kernel followed by mh_refine_loss_kernel, in the same order, so the
// result is bit-identical to the two-kernel path; views that do not see the point have weight 0 (PMVO.py:212) and
// are skipped, as in mh_search_kernel.
// ---------------------------------------------------------------------------------------------
// Round 6: lane = TAP for the patches.  A wave owns one point.  Phase 1 (lane = view, 64 views at a time): projection,
// depth test, the projected direction of the candidate.  Phase 2: the views that see the point are walked on the ballot
// mask; for each, the wave's lanes gather the P taps of the patch as PATCH contiguous runs (one coalesced request per view
// instead of 2 P per-lane gathers with one address per view -- the round-1..5 form spent 5.1 ms per 288 k points, 4 % of
// HBM), evaluate 1 - |cos| one tap per lane, and find (a) the patch maximum of the confidence and (b) the lexicographic
// minimum of (loss, tap index) over tap 0 and the eligible taps with two shuffle reductions.  That IS the sequential rule
// of compute_prj_loss (PMVO.py:160-190: tap 0 unconditionally, a later tap only if strictly smaller and eligible), NaN
// cases included: a NaN loss never wins a `<`; a NaN at tap 0 stays.  The next view's taps are requested before the
// current view is reduced.  Per-view terms go to LDS and lane 0 adds them in ATen's order, as before.
template <int PATCH>
__global__ __launch_bounds__(256) void mh_refine_loss_maps_kernel(MhViews vw, const float *__restrict__ pts,
                                                                  const float *__restrict__ dir, float mul, float dv,
                                                                  int N, float thr, float *__restrict__ loss,
                                                                  uint8_t *__restrict__ hcout, MhBatch bt) {
    constexpr int P = PATCH * PATCH, ROUNDS = (P + MH_WAVE - 1) / MH_WAVE;
    __shared__ float s_num[4][MH_REFINE_VMAX], s_den[4][MH_REFINE_VMAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + wave;
    if (n >= N) return;
    const int V = vw.V, H = vw.H, W = vw.W;
    const float Hf = (float)H, Wf = (float)W;
    const float P0 = pts[3 * n], P1 = pts[3 * n + 1], P2 = pts[3 * n + 2];
    const float Q0 = P0 + dir[3 * n] * mul / dv, Q1 = P1 + dir[3 * n + 1] * mul / dv,
                Q2 = P2 + dir[3 * n + 2] * mul / dv;
    // a batch of ONE point: its [V,1] sums over the views are ATen's inner sums whenever the outer-sum rule is on (sum_block > 0)
    // and -- with the batch rule of the products (reproject_rule 0) -- its projections are single-column products
    const bool one_point = mh_batch_single(bt, n);
    const bool single = bt.single_ok && one_point;
    int ti[ROUNDS], tj[ROUNDS];
#pragma unroll
    for (int t = 0; t < ROUNDS; ++t) mh_tap_offset(min(lane + MH_WAVE * t, P - 1), PATCH, ti[t], tj[t]);
    auto rdf = [](float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); };
    for (int v0 = 0; v0 < V; v0 += MH_WAVE) {
        const int v = v0 + lane;
        float visv = -1.0f, dx = 0.0f, dy = 0.0f;
        int r = 0, c = 0;
        if (v < V) {
            const float *cam = vw.cams + v * MH_CAM_STRIDE;
            const MhCentre s = mh_centre_sample(cam, P0, P1, P2, H, W, single);
            const float r0 = s.rowf, c0 = s.colf;
            r = s.r, c = s.c;
            const float4 q = vw.rec[(size_t)v * H * W + (size_t)r * W + c];
            visv = mh_centre_visible(s, q);
            if (visv != -1.0f) {
                float r1, c1;
                mh_pixel_of_b(cam, Q0, Q1, Q2, Hf, Wf, r1, c1, single);
                mh_unit2(r1 - r0, c1 - c0, dx, dy);
            } else {
                // weight 0, but the reference still adds loss x 0 (PMVO.py:191-198): NaN where this view's D is not finite
                float r1, c1;
                mh_pixel_of_b(cam, Q0, Q1, Q2, Hf, Wf, r1, c1, single);
                mh_unit2(r1 - r0, c1 - c0, dx, dy);
                s_num[wave][v] = (dx != dx || dy != dy) ? __builtin_nanf("") : 0.0f;
                s_den[wave][v] = 0.0f;
            }
        }
        unsigned long long m = __ballot(visv != -1.0f);
        // taps of one view: {unit ori_row, unit ori_col, clamped conf} per lane and round
        float o0[ROUNDS], o1[ROUNDS], cf[ROUNDS], no0[ROUNDS], no1[ROUNDS], ncf[ROUNDS];
        auto gather = [&](int src, float *a0, float *a1, float *ac) {
            const int rv = __builtin_amdgcn_readlane(r, src), cv = __builtin_amdgcn_readlane(c, src);
            const size_t base = (size_t)(v0 + src) * H * W;
#pragma unroll
            for (int t = 0; t < ROUNDS; ++t) {
                const size_t pix = base + mh_tap_pixel(rv, cv, ti[t], tj[t], H, W);
                if (vw.tap) {   // (the plane of ready-made taps, MhViews::tap: the same values, made once at upload)
                    const float4 tq = vw.tap[pix];
                    a0[t] = tq.x;
                    a1[t] = tq.y;
                    ac[t] = tq.z;
                } else {
                    const float4 tq = vw.rec[pix];
                    mh_unit2(tq.x, tq.y, a0[t], a1[t]);
                    ac[t] = mh_clampf(tq.z, 1e-6f, 1.0f);
                }
            }
        };
        int src = m ? __builtin_amdgcn_readfirstlane(__builtin_ctzll(m)) : 0;
        if (m) gather(src, no0, no1, ncf);
        while (m) {
            const int cur = src;
            m &= m - 1;
#pragma unroll
            for (int t = 0; t < ROUNDS; ++t) {
                o0[t] = no0[t];
                o1[t] = no1[t];
                cf[t] = ncf[t];
            }
            if (m) {
                src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
                gather(src, no0, no1, ncf);
            }
            const float dxv = rdf(dx, cur), dyv = rdf(dy, cur);
            // (a) cmax as `cmax = (p == 0 || cf > cmax) ? cf : cmax` leaves it: the maximum, NaNs skipped -- unless tap 0 is NaN
            const float cf0 = rdf(cf[0], 0);
            float mx = -__builtin_inff();
#pragma unroll
            for (int t = 0; t < ROUNDS; ++t)
                if (lane + MH_WAVE * t < P && cf[t] == cf[t]) mx = fmaxf(mx, cf[t]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            const float cmax = (cf0 != cf0) ? cf0 : mx;
            const bool hc = cmax > thr;
            // (b) lexicographic minimum of (loss, tap) over tap 0 and the eligible taps
            float bl = __builtin_inff(), bcf = 0.0f;
            int bp = 0x7fffffff;
            float l0 = 0.0f;
#pragma unroll
            for (int t = 0; t < ROUNDS; ++t) {
                const int p = lane + MH_WAVE * t;
                const float cs = o0[t] * dxv + o1[t] * dyv;
                const float l = 1.0f - __builtin_fabsf(cs);
                if (t == 0) l0 = l;
                const bool cand = p < P && mh_tap_eligible(p, hc, &cf[t], thr) && (p == 0 || l == l);
                if (cand && (bp == 0x7fffffff || l < bl)) {   // (rounds ascend in p: a tie keeps the earlier tap)
                    bl = l;
                    bp = p;
                    bcf = cf[t];
                }
            }
            l0 = rdf(l0, 0);
            const float c0v = cf0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ol = __shfl_xor(bl, o), oc = __shfl_xor(bcf, o);
                const int op = __shfl_xor(bp, o);
                const bool take = op != 0x7fffffff && (bp == 0x7fffffff || ol < bl || (ol == bl && op < bp));
                bl = take ? ol : bl;
                bcf = take ? oc : bcf;
                bp = take ? op : bp;
            }
            // a NaN at tap 0 is never replaced (`l < NaN` is false for every later tap)
            const float ml = (l0 != l0) ? l0 : bl, bc = (l0 != l0) ? c0v : bcf;
            if (lane == 0) {
                s_num[wave][v0 + cur] = ml * bc;
                s_den[wave][v0 + cur] = bc;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        MhCascV nm = {0.f, 0.f, 0.f}, dn = {0.f, 0.f, 0.f};
        int cnt = 0;
        for (int v = 0; v < V; ++v) {
            if (v > 0 && (v & 15) == 0) {
                mh_cascv_flush(nm, v);
                mh_cascv_flush(dn, v);
            }
            const float w = s_den[wave][v];
            nm.a0 = nm.a0 + s_num[wave][v];
            dn.a0 = dn.a0 + w;
            cnt += (w > 0.0f) ? 1 : 0;
        }
        float d = mh_cascv_done(dn), m = mh_cascv_done(nm);
        if (one_point && bt.block > 0) {   // [V, 1]: ATen's sum over a contiguous innermost dimension
            m = mh_inner_sum_views(V, [&](int v) { return s_num[wave][v]; });
            d = mh_inner_sum_views(V, [&](int v) { return s_den[wave][v]; });
        } else if (mh_tail_row(bt, n)) {   // a trailing column of the batch's [V, N] sums (ATen's row_sum order)
            m = mh_row_sum_views(V, [&](int v) { return s_num[wave][v]; });
            d = mh_row_sum_views(V, [&](int v) { return s_den[wave][v]; });
        }
        loss[n] = m / d;
        if (hcout) hcout[n] = (d / (float)cnt > thr) ? 1 : 0;
    }
}

// loss[n] <- -1 where the head filter fires (PMVO.py:91-92), the replacement rule of the smoothing loop on the
// orientations in place (:631-636, as mh_replace_dissimilar_kernel), and loss -1 -> 0.5 (:641-642) into loss_out
__global__ __launch_bounds__(256) void mh_refine_combine_kernel(const float *__restrict__ center,
                                                                const float *__restrict__ loss_u,
                                                                const uint8_t *__restrict__ head,
                                                                const uint8_t *__restrict__ head_top, float thr,
                                                                float *__restrict__ ori, float *__restrict__ loss_out,
                                                                int N) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const bool filt = head[n] && !head_top[n];
    const float ul = filt ? -1.0f : loss_u[n];
    loss_out[n] = (ul == -1.0f) ? 0.5f : ul;
    if (!ori) return;   // (the replacement was applied already: mh_replace_dissimilar in the chain of the smoothing loop)
    float c[3], o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = center[3 * n + k];
        o[k] = ori[3 * n + k];
    }
    float sc = c[0] * c[0];
    sc = mh_fma(c[1], c[1], sc);
    sc = mh_fma(c[2], c[2], sc);
    float so = o[0] * o[0];
    so = mh_fma(o[1], o[1], so);
    so = mh_fma(o[2], o[2], so);
    float nc = __builtin_sqrtf(sc), no = __builtin_sqrtf(so);
    nc = (nc < 1e-8f) ? 1e-8f : nc;
    no = (no < 1e-8f) ? 1e-8f : no;
    const float cs = ((c[0] / nc) * (o[0] / no) + (c[1] / nc) * (o[1] / no)) + (c[2] / nc) * (o[2] / no);
    if (__builtin_fabsf(cs) < thr) {
#pragma unroll
        for (int k = 0; k < 3; ++k) ori[3 * n + k] = c[k];
    }
}

// ---------------------------------------------------------------------------------------------
extern "C" int mh_launch_refine_loss_maps(MhViews vw, const float *pts, const float *dir, float mul, float dv, int N,
                                         int patch, float thr, float *loss, uint8_t *hc, int batch, long long row0,
                                         long long total, int sum_block, hipStream_t st) {
    if (vw.V > MH_REFINE_VMAX) return -1;
    const MhBatch bt = {row0, total, batch, sum_block, vw.batch_rule};
    const dim3 grid((N + 3) / 4), block(256);
    return mh_dispatch_patch(patch, [&](auto ps) {
        hipLaunchKernelGGL(mh_refine_loss_maps_kernel<decltype(ps)::value>, grid, block, 0, st, vw, pts, dir, mul, dv, N, thr,
                           loss, hc, bt);
    });
}

extern "C" int mh_launch_refine_combine(const float *center, const float *loss_u, const uint8_t *head,
                                        const uint8_t *head_top, float thr, float *ori, float *loss_out, int N,
                                        hipStream_t st) {
    hipLaunchKernelGGL(mh_refine_combine_kernel, dim3((N + 255) / 256), dim3(256), 0, st, center, loss_u, head,
                       head_top, thr, ori, loss_out, N);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_refine_loss(MhViews vw, const float *pts, const float *dir, float mul, float dv, int N,
                                     int P, float thr, const float *vis, const float *ori_patch,
                                     const float *conf_patch, float *loss, uint8_t *hc, int sum_block, hipStream_t st) {
    if (vw.V > MH_REFINE_VMAX) return -1;
    const MhBatch bt = {0, N, 0, sum_block, vw.batch_rule};   // (the stand-alone method: its N points are one batch of the reference)
    hipLaunchKernelGGL(mh_refine_loss_kernel, dim3((N + 3) / 4), dim3(256), 0, st, vw, pts, dir, mul, dv, N, P, thr,
                       vis, ori_patch, conf_patch, loss, hc, bt);
    return (int)hipGetLastError();
}

// forces this translation unit's code object onto the device before the first refine stage (see mh_preload_pmvo_search); called
// from mh_ctx_create
extern "C" int mh_preload_pmvo_refine() {
    hipFuncAttributes a;
    return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&mh_refine_combine_kernel));
}
