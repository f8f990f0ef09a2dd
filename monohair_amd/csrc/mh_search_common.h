// mh_search_common.h -- what the two search kernels of pmvo_search.hip (the portable mh_search_kernel and the shipped
// mh_search3_kernel) share as functions: the item positions in two parts (rank part + item part), the trailing-column sums
// and the order of torch.min.  (The two epilogues are NOT here: see DESIGN.md 4.14.)
#pragma once
#include "mh_device.h"

// (MH_MAX_ITEMS / MH_MAX_RANKS: mh_launch.h -- the C ABI refuses what exceeds them before anything is launched)

// PMVO.sample_next_3d_pos for one item (pixel(unrounded) + 2*(ori_col, ori_row) -> ndc -> unproject), split at what the S
// samples of one base-view rank have in common (the point's pixel in the base view, the shifted pixel in NDC, the two quotients
// of the unprojection) and what is per sample (depth + offset onwards).  The shipped search evaluates the rank part once per
// (point, rank) instead of once per item (90 times) and keeps it in LDS; the portable one runs both parts per item.
// rec[16] = { A, B, z, t0 | t1, t2, Ri0, Ri1 | Ri2 .. Ri5 | Ri6, Ri7, Ri8, forms }
// forms (mh_group_forms): how the sgemms of this (rank, base view) group round in the reference -- MH_FORM_GEMV here,
// MH_FORM_CHAIN in the item part.
__device__ __forceinline__ void mh_sample_rank(const float *__restrict__ cam, float X0, float X1, float X2, float ori_r,
                                               float ori_c, float Hf, float Wf, float *__restrict__ rec, int forms = 0) {
    float u, v, z, row, col;
    if (forms & MH_FORM_GEMV) mh_cam_project_single(cam, X0, X1, X2, u, v, z);
    else mh_cam_project(cam, X0, X1, X2, u, v, z);
    mh_ndc_to_pixel(u, v, Hf, Wf, row, col);
    float nx = col + ori_c * 2.0f;
    float ny = row + ori_r * 2.0f;
    nx = nx / Wf;
    ny = ny / Hf;
    nx = nx * 2.0f - 1.0f;
    ny = ny * 2.0f - 1.0f;
    nx = -nx;
    rec[0] = (nx - cam[18]) / cam[16];
    rec[1] = (ny - cam[22]) / cam[21];
    rec[2] = z;
    rec[3] = cam[3];
    rec[4] = cam[7];
    rec[5] = cam[11];
#pragma unroll
    for (int i = 0; i < 9; ++i) rec[6 + i] = cam[32 + i];
    rec[15] = __int_as_float(forms);
}

__device__ __forceinline__ void mh_sample_item(const float4 *__restrict__ rec, float off, float &S0, float &S1, float &S2) {
    const float4 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
    const float z = a.z + off;
    const float c0 = a.x * z, c1 = a.y * z;
    const float d0 = c0 - a.w, d1 = c1 - b.x, d2 = z - b.y;
    if (__float_as_int(d.w) & MH_FORM_CHAIN) {   // (prologue / epilogue only: once per item)
        S0 = mh_fma(c.x, d2, mh_fma(b.w, d1, b.z * d0));
        S1 = mh_fma(c.w, d2, mh_fma(c.z, d1, c.y * d0));
        S2 = mh_fma(d.z, d2, mh_fma(d.y, d1, d.x * d0));
    } else {
        S0 = (b.z * d0 + c.x * d2) + b.w * d1;
        S1 = (c.y * d0 + c.w * d2) + c.z * d1;
        S2 = (d.x * d0 + d.z * d2) + d.y * d1;
    }
}

// where the trailing columns of the batch's [V, N*S] sums fall in point n: its first trailing sample (S if none)
__device__ __forceinline__ int mh_tail_from(const MhRule &rule, int n, int S) {
    const long long c0 = (long long)n * S;
    if (c0 + S <= rule.tail_col0) return S;
    return c0 >= rule.tail_col0 ? 0 : (int)(rule.tail_col0 - c0);
}

// The weighted sums over the views of ONE candidate (item position X) of point n in ATen's row_sum order (mh_device.h:
// mh_row_sum_views) -- for the trailing columns of the batch's [V, N*S] sums.  The per-view terms are evaluated as the
// portable kernel evaluates them (same operations as the shipped bodies, bit for bit): tap lists from the scratch records,
// views that do not see the point (list length 0) add +0; cnt = the number of views with a positive weight.  It runs for a few
// dozen items per launch, after the view loops, from the item's rank record in LDS -- nothing of it is live in those loops
// (inside mh_search_slices_lds the same code cost the hot kernel 20 spilled registers).
__device__ __forceinline__ void mh_tail_item_sums(const float *__restrict__ cams, int V, float Hf, float Wf,
                                                  const float4 *__restrict__ taps_n, size_t vstride,
                                                  const uint8_t *__restrict__ vcnt_n, int N, float X0, float X1, float X2,
                                                  float &nm_out, float &dn_out, int &cnt_out) {
    int cnt = 0;
    auto term = [&](int v, float &tn, float &td) {
        tn = td = 0.0f;
        const int ntap = vcnt_n ? (int)vcnt_n[(size_t)v * N] : -1;
        if (ntap == 0) return;
        const float4 *__restrict__ rec = taps_n + (size_t)v * vstride;
        const float4 hdr = rec[0];
        if (hdr.y == -1.0f) return;
        const int nt = ntap > 0 ? ntap : __float_as_int(hdr.x);
        float row, col, dx, dy;
        mh_pixel_of(cams + v * MH_CAM_STRIDE, X0, X1, X2, Hf, Wf, row, col);
        mh_unit2(row - hdr.z, col - hdr.w, dx, dy);
        const float4 t0 = rec[1];
        float ml = 1.0f - __builtin_fabsf(t0.x * dx + t0.y * dy), bc = t0.z;
#pragma unroll 4
        for (int t = 1; t < nt; ++t) {
            const float4 tp = rec[1 + t];
            const float l = 1.0f - __builtin_fabsf(tp.x * dx + tp.y * dy);
            const bool upd = l < ml;
            ml = upd ? l : ml;
            bc = upd ? tp.z : bc;
        }
        tn = ml * bc;
        td = bc;
        cnt += (bc > 0.0f) ? 1 : 0;
    };
    const int L = V >> 2;
    float pn[4][3] = {}, pd[4][3] = {};   // partial k (rows k, k+4, ...): cascade levels 0, 1, 2
    for (int i = 0; i < L; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float tn, td;
            term(4 * i + k, tn, td);
            pn[k][0] = pn[k][0] + tn;
            pd[k][0] = pd[k][0] + td;
        }
        if (((i + 1) & 15) == 0) {   // a full block of 16 rows per partial: level 0 -> 1, every 256 rows level 1 -> 2
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                pn[k][1] = pn[k][1] + pn[k][0];
                pn[k][0] = 0.0f;
                pd[k][1] = pd[k][1] + pd[k][0];
                pd[k][0] = 0.0f;
                if (((i + 1) & 0xF0) == 0) {
                    pn[k][2] = pn[k][2] + pn[k][1];
                    pn[k][1] = 0.0f;
                    pd[k][2] = pd[k][2] + pd[k][1];
                    pd[k][1] = 0.0f;
                }
            }
        }
    }
    float sn[4], sd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sn[k] = (pn[k][0] + pn[k][1]) + pn[k][2];
        sd[k] = (pd[k][0] + pd[k][1]) + pd[k][2];
    }
    for (int v = L * 4; v < V; ++v) {
        float tn, td;
        term(v, tn, td);
        sn[0] = sn[0] + tn;
        sd[0] = sd[0] + td;
    }
    nm_out = ((sn[0] + sn[1]) + sn[2]) + sn[3];
    dn_out = ((sd[0] + sd[1]) + sd[2]) + sd[3];
    cnt_out = cnt;
}

// A view that does not see the point still enters the reference's sums over views, as loss x weight 0 (PMVO.py:191-198).  Where
// the point's own pixel position in such a view is not finite (the point lies in that camera's plane, or is not finite itself)
// D = pix(sample) - pix(point) is NaN for every sample, NaN x 0 = NaN, and every loss of the point is NaN.  The searches skip
// the views that do not see the point, so they ask here, once per point, whether there is such a view (a view with a non-finite
// position never sees the point: out_index).  Uniform over the workgroup; holds a barrier.  Pinned by pmvo_border.npz.
__device__ __forceinline__ bool mh_point_pixel_not_finite(const MhViews &vw, float P0, float P1, float P2, int N, int tid,
                                                          int T) {
    const bool single = vw.batch_rule && N == 1;
    bool bad = false;
    for (int v = tid; v < vw.V; v += T) {
        float row, col;
        mh_pixel_of_b(vw.cams + v * MH_CAM_STRIDE, P0, P1, P2, (float)vw.H, (float)vw.W, row, col, single);
        bad |= !(__builtin_fabsf(row) < __builtin_inff()) || !(__builtin_fabsf(col) < __builtin_inff());
    }
    return __syncthreads_or(bad ? 1 : 0) != 0;
}

// torch.min over a row with NaN propagation: NaN beats numbers, first index wins among equals
__device__ __forceinline__ bool mh_min_better(float al, int ai, float bl, int bi) {
    const bool an = al != al, bn = bl != bl;
    if (an || bn) return (an && bn) ? (ai < bi) : an;
    return (al < bl) || (al == bl && ai < bi);
}
