// pmvo_search.hip -- the fused loss search of PMVO.forward (PMVO.py:50-78), gfx950 only.
//
// One workgroup = one candidate 3D point.  Its nrank*S (= 10*90 = 900) candidate segment end-points
// ("items") are spread over the lanes, K items per lane, and live in registers for the whole kernel:
//   sample_next_3d_pos (PMVO.py:263-335)      -> item position X            (once, prologue)
//   compute_reproject_ori (PMVO.py:219-241)    -> unit direction d_hat per view (registers)
//   compute_prj_loss (PMVO.py:151-209)         -> masked min over the taps of the patch, weighted
//                                                 sums over views in ATen's cascade order
//   forward's best-so-far update (PMVO.py:57-70) -> LDS epilogue.
// No [V,N,S] tensor ever exists.  The patch of (view, point) is the same for every lane of the
// workgroup, so the tap list (pmvo_project.hip: mh_prep_taps_kernel) is read with wave-uniform loads (header
// and first tap: scalar loads; the rest: broadcast vector loads, what the backend selects for the ping-pong
// groups) and the inner loop is pure VALU: per (item, tap) 2 mul + add + (1-|x|) + cmp + 2 cndmask in the portable kernel and
// the select body of the shipped one; its key body keeps the running (loss, tap) minimum as one integer key per item and
// needs 2 mul + add + sub + lshl_or + half a min3 (see MH_KEY_C) -- for patches up to 8 x 8 the key is that of a four-tap
// block, 2 mul + add per tap and max, max3, sub, lshl_or + half a min3 per block (see MH_KEY_C, mh_seed_key); a list's last tap
// seeds the minimum instead of padding a four-tap block (see mh_key_walked).
// Views in which the point is not visible (vis == -1 => weight 0, PMVO.py:212) are skipped: adding
// their exact zeros would not change any sum.
#include "mh_search_common.h"
#include "../../include/mh_pmvo_lab.h"   // mh_debug_key_stats

// PMVO.sample_next_3d_pos for one item from scratch: rank part + item part (mh_search_common.h).  Only the portable kernel
// uses it; the shipped one evaluates the rank part once per (point, rank) and keeps it in LDS.
__device__ __forceinline__ void mh_sample_next(const float *__restrict__ cam, float X0, float X1, float X2,
                                               float ori_r, float ori_c, float Hf, float Wf, float off, float &S0,
                                               float &S1, float &S2, int forms) {
    alignas(16) float rec[16];
    mh_sample_rank(cam, X0, X1, X2, ori_r, ori_c, Hf, Wf, rec, forms);
    mh_sample_item(reinterpret_cast<const float4 *>(rec), off, S0, S1, S2);
}

// 1 - |x| as ONE instruction (abs is a source modifier); kept out of the SLP vectoriser's reach
__device__ __forceinline__ float mh_one_minus_abs(float x) {
    float r;
    asm("v_sub_f32_e64 %0, 1.0, |%1|" : "=v"(r) : "v"(x));
    return r;
}

// mh_search_kernel -- the PORTABLE form of the fused loss search: plain C++ loops over views and taps, the compiler's
// schedule, tap lists read from the scratch records.  It is the cross-check of the shipped mh_search3_kernel (every test that
// compares the search with the oracle runs both: search_variant 1256) and what runs when no list lengths are available.
// (Rounds 1-2 carried this kernel's hand-shaped FAST forms and mh_search2_kernel as variants; they are gone: three
// generations of one arithmetic contract were two too many to keep in step.)
template <int K, int T>
__global__ __launch_bounds__(T) void mh_search_kernel(MhViews vw, const float *__restrict__ offs, int S, int nrank,
                                                      int rank_step, const float *__restrict__ pts, int N, int P1,
                                                      float thr, const float *__restrict__ ori_c,
                                                      const int32_t *__restrict__ base_idx,
                                                      const float *__restrict__ base_val,
                                                      const float4 *__restrict__ taps, float *__restrict__ line_ori,
                                                      float *__restrict__ min_loss, uint8_t *__restrict__ high_conf,
                                                      float *__restrict__ best_sample, int32_t *__restrict__ best_rank,
                                                      int32_t *__restrict__ best_s, MhRule rule) {
    __shared__ float s_loss[MH_MAX_ITEMS];
    __shared__ uint8_t s_pos[MH_MAX_ITEMS];
    __shared__ float s_rl[MH_MAX_RANKS];
    __shared__ int s_ri[MH_MAX_RANKS];
    __shared__ int s_rh[MH_MAX_RANKS];

    const int n = blockIdx.x, tid = threadIdx.x;
    const int nitems = nrank * S;
    const int V = vw.V;
    const float Hf = (float)vw.H, Wf = (float)vw.W;
    const float P0 = pts[3 * n], P1x = pts[3 * n + 1], P2 = pts[3 * n + 2];

    float X0[K], X1[K], X2[K];
    MhCascV num[K], den[K];
    int cnt[K];
    const int tail_from = mh_tail_from(rule, n, S);   // first trailing sample of the batch's [V, N*S] sums in this point
#pragma unroll
    for (int j = 0; j < K; ++j) {
        int it = j * T + tid;
        it = it < nitems ? it : 0;
        const int r = it / S, s = it - r * S;
        // (ranks with base_val <= 0 are unusable and their indices may be anything: clamped, as in mh_search3_kernel)
        const int b = min(max(base_idx[(size_t)(r * rank_step) * N + n], 0), V - 1);
        const float2 oc = reinterpret_cast<const float2 *>(ori_c)[(size_t)b * N + n];
        mh_sample_next(vw.cams + b * MH_CAM_STRIDE, P0, P1x, P2, oc.x, oc.y, Hf, Wf, offs[s], X0[j], X1[j], X2[j],
                       mh_group_forms(rule, r, V, b, S));
        num[j] = den[j] = MhCascV{0.0f, 0.0f, 0.0f};
        cnt[j] = 0;
    }

    for (int v = 0; v < V; ++v) {
        if (v > 0 && (v & 15) == 0) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                mh_cascv_flush(num[j], v);
                mh_cascv_flush(den[j], v);
            }
        }
        const float4 *__restrict__ rec = taps + ((size_t)v * N + n) * P1;
        const float4 hdr = rec[0];
        if (hdr.y == -1.0f) continue;   // uniform: point not visible in this view, weight 0
        const int ntap = __float_as_int(hdr.x);
        const float *__restrict__ cam = vw.cams + v * MH_CAM_STRIDE;
        const float4 t0 = rec[1];
        {
            float dx[K], dy[K], ml[K], bc[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                float row, col;
                mh_pixel_of(cam, X0[j], X1[j], X2[j], Hf, Wf, row, col);
                mh_unit2(row - hdr.z, col - hdr.w, dx[j], dy[j]);
                const float cs = t0.x * dx[j] + t0.y * dy[j];
                ml[j] = 1.0f - __builtin_fabsf(cs);
                bc[j] = t0.z;
            }
            for (int t = 1; t < ntap; ++t) {
                const float4 tp = rec[1 + t];
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const float cs = tp.x * dx[j] + tp.y * dy[j];
                    const float l = 1.0f - __builtin_fabsf(cs);
                    const bool upd = l < ml[j];
                    ml[j] = upd ? l : ml[j];
                    bc[j] = upd ? tp.z : bc[j];
                }
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float w = bc[j];   // (vis != -1) * best_conf
                num[j].a0 = num[j].a0 + ml[j] * w;
                den[j].a0 = den[j].a0 + w;
                cnt[j] += (w > 0.0f) ? 1 : 0;
            }
        }
    }

    // ---- per-sample loss and "positive" flag (PMVO.py:198-201)
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int it = j * T + tid;
        if (it < nitems) {
            float dn = mh_cascv_done(den[j]);
            float nm = mh_cascv_done(num[j]);
            int cn = cnt[j];
            if (it - (it / S) * S >= tail_from)   // a trailing column: the same terms in ATen's row_sum order
                mh_tail_item_sums(vw.cams, V, Hf, Wf, taps + (size_t)n * P1, (size_t)N * P1, nullptr, N, X0[j], X1[j], X2[j],
                                  nm, dn, cn);
            const float ratio = dn / (float)cn;
            s_pos[it] = (ratio > thr) ? 1 : 0;
            s_loss[it] = nm / dn;
        }
    }
    const bool all_nan = mh_point_pixel_not_finite(vw, P0, P1x, P2, N, tid, T);   // (its barrier covers s_loss / s_pos)

    // ---- per rank: low-confidence escape hatch, min / argmin over the S samples (PMVO.py:199-206)
    const int wave = tid >> 6, lane = tid & 63, nwaves = T >> 6;
    for (int r = wave; r < nrank; r += nwaves) {
        int npos = 0;
        for (int s0 = 0; s0 < S; s0 += MH_WAVE) {
            const int s = s0 + lane;
            npos += __popcll(__ballot(s < S && s_pos[r * S + s]));
        }
        const bool low = npos < 5;
        float bl = 0.0f;
        int bi = 0x7fffffff;
        for (int s = lane; s < S; s += MH_WAVE) {
            float l = all_nan ? __builtin_nanf("") : s_loss[r * S + s];
            if (!low && !s_pos[r * S + s]) l = 1.0f;
            if (bi == 0x7fffffff || mh_min_better(l, s, bl, bi)) {
                bl = l;
                bi = s;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ol = __shfl_xor(bl, o);
            const int oi = __shfl_xor(bi, o);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || mh_min_better(ol, oi, bl, bi))) {
                bl = ol;
                bi = oi;
            }
        }
        if (lane == 0) {
            s_rl[r] = bl;
            s_ri[r] = bi;
            s_rh[r] = s_pos[r * S + bi];
        }
    }
    __syncthreads();

    // ---- best candidate across base-view ranks (PMVO.py:57-70) and the 3D direction (:73-74)
    if (tid == 0) {
        const float Hf = (float)vw.H, Wf = (float)vw.W;
        float ml = s_rl[0];
        int br = 0, bs = s_ri[0], hc = s_rh[0];
        for (int r = 1; r < nrank; ++r) {
            const float l = s_rl[r];
            if ((l < ml) && (base_val[(size_t)(r * rank_step) * N + n] > 0.0f)) {
                ml = l;
                br = r;
                bs = s_ri[r];
                hc = s_rh[r];
            }
        }
        const int b = min(max(base_idx[(size_t)(br * rank_step) * N + n], 0), V - 1);
        const float2 oc = reinterpret_cast<const float2 *>(ori_c)[(size_t)b * N + n];
        float B0, B1, B2;
        mh_sample_next(vw.cams + b * MH_CAM_STRIDE, P0, P1x, P2, oc.x, oc.y, Hf, Wf, offs[bs], B0, B1, B2,
                       mh_group_forms(rule, br, V, b, S));
        const float d0 = B0 - P0, d1 = B1 - P1x, d2 = B2 - P2;
        float s2 = d0 * d0;
        s2 = mh_fma(d1, d1, s2);
        s2 = mh_fma(d2, d2, s2);
        const float nrm = __builtin_sqrtf(s2);
        line_ori[3 * n] = d0 / nrm;
        line_ori[3 * n + 1] = d1 / nrm;
        line_ori[3 * n + 2] = d2 / nrm;
        min_loss[n] = ml;
        high_conf[n] = (uint8_t)hc;
        if (best_sample) {
            best_sample[3 * n] = B0;
            best_sample[3 * n + 1] = B1;
            best_sample[3 * n + 2] = B2;
        }
        if (best_rank) best_rank[n] = br;
        if (best_s) best_s[n] = bs;
    }
}

// ---------------------------------------------------------------------------------------------
// Building blocks of the shipped search (mh_search3_kernel below).  What rounds 1-2 measured about the tap body
// (tools/ubench/valu2.hip, valu3.hip): plain v_mul/v_mul/v_add/v_sub are full-rate VALU operations (~2 cycles per
// wave-instruction) and overlap with the half-rate v_cmp / v_cndmask, the packed v_pk_mul/v_pk_add do not (82 -> 69 cycles
// per tap per 4 items); candidates of base-view ranks that can never be taken are not evaluated (ranks > 0 only replace the
// best-so-far when base_view_conf[rank] > 0, PMVO.py:64, and the ranking is sorted by that value, so the usable ranks are a
// prefix); every wave evaluates only the item slices it has (900 items = 15 wave-slices, not 16); workgroups take the points
// in descending order of work (order[], mh_search_order_kernel), so the tail of the launch is made of cheap points.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float mh_vmul(float a, float b) {
    float r;
    asm("v_mul_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float mh_vadd(float a, float b) {
    float r;
    asm("v_add_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// running minimum over the taps with first-index ties (strict '<', PMVO.py:177): compares of all items first, then the
// selects (gfx950 wants 2 wait states between a VALU write of an SGPR mask and a VALU read of it)
template <int KA>
__device__ __forceinline__ void mh_tap_update(float (&ML)[KA], float (&BC)[KA], const float (&l)[KA], float cf) {
    if constexpr (KA == 4) {
        unsigned long long m0, m1, m2, m3;
        asm("v_cmp_lt_f32_e64 %[m0], %[l0], %[a0]\n\t"
            "v_cmp_lt_f32_e64 %[m1], %[l1], %[a1]\n\t"
            "v_cmp_lt_f32_e64 %[m2], %[l2], %[a2]\n\t"
            "v_cmp_lt_f32_e64 %[m3], %[l3], %[a3]\n\t"
            "v_cndmask_b32_e64 %[a0], %[a0], %[l0], %[m0]\n\t"
            "v_cndmask_b32_e64 %[a1], %[a1], %[l1], %[m1]\n\t"
            "v_cndmask_b32_e64 %[a2], %[a2], %[l2], %[m2]\n\t"
            "v_cndmask_b32_e64 %[a3], %[a3], %[l3], %[m3]\n\t"
            "v_cndmask_b32_e64 %[b0], %[b0], %[cf], %[m0]\n\t"
            "v_cndmask_b32_e64 %[b1], %[b1], %[cf], %[m1]\n\t"
            "v_cndmask_b32_e64 %[b2], %[b2], %[cf], %[m2]\n\t"
            "v_cndmask_b32_e64 %[b3], %[b3], %[cf], %[m3]"
            : [a0] "+v"(ML[0]), [a1] "+v"(ML[1]), [a2] "+v"(ML[2]), [a3] "+v"(ML[3]), [b0] "+v"(BC[0]),
              [b1] "+v"(BC[1]), [b2] "+v"(BC[2]), [b3] "+v"(BC[3]), [m0] "=&s"(m0), [m1] "=&s"(m1), [m2] "=&s"(m2),
              [m3] "=&s"(m3)
            : [l0] "v"(l[0]), [l1] "v"(l[1]), [l2] "v"(l[2]), [l3] "v"(l[3]), [cf] "v"(cf));
    } else if constexpr (KA == 3) {
        unsigned long long m0, m1, m2;
        asm("v_cmp_lt_f32_e64 %[m0], %[l0], %[a0]\n\t"
            "v_cmp_lt_f32_e64 %[m1], %[l1], %[a1]\n\t"
            "v_cmp_lt_f32_e64 %[m2], %[l2], %[a2]\n\t"
            "v_cndmask_b32_e64 %[a0], %[a0], %[l0], %[m0]\n\t"
            "v_cndmask_b32_e64 %[a1], %[a1], %[l1], %[m1]\n\t"
            "v_cndmask_b32_e64 %[a2], %[a2], %[l2], %[m2]\n\t"
            "v_cndmask_b32_e64 %[b0], %[b0], %[cf], %[m0]\n\t"
            "v_cndmask_b32_e64 %[b1], %[b1], %[cf], %[m1]\n\t"
            "v_cndmask_b32_e64 %[b2], %[b2], %[cf], %[m2]"
            : [a0] "+v"(ML[0]), [a1] "+v"(ML[1]), [a2] "+v"(ML[2]), [b0] "+v"(BC[0]), [b1] "+v"(BC[1]),
              [b2] "+v"(BC[2]), [m0] "=&s"(m0), [m1] "=&s"(m1), [m2] "=&s"(m2)
            : [l0] "v"(l[0]), [l1] "v"(l[1]), [l2] "v"(l[2]), [cf] "v"(cf));
    } else if constexpr (KA == 2) {
        unsigned long long m0, m1;
        asm("v_cmp_lt_f32_e64 %[m0], %[l0], %[a0]\n\t"
            "v_cmp_lt_f32_e64 %[m1], %[l1], %[a1]\n\t"
            "s_nop 0\n\t"
            "v_cndmask_b32_e64 %[a0], %[a0], %[l0], %[m0]\n\t"
            "v_cndmask_b32_e64 %[a1], %[a1], %[l1], %[m1]\n\t"
            "v_cndmask_b32_e64 %[b0], %[b0], %[cf], %[m0]\n\t"
            "v_cndmask_b32_e64 %[b1], %[b1], %[cf], %[m1]"
            : [a0] "+v"(ML[0]), [a1] "+v"(ML[1]), [b0] "+v"(BC[0]), [b1] "+v"(BC[1]), [m0] "=&s"(m0), [m1] "=&s"(m1)
            : [l0] "v"(l[0]), [l1] "v"(l[1]), [cf] "v"(cf));
    } else {
#pragma unroll
        for (int j = 0; j < KA; ++j) {
            const bool upd = l[j] < ML[j];
            ML[j] = upd ? l[j] : ML[j];
            BC[j] = upd ? cf : BC[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The running minimum as ONE integer key per item (round 4; tools/ubench/valu5.hip: 69 -> 54 cycles per tap per 4 items).
// compute_prj_loss keeps, per (item, view), the lexicographic minimum of (loss_t, t) over the taps of the list -- tap 0
// seeds, a later tap replaces it only on a strictly smaller loss (PMVO.py:173-182) -- and wants the loss and the confidence
// of that tap.  loss_t = fl(1 - x), x = |cs_t|.  With C = 1 + 2^-14 the value t' = fl(C - x) is
//   * exactly loss_t + 2^-14 for 2^-14 < x: for x >= 0.5 both subtractions are exact (x is a multiple of 2^-24 there,
//     and |cs| <= 1 + 7 * 2^-24 for two vectors normalised in fp32, so t' > 0 where the loss itself goes negative); for
//     x < 0.5 both results lie in [0.5, 1), where the grid is 2^-24 and round-to-nearest-even commutes with adding the
//     even multiple 2^10 of the grid;
//   * a positive float in [2^-15, 2), whose bits all start 0b00111: (bits << 5) drops only those constant bits and is
//     monotone in t', which leaves five bits for a tap index.
// A list is walked in groups of 64 taps (one group for every patch up to 8 x 8); the even taps of a group fold into one
// accumulator, the odd taps into a second one, key = (bits(t') << 5) | (place of the tap among them, 0..31), two taps per
// v_min3_u32.  The group's first-index minimum is the odd accumulator's key if it is STRICTLY smaller than the even one's
// (equal loss and place: tap 2i is earlier than 2i + 1; equal loss, smaller place i' < i: 2i' + 1 < 2i), else the even
// one's; its tap = 2 * place + parity.  A later group replaces an earlier one only on a strictly smaller loss.  mul, mul,
// add, sub, lshl_or per evaluation + half a min3: 5.5 instructions instead of 7, two accumulators per item, one compare
// and two selects per (item, view) to merge them.
// The one-group kernels (patch <= 8 x 8: !BIGP) key the four-tap BLOCK instead of the tap (mh_key_blockm4): the tap's place is
// wanted once per (item, view), for the winner, and lshl_or, min3 and max3 issue at half the rate of mul / add / sub.  m = the
// minimum of the block's four t', key = (m << 4) | block (16 blocks of a 64-tap group; the top bit of the key, the last of the
// constant 0b00111, stays set), ONE accumulator per item, the key of a block kept until the next block folds both with one
// v_min3_u32.  An earlier block wins a tie in m by its smaller number.
// The block does not make four t': fl(C - x) is monotone non-increasing in x = |cs| and rounding keeps that order, so
//   min over the block's taps of fl(C - |cs_t|) == fl(C - max over the taps of |cs_t|)
// bit for bit, for every input.  The four cs as above (mul, mul, add each, the same order and bits), their maximum of |cs| with
// v_max_f32 (taps 0 and 2) and v_max3_f32 (taps 1 and 3), |.| as source modifiers, and ONE v_sub_f32: per block and item 13
// full-rate + max, max3, lshl_or + half a min3 = 3.5 half-rate instructions (16 + 3.5 with four subtractions and v_min_u32 /
// v_min3_u32 on the raw bits, tools/gen_key_blocks.py --form sub4; 16 + 6 with per-tap keys).  NaN: a NaN cs comes out of
// v_add_f32, so it is quiet, and v_max_f32 / v_max3_f32 return the other operand(s): the tap is ignored, as the raw bits of a
// NaN t' above every valid t' ignored it; four NaN taps give a NaN maximum, a NaN t' and a key >= MH_KEY_BAD, which matters
// only where it is the list's minimum.  (0, 0) records give |cs| = 0, which never raises a maximum; a block of them gives
// t' = C.  A denormal x gives C whether or not it is flushed.
// After the walk the lane reads the taps of ITS winning block again (per-lane LDS addresses), makes the t' of each -- the
// instructions of mh_key_tprime on the same operands -- and takes the first that equals m: the lexicographic minimum of
// (loss, tap) as before; two taps of different |cs| and the same loss are decided there, on t', not on |cs|.
// What the key cannot state -- a winner with x <= 2^-14 (t' >= 1 lands on the coarser grid of [1, 2)), a NaN -- shows as
// key >= MH_KEY_BAD (MH_KEY_BAD_TAP for the per-tap keys); a wave that sees one on any of its lanes evaluates that view again with the compare-and-select body
// (mh_tap_update), which is also what runs for one-tap lists and for a NaN seed tap.  Both bodies give the same bits
// wherever the key is valid, so the outputs are those of the select body everywhere.
// ---------------------------------------------------------------------------------------------
#define MH_KEY_C 1.00006103515625f   // 1 + 2^-14
#define MH_KEY_E 6.103515625e-05f    // 2^-14
#define MH_KEY_BAD 0xF8000000u       // block key of t' = 1.0 (block 0)
#define MH_KEY_BAD_TAP 0xF0000000u   // per-tap key of t' = 1.0 (place 0)
#ifndef MH_KEY_MIN_TAPS
#define MH_KEY_MIN_TAPS 10           // lists up to this length go through the select body directly
#endif
#define MH_KEY_PAD 4                 // the key block takes this many taps; (0, 0) records fill a last block: cs = 0, t' = C
#define MH_KEY_WALK_TAPS 49          // lists of this length (a complete 7 x 7 patch) take mh_key_walk instead of the loop over blocks
// How many taps of a list of c > MH_KEY_MIN_TAPS taps the key blocks walk, and how many tap records the list takes in LDS.
// Padded to whole blocks, a complete 7 x 7 patch (49 taps: 85 % of the bench scene's lists) ran a thirteenth block for one
// tap.  The LAST tap of a list does not need a block: its key is the initial value of the accumulator of its parity (a key
// carries its place, so the order in which it enters the minimum does not matter) -- 5 instructions per item + 2 selects
// in place of the two initialising moves, against the 22 per item of a block.  The blocks walk the c - 1 taps in front of it,
// padded to whole blocks -- always, without a branch on c & 3: one block less for c = 1 mod 4, the same blocks otherwise;
// where the padding reaches the last tap (c = 2, 3 mod 4) that tap is evaluated twice, to the same key.  (Seeding the last
// TWO taps, one even and one odd, needs no select and also saves the block of c = 2 mod 4, for 8 instead of 5 more
// instructions per item on every other list: the same speed on the bench scene within the noise, not kept.)  Lists of
// more than one 64-tap group (BIGP: patch 9 and 11) stay padded.
template <bool BIGP>
__device__ __forceinline__ int mh_key_walked(int c) {
    return (c - (BIGP ? 0 : 1) + MH_KEY_PAD - 1) & ~(MH_KEY_PAD - 1);
}
template <bool BIGP>
__device__ __forceinline__ int mh_key_staged(int c) {
    const int w = mh_key_walked<BIGP>(c);
    return w > c ? w : c;
}
// (wave, view) visits of the key body: [0] all, [1] one-tap / short / NaN-seed lists (select body directly), [2] evaluated
// again with the select body after the key body.  [2] is always counted -- one atomic in a branch the bench scene takes 0 times
// in 95 M -- so that a test can assert that it was inside that branch (tests/test_key_reeval_gpu.py); [0] and [1] sit in the
// hot path and are counted only in the -DMH_KEY_STATS build of tools/exp_key_stats.py.
__device__ unsigned long long mh_key_stats_dev[4];
extern "C" int mh_debug_key_stats(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mh_key_stats_dev), sizeof(unsigned long long) * 4) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[4] = {0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(mh_key_stats_dev), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#define MH_KEY_COUNT_ALWAYS(i) do { if ((tid & 63) == 0) atomicAdd(&mh_key_stats_dev[i], 1ull); } while (0)
#ifdef MH_KEY_STATS
#define MH_KEY_COUNT(i) MH_KEY_COUNT_ALWAYS(i)
#else
#define MH_KEY_COUNT(i) do { } while (0)
#endif
__device__ __forceinline__ float mh_key_tprime(float cs) {
    float t;
    asm("v_sub_f32_e64 %0, %2, |%1|" : "=v"(t) : "v"(cs), "s"(MH_KEY_C));
    return t;
}
// the block key of ONE tap (the seeded last tap of a list): its t' under the number of its block
__device__ __forceinline__ unsigned mh_seed_key(float cs, int blk) {
    const float t = mh_key_tprime(cs);
    unsigned k;
    asm("v_lshl_or_b32 %0, %1, 4, %2" : "=v"(k) : "v"(t), "s"(blk));
    return k;
}
__device__ __forceinline__ unsigned mh_min3u(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// Four taps x NI items of the per-tap key body as ONE hand-ordered block (mh_key_block4; the block-key body's mh_key_blockm4 is
// made the same way, two items at a time: with four the headline kernel spills -- per item 13 full-rate + max, max3, lshl_or and
// a min3 in every second block, no result of a pair of items read by the next instruction; see MH_KEY_C): per item 16 full-rate
// (mul, mul, add, sub) + 4 v_lshl_or + 2 v_min3 (88 instructions for four items), every result used at least NI - 1
// instructions after it is produced.  (Left to
// the compiler as one asm statement per instruction, its hazard recogniser pads every inline-asm result that is read by
// the very next instruction with an s_nop -- it cannot see that no dst_sel is involved: ~9 per block.)  The "memory"
// clobber keeps the LDS reads of the NEXT tap group, issued in front of the block, in front of it.
// (mh_key_blocks.h is written by tools/gen_key_blocks.py; tests/test_host.py compares the two.)
// Taps g[0], g[2] (places ib, ib + 1 among the even taps) go into ke, taps g[1], g[3] (the same places among the odd taps)
// into ko; the first NI entries of the caller's arrays are used.  (Padding lists to two taps instead of four, with a
// two-tap block for the tail, was measured: the choice between two asm blocks that update the same registers costs eight
// register copies and a wait for every LDS read per call -- 0.634 instead of 0.582 ms.)
// A list of exactly MH_KEY_WALK_TAPS taps (a complete 7 x 7 patch: 85 % of the bench scene's lists) does not loop over its blocks:
// mh_key_walk<12> is the twelve mh_key_blockm4 statements in a row, FOLD = false and FOLD = true in turn, the block's number and
// the offsets of its taps constants.  In the loop the waiting keys kk are copied between the registers of the two variants (KA
// copies per iteration and KA on the back edge), a v_mov_b32 v, s per group rebuilds the LDS address, and a counter, a compare and
// a branch sit around every block; in straight-line code kk stays where the FOLD = false statement wrote it, ONE base register
// serves every read through immediate offsets, and nothing is read past the list: 813 / 610 / 407 / 204 instead of 870 / 656 /
// 442 / 228 VALU instructions per (wave, view) visit for KA = 4 / 3 / 2 / 1, a third of the scalar instructions of the launch
// gone.  The reads stay C++ statements between the asm statements (their "memory" clobbers keep them in place; the compiler
// waits with lgkmcnt(2)): an asm operand is a whole register, and v_mul_f32 needs the halves of the pair a 64-bit read writes.
// Each path makes its own first reads and seed (the walk's at constant offsets): shared in front of the branch they cost the
// headline kernel six registers and a spill.  The kernels for more than 256 views keep the loop (the walk spills one value
// there).  profiles/search_walk.txt; tests/test_key_walk_gpu.py.
#include "mh_key_blocks.h"

// ---------------------------------------------------------------------------------------------
// mh_search3_kernel -- the shipped search: the arithmetic of mh_search_kernel in the same order, laid out for the machine.
// Where the wave-uniform tap records come from:
//   * round 2's first form read them with broadcast vector loads: every one of the 4 waves of the workgroup loaded every tap
//     record of every visible view (20.9 M wave-level loads per launch, 768 B of register return each through the CU's one
//     vector-memory path), and the first two loads of a view (first tap, first group) were waited for at full L2 latency;
//   * here the 256 threads copy the lists of the visible views into LDS once (coalesced 16-B loads, one copy per
//     workgroup instead of four), one barrier, and the tap loop reads them back with same-address ds_read (broadcast, no
//     bank conflict, ~100 cycles of latency that the ping-pong groups cover).  Lists that do not fit (MH_S3_CAP records)
//     go in several batches; the typical point (22 visible views x 46 taps) needs one.
//   * the visible views, their list lengths and LDS offsets come from the compact [V,N] byte array of list lengths: one
//     lane per view, a wave prefix sum, v_readlane -- no per-view header load, no branch on it.
// How the items are dealt to the waves: 256 lanes x up to 4 item slots, slice j of wave w = the items from j * 256 + w * 64, so
// 900 items (14 slices + 4 leftover items) are 4, 4, 3, 3 slices.  How a wave projects its items per view depends on what runs
// beside it (profiles/search_projection_plain.txt; this file is built with -fno-slp-vectorize, or the compiler packs the plain
// chains again and spills).  The KEY kernels project every item through the one-item forms (mh_pixel_of_fast1 / mh_unit2_fast1:
// plain registers, no v_pk_*_f32 anywhere in them): a projecting wave there shares its SIMD with waves in their key blocks, and
// beside those the packed chain of four items costs the SIMD 1103 cycles where four plain chains cost 819 (tools/ubench/
// proj_forms.hip) -- +0.8 % on the headline.  The SELECT-ONLY kernel (8-bit contexts: lists of 2.5 taps, three quarters of it
// projection) keeps the items two at a time (mh_pixel_of_fast2: v_pk_*_f32, the pair's divisions share their instructions) and
// only the ODD item of a 3- or 1-slice wave on the one-item twins: its waves project beside waves that project, where the packed
// form is the cheaper one (483 against 579 cycles); all items plain cost it 4 % (same file).  Both forms are the same operations
// in the same order: the same bits.
// The two 3-slice waves still end every staging batch a quarter early; a workgroup of 320 lanes x 3 slots (five waves of 3, 3,
// 3, 3, 2) was built against that and LOST 17 % (profiles/search_five_waves.txt): five waves do not spread evenly over a CU's
// four SIMDs, and the kernel runs at the pace of the fullest SIMD.
// ---------------------------------------------------------------------------------------------
#define MH_S3_GRP 4      // tap records per ping-pong group
#ifndef MH_S3_WAVES
#define MH_S3_WAVES 5   // waves per SIMD the register allocation aims at (A/B builds: -DMH_S3_WAVES=4|6)
#endif
#ifndef MH_S3_WAVES_SELECT
#define MH_S3_WAVES_SELECT MH_S3_WAVES   // the same aim for the select-only kernel (A/B builds: -DMH_S3_WAVES_SELECT=4)
#endif
#define MH_S3_CAP 1280   // float4 records per workgroup (20 KB; 6 workgroups of 25 KB per CU)

// the cascade of mh_device.h (MhCascV) with the third level only where it can be reached
template <bool BIG>
struct MhCascS {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    __device__ __forceinline__ void flush(int v) {   // v > 0, v % 16 == 0, before adding row v
        a1 = a1 + a0;
        a0 = 0.0f;
        if constexpr (BIG) {
            if ((v & 0xF0) == 0) {
                a2 = a2 + a1;
                a1 = 0.0f;
            }
        }
    }
    __device__ __forceinline__ float done() const { return BIG ? (a0 + a1) + a2 : (a0 + a1); }
};

// Inclusive prefix sum over the 64 lanes of a wave in the VALU's data path (DPP): four shifts inside every row of 16 lanes, then
// lane 15 of a row into the next row and lane 31 into the upper half -- no LDS round trip (six ds_bpermute_b32, each waited
// for, as __shfl_up gives it).  A lane a shift has no source for, and a row a broadcast is not meant for, adds 0.
__device__ __forceinline__ int mh_wave_prefix_sum(int x) {
#define MH_DPP_ADD(CTRL, ROWS) x += __builtin_amdgcn_update_dpp(0, x, CTRL, ROWS, 0xF, false)
    MH_DPP_ADD(0x111, 0xF);   // row_shr:1
    MH_DPP_ADD(0x112, 0xF);   // row_shr:2
    MH_DPP_ADD(0x114, 0xF);   // row_shr:4
    MH_DPP_ADD(0x118, 0xF);   // row_shr:8
    MH_DPP_ADD(0x142, 0xA);   // row_bcast:15 into rows 1 and 3
    MH_DPP_ADD(0x143, 0xC);   // row_bcast:31 into rows 2 and 3
#undef MH_DPP_ADD
    return x;
}

// the lane's index in its wave, made where it is asked for: what follows from it (an item, a global address) is then made
// there too, and is not a register kept across the view loops
__device__ __forceinline__ int mh_lane_now() {
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    return lane;
}

// One wave copies a tap list from global memory to dst in LDS (dst wave-uniform, both 16-byte aligned) with loads that write
// LDS themselves (global_load_lds_dwordx4: lane i's 16 bytes land at dst + 16 * i, no register result, no ds_write; retired
// by vmcnt): one instruction per 64 records, none of them waited for here -- the caller's next __syncthreads() is the wait.
// Records [0, nrec) come from src, records [nrec, nfill) are the neutral (0, 0) taps behind a key-body list
// (mh_key_staged), read from one zero record in global memory: an ordinary LDS store of zeros beside the copies in flight
// makes the compiler wait for every one of them first.
__device__ const float4 mh_zero_tap = {0.0f, 0.0f, 0.0f, 0.0f};
__device__ __forceinline__ void mh_stage_list(const float4 *__restrict__ src, float4 *dst, int nrec, int nfill, int lane) {
    for (int i0 = 0; i0 < nfill; i0 += 64) {
        const int i = i0 + lane;
        if (i < nfill) {
            const float4 *g = (i < nrec) ? src + i : &mh_zero_tap;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                             (__attribute__((address_space(3))) void *)(dst + i0), 16, 0, 0);
        }
    }
}

// Records of a list of c taps in LDS: header + taps (KEYS: behind the taps of a list that goes through the key body, the
// neutral (0, 0) records that fill its last block -- mh_key_staged); 0 for a view that does not see the point.
template <bool KEYS, bool BIGP>
__device__ __forceinline__ int mh_list_records(int c) {
    return c ? ((KEYS && c > MH_KEY_MIN_TAPS) ? mh_key_staged<BIGP>(c) : c) + 1 : 0;
}
// One batch of a 64-view block (views vb + the set bits of take; lane b holds view vb + b's taps c and the inclusive prefix
// sum pre of the lists' records, mh_list_records(c); base = records of the block's earlier batches): this wave issues the copies of the
// wave-th, wave + 4-th, ... list of the batch (a lane's place among the set bits of take), all in flight together.
template <int T, bool KEYS, bool BIGP>
__device__ __forceinline__ void mh_stage_batch(const float4 *__restrict__ taps, float4 *s_taps, int vb, int n, int N, int P1,
                                               int c, int pre, int base, unsigned long long take, int wave) {
    const int lane = mh_lane_now();   // (the lists' global addresses are made per batch)
    const unsigned place = __builtin_amdgcn_mbcnt_hi((unsigned)(take >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)take, 0u));
    unsigned long long m = take & __ballot((int)(place & (T / 64 - 1)) == wave);
    while (m) {
        const int b = (int)__builtin_ctzll(m);
        m &= m - 1;
        const int cb = __builtin_amdgcn_readlane(c, b);
        const int L = mh_list_records<KEYS, BIGP>(cb);
        const int off = __builtin_amdgcn_readlane(pre, b) - L - base;
        const int lr = cb + 1;   // records the list really has
        mh_stage_list(taps + ((size_t)(vb + b) * N + n) * P1, s_taps + off, lr, L, lane);
    }
}

// ---------------------------------------------------------------------------------------------
// The leftover items of a point: nact = nvalid * S items fill nact / 64 wave-slices and leave L = nact % 64 items (900 = 14
// slices + 4).  As a slice of their own they cost a wave every tap block of every visible view with 64 - L idle lanes.  For
// 0 < L <= MH_S3_LEFT_MAX they are not a slice: the workgroup's last wave -- which never has more full slices than any other --
// evaluates them one (item, view) PAIR per lane, per staging batch, in front of the batch's closing barrier, from the lists
// that are in LDS for the slices anyway (mh_left_batch), and adds a pair's terms up per item after the last batch
// (mh_left_sums) in the order and with the cascade of the slices.  A lane walks its own view's list with the
// compare-and-select arithmetic of the portable kernel (exact for every input: no key, no re-evaluation).
// LDS: (loss, weight) per (leftover item, view), the batch's visible views by place, the visible views per 64-view block --
// 4 640 B, 31 912 B per workgroup: five workgroups per CU as before.  Points with L * V > MH_S3_LEFT_PAIRS, L > MH_S3_LEFT_MAX
// or more than 256 views (the BIGV kernels) keep the slice, and so does the select-only kernel: the lists of 8-bit maps hold
// 2.5 taps on average, a slice costs little there and the pairs' fixed cost per pass lost 4 % (profiles/search_leftover.txt).
// ---------------------------------------------------------------------------------------------
#define MH_S3_LEFT_MAX 16      // 900, 450, 270 and 720 items leave 4, 2, 14 and 16; the next remainders (26, 28) are nearly half a slice
#define MH_S3_LEFT_PAIRS 544   // (leftover item, view) pairs that fit: L = 4 up to 136 views, L = 16 up to 34
struct MhLeft {
    float2 *pair;                // [L][V] (min loss, confidence of its tap)
    unsigned *view;              // [64] the batch's visible views by place: LDS record offset | taps << 11 | lane of the view << 18
    unsigned long long *vis;     // [4] visible views of every 64-view block
};

// One staging batch (views vb + the set bits of take, lane b holding view vb + b's taps c, records len and prefix sum pre, as in
// mh_search_slices_lds): the L leftover items x the batch's views, one pair per lane, lane = (place of the view << lg) | item
// with 2^lg >= L, in as many passes as that takes.
__device__ __forceinline__ void mh_left_batch(const float *__restrict__ cams, float Hf, float Wf, int V,
                                                        const float *__restrict__ offs, int S, const float4 *s_rank,
                                                        const float4 *s_taps, MhLeft lf, int nact, int L, int vb, int c,
                                                        int len, int pre, int base, unsigned long long take) {
    // (the lane and what follows from it -- the lane's item, its position -- are made here, per batch: hoisted in front of the
    // view loops they would be registers the slices' tap loops do not have)
    const int lane = mh_lane_now();
    const unsigned place = __builtin_amdgcn_mbcnt_hi((unsigned)(take >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)take, 0u));
    if ((take >> lane) & 1ull) lf.view[place] = (unsigned)(pre - len - base) | ((unsigned)c << 11) | ((unsigned)lane << 18);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int nv = __popcll(take);
    const int lg = L > 1 ? 32 - __builtin_clz((unsigned)(L - 1)) : 0;
    const int i = lane & ((1 << lg) - 1);
    const bool mine = i < L;
    const int it = nact - L + (mine ? i : 0);
    const int r = (int)(((unsigned)it * ((1u << 20) / (unsigned)S + 1u)) >> 20), s = it - r * S;   // (see mh_search_slices_lds)
    float X0, X1, X2;
    mh_sample_item(s_rank + 4 * r, offs[s], X0, X1, X2);
    for (int k0 = 0; k0 < nv; k0 += 64 >> lg) {
        const int k = k0 + (lane >> lg);
        const bool act = mine && k < nv;
        const unsigned e = lf.view[act ? k : k0];
        const int v = vb + (int)((e >> 18) & 63u);
        const int ntap = act ? (int)((e >> 11) & 127u) : 0;
        const float4 *rec = s_taps + (e & 2047u);
        const float4 hdr = rec[0];
        float row, col, dx, dy;
        mh_pixel_of(cams + v * MH_CAM_STRIDE, X0, X1, X2, Hf, Wf, row, col);
        mh_unit2(row - hdr.z, col - hdr.w, dx, dy);
        const float4 t0 = rec[1];
        float ml = 1.0f - __builtin_fabsf(t0.x * dx + t0.y * dy), bc = t0.z;
        // to the longest list among the lanes, four records in flight (up to three are read past a list's end: inside s_taps,
        // like the slices' last prefetch group)
        for (int t = 1; t < ntap; t += 4) {
            float4 g[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] = rec[1 + t + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float l = 1.0f - __builtin_fabsf(g[u].x * dx + g[u].y * dy);
                const bool upd = (t + u < ntap) && (l < ml);
                ml = upd ? l : ml;
                bc = upd ? g[u].z : bc;
            }
        }
        if (act) lf.pair[i * V + v] = float2{ml, bc};
    }
}

// After the last batch: lane i < L adds item nact - L + i's terms over the visible views in ascending order, flushing the
// cascade at every multiple of 16 below V as the slices do (V <= 256: two levels), and writes the item's loss and flag.
__device__ __forceinline__ void mh_left_sums(MhLeft lf, int V, int nact, int L, float thr, float *s_loss,
                                                       uint8_t *s_pos) {
    const int lane = mh_lane_now();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane >= L) return;
    MhCascS<false> num, den;
    int cnt = 0, nf = 16;
    for (int vb = 0; vb < V; vb += 64) {
        unsigned long long m = lf.vis[vb >> 6];
        while (m) {   // four views' terms in flight
            int v[4];
            float2 e[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = m ? vb + (int)__builtin_ctzll(m) : -1;
                m &= m - 1;
                e[u] = lf.pair[lane * V + (v[u] < 0 ? 0 : v[u])];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (v[u] < 0) break;
                for (; nf <= v[u]; nf += 16) {
                    num.flush(nf);
                    den.flush(nf);
                }
                const float w = e[u].y;   // (vis != -1) * best_conf
                num.a0 = num.a0 + e[u].x * w;
                den.a0 = den.a0 + w;
                cnt += (w > 0.0f) ? 1 : 0;
            }
        }
    }
    for (; nf <= V - 1; nf += 16) {
        num.flush(nf);
        den.flush(nf);
    }
    const int it = nact - L + lane;
    const float dn = den.done();
    const float nm = num.done();
    const float ratio = dn / (float)cnt;
    s_pos[it] = (ratio > thr) ? 1 : 0;
    s_loss[it] = nm / dn;
}

template <int KA, int T, bool BIGV, bool KEYS, bool BIGP, bool LEFT = false>
__device__ __forceinline__ void mh_search_slices_lds(const MhViews &vw, const float *__restrict__ offs, int S,
                                                     int n, int N, int P1, float thr,
                                                     const float4 *__restrict__ taps, const uint8_t *__restrict__ vcnt,
                                                     int nact, int tid, float *s_loss, uint8_t *s_pos, float4 *s_taps,
                                                     const float4 *s_rank, int c_first, int pre_first, MhLeft lf,
                                                     int left /* LEFT: the leftover items, which this wave evaluates (mh_left_batch) */) {
    constexpr int KN = KA > 0 ? KA : 1;   // a wave without items (KA == 0) only helps to stage the lists
    constexpr int KM = KA;
    const int V = vw.V;
    const float Hf = (float)vw.H, Wf = (float)vw.W;
    float X0[KN], X1[KN], X2[KN];
    // BIGV = more than 256 views: only then does the cascade of the weighted sums reach its third level (the level stays
    // +0 otherwise and x + (+0) = x for the non-negative sums: 8 registers less)
    MhCascS<BIGV> num[KN], den[KN];
    int cnt[KN];
    if constexpr (KA > 0) {
        const unsigned inv = (1u << 20) / (unsigned)S + 1u;   // it / S for it < 1024 >= S: (it * inv) >> 20 (error < 2^-10 <= 1/S)
#pragma unroll
        for (int j = 0; j < KA; ++j) {
            int it = j * T + tid;
            it = it < nact ? it : 0;
            const int r = (int)(((unsigned)it * inv) >> 20), s = it - r * S;
            mh_sample_item(s_rank + 4 * r, offs[s], X0[j], X1[j], X2[j]);   // (the rank part: mh_search3_kernel's prologue)
            num[j] = den[j] = MhCascS<BIGV>{};
            cnt[j] = 0;
        }
    }
    int nf = 16;   // next view index at which the cascade of the weighted sums is flushed (every multiple of 16 below V)
    auto flush_upto = [&](int v) {
        while (nf <= v) {
#pragma unroll
            for (int j = 0; j < KN; ++j) {
                num[j].flush(nf);
                den[j].flush(nf);
            }
            nf += 16;
        }
    };
    // one visible view: rec = its list in LDS (header, then ntap taps)
    auto one_view = [&](int v, const float4 *rec, int ntap) {
        const float *__restrict__ cam = vw.cams + v * MH_CAM_STRIDE;
        const float4 hdr = rec[0];
        const float4 t0 = rec[1];
        float DX[KN], DY[KN], ML[KN], BC[KN];
        if constexpr (KEYS) {
            // beside waves that are in a key block every item goes through the one-item forms (plain registers, no v_pk_*_f32:
            // this file is built without SLP packing); see the comment above mh_search3_kernel
#pragma unroll
            for (int j = 0; j < KA; ++j) {
                float row, col;
                mh_pixel_of_fast1(cam, X0[j], X1[j], X2[j], Hf, Wf, row, col);
                mh_unit2_fast1(row - hdr.z, col - hdr.w, DX[j], DY[j]);
            }
        } else {
            // the select-only kernel: two items at a time on register pairs, the odd item through the one-item twins
#pragma unroll
            for (int jp = 0; jp < KA / 2; ++jp) {
                mh_v2f row, col, dx, dy;
                mh_pixel_of_fast2(cam, mh_v2f{X0[2 * jp], X0[2 * jp + 1]}, mh_v2f{X1[2 * jp], X1[2 * jp + 1]},
                                  mh_v2f{X2[2 * jp], X2[2 * jp + 1]}, Hf, Wf, row, col);
                mh_unit2_fast2(row - mh_splat(hdr.z), col - mh_splat(hdr.w), dx, dy);
                DX[2 * jp] = dx.x;
                DX[2 * jp + 1] = dx.y;
                DY[2 * jp] = dy.x;
                DY[2 * jp + 1] = dy.y;
            }
            if constexpr (KA & 1) {
                float row, col;
                mh_pixel_of_fast1(cam, X0[KA - 1], X1[KA - 1], X2[KA - 1], Hf, Wf, row, col);
                mh_unit2_fast1(row - hdr.z, col - hdr.w, DX[KA - 1], DY[KA - 1]);
            }
        }
        constexpr int GRP = MH_S3_GRP;
        // the compare-and-select body: exact everywhere (the one body of rounds 1-3; with KEYS the re-evaluation path)
        auto select_body = [&]() {
#pragma unroll
            for (int j = 0; j < KA; ++j) {
                ML[j] = mh_one_minus_abs(mh_vadd(mh_vmul(t0.x, DX[j]), mh_vmul(t0.y, DY[j])));
                BC[j] = t0.z;
            }
            auto process = [&](const float4 (&g)[GRP], int t) {
#pragma unroll
                for (int u = 0; u < GRP; ++u) {
                    if (t + u < ntap) {   // uniform
                        const float4 tp = g[u];
                        float l[KN];
#pragma unroll
                        for (int j = 0; j < KA; ++j)
                            l[j] = mh_one_minus_abs(mh_vadd(mh_vmul(tp.x, DX[j]), mh_vmul(tp.y, DY[j])));
                        mh_tap_update<KN>(ML, BC, l, tp.z);
                    }
                }
            };
            float4 ga[GRP], gb[GRP];
#pragma unroll
            for (int u = 0; u < GRP; ++u) ga[u] = rec[2 + u];
            for (int t = 1; t < ntap;) {
#pragma unroll
                for (int u = 0; u < GRP; ++u) gb[u] = rec[1 + t + GRP + u];
                process(ga, t);
                t += GRP;
                if (t >= ntap) break;
#pragma unroll
                for (int u = 0; u < GRP; ++u) ga[u] = rec[1 + t + GRP + u];
                process(gb, t);
                t += GRP;
            }
        };
        __builtin_amdgcn_s_setprio(0);   // the tap loop: see mh_search3_kernel
        if constexpr (!KEYS) {
            select_body();
        } else {
            // the key body (see MH_KEY_C): taps in groups of 64, blocks of MH_KEY_PAD taps (see mh_key_walked)
            // uniform: a short list (the key body's fixed cost per view -- padding, decode -- only pays from about a dozen
            // taps on: lists of 8-bit maps are mostly shorter, lists of continuous maps hardly ever) / a NaN seed tap
            bool again = (ntap <= MH_KEY_MIN_TAPS) || !(t0.x == t0.x && t0.y == t0.y);
            MH_KEY_COUNT(0);
            if (again) MH_KEY_COUNT(1);
            if constexpr (!BIGP) {
              if (!again) {
                // patch <= 8x8, one 64-tap group: the block-key body (see mh_seed_key) -- one accumulator per item, the
                // key of a block in kk until the next block folds both with one v_min3_u32
                const int ntp = mh_key_walked<false>(ntap);
                unsigned acc[KN], kk[KN];
                const unsigned rec1 = (unsigned)(size_t)(const __attribute__((address_space(3))) float4 *)(rec + 1);
                static_assert(MH_KEY_PAD == 4 && GRP == 4, "the key block takes four taps");
                {
                    // (tx, ty) of tap i is the first half of record 1 + i
                    const float2 *__restrict__ t2 = reinterpret_cast<const float2 *>(rec + 1);
                    float2 ga[GRP], gb[GRP];
                    // block 0's taps; the list's last tap seeds the accumulator, under its own block's number
                    auto first = [&](int is) {
#pragma unroll
                        for (int u = 0; u < GRP; ++u) ga[u] = t2[2 * u];
                        const float2 ts = t2[2 * is];
#pragma unroll
                        for (int j = 0; j < KM; ++j)
                            acc[j] = mh_seed_key(mh_vadd(mh_vmul(ts.x, DX[j]), mh_vmul(ts.y, DY[j])), is >> 2);
                    };
                    // uniform: a complete 7 x 7 patch walks its twelve blocks as straight-line code (mh_key_walk; the kernels for
                    // more than 256 views spill with it and keep the loop)
                    if (!BIGV && ntap == MH_KEY_WALK_TAPS) {
                        first(MH_KEY_WALK_TAPS - 1);
                        if constexpr (KM > 0) mh_key_walk<(MH_KEY_WALK_TAPS - 1) / MH_KEY_PAD, KM, KN>(acc, ga, t2, DX, DY);
                    } else {
                        first(ntap - 1);
                        for (int t = 0; t < ntp;) {
#pragma unroll
                            for (int u = 0; u < GRP; ++u) gb[u] = t2[2 * (t + GRP + u)];
                            if constexpr (KM > 0) mh_key_blockm4<KM, KN, false>(acc, kk, ga, DX, DY, t >> 2);
                            t += GRP;
                            if (t >= ntp) {   // an odd number of blocks: the last one folds alone
#pragma unroll
                                for (int j = 0; j < KM; ++j) acc[j] = min(acc[j], kk[j]);
                                break;
                            }
#pragma unroll
                            for (int u = 0; u < GRP; ++u) ga[u] = t2[2 * (t + GRP + u)];
                            if constexpr (KM > 0) mh_key_blockm4<KM, KN, true>(acc, kk, gb, DX, DY, t >> 2);
                            t += GRP;
                        }
                    }
                }
                // decode: one compare for "any key past the valid range"; m = the key's upper bits with the constant 0b0011
                // back in front (v_alignbit), loss = m - 2^-14.  The winning TAP: the lane reads its winning block's four
                // (tx, ty) again, makes the four t' again -- the same instructions on the same operands, the same bits --
                // and takes the first that equals m (three of them: if none is, it is the fourth); then that tap's confidence from its record.  (A seed that wins under
                // the number of a block the walk did not reach, c = 1 mod 4, is that block's first tap: what lies behind
                // it in LDS is read and never chosen.)
                unsigned worst = acc[0];
#pragma unroll
                for (int j = 1; j < KM; ++j) worst = max(worst, acc[j]);
                const bool bad = worst >= MH_KEY_BAD;
                typedef const __attribute__((address_space(3))) mh_v2f *lds_f2;
                typedef const __attribute__((address_space(3))) float *lds_f1;
                // (two items at a time, a scheduling barrier between the pairs: all four at once hold 24 registers of taps)
#pragma unroll
                for (int j0 = 0; j0 < KM; j0 += 2) {
                    if (j0) __builtin_amdgcn_sched_barrier(0);
                    unsigned ad[2], mb[2];
                    mh_v2f w[2][3];
#pragma unroll
                    for (int j = j0; j < KM && j < j0 + 2; ++j) {
                        ad[j - j0] = rec1 + ((acc[j] & 15u) << 6);
                        mb[j - j0] = __builtin_amdgcn_alignbit(3u, acc[j], 4u);
#pragma unroll
                        for (int u = 0; u < 3; ++u) w[j - j0][u] = *reinterpret_cast<lds_f2>((size_t)(ad[j - j0] + 16u * u));
                    }
#pragma unroll
                    for (int j = j0; j < KM && j < j0 + 2; ++j) {
                        unsigned off = 56u;   // (the fourth tap, where none of the three in front of it is the one)
#pragma unroll
                        for (int u = 2; u >= 0; --u) {
                            const mh_v2f tp = w[j - j0][u];
                            const float tq = mh_key_tprime(mh_vadd(mh_vmul(tp.x, DX[j]), mh_vmul(tp.y, DY[j])));
                            off = (__float_as_uint(tq) == mb[j - j0]) ? 8u + 16u * u : off;
                        }
                        BC[j] = *reinterpret_cast<lds_f1>((size_t)(ad[j - j0] + off));
                        ML[j] = __uint_as_float(mb[j - j0]) - MH_KEY_E;
                    }
                }
                again = __ballot(bad) != 0ull;
                if (again) MH_KEY_COUNT_ALWAYS(2);
              }
            } else if (!again) {
                // patch 9 and 11: the per-tap keys
                const int ntp = mh_key_walked<BIGP>(ntap);
                // even taps of a 64-tap group into ke, odd taps into ko, the key's index = the tap's place among them
                unsigned ke[KN], ko[KN];
                const unsigned rec1 = (unsigned)(size_t)(const __attribute__((address_space(3))) float4 *)(rec + 1);
                auto process = [&](const float2 (&g)[GRP], int t) {
                    const int ib = (t & 63) >> 1;
                    static_assert(MH_KEY_PAD == 4 && GRP == 4, "the key block takes four taps");
                    if constexpr (KM > 0) mh_key_block4<KM, KN>(ke, ko, g, DX, DY, ib);
                };
                // taps [ta, tb) of one 64-tap group: (tx, ty) of tap i is the first half of record 1 + i
                auto group = [&](int ta, int tb) {
                    const float2 *__restrict__ t2 = reinterpret_cast<const float2 *>(rec + 1);
                    float2 ga[GRP], gb[GRP];
#pragma unroll
                    for (int u = 0; u < GRP; ++u) ga[u] = t2[2 * (ta + u)];
#pragma unroll
                    for (int j = 0; j < KN; ++j) ke[j] = ko[j] = 0xFFFFFFFFu;
                    for (int t = ta; t < tb;) {
#pragma unroll
                        for (int u = 0; u < GRP; ++u) gb[u] = t2[2 * (t + GRP + u)];
                        process(ga, t);
                        t += GRP;
                        if (t >= tb) break;
#pragma unroll
                        for (int u = 0; u < GRP; ++u) ga[u] = t2[2 * (t + GRP + u)];
                        process(gb, t);
                        t += GRP;
                    }
                };
                // the group's winner: the odd key only when it is strictly smaller (equal loss and place: the even tap is the
                // earlier one; equal loss, smaller place: 2i + 1 < 2i'); its tap = 2 * place + parity
                unsigned best[KN], badr[KN];   // winning key, LDS byte address of the winner's record
                auto winner = [&](int ta, bool first) {
#pragma unroll
                    for (int j = 0; j < KM; ++j) {
                        const bool odd = ko[j] < ke[j];
                        const unsigned kb = odd ? ko[j] : ke[j];
                        const unsigned ad = rec1 + 16u * (unsigned)ta + ((kb & 31u) << 5) + (odd ? 16u : 0u);
                        const bool take = first || kb < (best[j] & ~31u);   // a later group only on a strictly smaller loss
                        best[j] = take ? kb : best[j];
                        badr[j] = take ? ad : badr[j];
                    }
                };
                // patch 9 and 11: up to two groups (a later group wins only on a strictly smaller loss)
                group(0, ntp < 64 ? ntp : 64);
                winner(0, true);
                for (int ta = 64; ta < ntp; ta += 64) {
                    group(ta, ntp < ta + 64 ? ntp : ta + 64);
                    winner(ta, false);
                }
                // decode: one compare for "any key past the valid range", loss = t' - 2^-14 from the key's upper bits
                // (v_alignbit puts the constant 0b00111 back in front), confidence of the winning tap from its record
                unsigned worst = best[0];
#pragma unroll
                for (int j = 1; j < KM; ++j) worst = max(worst, best[j]);
                const bool bad = worst >= MH_KEY_BAD_TAP;
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    BC[j] = *reinterpret_cast<const __attribute__((address_space(3))) float *>((size_t)(badr[j] + 8u));
                    ML[j] = __uint_as_float(__builtin_amdgcn_alignbit(7u, best[j], 5u)) - MH_KEY_E;
                }
                again = __ballot(bad) != 0ull;
                if (again) MH_KEY_COUNT_ALWAYS(2);
            }
            if (again) select_body();
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < KA; ++j) {
            const float w = BC[j];   // (vis != -1) * best_conf
            num[j].a0 = num[j].a0 + ML[j] * w;
            den[j].a0 = den[j].a0 + w;
            cnt[j] += (w > 0.0f) ? 1 : 0;
        }
    };
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // list length of view vb + lane (0: the view does not see the point) and the inclusive prefix sum of the lists' records over
    // the lanes: the first block's were made in the kernel's prologue, which requested the lengths and staged that block's
    // first batch in front of its barrier (they are this loop's c and pre from the start: no registers of their own)
    int c = c_first, pre = pre_first;
    for (int vb = 0; vb < V; vb += 64) {
        if (vb) {
            const int vv = vb + lane;
            c = (vv < V) ? (int)vcnt[(size_t)vv * N + n] : 0;
            pre = mh_wave_prefix_sum(mh_list_records<KEYS, BIGP>(c));
        }
        bool staged = vb == 0;
        unsigned long long todo = __ballot(c != 0);
        int base = 0;
        if constexpr (LEFT) {
            if (left && lane == 0) lf.vis[vb >> 6] = todo;
        }
        while (todo) {
            // the next lists that fit together (pre is monotone: a prefix of the views left; one list always fits)
            const unsigned long long take = todo & __ballot(pre - base <= MH_S3_CAP);
            if (!staged) {
                mh_stage_batch<T, KEYS, BIGP>(taps, s_taps, vb, n, N, P1, c, pre, base, take, wave);
                __syncthreads();   // (waits for the copies: they count on vmcnt, and the barrier's fence drains it)
            }
            staged = false;
            if constexpr (KA > 0) {
                unsigned long long m = take;
                while (m) {
                    const int b = (int)__builtin_ctzll(m);
                    m &= m - 1;
                    flush_upto(vb + b);
                    const int cb = __builtin_amdgcn_readlane(c, b);   // (the list's records from its taps, on the scalar side:
                    const int L = mh_list_records<KEYS, BIGP>(cb);    // len is not a register of the tap loops)
                    const int off = __builtin_amdgcn_readlane(pre, b) - L - base;
                    one_view(vb + b, s_taps + off, cb);
                }
            }
            if constexpr (LEFT) {   // 
                if (left) mh_left_batch(vw.cams, Hf, Wf, V, offs, S, s_rank, s_taps, lf, nact, left, vb, c, mh_list_records<KEYS, BIGP>(c), pre, base, take);
            }
            __syncthreads();
            base = __builtin_amdgcn_readlane(pre, 63 - (int)__builtin_clzll(take));
            todo &= ~take;
        }
    }
    if constexpr (KA > 0) {
        flush_upto(V - 1);
#pragma unroll
        for (int j = 0; j < KA; ++j) {
            const int it = j * T + tid;
            if (it < nact) {
                const float dn = den[j].done();
                const float nm = num[j].done();
                const float ratio = dn / (float)cnt[j];
                s_pos[it] = (ratio > thr) ? 1 : 0;
                s_loss[it] = nm / dn;
            }
        }
    }
    if constexpr (LEFT) {
        if (left) mh_left_sums(lf, V, nact, left, thr, s_loss, s_pos);
    }
}

template <int T, bool BIGV, bool KEYS, bool BIGP>
// amdgpu_waves_per_eu(5): the register allocator stops at 96 VGPRs (it takes 109 unconstrained = 4 waves per SIMD); the
// few values it spills are reloaded once per view.  Measured: 4 waves 1305 it/s, 5 waves 1345, 6 waves (80 VGPRs) 1328.
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(KEYS ? MH_S3_WAVES : MH_S3_WAVES_SELECT))) void mh_search3_kernel(MhViews vw, const float *__restrict__ offs, int S, int nrank,
                                                       int rank_step, const float *__restrict__ pts, int N, int P1,
                                                       float thr, const float *__restrict__ ori_c,
                                                       const int32_t *__restrict__ base_idx,
                                                       const float *__restrict__ base_val,
                                                       const float4 *__restrict__ taps,
                                                       const uint8_t *__restrict__ vcnt,
                                                       const int32_t *__restrict__ order, float *__restrict__ line_ori,
                                                       float *__restrict__ min_loss, uint8_t *__restrict__ high_conf,
                                                       float *__restrict__ best_sample, int32_t *__restrict__ best_rank,
                                                       int32_t *__restrict__ best_s, MhRule rule) {
    __shared__ float4 s_taps[MH_S3_CAP + 8];   // (+8: the last prefetch group of a list reads past its end)
    __shared__ float s_loss[MH_MAX_ITEMS];
    __shared__ uint8_t s_pos[MH_MAX_ITEMS];
    __shared__ float s_rl[MH_MAX_RANKS];
    __shared__ int s_ri[MH_MAX_RANKS];
    __shared__ int s_rh[MH_MAX_RANKS];
    __shared__ float4 s_rank[MH_MAX_RANKS * 4];   // mh_sample_rank's record of every base-view rank
    __shared__ float s_bval[MH_MAX_RANKS];        // base_view_conf of the ranks
    __shared__ int s_tail;                        // first trailing sample of this point (mh_tail_from); S = none
    __shared__ float2 s_left[BIGV ? 1 : MH_S3_LEFT_PAIRS];   // the leftover items' terms (MhLeft)
    __shared__ unsigned s_lview[BIGV ? 1 : 64];
    __shared__ unsigned long long s_lvis[BIGV ? 1 : 4];

    // Wave priority: everything that is not the tap loop -- prologue, staging, the per-view projection, the epilogue -- runs
    // at priority 1, the tap loop at 0.  The tap loops saturate the VALU whatever the arbiter picks; the other phases are
    // chains of dependent long-latency operations (loads, LDS, rcp / sqrt) whose waves should get their instruction in as
    // soon as it is ready, so that they are back in a tap loop sooner: +5 % (the other way round: -8 %).
    __builtin_amdgcn_s_setprio(1);
    const int tid = threadIdx.x;
    const int n = order ? order[blockIdx.x] : (int)blockIdx.x;
    const float P0 = pts[3 * n], P1x = pts[3 * n + 1], P2 = pts[3 * n + 2];
    // what the S samples of a rank share (mh_sample_rank), once per (point, rank): lane r of the first wave -- for every
    // rank, usable or not, so that the rank's confidence, its base view, that view's centre orientation and camera are one
    // chain of loads per lane, all ranks in parallel (a scalar loop over base_view_conf first cost five more round trips
    // before the workgroup's first barrier)
    const int c_first = ((tid & 63) < vw.V) ? (int)vcnt[(size_t)(tid & 63) * N + n] : 0;   // (see mh_search_slices_lds)
    // the first batch of the first 64-view block goes to LDS from here (mh_search_slices_lds has the batches): the copies are
    // in flight while the rank records are made, and the barrier behind those waits for both
    const int len_first = mh_list_records<KEYS, BIGP>(c_first);
    const int pre_first = mh_wave_prefix_sum(len_first);
    mh_stage_batch<T, KEYS, BIGP>(taps, s_taps, 0, n, N, P1, c_first, pre_first, 0,
                            __ballot(c_first != 0) & __ballot(pre_first <= MH_S3_CAP),
                            __builtin_amdgcn_readfirstlane(tid >> 6));
    if (tid == 64) s_tail = mh_tail_from(rule, n, S);
    if (tid < nrank) {
        const size_t ro = (size_t)(tid * rank_step) * N + n;
        s_bval[tid] = base_val[ro];
        const int b = min(max(base_idx[ro], 0), vw.V - 1);   // (a caller's unusable ranks may carry any index)
        const float2 oc = reinterpret_cast<const float2 *>(ori_c)[(size_t)b * N + n];
        mh_sample_rank(vw.cams + b * MH_CAM_STRIDE, P0, P1x, P2, oc.x, oc.y, (float)vw.H, (float)vw.W,
                       reinterpret_cast<float *>(s_rank + 4 * tid), mh_group_forms(rule, tid, vw.V, b, S));
    }
    __syncthreads();
    // usable base-view ranks: rank 0 always, rank r > 0 only if base_view_conf[r] > 0 (PMVO.py:57-64); keep every rank up
    // to the last usable one
    int nvalid = 1;
    for (int r = 1; r < nrank; ++r)
        if (s_bval[r] > 0.0f) nvalid = r + 1;
    const int nact = nvalid * S;
    // the items behind the last full slice (mh_left_batch): not a slice of the wave they fall to but a job of the last wave
    const int nrest = __builtin_amdgcn_readfirstlane(nact & 63);   // (nact comes out of LDS: uniform, but in a vector register)
    const int nleft = (!BIGV && KEYS && nrest <= MH_S3_LEFT_MAX && nrest * vw.V <= MH_S3_LEFT_PAIRS) ? nrest : 0;
    const int wave0 = tid & ~63;   // first item of this wave in slice 0
    int ka = 0;
    for (int j = 0; j < 4; ++j) ka += (j * T + wave0 < nact - nleft) ? 1 : 0;
    const MhLeft lf{s_left, s_lview, s_lvis};
#define MH_S3_ARGS vw, offs, S, n, N, P1, thr, taps, vcnt, nact, tid, s_loss, s_pos, s_taps, s_rank, c_first, pre_first, lf, nleft
    if (!BIGV && wave0 == T - 64 && nleft) {   // the last wave, with the leftover items: it never has four slices
        if constexpr (!BIGV) {
            if (ka == 3) mh_search_slices_lds<3, T, BIGV, KEYS, BIGP, true>(MH_S3_ARGS);
            else if (ka == 2) mh_search_slices_lds<2, T, BIGV, KEYS, BIGP, true>(MH_S3_ARGS);
            else if (ka == 1) mh_search_slices_lds<1, T, BIGV, KEYS, BIGP, true>(MH_S3_ARGS);
            else mh_search_slices_lds<0, T, BIGV, KEYS, BIGP, true>(MH_S3_ARGS);
        }
    } else if (ka == 4) mh_search_slices_lds<4, T, BIGV, KEYS, BIGP>(MH_S3_ARGS);
    else if (ka == 3) mh_search_slices_lds<3, T, BIGV, KEYS, BIGP>(MH_S3_ARGS);
    else if (ka == 2) mh_search_slices_lds<2, T, BIGV, KEYS, BIGP>(MH_S3_ARGS);
    else if (ka == 1) mh_search_slices_lds<1, T, BIGV, KEYS, BIGP>(MH_S3_ARGS);
    else mh_search_slices_lds<0, T, BIGV, KEYS, BIGP>(MH_S3_ARGS);
#undef MH_S3_ARGS
    __syncthreads();
    // ---- the trailing columns of the batch's [V, N*S] sums (samples >= s_tail of the batch's last point(s); s_tail == S, i.e.
    // none, in every other workgroup): ATen adds those in its row_sum order -- their losses once more, that way
    if (s_tail < S) {   // uniform
        const int tail_from = s_tail;
        for (int it = tid; it < nact; it += T) {
            const int r = it / S, s = it - r * S;
            if (s < tail_from) continue;
            float X0, X1, X2, nm, dn;
            int cnt;
            mh_sample_item(s_rank + 4 * r, offs[s], X0, X1, X2);
            mh_tail_item_sums(vw.cams, vw.V, (float)vw.H, (float)vw.W, taps + (size_t)n * P1, (size_t)N * P1, vcnt + n, N, X0, X1,
                              X2, nm, dn, cnt);
            s_pos[it] = (dn / (float)cnt > thr) ? 1 : 0;
            s_loss[it] = nm / dn;
        }
        __syncthreads();
    }

    const bool all_nan = mh_point_pixel_not_finite(vw, P0, P1x, P2, N, tid, T);
    // ---- per rank: low-confidence escape hatch, min / argmin over the S samples (PMVO.py:199-206)
    const int wave = tid >> 6, lane = tid & 63, nwaves = T >> 6;
    for (int r = wave; r < nvalid; r += nwaves) {
        int npos = 0;
        for (int s0 = 0; s0 < S; s0 += MH_WAVE) {
            const int s = s0 + lane;
            npos += __popcll(__ballot(s < S && s_pos[r * S + s]));
        }
        const bool low = npos < 5;
        float bl = 0.0f;
        int bi = 0x7fffffff;
        for (int s = lane; s < S; s += MH_WAVE) {
            float l = all_nan ? __builtin_nanf("") : s_loss[r * S + s];
            if (!low && !s_pos[r * S + s]) l = 1.0f;
            if (bi == 0x7fffffff || mh_min_better(l, s, bl, bi)) {
                bl = l;
                bi = s;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ol = __shfl_xor(bl, o);
            const int oi = __shfl_xor(bi, o);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || mh_min_better(ol, oi, bl, bi))) {
                bl = ol;
                bi = oi;
            }
        }
        if (lane == 0) {
            s_rl[r] = bl;
            s_ri[r] = bi;
            s_rh[r] = s_pos[r * S + bi];
        }
    }
    __syncthreads();

    // ---- best candidate across base-view ranks (PMVO.py:57-70) and the 3D direction (:73-74)
    if (tid == 0) {
        float ml = s_rl[0];
        int br = 0, bs = s_ri[0], hc = s_rh[0];
        for (int r = 1; r < nvalid; ++r) {
            const float l = s_rl[r];
            if ((l < ml) && (s_bval[r] > 0.0f)) {
                ml = l;
                br = r;
                bs = s_ri[r];
                hc = s_rh[r];
            }
        }
        float B0, B1, B2;
        mh_sample_item(s_rank + 4 * br, offs[bs], B0, B1, B2);
        const float d0 = B0 - P0, d1 = B1 - P1x, d2 = B2 - P2;
        float s2 = d0 * d0;
        s2 = mh_fma(d1, d1, s2);
        s2 = mh_fma(d2, d2, s2);
        const float nrm = __builtin_sqrtf(s2);
        line_ori[3 * n] = d0 / nrm;
        line_ori[3 * n + 1] = d1 / nrm;
        line_ori[3 * n + 2] = d2 / nrm;
        min_loss[n] = ml;
        high_conf[n] = (uint8_t)hc;
        if (best_sample) {
            best_sample[3 * n] = B0;
            best_sample[3 * n + 1] = B1;
            best_sample[3 * n + 2] = B2;
        }
        if (best_rank) best_rank[n] = br;
        if (best_s) best_s[n] = bs;
    }
}

// A batch of ONE candidate in all (N == 1 and S == 1): the reference's tensors are [V, 1], and two of its steps take other forms
// there (oracle/pmvo_oracle.c: batch_is_single, tail_from_of).  compute_reproject_ori projects the sample, like the point,
// through the single-column sgemm (single: option reproject_rule 0), and the sums over the views are ATen's sums over a
// contiguous innermost dimension, not outer sums (inner_sum: option sum_block > 0; mh_inner_sum_views, as in the refine
// kernels).  mh_launch_search sends this shape here and the search kernels above never see it.  One wave: the usable ranks
// one after the other, a view per lane with the portable kernel's tap walk, then every lane the same sums over the views.
__global__ __launch_bounds__(64) void mh_search_one_column_kernel(MhViews vw, const float *__restrict__ offs, int nrank,
                                                                  int rank_step, const float *__restrict__ pts, int P1, float thr,
                                                                  const float *__restrict__ ori_c,
                                                                  const int32_t *__restrict__ base_idx,
                                                                  const float *__restrict__ base_val,
                                                                  const float4 *__restrict__ taps,
                                                                  const uint8_t *__restrict__ vcnt /* may be null */,
                                                                  float *__restrict__ line_ori, float *__restrict__ min_loss,
                                                                  uint8_t *__restrict__ high_conf, float *__restrict__ best_sample,
                                                                  int32_t *__restrict__ best_rank, int32_t *__restrict__ best_s,
                                                                  MhRule rule, int single, int inner_sum) {
    extern __shared__ float s_term[];   // [2][V]: (loss x weight, weight) of every view
    const int lane = threadIdx.x, V = vw.V;
    const float Hf = (float)vw.H, Wf = (float)vw.W;
    const float P0 = pts[0], P1x = pts[1], P2 = pts[2];
    const bool all_nan = mh_point_pixel_not_finite(vw, P0, P1x, P2, 1, lane, 64);
    float ml = 0.0f, B0 = 0.0f, B1 = 0.0f, B2 = 0.0f;
    int br = 0, hc = 0;
    for (int r = 0; r < nrank; ++r) {
        if (r > 0 && !(base_val[r * rank_step] > 0.0f)) continue;   // (PMVO.py:64 never takes such a rank; uniform)
        const int b = min(max(base_idx[r * rank_step], 0), V - 1);
        const float2 oc = reinterpret_cast<const float2 *>(ori_c)[b];
        float X0, X1, X2;
        mh_sample_next(vw.cams + b * MH_CAM_STRIDE, P0, P1x, P2, oc.x, oc.y, Hf, Wf, offs[0], X0, X1, X2,
                       mh_group_forms(rule, r, V, b, 1));
        for (int v = lane; v < V; v += MH_WAVE) {
            float tn = 0.0f, td = 0.0f;
            const float4 *__restrict__ rec = taps + (size_t)v * P1;
            const float4 hdr = rec[0];
            const int ntap = vcnt ? (int)vcnt[v] : __float_as_int(hdr.x);
            if (ntap != 0 && hdr.y != -1.0f) {
                float row, col, dx, dy;
                mh_pixel_of_b(vw.cams + v * MH_CAM_STRIDE, X0, X1, X2, Hf, Wf, row, col, single != 0);
                mh_unit2(row - hdr.z, col - hdr.w, dx, dy);
                const float4 t0 = rec[1];
                float l0 = 1.0f - __builtin_fabsf(t0.x * dx + t0.y * dy), bc = t0.z;
                for (int t = 1; t < ntap; ++t) {
                    const float4 tp = rec[1 + t];
                    const float l = 1.0f - __builtin_fabsf(tp.x * dx + tp.y * dy);
                    const bool upd = l < l0;
                    l0 = upd ? l : l0;
                    bc = upd ? tp.z : bc;
                }
                tn = l0 * bc;
                td = bc;
            }
            s_term[v] = tn;
            s_term[V + v] = td;
        }
        __syncthreads();
        int cnt = 0;
        for (int v = 0; v < V; ++v) cnt += (s_term[V + v] > 0.0f) ? 1 : 0;
        float nm, dn;
        if (inner_sum) {
            nm = mh_inner_sum_views(V, [&](int v) { return s_term[v]; });
            dn = mh_inner_sum_views(V, [&](int v) { return s_term[V + v]; });
        } else {   // the cascade of the outer sums, as the search kernels add the views
            MhCascV num = {0.0f, 0.0f, 0.0f}, den = {0.0f, 0.0f, 0.0f};
            for (int v = 0; v < V; ++v) {
                if (v > 0 && (v & 15) == 0) {
                    mh_cascv_flush(num, v);
                    mh_cascv_flush(den, v);
                }
                num.a0 = num.a0 + s_term[v];
                den.a0 = den.a0 + s_term[V + v];
            }
            nm = mh_cascv_done(num);
            dn = mh_cascv_done(den);
        }
        __syncthreads();
        // one sample: fewer than five positive ones, the low-confidence rule keeps its loss (PMVO.py:199-206)
        const float l = all_nan ? __builtin_nanf("") : nm / dn;
        if (r == 0 || l < ml) {
            ml = l;
            br = r;
            hc = (dn / (float)cnt > thr) ? 1 : 0;
            B0 = X0;
            B1 = X1;
            B2 = X2;
        }
    }
    if (lane == 0) {
        const float d0 = B0 - P0, d1 = B1 - P1x, d2 = B2 - P2;
        float s2 = d0 * d0;
        s2 = mh_fma(d1, d1, s2);
        s2 = mh_fma(d2, d2, s2);
        const float nrm = __builtin_sqrtf(s2);
        line_ori[0] = d0 / nrm;
        line_ori[1] = d1 / nrm;
        line_ori[2] = d2 / nrm;
        min_loss[0] = ml;
        high_conf[0] = (uint8_t)hc;
        if (best_sample) {
            best_sample[0] = B0;
            best_sample[1] = B1;
            best_sample[2] = B2;
        }
        if (best_rank) best_rank[0] = br;
        if (best_s) best_s[0] = 0;
    }
}

// Launch order of the search: points sorted by descending work = (taps of the views that see the point) x (item slices
// it needs).  mh_search_work_kernel: one lane per point -> work class (0 = heaviest) in order[0..N);
// mh_search_order_kernel: one workgroup -- histogram of the MH_ORDER_BUCKETS classes, exclusive scan, scatter of the
// point indices into order[N..2N).  The order inside a class is whatever the atomics give: it only decides WHEN a
// point is processed, never what is computed for it.
__global__ __launch_bounds__(256) void mh_search_work_kernel(const uint8_t *__restrict__ cnt, int V, int N, int P1,
                                                             const float *__restrict__ base_val, int nrank,
                                                             int rank_step, int S, int T, int32_t *__restrict__ order,
                                                             int tail_n0) {
    // one wave per point: lanes over the views (list lengths, 0 for views that do not see the point) and over the ranks
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + wave;
    if (n >= N) return;
    int nt = 0;
    for (int v = lane; v < V; v += MH_WAVE) nt += cnt[(size_t)v * N + n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nt += __shfl_xor(nt, o);
    const bool usable = lane > 0 && lane < nrank && base_val[(size_t)(lane * rank_step) * N + n] > 0.0f;
    const unsigned long long m = __ballot(usable);
    const int nvalid = m ? (64 - __builtin_clzll(m)) : 1;   // last usable rank + 1
    if (lane == 0) order[n] = n >= tail_n0 ? 0 : mh_work_class(nt, nvalid, V, P1, S, T);   // (MhWorkArgs::tail_n0)
}

// Points per (rank, base view) of the batch -- the M of mh_group_forms: gcnt[r * V + b] = #{n : base_idx[r * rank_step, n] == b}.
// Workgroup (x, r) counts 256 points of rank r in LDS and adds its non-zero cells to the zeroed global array.  (The fused
// forward does not launch this: its ranking kernel adds the counts itself, mh_topk_wave_kernel.  A first form -- one
// workgroup, all ranks, inside mh_search_order_kernel -- took 146 us at the headline size: up to 670 LDS atomics on one address.)
__global__ __launch_bounds__(256) void mh_group_sizes_kernel(const int32_t *__restrict__ base_idx, int N, int V,
                                                             int rank_step, int32_t *__restrict__ gcnt) {
    extern __shared__ int s_g[];   // V
    const int r = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < V; i += 256) s_g[i] = 0;
    __syncthreads();
    const int n = blockIdx.x * 256 + tid;
    if (n < N) {
        const int b = base_idx[(size_t)(r * rank_step) * N + n];
        if (b >= 0 && b < V) atomicAdd(&s_g[b], 1);
    }
    __syncthreads();
    for (int i = tid; i < V; i += 256)
        if (s_g[i]) atomicAdd(&gcnt[(((int)blockIdx.x & (MH_GROUP_COPIES - 1)) * MH_GROUP_RANKS + r) * V + i], s_g[i]);
}

__global__ __launch_bounds__(1024) void mh_search_order_kernel(int N, int32_t *__restrict__ order) {
    __shared__ int s_hist[MH_ORDER_BUCKETS];
    __shared__ int s_part[1024 / 64];
    const int tid = threadIdx.x;
    s_hist[tid] = 0;
    __syncthreads();
    for (int n = tid; n < N; n += 1024) atomicAdd(&s_hist[order[n]], 1);
    __syncthreads();
    const int mine = s_hist[tid];   // lane = class
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(incl, o);
        if ((tid & 63) >= o) incl += x;
    }
    if ((tid & 63) == 63) s_part[tid >> 6] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < (tid >> 6); ++w) base += s_part[w];
    __syncthreads();
    s_hist[tid] = base + incl - mine;   // first position of this class
    __syncthreads();
    for (int n = tid; n < N; n += 1024) order[N + atomicAdd(&s_hist[order[n]], 1)] = n;
}

// ---------------------------------------------------------------------------------------------
extern "C" int mh_launch_search(MhViews vw, const float *offs, int S, int nrank, int rank_step, const float *pts,
                                int N, int P1, float thr, const float *ori_c, const int32_t *base_idx,
                                const float *base_val, const float4 *taps, int32_t *order /* 2N ints of work space */,
                                const uint8_t *cnt /* [V,N] list lengths */,
                                float *line_ori, float *min_loss, uint8_t *high_conf, float *best_sample,
                                int32_t *best_rank, int32_t *best_s, MhSearchPlan plan, int rule_mode, int fma_min_cols,
                                int sum_block, int32_t *gcnt /* MH_GROUP_COPIES * MH_GROUP_RANKS * V ints of work space */,
                                int groups_ready /* gcnt holds the batch's group sizes already (the fused forward) */,
                                hipStream_t st) {
    const int nitems = nrank * S;
    if (nitems > MH_MAX_ITEMS || nrank > MH_MAX_RANKS || nitems < 1) return -1;
    // the batch in the arithmetic (MhRule, mh_device.h): group sizes per (rank, base view) and the trailing columns of the
    // [V, N*S] sums.  rule_mode 0 needs gcnt (the C API hands it out of its scratch).
    if (sum_block < 0) return -1;
    MhRule rule;
    rule.mode = rule_mode;
    rule.fma_min_cols = fma_min_cols;
    rule.gcnt = (rule_mode == 0) ? gcnt : nullptr;
    if (rule_mode == 0 && !gcnt) return -1;
    const long long cols = (long long)N * S;
    rule.tail_col0 = sum_block ? cols - cols % sum_block : cols;
    const bool portable = plan.portable || !cnt;   // (mh_search3_kernel needs the list lengths)
    // the group sizes, unless the caller counted them or an earlier PART_PRE_ONLY launch left them in gcnt
    if (rule.gcnt && !groups_ready && plan.part != MhSearchPlan::PART_KERNEL_ONLY) {
        if (hipMemsetAsync(gcnt, 0, sizeof(int32_t) * (size_t)MH_GROUP_COPIES * MH_GROUP_RANKS * vw.V, st) != hipSuccess) return -1;
        hipLaunchKernelGGL(mh_group_sizes_kernel, dim3((N + 255) / 256, nrank), dim3(256), sizeof(int) * (size_t)vw.V, st,
                           base_idx, N, vw.V, rank_step, gcnt);
    }
    // a batch of one candidate in all: its own forms (mh_search_one_column_kernel)
    if ((long long)N * S == 1 && (rule_mode == 0 || sum_block > 0) && plan.part != MhSearchPlan::PART_PRE_ONLY) {
        hipLaunchKernelGGL(mh_search_one_column_kernel, dim3(1), dim3(64), 2 * sizeof(float) * (size_t)vw.V, st, vw, offs, nrank,
                           rank_step, pts, P1, thr, ori_c, base_idx, base_val, taps, cnt, line_ori, min_loss, high_conf,
                           best_sample, best_rank, best_s, rule, rule_mode == 0 ? 1 : 0, sum_block > 0 ? 1 : 0);
        return (int)hipGetLastError();
    }
    if (!portable) {
        // the launch order: work classes into order[0..N) unless the caller wrote them, then the points by class into order[N..2N)
        const int32_t *ord = nullptr;
        if (plan.order != MhSearchPlan::ORDER_NATURAL && order && N > 1) {
            if (plan.part != MhSearchPlan::PART_KERNEL_ONLY) {
                if (plan.order == MhSearchPlan::ORDER_BY_WORK)
                    hipLaunchKernelGGL(mh_search_work_kernel, dim3((N + 3) / 4), dim3(256), 0, st, cnt, vw.V, N, P1, base_val,
                                       nrank, rank_step, S, 256, order, (int)(rule.tail_col0 / S));
                hipLaunchKernelGGL(mh_search_order_kernel, dim3(1), dim3(1024), 0, st, N, order);
            }
            ord = order + N;
        }
        if (plan.part == MhSearchPlan::PART_PRE_ONLY) return (int)hipGetLastError();
#define MH_S3_LAUNCH(BIG, KEYS, BIGP)                                                                                   \
    hipLaunchKernelGGL((mh_search3_kernel<256, BIG, KEYS, BIGP>), dim3(N), dim3(256), 0, st, vw, offs, S, nrank, rank_step, \
                       pts, N, P1, thr, ori_c, base_idx, base_val, taps, cnt, ord, line_ori, min_loss, high_conf,       \
                       best_sample, best_rank, best_s, rule)
        // (the key kernel for lists of up to 64 taps -- every patch up to 8 x 8 -- keeps two key registers per item; the one
        // for longer lists two more)
        const bool bigp = P1 - 1 > 64;
        if (vw.V > 256) {
            if (plan.select_body) MH_S3_LAUNCH(true, false, false);
            else if (bigp) MH_S3_LAUNCH(true, true, true);
            else MH_S3_LAUNCH(true, true, false);
        } else {
            if (plan.select_body) MH_S3_LAUNCH(false, false, false);
            else if (bigp) MH_S3_LAUNCH(false, true, true);
            else MH_S3_LAUNCH(false, true, false);
        }
#undef MH_S3_LAUNCH
    } else {
        hipLaunchKernelGGL((mh_search_kernel<4, 256>), dim3(N), dim3(256), 0, st, vw, offs, S, nrank, rank_step, pts, N, P1,
                           thr, ori_c, base_idx, base_val, taps, line_ori, min_loss, high_conf, best_sample, best_rank,
                           best_s, rule);
    }
    return (int)hipGetLastError();
}

// forces this translation unit's code object onto the device (HIP loads a fat binary on the first use of one of its kernels:
// 2-20 ms each, which a one-shot pass would pay in the middle of its stages); called from mh_ctx_create
extern "C" int mh_preload_pmvo_search() {
    hipFuncAttributes a;
    return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&mh_search_order_kernel));
}
