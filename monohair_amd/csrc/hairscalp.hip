// Scalp attachment of HairGrow.py (connect_to_scalp :606-784 with compute_strands_similar :788-812, the push_back=False /
// add_mid=False branch of connect_strands :384-416 and random_move_strands, Utils/PMVO_utils.py:618-658): ONE pass of the
// reference's while loop.  Inside a pass the floating strands are independent: the core set (the strands rooted when the
// pass starts) is read-only, and a strand writes only its own points, flags and out_ratio.
//
//   mh_scalp_ball_count_kernel   members of KDTree(core).query_ball_point(strand[0], thr_dist) per floating strand
//   mh_scalp_choose_kernel       the ball in the order scipy returns it, the flip test, the candidate loop and the choice
//   mh_scalp_emit_kernel         every strand copied to its new place (reversed if flipped); a chosen join is built in
//                                front of it and put through the occupancy / orientation check
//
// One wave per strand.  query_ball_point returns the points with float64 distance <= r in ascending position in
// tree.indices, so no kd-tree is needed: the caller hands in rank[tree.indices[j]] = j and the ball is ordered by it.
// Strands are float32; nearest points and the ball are float64 as scipy computes them, compute_similar / the loss are
// float32 as numpy 2 promotes them, the loss plus out_ratio[neighbour] is float64.  -ffp-contract=off: nothing is fused.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_device.h"

#define MH_SC_FIRSTBIT 0x8000000000000000ull   // set on a ball member that is NOT the lowest rank of its strand

struct MhScalpGrid {   // uniform grid over the core points (mh_grid_build): cells no smaller than thr_dist
    const int32_t *order, *cstart;
    float ox, oy, oz, h;
    int dx, dy, dz;
};

__device__ __forceinline__ unsigned long long mh_sc_min_u64(unsigned long long v) {
    for (int s = 1; s < MH_WAVE; s <<= 1) {
        const unsigned long long o = __shfl_xor(v, s);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ double mh_sc_sum_f64(double v) {
    for (int s = 1; s < MH_WAVE; s <<= 1) v += __shfl_xor(v, s);
    return v;
}

// calls fn(is_member, core index) for every slot of the 27 cells around q, all lanes together (wave-uniform trip count).
// Membership is scipy's: ((d0*d0 + d1*d1) + d2*d2) <= r*r in float64, bound included.
template <class F>
__device__ __forceinline__ void mh_sc_ball_scan(const float *__restrict__ core, MhScalpGrid g, float qx, float qy,
                                                float qz, double r2, int lane, F fn) {
    const int cx = mh_grid_cell(qx, g.ox, g.h, g.dx), cy = mh_grid_cell(qy, g.oy, g.h, g.dy),
              cz = mh_grid_cell(qz, g.oz, g.h, g.dz);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dx - 1);
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.dz - 1); ++z)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.dy - 1); ++y) {
            const int row = (z * g.dy + y) * g.dx;
            const int s0 = g.cstart[row + x0], s1 = g.cstart[row + x1 + 1];   // cells x0..x1 are one contiguous range
            for (int base = s0; base < s1; base += MH_WAVE) {
                const int s = base + lane;
                bool in = false;
                int j = 0;
                if (s < s1) {
                    j = g.order[s];
                    const double d0 = (double)qx - (double)core[3 * (size_t)j],
                                 d1 = (double)qy - (double)core[3 * (size_t)j + 1],
                                 d2 = (double)qz - (double)core[3 * (size_t)j + 2];
                    in = ((d0 * d0 + d1 * d1) + d2 * d2) <= r2;
                }
                fn(in, j);
            }
        }
}

__global__ __launch_bounds__(256) void mh_scalp_ball_count_kernel(const float *__restrict__ P,
                                                                  const int64_t *__restrict__ offs,
                                                                  const int32_t *__restrict__ act, int nact,
                                                                  const float *__restrict__ core, MhScalpGrid g, double r2,
                                                                  int64_t *__restrict__ count) {
    const int a = blockIdx.x * (blockDim.x / MH_WAVE) + (threadIdx.x / MH_WAVE), lane = threadIdx.x & (MH_WAVE - 1);
    if (a >= nact) return;
    const float *q = P + 3 * offs[act[a]];
    int n = 0;
    mh_sc_ball_scan(core, g, q[0], q[1], q[2], r2, lane, [&](bool in, int) { n += __popcll(__ballot(in)); });
    if (lane == 0) count[a] = n;
}

// KDTree(strand).query(p, 1): squared distance and index of the nearest of the L points at S, the lanes sharing the points;
// the lower index wins an exact tie (scipy's answer at a tie follows its tree layout: the fixtures and sweeps hold none)
__device__ __forceinline__ void mh_sc_nearest(const float *__restrict__ S, int L, float px, float py, float pz, int lane,
                                              double &dmin, int &imin) {
    double m = __builtin_inf();
    int mi = 0x7fffffff;
    for (int k = lane; k < L; k += MH_WAVE) {
        const double d0 = (double)px - (double)S[3 * k], d1 = (double)py - (double)S[3 * k + 1],
                     d2 = (double)pz - (double)S[3 * k + 2];
        const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
        if (dd < m) {
            m = dd;
            mi = k;
        }
    }
    for (int s = 1; s < MH_WAVE; s <<= 1) {
        const double om = __shfl_xor(m, s);
        const int oi = __shfl_xor(mi, s);
        if (om < m || (om == m && oi < mi)) {
            m = om;
            mi = oi;
        }
    }
    dmin = m;
    imin = mi;
}

// compute_similar (Utils/Utils.py:1200) on float32 vectors: sum(A*B) / max(|A|*|B|, 1e-4)
__device__ __forceinline__ float mh_sc_similar(float a0, float a1, float a2, float b0, float b1, float b2) {
    const float dot = (a0 * b0 + a1 * b1) + a2 * b2;
    const float na = sqrtf((a0 * a0 + a1 * a1) + a2 * a2), nb = sqrtf((b0 * b0 + b1 * b1) + b2 * b2);
    const float den = na * nb;
    return dot / ((den > 1e-4f || den != den) ? den : 1e-4f);
}

// lowest key (rank << 32 | strand) above `prev` among the members that are the first of their strand, or ~0
__device__ __forceinline__ unsigned long long mh_sc_next(const unsigned long long *__restrict__ seg, int B, bool any_prev,
                                                         unsigned long long prev, int lane) {
    unsigned long long best = ~0ull;
    for (int t = lane; t < B; t += MH_WAVE) {
        const unsigned long long k = seg[t];
        if (!(k & MH_SC_FIRSTBIT) && (!any_prev || k > prev) && k < best) best = k;
    }
    return mh_sc_min_u64(best);
}

__global__ __launch_bounds__(256) void mh_scalp_choose_kernel(
    const float *__restrict__ P, const int64_t *__restrict__ offs, const int32_t *__restrict__ act, int nact,
    const float *__restrict__ core, const int32_t *__restrict__ csid, const int32_t *__restrict__ crank, MhScalpGrid g,
    double r2, float thr_dist, float thr_dot, float loss_base, const double *__restrict__ out_ratio,
    const int64_t *__restrict__ boff, unsigned long long *__restrict__ bscr, uint8_t *__restrict__ flip,
    int32_t *__restrict__ best_sid, int32_t *__restrict__ best_idx) {
    const int a = blockIdx.x * (blockDim.x / MH_WAVE) + (threadIdx.x / MH_WAVE), lane = threadIdx.x & (MH_WAVE - 1);
    if (a >= nact) return;
    const int i = act[a];
    const float *S = P + 3 * offs[i];
    const int L = (int)(offs[i + 1] - offs[i]);
    unsigned long long *seg = bscr + boff[a];
    const int B = (int)(boff[a + 1] - boff[a]);
    if (B == 0) return;   // an empty ball: no flip, no candidate.  (The reference's second query, of strand[-1] at twice
                          // the radius, feeds a test that can never hold -- len(inv) != 0 and len(union1d(inv, nei)) == 0
                          // -- and is not run.)
    // the ball, unordered: (rank, strand) per member
    int w = 0;
    mh_sc_ball_scan(core, g, S[0], S[1], S[2], r2, lane, [&](bool in, int j) {
        const unsigned long long m = __ballot(in);
        if (in) {
            const int at = w + __popcll(m & ((1ull << lane) - 1ull));
            if (at < B) seg[at] = ((unsigned long long)(uint32_t)crank[j] << 32) | (uint32_t)csid[j];
        }
        w += __popcll(m);
    });
    __threadfence_block();
    // the candidate loop visits strands in order of first appearance: keep the lowest rank of every strand
    for (int base = 0; base < B; base += MH_WAVE) {
        const int t = base + lane;
        const unsigned long long kt = t < B ? seg[t] : 0ull;
        bool later = false;
        for (int u = 0; u < B; ++u) {
            const unsigned long long ku = seg[u] & ~MH_SC_FIRSTBIT;
            later |= (uint32_t)ku == (uint32_t)kt && ku < (kt & ~MH_SC_FIRSTBIT);
        }
        if (t < B && later) seg[t] = kt | MH_SC_FIRSTBIT;
    }
    __threadfence_block();

    // ---- the flip test against nei_strands[0], the strand of the lowest rank (:669-685)
    unsigned long long key = mh_sc_next(seg, B, false, 0ull, lane);
    bool fl = false;
    {
        const int c = (int)(uint32_t)key;
        const float *C = P + 3 * offs[c];
        const int Lc = (int)(offs[c + 1] - offs[c]);
        double sum = 0.0;
        int ib = 0, ie = 0;
        for (int base = 0; base < L; base += MH_WAVE) {   // lanes split the points of the floating strand
            const int k = base + lane;
            double m = __builtin_inf();
            int mi = 0;
            if (k < L)
                for (int s = 0; s < Lc; ++s) {
                    const double d0 = (double)S[3 * k] - (double)C[3 * s], d1 = (double)S[3 * k + 1] - (double)C[3 * s + 1],
                                 d2 = (double)S[3 * k + 2] - (double)C[3 * s + 2];
                    const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
                    if (dd < m) {
                        m = dd;
                        mi = s;
                    }
                }
            // np.mean(nei_pos_dist) only meets `< 5`: the sum is taken in wave order, not numpy's pairwise order
            sum += mh_sc_sum_f64(k < L ? sqrt(m) : 0.0);
            if (base == 0) ib = __shfl(mi, 0);
            if (base + MH_WAVE >= L) ie = __shfl(mi, (L - 1) - base);
        }
        float t0, t1, t2;
        if (ib == Lc - 1) {
            const int p = ib - 1 < 0 ? ib - 1 + Lc : ib - 1;   // numpy's negative index
            t0 = C[3 * ib] - C[3 * p], t1 = C[3 * ib + 1] - C[3 * p + 1], t2 = C[3 * ib + 2] - C[3 * p + 2];
        } else {
            t0 = C[3 * ib + 3] - C[3 * ib], t1 = C[3 * ib + 4] - C[3 * ib + 1], t2 = C[3 * ib + 5] - C[3 * ib + 2];
        }
        const float sim = mh_sc_similar(t0, t1, t2, S[3] - S[0], S[4] - S[1], S[5] - S[2]);
        fl = sim < 0.0f && ib > ie && sum / (double)L < 5.0;
    }
    auto pt = [&](int k, int ax) { return S[3 * (fl ? L - 1 - k : k) + ax]; };
    const float s0x = pt(0, 0), s0y = pt(0, 1), s0z = pt(0, 2);
    const float tx = pt(1, 0) - s0x, ty = pt(1, 1) - s0y, tz = pt(1, 2) - s0z;   // Tan = strand[1] - strand[0]

    // ---- the candidate loop (:696-730)
    double min_loss = __builtin_inf();
    int bs = -1, bi = 0, count = 0;
    while (key != ~0ull) {
        const int j = (int)(uint32_t)key;
        ++count;
        const float *Nn = P + 3 * offs[j];
        const int Lj = (int)(offs[j + 1] - offs[j]);
        double dd;
        int pi;
        mh_sc_nearest(Nn, Lj, s0x, s0y, s0z, lane, dd, pi);
        double msum = sqrt(dd);                     // np.mean(query(strand[:5])): fewer than 8 values add in order
        const int n5 = L < 5 ? L : 5;
        for (int k = 1; k < n5; ++k) {
            double dk;
            int ik;
            mh_sc_nearest(Nn, Lj, pt(k, 0), pt(k, 1), pt(k, 2), lane, dk, ik);
            msum += sqrt(dk);
        }
        const bool refused = msum / (double)n5 < 1.0 || (L > 60 && L + pi > 150) || pi <= 1;
        if (!refused) {
            const float *np_ = Nn + 3 * pi;
            // compute_strands_similar on the one-point slice nei_strand[pi:pi+1] (:788-812); pos_index is 0
            const float e0 = np_[0] - s0x, e1 = np_[1] - s0y, e2 = np_[2] - s0z;
            // np.linalg.norm of the float32 difference: its three products summed without intermediate rounding
            const float dist = sqrtf((float)(((double)e0 * e0 + (double)e1 * e1) + (double)e2 * e2));
            const float sc = mh_sc_similar(s0x - np_[0], s0y - np_[1], s0z - np_[2], tx, ty, tz);
            const float sm = mh_sc_similar(np_[0] - np_[-3], np_[1] - np_[-2], np_[2] - np_[-1], tx, ty, tz);
            double loss = __builtin_inf();
            if (sm > thr_dot && dist < thr_dist) loss = (double)((1.0f - sc) + loss_base);
            loss += out_ratio[j];
            if (loss < min_loss) {   // the first of equal losses stays
                min_loss = loss;
                bs = j;
                bi = pi;
            }
            if (count >= 30) break;   // only a candidate that was not refused ends the loop
        }
        key = mh_sc_next(seg, B, true, key, lane);
    }
    if (lane == 0) {
        flip[i] = fl ? 1 : 0;
        best_sid[i] = bs;
        best_idx[i] = bi;
    }
}

// status of a strand after the pass, in flags[]: bit 0 rooted, bit 1 out; counters: newly rooted, newly out, strands whose
// joined part indexes outside the volume (torch's indexing raises there)
__global__ __launch_bounds__(256) void mh_scalp_emit_kernel(
    const float *__restrict__ P, const int64_t *__restrict__ offs, int n, const uint8_t *__restrict__ flip,
    const int32_t *__restrict__ best_sid, const int32_t *__restrict__ best_idx, const int64_t *__restrict__ noffs,
    const float4 *__restrict__ vox, int W, int H, int Z, float ratio_thr, float *__restrict__ Pn,
    uint8_t *__restrict__ flags, double *__restrict__ out_ratio, float *__restrict__ similar_out,
    int32_t *__restrict__ counters) {
    const int i = blockIdx.x * (blockDim.x / MH_WAVE) + (threadIdx.x / MH_WAVE), lane = threadIdx.x & (MH_WAVE - 1);
    if (i >= n) return;
    const float *S = P + 3 * offs[i];
    const int L = (int)(offs[i + 1] - offs[i]);
    const int bs = best_sid[i], m = best_idx[i];
    const bool fl = flip[i] != 0;
    float *O = Pn + 3 * noffs[i];
    float *own = O + (bs >= 0 ? 3 * (m + 1) : 0);
    for (int k = lane; k < L; k += MH_WAVE) {
        const float *s = S + 3 * (fl ? L - 1 - k : k);
        own[3 * k] = s[0];
        own[3 * k + 1] = s[1];
        own[3 * k + 2] = s[2];
    }
    if (bs < 0 || lane != 0) return;
    // connect_strands(push_back=False, add_mid=False) below mid_point = strand[0]*0.95 + ss[m]*0.05: a sequential float32
    // chain, walked by one lane together with random_move_strands' test of strand[:m+1] (the chain and the mid point)
    const float *N = P + 3 * offs[bs];
    const float *s0 = S + 3 * (fl ? L - 1 : 0);
    float seed[3], nx[3];
    for (int ax = 0; ax < 3; ++ax) {
        seed[ax] = s0[ax] * 0.95f + N[3 * m + ax] * 0.05f;
        O[3 * m + ax] = seed[ax];
    }
    int seen = 0;   // MH_VOX_BOX | MH_VOX_REFUSED over the points visited
    float occ_sum = 0.0f;
    double cos_sum = 0.0;
    auto visit = [&](const float *p, float o0, float o1, float o2) {   // one point of ss with its strand_ori
        int64_t at;   // torch.round: half to even
        const int r = mh_voxel_index((int64_t)rintf(p[0]), (int64_t)rintf(p[1]), (int64_t)rintf(p[2]), W, H, Z, at);
        seen |= r;
        if (r & MH_VOX_REFUSED) return;
        const float4 v = vox[at];   // {ori (y/z negated), occ}
        occ_sum += v.w;
        // torch.cosine_similarity: x / max(|x|, 1e-8) . y / max(|y|, 1e-8); max(cos, -cos) = |cos|
        const float na = fmaxf(sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z), 1e-8f),
                    nb = fmaxf(sqrtf((o0 * o0 + o1 * o1) + o2 * o2), 1e-8f);
        cos_sum += (double)fabsf(((v.x / na) * (o0 / nb) + (v.y / na) * (o1 / nb)) + (v.z / na) * (o2 / nb));
    };
    for (int t = 0; t < m; ++t) {   // strand2 = ss[:m+1]: nextPos = seedPos + (strand2[-2-t] - strand2[-1-t])
        const float *a = N + 3 * (m - 1 - t), *b = N + 3 * (m - t);
        for (int ax = 0; ax < 3; ++ax) {
            nx[ax] = seed[ax] + (a[ax] - b[ax]);
            nx[ax] = nx[ax] * 1.0f + a[ax] * 0.0f;   // nextPos*(1-weight) + strand2[-2-t]*weight with weight 0
            O[3 * (m - 1 - t) + ax] = nx[ax];
        }
        const float o0 = seed[0] - nx[0], o1 = seed[1] - nx[1], o2 = seed[2] - nx[2];   // ss[k+1] - ss[k]
        if (t == 0) visit(seed, o0, o1, o2);   // the last point repeats the last difference
        visit(nx, o0, o1, o2);
        for (int ax = 0; ax < 3; ++ax) seed[ax] = nx[ax];
    }
    int st;      // 1 rooted, 2 out, 3 an index torch refuses
    float orat = 0.0f, sim = 0.0f;
    if (seen & MH_VOX_BOX) {
        st = 2;   // leaves the 256 x 256 x 192 box: check False, out_ratio 0
    } else if (seen & MH_VOX_REFUSED) {
        st = 3;
    } else {
        const float ratio = occ_sum / (float)(m + 1);
        orat = 1.0f - ratio;
        sim = (float)cos_sum / occ_sum;
        st = (ratio > ratio_thr && sim > 0.3f) ? 1 : 2;
    }
    out_ratio[i] = (double)orat;
    similar_out[i] = sim;
    if (st != 3) flags[i] |= (uint8_t)st;
    atomicAdd(&counters[st - 1], 1);
}

// ---------------------------------------------------------------------------------------------- launchers
static MhScalpGrid mh_sc_grid(const int32_t *order, const int32_t *cstart, const float *g, const int32_t *d) {
    MhScalpGrid G;
    G.order = order;
    G.cstart = cstart;
    G.ox = g[0], G.oy = g[1], G.oz = g[2], G.h = g[3];
    G.dx = d[0], G.dy = d[1], G.dz = d[2];
    return G;
}

extern "C" int mh_launch_scalp_ball_count(const float *P, const int64_t *offs, const int32_t *act, int nact,
                                          const float *core, const int32_t *order, const int32_t *cstart, const float *grid,
                                          const int32_t *dims, double thr_dist, int64_t *count, hipStream_t st) {
    if (nact <= 0) return 0;
    hipLaunchKernelGGL(mh_scalp_ball_count_kernel, dim3((nact + 3) / 4), dim3(256), 0, st, P, offs, act, nact, core,
                       mh_sc_grid(order, cstart, grid, dims), thr_dist * thr_dist, count);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_scalp_choose(const float *P, const int64_t *offs, const int32_t *act, int nact, const float *core,
                                      const int32_t *csid, const int32_t *crank, const int32_t *order,
                                      const int32_t *cstart, const float *grid, const int32_t *dims, double thr_dist,
                                      double thr_dot, const double *out_ratio, const int64_t *boff,
                                      unsigned long long *bscr, uint8_t *flip, int32_t *best_sid, int32_t *best_idx,
                                      hipStream_t st) {
    if (nact <= 0) return 0;
    // the float32 side of numpy's mixed expressions: similar > thr_dot, dist < thr_dist, (1 - s) + 0.1*thr_dist
    hipLaunchKernelGGL(mh_scalp_choose_kernel, dim3((nact + 3) / 4), dim3(256), 0, st, P, offs, act, nact, core, csid,
                       crank, mh_sc_grid(order, cstart, grid, dims), thr_dist * thr_dist, (float)thr_dist, (float)thr_dot,
                       (float)(0.1 * thr_dist), out_ratio, boff, bscr, flip, best_sid, best_idx);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_scalp_emit(const float *P, const int64_t *offs, int n, const uint8_t *flip,
                                    const int32_t *best_sid, const int32_t *best_idx, const int64_t *noffs,
                                    const float4 *vox, int W, int H, int Z, double ratio_thr, float *Pn, uint8_t *flags,
                                    double *out_ratio, float *similar, int32_t *counters, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(mh_scalp_emit_kernel, dim3((n + 3) / 4), dim3(256), 0, st, P, offs, n, flip, best_sid, best_idx,
                       noffs, vox, W, H, Z, (float)ratio_thr, Pn, flags, out_ratio, similar, counters);
    return (int)hipGetLastError();
}
