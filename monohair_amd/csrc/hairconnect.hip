// Segment connection of HairGrow.py (find_connect_info :434-547, find_best_connect_strands :550-590,
// connect_segments / connect_strands :303-420) and the Laplacian smoothing of Utils/Utils.py:1148-1198, in float64.
//
//   mh_end_knn64_kernel       radius-bounded k-NN over strand ends (KDTree.query(p, k, distance_upper_bound)), one lane
//                             per query, uniform grid of cells no smaller than the bound
//   mh_connect_cand_kernel    find_best_connect_strands for the roots' and then the tips' list of one end: one wave
//                             per (segment, end); lanes split the points of the segment for the nearest-point distances
//   mh_chain_count_kernel /   connect_segments(add_mid=True, weight 0): one lane per segment walks its root-side chain,
//   mh_chain_emit_kernel      then its tip-side chain (count pass, exclusive scan by the caller, emit pass)
//   mh_occ_check_kernel       attempt 0 of the occupancy acceptance loop (:514-544) for every connected strand
//   mh_smooth_kernel          smnooth_strand: banded Cholesky solve of (A^T A) x = A^T b, one lane per strand (3 axes)
//
// Every float64 expression follows the reference's numpy evaluation order; -ffp-contract=off keeps the compiler from
// fusing, and the one fused multiply-add (the strand length, numpy's 1-D norm through BLAS ddot) is spelled out.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_device.h"

#define MH_CK 50   // k of the reference's end queries (HairGrow.py:469,485,497,505)

// ---------------------------------------------------------------------------------------------- end k-NN (float64)
// data points sorted by cell (order[]), cell c holds order[cstart[c] .. cstart[c+1]); qcell = cell of each query
// (computed by the caller with the formula it used for the data).  Keeps the k nearest with d2 < bound2 (ties: lower
// index first), then drops the query's own index when skip_self (the reference's delet_self_index).
__global__ __launch_bounds__(256) void mh_end_knn64_kernel(const double *__restrict__ q, const int32_t *__restrict__ qcell,
                                                           int nq, const double *__restrict__ data,
                                                           const int32_t *__restrict__ order,
                                                           const int32_t *__restrict__ cstart, int gx, int gy, int gz,
                                                           double bound2, int skip_self, int32_t *__restrict__ out_idx,
                                                           double *__restrict__ out_dist, int32_t *__restrict__ out_cnt) {
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    const double px = q[3 * qi], py = q[3 * qi + 1], pz = q[3 * qi + 2];
    const int cx = qcell[3 * qi], cy = qcell[3 * qi + 1], cz = qcell[3 * qi + 2];
    double bd[MH_CK];
    int32_t bi[MH_CK];
    int cnt = 0;
    for (int z = cz - 1; z <= cz + 1; ++z) {
        if (z < 0 || z >= gz) continue;
        for (int y = cy - 1; y <= cy + 1; ++y) {
            if (y < 0 || y >= gy) continue;
            for (int x = cx - 1; x <= cx + 1; ++x) {
                if (x < 0 || x >= gx) continue;
                const int c = (z * gy + y) * gx + x;
                for (int s = cstart[c]; s < cstart[c + 1]; ++s) {
                    const int j = order[s];
                    // scipy's sqeuclidean_distance_double for m = 3: ((d0*d0 + d1*d1) + d2*d2)
                    const double d0 = px - data[3 * j], d1 = py - data[3 * j + 1], d2 = pz - data[3 * j + 2];
                    const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
                    if (!(dd < bound2)) continue;
                    if (cnt == MH_CK && !(dd < bd[MH_CK - 1] || (dd == bd[MH_CK - 1] && j < bi[MH_CK - 1]))) continue;
                    int t = cnt < MH_CK ? cnt++ : MH_CK - 1;
                    while (t > 0 && (dd < bd[t - 1] || (dd == bd[t - 1] && j < bi[t - 1]))) {
                        bd[t] = bd[t - 1];
                        bi[t] = bi[t - 1];
                        --t;
                    }
                    bd[t] = dd;
                    bi[t] = j;
                }
            }
        }
    }
    int w = 0;
    for (int t = 0; t < cnt; ++t) {
        if (skip_self && bi[t] == qi) continue;
        out_idx[(size_t)qi * MH_CK + w] = bi[t];
        out_dist[(size_t)qi * MH_CK + w] = sqrt(bd[t]);
        ++w;
    }
    out_cnt[qi] = w;
}

// ---------------------------------------------------------------------------------------------- candidates
struct MhEndLists {
    const int32_t *idx[4];   // 0 root->roots, 1 root->tips, 2 tip->roots, 3 tip->tips; [N][MH_CK]
    const double *dist[4];
    const int32_t *cnt[4];
};

__device__ __forceinline__ void mh_end_ori(const double *__restrict__ P, int64_t o, int L, int tip, double &a0,
                                           double &a1, double &a2) {
    const double *p = P + 3 * (tip ? o + L - 2 : o);   // root: s[1]-s[0]; tip: s[-1]-s[-2]
    a0 = p[3] - p[0];
    a1 = p[4] - p[1];
    a2 = p[5] - p[2];
}

// best candidate of one list (find_best_connect_strands): returns the neighbour or -1.  Wave-uniform control flow.
__device__ int mh_best_of_list(const double *__restrict__ P, const int64_t *__restrict__ offs, int i, int tip_end,
                               const int32_t *__restrict__ nb, const double *__restrict__ nd, int n, int nb_tip,
                               int same_type, double thr, int lane) {
    const int64_t oi = offs[i];
    const int Li = (int)(offs[i + 1] - oi);
    double a0, a1, a2;
    mh_end_ori(P, oi, Li, tip_end, a0, a1, a2);
    const double na = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
    // strand_lenght = np.linalg.norm(strand[0]-strand[-1], 2): BLAS ddot accumulates with fused multiply-adds
    const double *s0 = P + 3 * oi, *se = P + 3 * (oi + Li - 1);
    const double v0 = s0[0] - se[0], v1 = s0[1] - se[1], v2 = s0[2] - se[2];
    const double slen = sqrt(__builtin_fma(v2, v2, __builtin_fma(v1, v1, v0 * v0)));
    const double lim = slen * 2.0 / 3.0;
    int best = -1;
    double best_loss = 0.0;
    for (int c = 0; c < n; ++c) {
        const int j = nb[c];
        const int64_t oj = offs[j];
        const int Lj = (int)(offs[j + 1] - oj);
        double b0, b1, b2;
        mh_end_ori(P, oj, Lj, nb_tip, b0, b1, b2);
        const double nbn = sqrt((b0 * b0 + b1 * b1) + b2 * b2);
        const double cs = ((a0 * b0 + a1 * b1) + a2 * b2) / (na * nbn);
        if (!(same_type ? cs < -thr : cs > thr)) continue;
        // dist, _ = KDTree(strand_j).query(strand_i, 1), brute force over Li x Lj
        int close = 0;
        double dfirst = 0.0, dlast = 0.0;
        const double t = Li < 6 ? 0.005 : 0.01;
        for (int base = 0; base < Li; base += MH_WAVE) {
            const int k = base + lane;
            double dk = 0.0;
            if (k < Li) {
                const double *pk = P + 3 * (oi + k);
                const double x = pk[0], y = pk[1], z = pk[2];
                double m = __builtin_inf();
                for (int s = 0; s < Lj; ++s) {
                    const double *ps = P + 3 * (oj + s);
                    const double d0 = x - ps[0], d1 = y - ps[1], d2 = z - ps[2];
                    const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
                    m = dd < m ? dd : m;
                }
                dk = sqrt(m);
            }
            close += __popcll(__ballot(k < Li && dk < t));
            if (base == 0) dfirst = __shfl(dk, 0);
            if (base + MH_WAVE >= Li) dlast = __shfl(dk, (Li - 1) - base);
        }
        bool ok = Li < 6 ? close < 4 : close <= 6;
        if (dfirst < lim && dlast < lim && Li > 20) ok = false;
        if (!ok) continue;
        const double loss = nd[c] * (1.0 - fabs(cs));
        if (best < 0 || loss < best_loss) {
            best = j;
            best_loss = loss;
        }
    }
    return best;
}

// out_nb[2i+e] = neighbour joined at end e (0 root, 1 tip) or -1; out_ty = 0 joined at its root, 1 at its tip
__global__ __launch_bounds__(256) void mh_connect_cand_kernel(const double *__restrict__ P,
                                                              const int64_t *__restrict__ offs, int N, MhEndLists L,
                                                              double thr, int32_t *__restrict__ out_nb,
                                                              int32_t *__restrict__ out_ty) {
    const int w = blockIdx.x * (blockDim.x / MH_WAVE) + (threadIdx.x / MH_WAVE), lane = threadIdx.x & (MH_WAVE - 1);
    if (w >= 2 * N) return;
    const int i = w >> 1, e = w & 1;
    // both ends try the roots' list first (root2root / tip2root) and fall back to the tips' (root2tip / tip2tip) when it
    // yields nothing (HairGrow.py:469-510); same-type pairs need cos < -thr, root-to-tip pairs cos > thr
    int best = mh_best_of_list(P, offs, i, e, L.idx[2 * e] + (size_t)i * MH_CK, L.dist[2 * e] + (size_t)i * MH_CK,
                               L.cnt[2 * e][i], 0, e == 0, thr, lane);
    int ty = 0;
    if (best < 0) {
        best = mh_best_of_list(P, offs, i, e, L.idx[2 * e + 1] + (size_t)i * MH_CK, L.dist[2 * e + 1] + (size_t)i * MH_CK,
                               L.cnt[2 * e + 1][i], 1, e == 1, thr, lane);
        ty = 1;
    }
    if (lane == 0) {
        out_nb[w] = best;
        out_ty[w] = best < 0 ? -1 : ty;
    }
}

// ---------------------------------------------------------------------------------------------- chains
// connect_segments' visited list (connect_list) = [i] + root-side nodes so far + tip-side nodes so far; it is
// re-derived by replaying the known prefix of each side instead of being stored.
__device__ bool mh_chain_visited(const int32_t *__restrict__ nb, const int32_t *__restrict__ ty, int i, int c,
                                 int nroot, int ntip) {
    if (c == i) return true;
    for (int side = 0; side < 2; ++side) {
        int j = nb[2 * i + side], t = ty[2 * i + side];
        for (int s = 0; s < (side ? ntip : nroot); ++s) {
            if (j == c) return true;
            const int e = 2 * j + (1 - t);   // the neighbour's other end
            j = nb[e];
            t = ty[e];
        }
    }
    return false;
}

// visits the chain pieces of segment i in the reference's order: fn(side, neighbour, joined_at_tip)
template <class F>
__device__ void mh_chain_walk(const int32_t *__restrict__ nb, const int32_t *__restrict__ ty, int i, F fn) {
    int nroot = 0, ntip = 0;
    for (int side = 0; side < 2; ++side) {
        int j = nb[2 * i + side], t = ty[2 * i + side];
        if (j < 0) continue;
        while (true) {   // connect(): the first step of a side is unconditional, later ones check connect_list
            fn(side, j, t);
            if (side) ++ntip; else ++nroot;
            const int e = 2 * j + (1 - t);
            const int jn = nb[e];
            if (jn < 0 || mh_chain_visited(nb, ty, i, jn, nroot, ntip)) break;
            j = jn;
            t = ty[e];
        }
    }
}

__global__ __launch_bounds__(256) void mh_chain_count_kernel(const int64_t *__restrict__ offs, int N,
                                                             const int32_t *__restrict__ nb,
                                                             const int32_t *__restrict__ ty, int64_t *__restrict__ total,
                                                             int64_t *__restrict__ rootlen) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int64_t n[2] = {0, 0};
    mh_chain_walk(nb, ty, i, [&](int side, int j, int) { n[side] += offs[j + 1] - offs[j]; });
    rootlen[i] = n[0];
    total[i] = n[0] + (offs[i + 1] - offs[i]) + n[1];
}

__global__ __launch_bounds__(256) void mh_chain_emit_kernel(const double *__restrict__ P,
                                                            const int64_t *__restrict__ offs, int N,
                                                            const int32_t *__restrict__ nb,
                                                            const int32_t *__restrict__ ty,
                                                            const int64_t *__restrict__ rootlen,
                                                            const int64_t *__restrict__ ooffs, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t oi = offs[i], Li = offs[i + 1] - oi;
    const int64_t mid0 = ooffs[i] + rootlen[i];
    for (int64_t k = 0; k < 3 * Li; ++k) out[3 * mid0 + k] = P[3 * oi + k];
    int64_t pos[2] = {mid0, mid0 + Li};   // root side grows downwards from pos[0], tip side upwards from pos[1]
    double seed[2][3];
    for (int a = 0; a < 3; ++a) {
        seed[0][a] = P[3 * oi + a];
        seed[1][a] = P[3 * (oi + Li - 1) + a];
    }
    mh_chain_walk(nb, ty, i, [&](int side, int j, int t) {
        const int64_t oj = offs[j], n = offs[j + 1] - oj;
        // strand2 of connect_strands: root side (push_back False) takes strand[::-1] when joined at its root, the tip
        // side (push_back True) when joined at its tip
        const bool rev = side ? (t == 1) : (t == 0);
        auto s2 = [&](int64_t u, int a) { return P[3 * (oj + (rev ? n - 1 - u : u)) + a]; };
        double *sd = seed[side];
        for (int64_t u = 0; u < n; ++u) {
            double v[3];
            for (int a = 0; a < 3; ++a) {
                if (u == 0) {   // mid_point = seedPos*0.5 + strand2[first]*0.5
                    v[a] = sd[a] * 0.5 + s2(side ? 0 : n - 1, a) * 0.5;
                } else {         // nextPos = seedPos + (step); nextPos*(1-0) + strand2[...]*0
                    const int64_t cur = side ? u : n - 1 - u, prv = side ? u - 1 : n - u;
                    const double nx = sd[a] + (s2(cur, a) - s2(prv, a));
                    v[a] = nx * 1.0 + s2(cur, a) * 0.0;
                }
                sd[a] = v[a];
            }
            const int64_t dst = side ? pos[1] + u : pos[0] - 1 - u;
            for (int a = 0; a < 3; ++a) out[3 * dst + a] = v[a];
        }
        if (side) pos[1] += n; else pos[0] -= n;
    });
}

// ---------------------------------------------------------------------------------------------- occupancy, attempt 0
// idx = round((p*(1,-1,-1) - vmin) / vs) (points_to_voxel on float64, torch.round = half to even).  status: 1 accepted
// (occupied fraction > 0.8 in float32), 0 rejected (the caller retries), 2 outside the reference's hard-coded box (no
// retry), 3 an index torch would refuse (IndexError).
__global__ __launch_bounds__(256) void mh_occ_check_kernel(const double *__restrict__ S, const int64_t *__restrict__ offs,
                                                           int N, const float *__restrict__ occ, int64_t ostride, int W,
                                                           int H, int Z, double vx, double vy, double vz, double vs,
                                                           int32_t *__restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t o = offs[i], n = offs[i + 1] - o;
    int seen = n == 0 ? MH_VOX_REFUSED : 0;   // MH_VOX_BOX | MH_VOX_REFUSED over the strand's points
    float sum = 0.0f;                          // in point order; read only when every point is inside
    for (int64_t k = 0; k < n; ++k) {
        const double *p = S + 3 * (o + k);
        int64_t at;
        const int r = mh_voxel_index((int64_t)rint((p[0] - vx) / vs), (int64_t)rint((-p[1] - vy) / vs),
                                     (int64_t)rint((-p[2] - vz) / vs), W, H, Z, at);
        seen |= r;
        if (!r) sum += occ[at * ostride];
    }
    status[i] = (seen & MH_VOX_BOX) ? 2 : (seen ? 3 : ((sum / (float)n > 0.8f) ? 1 : 0));
}

// ---------------------------------------------------------------------------------------------- smoothing
// A = [lap * L ; pos * I] with L the open-chain Laplacian rows of smnooth_strand; A^T A is pentadiagonal.  work: 3
// doubles per point (the band of the Cholesky factor U).  Strands of fewer than 2 points are left
// untouched (the caller rejects them).
__global__ __launch_bounds__(256) void mh_smooth_kernel(double *__restrict__ S, const int64_t *__restrict__ offs, int N,
                                                        double lap, double pos, double *__restrict__ work) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t o = offs[i], n = offs[i + 1] - o;
    if (n < 2) return;
    double *d = work + 3 * o, *a = d + n, *b = a + n;   // d[k] = U[k][k], a[k] = U[k][k+1], b[k] = U[k][k+2]
    const double p2 = pos * pos;
    // bands of A^T A = sum over the rows r of A of (lap*c[r][p]) * (lap*c[r][q]), + pos^2 on the diagonal; c = row 0
    // (1,-1), rows 1..n-2 (-1,2,-1), row n-1 (-1,1)
    auto cf = [&](int64_t r, int64_t c) -> double {
        if (r < 0 || r >= n || c < 0 || c >= n) return 0.0;
        if (r == 0) return c == 0 ? 1.0 : (c == 1 ? -1.0 : 0.0);
        if (r == n - 1) return c == n - 1 ? 1.0 : (c == n - 2 ? -1.0 : 0.0);
        return c == r ? 2.0 : ((c == r - 1 || c == r + 1) ? -1.0 : 0.0);
    };
    auto band = [&](int64_t k, int off) {
        double s = 0.0;
        for (int64_t r = k - 1; r <= k + 2; ++r) s += (cf(r, k) * lap) * (cf(r, k + off) * lap);
        return s;
    };
    auto D = [&](int64_t k) { return band(k, 0) + p2; };
    auto E = [&](int64_t k) { return band(k, 1); };
    auto F = [&](int64_t k) { return band(k, 2); };
    // banded Cholesky A = U^T U in LAPACK's order (dpbtf2, upper, kd = 2: reciprocal scaling of the row, rank-1 update
    // of the trailing block), then dtbsv twice -- what scipy.linalg.solveh_banded does.  Its float32 casts agree with the
    // reference's SuperLU solve on the fixtures; an LDL^T solve missed one coordinate of strands.hair by 1 ulp
    for (int64_t k = 0; k < n; ++k) {
        d[k] = D(k);
        a[k] = k + 1 < n ? E(k) : 0.0;
        b[k] = k + 2 < n ? F(k) : 0.0;
    }
    for (int64_t j = 0; j < n; ++j) {
        const double ajj = sqrt(d[j]);
        d[j] = ajj;
        const double r = 1.0 / ajj;
        if (j + 1 < n) a[j] *= r;
        if (j + 2 < n) b[j] *= r;
        if (j + 1 < n) d[j + 1] = d[j + 1] + a[j] * (-a[j]);
        if (j + 2 < n) {
            const double t = -b[j];
            a[j + 1] = a[j + 1] + a[j] * t;
            d[j + 2] = d[j + 2] + b[j] * t;
        }
    }
    for (int ax = 0; ax < 3; ++ax) {
        double *x = S + 3 * o + ax;
        for (int64_t j = 0; j < n; ++j) {   // U^T y = A^T b, A^T b = pos * b with b = strand * pos (formed by the caller
                                             // in the strand's dtype, as numpy does)
            double t = pos * x[3 * j];
            if (j >= 2) t = t - b[j - 2] * x[3 * (j - 2)];
            if (j >= 1) t = t - a[j - 1] * x[3 * (j - 1)];
            x[3 * j] = t / d[j];
        }
        for (int64_t j = n - 1; j >= 0; --j) {   // U x = y
            const double t = x[3 * j] / d[j];
            x[3 * j] = t;
            if (j >= 1) x[3 * (j - 1)] = x[3 * (j - 1)] - t * a[j - 1];
            if (j >= 2) x[3 * (j - 2)] = x[3 * (j - 2)] - t * b[j - 2];
        }
    }
}

// ---------------------------------------------------------------------------------------------- launchers
extern "C" int mh_launch_end_knn64(const double *q, const int32_t *qcell, int nq, const double *data,
                                   const int32_t *order, const int32_t *cstart, int gx, int gy, int gz, double bound2,
                                   int skip_self, int32_t *out_idx, double *out_dist, int32_t *out_cnt, hipStream_t st) {
    if (nq <= 0) return 0;
    hipLaunchKernelGGL(mh_end_knn64_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, q, qcell, nq, data, order, cstart,
                       gx, gy, gz, bound2, skip_self, out_idx, out_dist, out_cnt);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_connect_cand(const double *P, const int64_t *offs, int N, const int32_t *const *idx,
                                      const double *const *dist, const int32_t *const *cnt, double thr, int32_t *out_nb,
                                      int32_t *out_ty, hipStream_t st) {
    if (N <= 0) return 0;
    MhEndLists L;
    for (int t = 0; t < 4; ++t) {
        L.idx[t] = idx[t];
        L.dist[t] = dist[t];
        L.cnt[t] = cnt[t];
    }
    const int waves = 2 * N;
    hipLaunchKernelGGL(mh_connect_cand_kernel, dim3((waves + 3) / 4), dim3(256), 0, st, P, offs, N, L, thr, out_nb,
                       out_ty);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_chain_count(const int64_t *offs, int N, const int32_t *nb, const int32_t *ty, int64_t *total,
                                     int64_t *rootlen, hipStream_t st) {
    if (N <= 0) return 0;
    hipLaunchKernelGGL(mh_chain_count_kernel, dim3((N + 255) / 256), dim3(256), 0, st, offs, N, nb, ty, total, rootlen);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_chain_emit(const double *P, const int64_t *offs, int N, const int32_t *nb, const int32_t *ty,
                                    const int64_t *rootlen, const int64_t *ooffs, double *out, hipStream_t st) {
    if (N <= 0) return 0;
    hipLaunchKernelGGL(mh_chain_emit_kernel, dim3((N + 255) / 256), dim3(256), 0, st, P, offs, N, nb, ty, rootlen, ooffs,
                       out);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_occ_check(const double *S, const int64_t *offs, int N, const float *occ, int64_t ostride, int W,
                                   int H, int Z, double vx, double vy, double vz, double vs, int32_t *status,
                                   hipStream_t st) {
    if (N <= 0) return 0;
    hipLaunchKernelGGL(mh_occ_check_kernel, dim3((N + 255) / 256), dim3(256), 0, st, S, offs, N, occ, ostride, W, H, Z,
                       vx, vy, vz, vs, status);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_smooth(double *S, const int64_t *offs, int N, double lap, double pos, double *work,
                                hipStream_t st) {
    if (N <= 0) return 0;
    hipLaunchKernelGGL(mh_smooth_kernel, dim3((N + 255) / 256), dim3(256), 0, st, S, offs, N, lap, pos, work);
    return (int)hipGetLastError();
}
