// hairmetrics.hip -- scoring one strand set against another (monohair_amd/hairmetrics.py), gfx950 only.  The reference has
// no counterpart: the specification is the point-wise precision / recall of Nam et al., CVPR 2019 (a point counts when SOME
// point of the other set lies within a distance AND runs within an angle of it), restated in numpy by
// tests/hair_metrics_np.py.  Everything is float64 on float32 coordinates with + - * / sqrt in one fixed order
// (-ffp-contract=off: nothing is fused), so the restatement gives the same bits.
//
//   mh_strand_arclen_kernel     one lane per strand: cumulative length per point, number of samples at spacing `step`
//   mh_strand_resample_kernel   one lane per sample: its segment by bisection of the cumulative lengths, the point on it
//   mh_strand_tangents_kernel   one lane per point: the unit central difference (one-sided at the ends) and whether it exists
//   mh_strand_match_kernel      the exists-query: per query the bits k for which a target lies within r2[k] and c[k]
//   mh_flag_counts_kernel       per-bit population counts of the flag bytes, and of `valid`
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_device.h"
#include "mh_strands.h"      // the strand lookup

#define MH_HM_SPAN 2   // cells along x whose queries share one pass over the targets (see mh_strand_match_kernel)

__device__ __forceinline__ double mh_hm_norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

__global__ __launch_bounds__(256) void mh_strand_arclen_kernel(const float *__restrict__ pts,
                                                               const int64_t *__restrict__ offs, int S, double step,
                                                               double *__restrict__ L, int64_t *__restrict__ m) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const int64_t a = offs[s], b = offs[s + 1];
    double acc = 0.0;
    for (int64_t i = a; i < b; ++i) {
        if (i > a)
            acc = acc + mh_hm_norm3((double)pts[3 * i] - (double)pts[3 * i - 3], (double)pts[3 * i + 1] - (double)pts[3 * i - 2],
                                    (double)pts[3 * i + 2] - (double)pts[3 * i - 1]);
        L[i] = acc;
    }
    m[s] = b == a ? 0 : (b - a >= 2 && acc > 0.0 ? (int64_t)floor(acc / step) + 1 : 1);
}

__global__ __launch_bounds__(256) void mh_strand_resample_kernel(const float *__restrict__ pts,
                                                                 const int64_t *__restrict__ offs,
                                                                 const double *__restrict__ L,
                                                                 const int64_t *__restrict__ soffs, int S, int total,
                                                                 double step, float *__restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int s = mh_strand_of(soffs, S, g);
    const int64_t a = offs[s];
    const int n = (int)(offs[s + 1] - a);
    const double *Ls = L + a;
    const float *P = pts + 3 * a;
    float *o = out + 3 * (size_t)g;
    const double last = Ls[n - 1];
    if (n < 2 || !(last > 0.0)) {
        o[0] = P[0], o[1] = P[1], o[2] = P[2];
        return;
    }
    const double arc = (double)(g - soffs[s]) * step;
    int lo = 1, hi = n;      // first k in [1, n) with L[k] > arc: the sample lies on segment k-1
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (Ls[mid] > arc) hi = mid;
        else lo = mid + 1;
    }
    if (lo == n) {           // arc reaches the end: the last segment of non-zero length ends at the first k with L[k] = last
        lo = 1, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (Ls[mid] >= last) hi = mid;
            else lo = mid + 1;
        }
    }
    const int k = lo;
    const double u = (arc - Ls[k - 1]) / (Ls[k] - Ls[k - 1]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double p0 = (double)P[3 * (k - 1) + c], p1 = (double)P[3 * k + c];
        o[c] = (float)(p0 + u * (p1 - p0));
    }
}

__global__ __launch_bounds__(256) void mh_strand_tangents_kernel(const float *__restrict__ pts,
                                                                 const int64_t *__restrict__ offs, int S, int n,
                                                                 double *__restrict__ tan, uint8_t *__restrict__ valid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = mh_strand_of(offs, S, i);
    const int64_t a = offs[s], b = offs[s + 1];
    const int64_t lo = i - 1 > a ? i - 1 : a, hi = i + 1 < b - 1 ? i + 1 : b - 1;
    const double x = (double)pts[3 * hi] - (double)pts[3 * lo], y = (double)pts[3 * hi + 1] - (double)pts[3 * lo + 1],
                 z = (double)pts[3 * hi + 2] - (double)pts[3 * lo + 2];
    const double len = mh_hm_norm3(x, y, z);
    const bool ok = b - a >= 2 && len > 0.0;
    tan[3 * (size_t)i] = ok ? x / len : 0.0;
    tan[3 * (size_t)i + 1] = ok ? y / len : 0.0;
    tan[3 * (size_t)i + 2] = ok ? z / len : 0.0;
    valid[i] = ok ? 1 : 0;
}

// One wave takes 64 queries that follow each other in the cell order of the TARGETS' grid (q_order: mh_grid_build run on the
// queries), so its lanes sit in a handful of cells.  A round serves the lanes of the first unfinished lane's row (same y, z)
// whose x cell is within MH_HM_SPAN of its own: the targets of the 9 neighbouring rows, x cells [x-1, x+SPAN], are staged 64
// at a time through LDS (each row's range is contiguous in the sorted targets) and every lane of the round tests all of
// them -- a superset of its own 27 cells, which the distance test makes harmless.  The grid's cells are wider than the
// largest radius by a slack that outweighs the float32 rounding of mh_grid_cell, so the 27 cells hold every target within
// reach, and a query whose unclamped cell lies more than one cell outside the grid can reach none.  A lane stops testing once
// all K bits are set and the wave leaves a round once all its lanes have.  Targets are the VALID targets only (the caller
// compacts them); the result does not depend on any order, no atomics.
__global__ __launch_bounds__(256) void mh_strand_match_kernel(
    const float *__restrict__ q_pts, const double *__restrict__ q_tan, const uint8_t *__restrict__ q_valid,
    const int32_t *__restrict__ q_order, int nq, const float *__restrict__ t_pts, const double *__restrict__ t_tan,
    const int32_t *__restrict__ cstart, float ox, float oy, float oz, float h, int dx, int dy, int dz, MhMatchPairs pr,
    uint8_t *__restrict__ out) {
    __shared__ double s_t[4][6][MH_WAVE];
    const int wave = threadIdx.x / MH_WAVE, lane = threadIdx.x & (MH_WAVE - 1);
    double(*T)[MH_WAVE] = s_t[wave];
    const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool have = slot < nq;
    const int qi = have ? q_order[slot] : 0;
    double px = 0.0, py = 0.0, pz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;
    int cx = 0, cy = 0, cz = 0;
    bool todo = false;
    if (have && q_valid[qi]) {
        const float fx = q_pts[3 * (size_t)qi], fy = q_pts[3 * (size_t)qi + 1], fz = q_pts[3 * (size_t)qi + 2];
        px = (double)fx, py = (double)fy, pz = (double)fz;
        tx = q_tan[3 * (size_t)qi], ty = q_tan[3 * (size_t)qi + 1], tz = q_tan[3 * (size_t)qi + 2];
        cx = mh_grid_cell(fx, ox, h, dx), cy = mh_grid_cell(fy, oy, h, dy), cz = mh_grid_cell(fz, oz, h, dz);
        const float ux = floorf((fx - ox) / h), uy = floorf((fy - oy) / h), uz = floorf((fz - oz) / h);
        todo = ux >= -1.0f && ux <= (float)dx && uy >= -1.0f && uy <= (float)dy && uz >= -1.0f && uz <= (float)dz;
    }
    const unsigned full = (1u << pr.K) - 1u;
    double r2max = pr.r2[0];
    for (int k = 1; k < pr.K; ++k) r2max = pr.r2[k] > r2max ? pr.r2[k] : r2max;
    unsigned flags = 0;
    for (;;) {
        const unsigned long long rest = __ballot(todo);
        if (!rest) break;
        const int lead = __ffsll((long long)rest) - 1;
        const int lx = __builtin_amdgcn_readlane(cx, lead), ly = __builtin_amdgcn_readlane(cy, lead),
                  lz = __builtin_amdgcn_readlane(cz, lead);
        const bool act = todo && cy == ly && cz == lz && cx >= lx && cx < lx + MH_HM_SPAN;
        const int x0 = max(lx - 1, 0), x1 = min(lx + MH_HM_SPAN, dx - 1);
        bool open = true;     // wave-uniform: some lane of the round still misses a bit
        for (int z = max(lz - 1, 0); open && z <= min(lz + 1, dz - 1); ++z)
            for (int y = max(ly - 1, 0); open && y <= min(ly + 1, dy - 1); ++y) {
                const int row = (z * dy + y) * dx;
                const int s1 = cstart[row + x1 + 1];
                for (int base = cstart[row + x0]; base < s1; base += MH_WAVE) {
                    open = __ballot(act && flags != full) != 0ull;
                    if (!open) break;
                    const int s = base + lane;
                    if (s < s1) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            T[c][lane] = (double)t_pts[3 * (size_t)s + c];
                            T[3 + c][lane] = t_tan[3 * (size_t)s + c];
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (act && flags != full) {
                        const int cnt = min(MH_WAVE, s1 - base);
                        for (int j = 0; j < cnt; ++j) {
                            const double ax = px - T[0][j], ay = py - T[1][j], az = pz - T[2][j];
                            const double d2 = (ax * ax + ay * ay) + az * az;
                            if (d2 <= r2max) {
                                const double dot = fabs((tx * T[3][j] + ty * T[4][j]) + tz * T[5][j]);
#pragma unroll
                                for (int k = 0; k < MH_MATCH_MAXK; ++k)
                                    if (k < pr.K && d2 <= pr.r2[k] && dot >= pr.c[k]) flags |= 1u << k;
                                if (flags == full) break;
                            }
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
            }
        todo = todo && !act;
    }
    if (have) out[qi] = (uint8_t)flags;
}

// out[k] = number of flag bytes with bit k (k < 8), out[8] = number of non-zero `valid` bytes (integer sums: any order)
__global__ __launch_bounds__(256) void mh_flag_counts_kernel(const uint8_t *__restrict__ flags,
                                                             const uint8_t *__restrict__ valid, int n,
                                                             unsigned long long *__restrict__ out) {
    int c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const unsigned f = flags[i];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] += (f >> k) & 1u;
        c[8] += valid[i] != 0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o);
        if ((threadIdx.x & (MH_WAVE - 1)) == 0 && c[k]) atomicAdd(out + k, (unsigned long long)c[k]);
    }
}

extern "C" int mh_launch_strand_arclen(const float *pts, const int64_t *offs, int S, double step, double *L, int64_t *m,
                                       hipStream_t st) {
    hipLaunchKernelGGL(mh_strand_arclen_kernel, dim3((S + 255) / 256), dim3(256), 0, st, pts, offs, S, step, L, m);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_strand_resample(const float *pts, const int64_t *offs, const double *L, const int64_t *soffs,
                                         int S, int total, double step, float *out, hipStream_t st) {
    hipLaunchKernelGGL(mh_strand_resample_kernel, dim3((total + 255) / 256), dim3(256), 0, st, pts, offs, L, soffs, S, total,
                       step, out);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_strand_tangents(const float *pts, const int64_t *offs, int S, int n, double *tan, uint8_t *valid,
                                         hipStream_t st) {
    hipLaunchKernelGGL(mh_strand_tangents_kernel, dim3((n + 255) / 256), dim3(256), 0, st, pts, offs, S, n, tan, valid);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_strand_match(const float *q_pts, const double *q_tan, const uint8_t *q_valid,
                                      const int32_t *q_order, int nq, const float *t_pts, const double *t_tan,
                                      const int32_t *cstart, float ox, float oy, float oz, float h, int dx, int dy, int dz,
                                      MhMatchPairs pr, uint8_t *out, hipStream_t st) {
    hipLaunchKernelGGL(mh_strand_match_kernel, dim3((unsigned)(((long long)nq + 255) / 256)), dim3(256), 0, st, q_pts, q_tan,
                       q_valid, q_order, nq, t_pts, t_tan, cstart, ox, oy, oz, h, dx, dy, dz, pr, out);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_flag_counts(const uint8_t *flags, const uint8_t *valid, int n, unsigned long long *out9,
                                     hipStream_t st) {
    hipError_t e = hipMemsetAsync(out9, 0, 9 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    if (n > 0) {
        const int nb = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
        hipLaunchKernelGGL(mh_flag_counts_kernel, dim3(nb), dim3(256), 0, st, flags, valid, n, out9);
    }
    return (int)hipGetLastError();
}
