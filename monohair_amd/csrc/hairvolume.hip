// hairvolume.hip -- a strand set turned into the volume the fit would ideally produce, and one sparse volume scored against
// another (monohair_amd/hairvolume.py), gfx950 only.  The reference has no counterpart: the specification is the rule written
// out in include/mh_pmvo.h ("Strand volume", "Volume scores") and restated in numpy by tests/hair_volume_np.py.  Everything is
// float64 on float32 values with + - * / sqrt in one fixed order (-ffp-contract=off: nothing is fused), and every per-voxel
// sum is an INTEGER sum, so the atomics below give the same bits whatever order the samples arrive in.
//
//   mh_strand_volume_accum_kernel     one lane per segment: its samples added to the dense accumulators (64 B per voxel:
//                                     cnt and the six products of the quantised world direction), the two counters
//   mh_strand_volume_resolve_kernel   one lane per occupied voxel: the principal axis of its 3x3 by 24 power steps
//   mh_volume_index_kernel            the dense index volume of a sparse voxel list (-1 = empty), duplicates counted
//   mh_volume_match_kernel            one lane per query voxel: the (2 reach + 1)^3 neighbourhood of the index volume
//
// A segment makes n <= MH_VOL_MAXN samples: a lane's loop is short (`sub` samples per voxel of travel, hair segments are a
// voxel or two long) and its seven atomics go to one 64-byte record.  A sample outside the grid is counted before any address
// is formed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_device.h"
#include "mh_fill.h"
#include "mh_strands.h"      // the strand lookup
#include "mh_volume.h"

__device__ __forceinline__ bool mh_vol_finite3(double x, double y, double z) {
    return fabs(x) < __builtin_inf() && fabs(y) < __builtin_inf() && fabs(z) < __builtin_inf();      // (NaN fails)
}

// acc: [nvox][8] -- cnt, xx, yy, zz, xy, xz, yz, unused; occ [nvox]: 1 where a sample landed; counters: dropped segments,
// outside samples
__global__ __launch_bounds__(256) void mh_strand_volume_accum_kernel(const float *__restrict__ pts,
                                                                     const int64_t *__restrict__ offs, int S, int n_points,
                                                                     MhVolGrid gr, int sub,
                                                                     unsigned long long *__restrict__ acc,
                                                                     uint8_t *__restrict__ occ,
                                                                     unsigned long long *__restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i + 1 >= n_points) return;
    const int s = mh_strand_of(offs, S, i);
    if (s >= S || i + 1 >= offs[s + 1]) return;
    const double wax = (double)pts[3 * i] + gr.bust[0], way = (double)pts[3 * i + 1] + gr.bust[1],
                 waz = (double)pts[3 * i + 2] + gr.bust[2];
    const double wbx = (double)pts[3 * i + 3] + gr.bust[0], wby = (double)pts[3 * i + 4] + gr.bust[1],
                 wbz = (double)pts[3 * i + 5] + gr.bust[2];
    const double gax = (wax - gr.vmin[0]) / gr.vs, gay = ((-way) - gr.vmin[1]) / gr.vs, gaz = ((-waz) - gr.vmin[2]) / gr.vs;
    const double gbx = (wbx - gr.vmin[0]) / gr.vs, gby = ((-wby) - gr.vmin[1]) / gr.vs, gbz = ((-wbz) - gr.vmin[2]) / gr.vs;
    if (!mh_vol_finite3(gax, gay, gaz) || !mh_vol_finite3(gbx, gby, gbz)) return;
    const double dx = gbx - gax, dy = gby - gay, dz = gbz - gaz;
    const double nn = fmax(1.0, ceil((double)sub * fmax(fmax(fabs(dx), fabs(dy)), fabs(dz))));
    if (!(nn <= (double)MH_VOL_MAXN)) {      // (an infinite difference of two finite ends is dropped here as well)
        atomicAdd(counters, 1ull);
        return;
    }
    const int n = (int)nn;
    const double ux = wbx - wax, uy = wby - way, uz = wbz - waz;
    const double len = sqrt((ux * ux + uy * uy) + uz * uz);
    long long qx = 0, qy = 0, qz = 0;
    if (len > 0.0 && len < __builtin_inf()) {
        qx = (long long)rint(4096.0 * (ux / len));
        qy = (long long)rint(4096.0 * (uy / len));
        qz = (long long)rint(4096.0 * (uz / len));
    }
    const unsigned long long pr[6] = {(unsigned long long)(qx * qx), (unsigned long long)(qy * qy),
                                      (unsigned long long)(qz * qz), (unsigned long long)(qx * qy),
                                      (unsigned long long)(qx * qz), (unsigned long long)(qy * qz)};
    unsigned long long outside = 0;
    for (int j = 0; j < n; ++j) {
        const double t = ((double)j + 0.5) / (double)n;
        const double vx = rint(gax + t * dx), vy = rint(gay + t * dy), vz = rint(gaz + t * dz);
        if (!(vx >= 0.0 && vx < (double)gr.X && vy >= 0.0 && vy < (double)gr.Y && vz >= 0.0 && vz < (double)gr.Z)) {
            ++outside;
            continue;
        }
        const size_t v = ((size_t)(int)vx * gr.Y + (size_t)(int)vy) * gr.Z + (size_t)(int)vz;
        unsigned long long *a = acc + 8 * v;
        atomicAdd(a, 1ull);
#pragma unroll
        for (int c = 0; c < 6; ++c)
            if (pr[c]) atomicAdd(a + 1 + c, pr[c]);      // two's complement: the signed sum
        occ[v] = 1;                                     // (every writer stores the same byte)
    }
    if (outside) atomicAdd(counters + 1, outside);
}

// per occupied voxel index[g] (ascending): voxel (x, y, z), cnt, the six sums, orientation, coherence; *refused += 1 for a
// voxel with more than MH_VOL_MAXCNT samples (its sums may not convert to float64 exactly: nothing is resolved for it)
__global__ __launch_bounds__(256) void mh_strand_volume_resolve_kernel(const long long *__restrict__ acc,
                                                                       const int32_t *__restrict__ index, int G, int Y, int Z,
                                                                       long long *__restrict__ voxels, float *__restrict__ ori,
                                                                       int32_t *__restrict__ cnt, double *__restrict__ coh,
                                                                       long long *__restrict__ sums,
                                                                       int32_t *__restrict__ refused) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int v = index[g];
    const long long *a = acc + 8 * (size_t)v;
    voxels[3 * (size_t)g] = v / (Y * Z);
    voxels[3 * (size_t)g + 1] = (v / Z) % Y;
    voxels[3 * (size_t)g + 2] = v % Z;
    const long long k = a[0];
    float *o = ori + 3 * (size_t)g;
    if (k > MH_VOL_MAXCNT) {
        atomicAdd(refused, 1);
        cnt[g] = 0, coh[g] = 0.0, o[0] = o[1] = o[2] = 0.0f;
        if (sums)
            for (int c = 0; c < 6; ++c) sums[6 * (size_t)g + c] = 0;
        return;
    }
    cnt[g] = (int32_t)k;
    if (sums)
        for (int c = 0; c < 6; ++c) sums[6 * (size_t)g + c] = a[1 + c];
    const double xx = (double)a[1], yy = (double)a[2], zz = (double)a[3], xy = (double)a[4], xz = (double)a[5],
                 yz = (double)a[6];
    const double trace = (xx + yy) + zz;
    if (!(trace > 0.0)) {      // (a sum of squares: zero only when every sample's direction was zero)
        coh[g] = 0.0, o[0] = o[1] = o[2] = 0.0f;
        return;
    }
    double x, y, z;
    coh[g] = mh_tensor_axis(xx, yy, zz, xy, xz, yz, trace, x, y, z);      // (mh_volume.h: shared with hairfill.hip)
    o[0] = (float)x, o[1] = (float)y, o[2] = (float)z;
}

// index[(x*Y + y)*Z + z] = g for voxel g; status[0] += voxels outside the grid, status[1] += voxels met a second time
__global__ __launch_bounds__(256) void mh_volume_index_kernel(const long long *__restrict__ voxels, int G, int X, int Y, int Z,
                                                              int32_t *__restrict__ index, int32_t *__restrict__ status) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const long long x = voxels[3 * (size_t)g], y = voxels[3 * (size_t)g + 1], z = voxels[3 * (size_t)g + 2];
    if (x < 0 || x >= X || y < 0 || y >= Y || z < 0 || z >= Z) {
        atomicAdd(status, 1);
        return;
    }
    if (atomicCAS(index + ((size_t)x * Y + (size_t)y) * Z + (size_t)z, -1, g) != -1) atomicAdd(status + 1, 1);
}

// One lane per query voxel; the queries of a wave follow each other in the caller's order (ascending key: neighbours along z),
// so their walks read neighbouring lines of the index volume.  The walk covers the largest reach of the pairs and stops once
// every bit is set.  Voxels of the query list outside the grid get no flag.
__global__ __launch_bounds__(256) void mh_volume_match_kernel(const long long *__restrict__ q_vox,
                                                              const float *__restrict__ q_ori, int nq,
                                                              const int32_t *__restrict__ t_index,
                                                              const float *__restrict__ t_ori, int X, int Y, int Z,
                                                              MhVolPairs pr, uint8_t *__restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const long long qx = q_vox[3 * (size_t)q], qy = q_vox[3 * (size_t)q + 1], qz = q_vox[3 * (size_t)q + 2];
    if (qx < 0 || qx >= X || qy < 0 || qy >= Y || qz < 0 || qz >= Z) {
        out[q] = 0;
        return;
    }
    const double ax = (double)q_ori[3 * (size_t)q], ay = (double)q_ori[3 * (size_t)q + 1], az = (double)q_ori[3 * (size_t)q + 2];
    const double na = (ax * ax + ay * ay) + az * az;
    const unsigned full = (1u << pr.K) - 1u;
    int R = 0;
    for (int k = 0; k < pr.K; ++k) R = pr.reach[k] > R ? pr.reach[k] : R;
    const int x0 = max((int)qx - R, 0), x1 = min((int)qx + R, X - 1);
    const int y0 = max((int)qy - R, 0), y1 = min((int)qy + R, Y - 1);
    const int z0 = max((int)qz - R, 0), z1 = min((int)qz + R, Z - 1);
    unsigned flags = 0;
    for (int x = x0; x <= x1 && flags != full; ++x)
        for (int y = y0; y <= y1 && flags != full; ++y) {
            const int32_t *row = t_index + ((size_t)x * Y + (size_t)y) * Z;
            const int dxy = max(abs(x - (int)qx), abs(y - (int)qy));
            for (int z = z0; z <= z1; ++z) {
                const int t = row[z];
                if (t < 0) continue;
                const int d = max(dxy, abs(z - (int)qz));
                const double bx = (double)t_ori[3 * (size_t)t], by = (double)t_ori[3 * (size_t)t + 1],
                             bz = (double)t_ori[3 * (size_t)t + 2];
                const double dot = (ax * bx + ay * by) + az * bz;
                const double nb = (bx * bx + by * by) + bz * bz;
                const bool dir = na > 0.0 && nb > 0.0;
                const double dd = dot * dot, nn = na * nb;
#pragma unroll
                for (int k = 0; k < MH_VOL_MAXK; ++k)
                    if (k < pr.K && d <= pr.reach[k] && (pr.cos2[k] < 0.0 || (dir && dd >= pr.cos2[k] * nn))) flags |= 1u << k;
                if (flags == full) break;
            }
        }
    out[q] = (uint8_t)flags;
}

extern "C" int mh_launch_strand_volume_accum(const float *pts, const int64_t *offs, int S, int n_points, MhVolGrid gr, int sub,
                                             unsigned long long *acc, uint8_t *occ, unsigned long long *counters,
                                             hipStream_t st) {
    const size_t nvox = (size_t)gr.X * gr.Y * gr.Z;
    hipError_t e = hipMemsetAsync(acc, 0, nvox * 64, st);
    if (e == hipSuccess) e = hipMemsetAsync(occ, 0, nvox, st);
    if (e == hipSuccess) e = hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    if (n_points < 2) return 0;
    hipLaunchKernelGGL(mh_strand_volume_accum_kernel, dim3((n_points - 1 + 255) / 256), dim3(256), 0, st, pts, offs, S,
                       n_points, gr, sub, acc, occ, counters);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_strand_volume_resolve(const long long *acc, const int32_t *index, int G, int Y, int Z,
                                               long long *voxels, float *ori, int32_t *cnt, double *coh, long long *sums,
                                               int32_t *refused, hipStream_t st) {
    hipError_t e = hipMemsetAsync(refused, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    if (G < 1) return 0;
    hipLaunchKernelGGL(mh_strand_volume_resolve_kernel, dim3((G + 255) / 256), dim3(256), 0, st, acc, index, G, Y, Z, voxels,
                       ori, cnt, coh, sums, refused);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_volume_index(const long long *voxels, int G, int X, int Y, int Z, int32_t *index, int32_t *status,
                                      hipStream_t st) {
    hipError_t e = (hipError_t)mh_fill_u32(index, 0xffffffffu /* -1 */, (size_t)X * Y * Z, st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    if (G < 1) return 0;
    hipLaunchKernelGGL(mh_volume_index_kernel, dim3((G + 255) / 256), dim3(256), 0, st, voxels, G, X, Y, Z, index, status);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_volume_match(const long long *q_vox, const float *q_ori, int nq, const int32_t *t_index,
                                      const float *t_ori, int X, int Y, int Z, MhVolPairs pr, uint8_t *out, hipStream_t st) {
    hipLaunchKernelGGL(mh_volume_match_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, q_vox, q_ori, nq, t_index, t_ori, X,
                       Y, Z, pr, out);
    return (int)hipGetLastError();
}
