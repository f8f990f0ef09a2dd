// hairfill.hip -- the hair interior filled without the network (monohair_amd/hairfill.py), gfx950 only: the voxels that lie
// inside the hair, outside the head and are seen by almost no view, and the exterior volume's orientations carried inward to
// them.  The reference has no counterpart (its interior is DeepMVSHair's raw.npy): the specification is the rule written out in
// include/mh_pmvo.h ("Inner fill") and restated in numpy by tests/hair_fill_np.py.  The votes are integer counts of float32
// comparisons made by the helpers the vote kernels use (mh_front.h); the sweeps are float64 + and / in one fixed order
// (-ffp-contract=off: nothing is fused), one lane per row reading the PREVIOUS sweep's buffers, so there is no atomic and no
// order of arrival anywhere in the arithmetic.
//
//   mh_inner_votes_kernel      one lane per voxel of the grid: its centre through every view, four int32 counts
//   mh_inner_domain_kernel     one lane per voxel: the domain flag from the counts and the exterior's index volume
//   mh_fill_sources_kernel     one lane per exterior voxel: the six products of its quantised direction, or "no source"
//   mh_fill_map_kernel         a voxel list written into the dense map (domain row d: d + 1, exterior row e: -(e + 1), 0: none)
//   mh_fill_sweep_kernel       one lane per domain row: the six neighbours' tensors averaged (ping-pong buffers)
//   mh_fill_resolve_kernel     one lane per domain row: principal axis (mh_volume.h), coherence, world centre, the emit flag
//
// Every address is formed after its bounds test: a neighbour outside the grid is not read, a row of a list that lies outside
// the grid is counted (status) and takes no part.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_front.h"
#include "mh_volume.h"

// counts [nvox][4] = n_in, n_vis, n_front, n_bad
__global__ __launch_bounds__(256) void mh_inner_votes_kernel(MhViews vw, const float *__restrict__ bust, MhVolGrid gr,
                                                             int32_t *__restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)gr.X * gr.Y * gr.Z) return;
    const int z = (int)(i % gr.Z), y = (int)((i / gr.Z) % gr.Y), x = (int)(i / ((size_t)gr.Y * gr.Z));
    float X0, X1, X2;
    mh_fill_centre(gr, x, y, z, X0, X1, X2);
    const int V = vw.V, H = vw.H, W = vw.W;
    int n_in = 0, n_vis = 0, n_front = 0, n_bad = 0;
    for (int v = 0; v < V; ++v) {
        const MhCentre s = mh_centre_sample(vw.cams + v * MH_CAM_STRIDE, X0, X1, X2, H, W, false);
        if (s.oob || !((-s.z / 2.0f) > 0.0f)) continue;      // abstains: outside the image, or not in front of the camera
        const size_t p = (size_t)v * H * W + (size_t)s.r * W + s.c;
        const float z255 = mh_centre_depth(s);
        const bool visible = !(z255 - vw.rec[p].w > 0.9f);   // compute_unvisible_points' comparison (PMVO.py:470)
        const bool front = z255 <= bust[p];
        const bool hair = vw.mask[p] > 0.2f;
        n_in += 1;
        n_vis += visible ? 1 : 0;
        n_front += front ? 1 : 0;
        n_bad += (front && !hair) ? 1 : 0;
    }
    reinterpret_cast<int4 *>(counts)[i] = make_int4(n_in, n_vis, n_front, n_bad);
}

// ext_index: the exterior volume's index volume (mh_volume_index: -1 = none), or nullptr for no exterior
__global__ __launch_bounds__(256) void mh_inner_domain_kernel(const int32_t *__restrict__ counts,
                                                              const int32_t *__restrict__ ext_index, size_t nvox, int max_bad,
                                                              uint8_t *__restrict__ flags) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvox) return;
    const int4 c = reinterpret_cast<const int4 *>(counts)[i];
    const bool ext = ext_index && ext_index[i] >= 0;
    flags[i] = (c.x >= 1 && c.y <= 2 && c.z >= 1 && c.w <= max_bad && !ext) ? 1 : 0;
}

// tensor [n][6] = xx, yy, zz, xy, xz, yz of q = rint(4096 a); source[e] = 0 for a direction that is not finite, rounds to
// q = 0, or has a component beyond MH_FILL_MAXQ (its products would not be exact)
__global__ __launch_bounds__(256) void mh_fill_sources_kernel(const float *__restrict__ ori, int n, double *__restrict__ tensor,
                                                              uint8_t *__restrict__ source) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double ax = (double)ori[3 * (size_t)e], ay = (double)ori[3 * (size_t)e + 1], az = (double)ori[3 * (size_t)e + 2];
    const double fx = rint(4096.0 * ax), fy = rint(4096.0 * ay), fz = rint(4096.0 * az);
    const bool ok = fabs(fx) <= MH_FILL_MAXQ && fabs(fy) <= MH_FILL_MAXQ && fabs(fz) <= MH_FILL_MAXQ &&      // (NaN fails)
                    !(fx == 0.0 && fy == 0.0 && fz == 0.0);
    long long qx = 0, qy = 0, qz = 0;
    if (ok) qx = (long long)fx, qy = (long long)fy, qz = (long long)fz;
    double *t = tensor + 6 * (size_t)e;
    t[0] = (double)(qx * qx), t[1] = (double)(qy * qy), t[2] = (double)(qz * qz);
    t[3] = (double)(qx * qy), t[4] = (double)(qx * qz), t[5] = (double)(qy * qz);
    source[e] = ok ? 1 : 0;
}

// map[(x*Y + y)*Z + z] = sign * (g + 1) for voxel g of the list; cell[g] (optional) = that index, -1 for a voxel outside the
// grid; status[0] += voxels outside the grid, status[1] += voxels whose cell was taken already (by either list)
__global__ __launch_bounds__(256) void mh_fill_map_kernel(const long long *__restrict__ voxels, int n, int X, int Y, int Z,
                                                          int sign, int32_t *__restrict__ map, int32_t *__restrict__ cell,
                                                          int32_t *__restrict__ status) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const long long x = voxels[3 * (size_t)g], y = voxels[3 * (size_t)g + 1], z = voxels[3 * (size_t)g + 2];
    if (x < 0 || x >= X || y < 0 || y >= Y || z < 0 || z >= Z) {
        atomicAdd(status, 1);
        if (cell) cell[g] = -1;
        return;
    }
    const size_t lin = ((size_t)x * Y + (size_t)y) * Z + (size_t)z;
    if (cell) cell[g] = (int32_t)lin;
    if (atomicCAS(map + lin, 0, sign * (g + 1)) != 0) atomicAdd(status + 1, 1);
}

// sweep k: row r of the domain from the buffers of sweep k - 1 (t0, known0) into (t1, known1); depth[r] = k when it becomes
// known.  The neighbours in the order (x-1), (x+1), (y-1), (y+1), (z-1), (z+1).
__global__ __launch_bounds__(256) void mh_fill_sweep_kernel(const int32_t *__restrict__ cell, int n_dom, int X, int Y, int Z,
                                                            const int32_t *__restrict__ map,
                                                            const double *__restrict__ ext_tensor,
                                                            const uint8_t *__restrict__ ext_source,
                                                            const double *__restrict__ t0, const uint8_t *__restrict__ known0,
                                                            double *__restrict__ t1, uint8_t *__restrict__ known1,
                                                            int32_t *__restrict__ depth, int k) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_dom) return;
    const int lin = cell[r];
    double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int c = 0;
    if (lin >= 0) {
        const int z = lin % Z, y = (lin / Z) % Y, x = lin / (Y * Z);
        const bool has[6] = {x > 0, x + 1 < X, y > 0, y + 1 < Y, z > 0, z + 1 < Z};
        const long long step[6] = {-(long long)Y * Z, (long long)Y * Z, -(long long)Z, (long long)Z, -1, 1};
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            if (!has[j]) continue;
            const int m = map[(long long)lin + step[j]];
            const double *t = nullptr;
            if (m < 0 && ext_source[-m - 1]) t = ext_tensor + 6 * (size_t)(-m - 1);
            else if (m > 0 && known0[m - 1]) t = t0 + 6 * (size_t)(m - 1);
            if (!t) continue;
#pragma unroll
            for (int q = 0; q < 6; ++q) S[q] = S[q] + t[q];
            ++c;
        }
    }
    double *o = t1 + 6 * (size_t)r;
    if (c > 0) {
        const double cd = (double)c;
#pragma unroll
        for (int q = 0; q < 6; ++q) o[q] = S[q] / cd;
        known1[r] = 1;
        if (!known0[r]) depth[r] = k;
    } else {
#pragma unroll
        for (int q = 0; q < 6; ++q) o[q] = t0[6 * (size_t)r + q];
        known1[r] = known0[r];
    }
}

__global__ __launch_bounds__(256) void mh_fill_resolve_kernel(const long long *__restrict__ voxels, int n_dom,
                                                              const double *__restrict__ tensor,
                                                              const uint8_t *__restrict__ known, MhVolGrid gr, double min_coh,
                                                              float *__restrict__ world, float *__restrict__ ori,
                                                              double *__restrict__ coh, uint8_t *__restrict__ emit) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_dom) return;
    const long long vx = voxels[3 * (size_t)r], vy = voxels[3 * (size_t)r + 1], vz = voxels[3 * (size_t)r + 2];
    float *w = world + 3 * (size_t)r, *o = ori + 3 * (size_t)r;
    const bool inside = vx >= 0 && vx < gr.X && vy >= 0 && vy < gr.Y && vz >= 0 && vz < gr.Z;
    w[0] = w[1] = w[2] = 0.0f;
    if (inside) mh_fill_centre(gr, (int)vx, (int)vy, (int)vz, w[0], w[1], w[2]);
    o[0] = o[1] = o[2] = 0.0f;
    coh[r] = 0.0;
    emit[r] = 0;
    if (!inside || !known[r]) return;
    const double *t = tensor + 6 * (size_t)r;
    const double xx = t[0], yy = t[1], zz = t[2], xy = t[3], xz = t[4], yz = t[5];
    const double trace = (xx + yy) + zz;
    if (!(trace > 0.0)) return;
    double x, y, z;
    const double c = mh_tensor_axis(xx, yy, zz, xy, xz, yz, trace, x, y, z);
    coh[r] = c;
    o[0] = (float)x, o[1] = (float)y, o[2] = (float)z;
    emit[r] = (c >= min_coh) ? 1 : 0;      // (NaN fails)
}

extern "C" int mh_launch_inner_votes(MhViews vw, const float *bust, MhVolGrid gr, int32_t *counts, hipStream_t st) {
    const size_t nvox = (size_t)gr.X * gr.Y * gr.Z;
    hipLaunchKernelGGL(mh_inner_votes_kernel, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, st, vw, bust, gr, counts);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_inner_domain(const int32_t *counts, const int32_t *ext_index, size_t nvox, int max_bad, uint8_t *flags,
                                      hipStream_t st) {
    hipLaunchKernelGGL(mh_inner_domain_kernel, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, st, counts, ext_index, nvox,
                       max_bad, flags);
    return (int)hipGetLastError();
}

// After the call the state of sweep `sweeps` is in (t_a, known_a); (t_b, known_b) is the other half of the ping-pong.
extern "C" int mh_launch_inner_diffuse(const long long *ext_voxels, const float *ext_ori, int n_ext, const long long *dom_voxels,
                                       int n_dom, int X, int Y, int Z, int sweeps, int32_t *map, double *ext_tensor,
                                       uint8_t *ext_source, int32_t *cell, double *t_a, double *t_b, uint8_t *known_a,
                                       uint8_t *known_b, int32_t *depth, int32_t *status, hipStream_t st) {
    const size_t nvox = (size_t)X * Y * Z;
    hipError_t e = hipMemsetAsync(map, 0, nvox * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    if (n_ext > 0) {
        hipLaunchKernelGGL(mh_fill_sources_kernel, dim3((n_ext + 255) / 256), dim3(256), 0, st, ext_ori, n_ext, ext_tensor,
                           ext_source);
        hipLaunchKernelGGL(mh_fill_map_kernel, dim3((n_ext + 255) / 256), dim3(256), 0, st, ext_voxels, n_ext, X, Y, Z, -1, map,
                           (int32_t *)nullptr, status);
    }
    if (n_dom < 1) return (int)hipGetLastError();
    e = hipMemsetAsync(t_a, 0, (size_t)n_dom * 6 * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(t_b, 0, (size_t)n_dom * 6 * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(known_a, 0, (size_t)n_dom, st);
    if (e == hipSuccess) e = hipMemsetAsync(known_b, 0, (size_t)n_dom, st);
    if (e == hipSuccess) e = hipMemsetAsync(depth, 0, (size_t)n_dom * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mh_fill_map_kernel, dim3((n_dom + 255) / 256), dim3(256), 0, st, dom_voxels, n_dom, X, Y, Z, 1, map, cell,
                       status);
    double *t0 = t_a, *t1 = t_b;
    uint8_t *k0 = known_a, *k1 = known_b;
    for (int k = 1; k <= sweeps; ++k) {
        hipLaunchKernelGGL(mh_fill_sweep_kernel, dim3((n_dom + 255) / 256), dim3(256), 0, st, cell, n_dom, X, Y, Z, map,
                           ext_tensor, ext_source, t0, k0, t1, k1, depth, k);
        double *t = t0;
        t0 = t1, t1 = t;
        uint8_t *q = k0;
        k0 = k1, k1 = q;
    }
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (t0 != t_a) {      // an odd number of sweeps ended in the other half
        e = hipMemcpyAsync(t_a, t0, (size_t)n_dom * 6 * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(known_a, k0, (size_t)n_dom, hipMemcpyDeviceToDevice, st);
    }
    return (int)e;
}

extern "C" int mh_launch_inner_resolve(const long long *dom_voxels, int n_dom, const double *tensor, const uint8_t *known,
                                       MhVolGrid gr, double min_coh, float *world, float *ori, double *coh, uint8_t *emit,
                                       hipStream_t st) {
    hipLaunchKernelGGL(mh_fill_resolve_kernel, dim3((n_dom + 255) / 256), dim3(256), 0, st, dom_voxels, n_dom, tensor, known, gr,
                       min_coh, world, ori, coh, emit);
    return (int)hipGetLastError();
}
