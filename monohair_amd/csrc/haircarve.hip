// haircarve.hip -- coarse geometry from the hair masks (monohair_amd/haircarve.py), gfx950 only: the voxels of the visual hull
// of the hair masks that lie outside the head, and the hull's boundary as a triangle mesh.  The reference has no counterpart
// (its coarse surface and depth maps come from instant-ngp): the specification is the rule written out in include/mh_pmvo.h
// ("Silhouette carve") and restated in numpy by tests/hair_carve_np.py.  The votes are integer counts of float32 comparisons
// made by the helpers the vote kernels use (mh_front.h); the mesh is counted, scanned and then written, every output position
// being a count of what precedes it in the rule's order, so there is no atomic and no order of arrival anywhere.
//
//   mh_carve_kernel<MODE>      one lane per voxel of the grid, z fastest: its centre through every view -> three int32 counts
//                              (MODE 0) or the INSIDE byte (1: all views, 2: leaves the view loop once n_miss > max_miss)
//   mh_carve_corner_kernel     one lane per grid corner: is it used by an exposed face -> one bit, one 64-bit word per wave
//   mh_carve_quad_count_kernel one lane per voxel: its exposed faces -> one sum per wave (= per 64 voxels)
//   mh_carve_scan_kernel       one block: the exclusive scan of the per-word counts, the total
//   mh_carve_vertex_kernel     one lane per corner: a used corner's position at its rank
//   mh_carve_face_kernel       one lane per voxel: two triangles per exposed face, from the voxel's position in the scan
//
// Every address is formed after its bounds test: a neighbour outside the grid is not read, an output row is written only
// below the size the caller states.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_front.h"
#include "mh_volume.h"

template <int MODE>
__global__ __launch_bounds__(256) void mh_carve_kernel(MhViews vw, const float *__restrict__ bust, MhVolGrid gr, int min_free,
                                                       int max_miss, int32_t *__restrict__ counts,
                                                       uint8_t *__restrict__ flags) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)gr.X * gr.Y * gr.Z) return;
    const int z = (int)(i % gr.Z), y = (int)((i / gr.Z) % gr.Y), x = (int)(i / ((size_t)gr.Y * gr.Z));
    float X0, X1, X2;
    mh_fill_centre(gr, x, y, z, X0, X1, X2);
    const int V = vw.V, H = vw.H, W = vw.W;
    int n_in = 0, n_free = 0, n_miss = 0;
    for (int v = 0; v < V; ++v) {
        const MhCentre s = mh_centre_sample(vw.cams + v * MH_CAM_STRIDE, X0, X1, X2, H, W, false);
        if (s.oob || !((-s.z / 2.0f) > 0.0f)) continue;      // abstains: outside the image, or not in front of the camera
        const size_t p = (size_t)v * H * W + (size_t)s.r * W + s.c;
        const bool free_ = mh_centre_depth(s) <= bust[p];
        const bool hair = vw.mask[p] > 0.2f;
        n_in += 1;
        n_free += free_ ? 1 : 0;
        n_miss += (free_ && !hair) ? 1 : 0;
        if (MODE == 2 && n_miss > max_miss) break;           // (the decision is taken: n_miss only grows)
    }
    if (MODE == 0) {
        counts[3 * i] = n_in, counts[3 * i + 1] = n_free, counts[3 * i + 2] = n_miss;
    } else {
        flags[i] = (n_free >= min_free && n_miss <= max_miss) ? 1 : 0;
    }
}

// ---- the mesh.  Corner (i, j, k) has the linear index (i*(Y+1) + j)*(Z+1) + k; its word is index / 64, its bit index % 64.
// the corners of face d (-x, +x, -y, +y, -z, +z) in cyclic order, each as (di << 2 | dj << 1 | dk): include/mh_pmvo.h
__device__ static const uint8_t MH_CARVE_CORNERS[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1},
                                                          {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};

// bit d: face d of the INSIDE voxel (x, y, z) = lin is exposed
__device__ __forceinline__ unsigned mh_carve_exposed(const uint8_t *__restrict__ flags, int X, int Y, int Z, int x, int y, int z,
                                                     size_t lin) {
    const bool has[6] = {x > 0, x + 1 < X, y > 0, y + 1 < Y, z > 0, z + 1 < Z};
    const long long step[6] = {-(long long)Y * Z, (long long)Y * Z, -(long long)Z, (long long)Z, -1, 1};
    unsigned bits = 0;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        bool inside = false;
        if (has[d]) inside = flags[(long long)lin + step[d]] != 0;
        bits |= inside ? 0u : (1u << d);
    }
    return bits;
}

// a corner is used iff the (up to eight) voxels around it are neither all INSIDE nor all not (a voxel outside the grid is not):
// then two of them that share a face differ, and that face is exposed and has the corner
__global__ __launch_bounds__(256) void mh_carve_corner_kernel(const uint8_t *__restrict__ flags, int X, int Y, int Z,
                                                              size_t ncorner, unsigned long long *__restrict__ cmask,
                                                              int32_t *__restrict__ cpre) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool used = false;
    if (c < ncorner) {
        const int k = (int)(c % (Z + 1)), j = (int)((c / (Z + 1)) % (Y + 1)), i = (int)(c / ((size_t)(Y + 1) * (Z + 1)));
        int n = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int x = i - 1 + (t >> 2), y = j - 1 + ((t >> 1) & 1), z = k - 1 + (t & 1);
            if (x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) n += flags[((size_t)x * Y + y) * Z + z] != 0 ? 1 : 0;
        }
        used = n > 0 && n < 8;
    }
    const unsigned long long m = __ballot(used);
    if ((threadIdx.x & 63) == 0 && c < ncorner) cmask[c >> 6] = m, cpre[c >> 6] = __popcll(m);
}

__global__ __launch_bounds__(256) void mh_carve_quad_count_kernel(const uint8_t *__restrict__ flags, int X, int Y, int Z,
                                                                  size_t nvox, long long *__restrict__ qpre) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int n = 0;
    if (i < nvox && flags[i] != 0) {
        const int z = (int)(i % Z), y = (int)((i / Z) % Y), x = (int)(i / ((size_t)Y * Z));
        n = __popc(mh_carve_exposed(flags, X, Y, Z, x, y, z, i));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off);
    if ((threadIdx.x & 63) == 0 && i < nvox) qpre[i >> 6] = n;
}

// v[0 .. n) <- its exclusive scan; total[0] = scale * the sum
template <typename T>
__global__ __launch_bounds__(1024) void mh_carve_scan_kernel(T *__restrict__ v, size_t n, long long scale,
                                                             long long *__restrict__ total) {
    __shared__ T s_w[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T carry = 0;
    for (size_t b0 = 0; b0 < n; b0 += 1024) {
        const size_t b = b0 + threadIdx.x;
        const T val = b < n ? v[b] : (T)0;
        T x = val;      // inclusive scan inside the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const T y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        T before = 0, all = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) before += s_w[w];
            all += s_w[w];
        }
        if (b < n) v[b] = carry + before + x - val;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = (long long)carry * scale;
}

__device__ __forceinline__ int32_t mh_carve_rank(const unsigned long long *__restrict__ cmask, const int32_t *__restrict__ cpre,
                                                 size_t c) {
    return cpre[c >> 6] + __popcll(cmask[c >> 6] & ((1ull << (c & 63)) - 1ull));
}

__global__ __launch_bounds__(256) void mh_carve_vertex_kernel(const unsigned long long *__restrict__ cmask,
                                                              const int32_t *__restrict__ cpre, MhVolGrid gr, size_t ncorner,
                                                              long long n_vertices, float *__restrict__ vertices) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncorner || !((cmask[c >> 6] >> (c & 63)) & 1ull)) return;
    const long long r = mh_carve_rank(cmask, cpre, c);
    if (r >= n_vertices) return;
    const int k = (int)(c % (gr.Z + 1)), j = (int)((c / (gr.Z + 1)) % (gr.Y + 1));
    const int i = (int)(c / ((size_t)(gr.Y + 1) * (gr.Z + 1)));
    float *o = vertices + 3 * (size_t)r;
    o[0] = (float)(gr.vmin[0] + ((double)i - 0.5) * gr.vs);
    o[1] = (float)(-(gr.vmin[1] + ((double)j - 0.5) * gr.vs));
    o[2] = (float)(-(gr.vmin[2] + ((double)k - 0.5) * gr.vs));
}

__global__ __launch_bounds__(256) void mh_carve_face_kernel(const uint8_t *__restrict__ flags, int X, int Y, int Z, size_t nvox,
                                                            const unsigned long long *__restrict__ cmask,
                                                            const int32_t *__restrict__ cpre,
                                                            const long long *__restrict__ qpre, long long n_triangles,
                                                            int32_t *__restrict__ faces) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned bits = 0;
    int x = 0, y = 0, z = 0;
    if (i < nvox && flags[i] != 0) {
        z = (int)(i % Z), y = (int)((i / Z) % Y), x = (int)(i / ((size_t)Y * Z));
        bits = mh_carve_exposed(flags, X, Y, Z, x, y, z, i);
    }
    const int n = __popc(bits);
    int incl = n;      // inclusive scan inside the wave: the wave is one word of qpre
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (!bits) return;
    long long q = qpre[i >> 6] + (incl - n);
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        if (!((bits >> d) & 1u)) continue;
        int32_t r[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int code = MH_CARVE_CORNERS[d][t];
            const size_t c = ((size_t)(x + (code >> 2)) * (Y + 1) + (size_t)(y + ((code >> 1) & 1))) * (Z + 1) +
                             (size_t)(z + (code & 1));
            r[t] = mh_carve_rank(cmask, cpre, c);
        }
        if (2 * q + 1 < n_triangles) {
            int32_t *o = faces + 6 * (size_t)q;
            o[0] = r[0], o[1] = r[1], o[2] = r[2];
            o[3] = r[0], o[4] = r[2], o[5] = r[3];
        }
        ++q;
    }
}

extern "C" int mh_launch_carve_votes(MhViews vw, const float *bust, MhVolGrid gr, int32_t *counts, hipStream_t st) {
    const size_t nvox = (size_t)gr.X * gr.Y * gr.Z;
    hipLaunchKernelGGL(mh_carve_kernel<0>, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, st, vw, bust, gr, 0, 0, counts,
                       (uint8_t *)nullptr);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_carve_inside(MhViews vw, const float *bust, MhVolGrid gr, int min_free, int max_miss, int early_exit,
                                      uint8_t *flags, hipStream_t st) {
    const size_t nvox = (size_t)gr.X * gr.Y * gr.Z;
    const dim3 blocks((unsigned)((nvox + 255) / 256));
    if (early_exit)
        hipLaunchKernelGGL(mh_carve_kernel<2>, blocks, dim3(256), 0, st, vw, bust, gr, min_free, max_miss, (int32_t *)nullptr,
                           flags);
    else
        hipLaunchKernelGGL(mh_carve_kernel<1>, blocks, dim3(256), 0, st, vw, bust, gr, min_free, max_miss, (int32_t *)nullptr,
                           flags);
    return (int)hipGetLastError();
}

// scratch: totals (two int64: vertices, triangles) 256 B | cmask, one 64-bit word per 64 corners | cpre, int32 per word |
// qpre, int64 per 64 voxels; every region on a 256 B boundary
struct MhCarveScratch {
    long long *totals;
    unsigned long long *cmask;
    int32_t *cpre;
    long long *qpre;
    size_t ncorner, nvox, wc, wv, bytes;
    MhCarveScratch(int X, int Y, int Z, void *base) {
        ncorner = (size_t)(X + 1) * (Y + 1) * (Z + 1), nvox = (size_t)X * Y * Z;
        wc = (ncorner + 63) / 64, wv = (nvox + 63) / 64;
        const auto a = [](size_t b) { return (b + 255) / 256 * 256; };
        const uintptr_t p = (uintptr_t)base;
        totals = (long long *)p;
        cmask = (unsigned long long *)(p + 256);
        cpre = (int32_t *)(p + 256 + a(wc * 8));
        qpre = (long long *)(p + 256 + a(wc * 8) + a(wc * 4));
        bytes = 256 + a(wc * 8) + a(wc * 4) + a(wv * 8);
    }
};

extern "C" size_t mh_carve_mesh_scratch_bytes_impl(int X, int Y, int Z) { return MhCarveScratch(X, Y, Z, nullptr).bytes; }

// the counting passes: the scratch holds the corner bits and both scans afterwards, totals = {vertices, triangles}
static void mh_carve_count_passes(const uint8_t *flags, int X, int Y, int Z, const MhCarveScratch &s, hipStream_t st) {
    hipLaunchKernelGGL(mh_carve_corner_kernel, dim3((unsigned)((s.ncorner + 255) / 256)), dim3(256), 0, st, flags, X, Y, Z,
                       s.ncorner, s.cmask, s.cpre);
    hipLaunchKernelGGL(mh_carve_quad_count_kernel, dim3((unsigned)((s.nvox + 255) / 256)), dim3(256), 0, st, flags, X, Y, Z,
                       s.nvox, s.qpre);
    hipLaunchKernelGGL(mh_carve_scan_kernel<int32_t>, dim3(1), dim3(1024), 0, st, s.cpre, s.wc, 1ll, s.totals);
    hipLaunchKernelGGL(mh_carve_scan_kernel<long long>, dim3(1), dim3(1024), 0, st, s.qpre, s.wv, 2ll, s.totals + 1);
}

extern "C" int mh_launch_carve_mesh_count(const uint8_t *flags, int X, int Y, int Z, void *scratch, long long *counts,
                                          hipStream_t st) {
    const MhCarveScratch s(X, Y, Z, scratch);
    mh_carve_count_passes(flags, X, Y, Z, s, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(counts, s.totals, 2 * sizeof(long long), hipMemcpyDeviceToDevice, st);
    return (int)e;
}

extern "C" int mh_launch_carve_mesh(const uint8_t *flags, MhVolGrid gr, void *scratch, long long n_vertices,
                                    long long n_triangles, float *vertices, int32_t *faces, hipStream_t st) {
    const MhCarveScratch s(gr.X, gr.Y, gr.Z, scratch);
    mh_carve_count_passes(flags, gr.X, gr.Y, gr.Z, s, st);
    if (n_vertices > 0)
        hipLaunchKernelGGL(mh_carve_vertex_kernel, dim3((unsigned)((s.ncorner + 255) / 256)), dim3(256), 0, st, s.cmask, s.cpre,
                           gr, s.ncorner, n_vertices, vertices);
    if (n_triangles > 0)
        hipLaunchKernelGGL(mh_carve_face_kernel, dim3((unsigned)((s.nvox + 255) / 256)), dim3(256), 0, st, flags, gr.X, gr.Y,
                           gr.Z, s.nvox, s.cmask, s.cpre, s.qpre, n_triangles, faces);
    return (int)hipGetLastError();
}
