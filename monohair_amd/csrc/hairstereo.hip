// hairstereo.hip -- the photo-consistent carve (monohair_amd/hairstereo.py), gfx950 only: census codes of the reduced gray
// photographs, the best photo-consistent candidate voxel per (view, cell), the views that agree on a winner, and the candidates
// that lie in front of a confirmed winner.  The reference has no counterpart: the specification is the rule written out in
// include/mh_pmvo.h ("Photo-consistent carve") and restated in numpy by tests/hair_stereo_np.py.  The per-(voxel, view) terms are
// those of the silhouette carve, made by the same helpers (mh_front.h, mh_volume.h); everything after them is integer
// arithmetic, and the one reduction is a 64-bit atomic minimum of (cost << 32 | index) keys, so no order of arrival shows.
//
//   mh_stereo_reduce_kernel    one lane per reduced pixel: the rounded mean of its block of the gray image
//   mh_stereo_census_kernel    one lane per reduced pixel: its census code over the clamped window
//   mh_stereo_fill_kernel      every key <- all ones
//   mh_stereo_winners_kernel   one lane per candidate: per view that takes part, the cost over the neighbour views (each
//                              projected again per pair: the simpler of the two forms) -> atomic minimum
//   mh_stereo_agree_kernel     one lane per voxel of the grid: the views whose winner lies within the margin of it
//   mh_stereo_refine_kernel    one lane per voxel: the views in which it lies in front of a confirmed winner -> refined flag
//   mh_stereo_depth_kernel     one lane per (view, cell): the depth of its confirmed winner, or 255
//
// Every address is formed after its bounds test: a candidate index, a neighbour view and a key's voxel index outside their
// ranges are skipped, not read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_front.h"
#include "mh_volume.h"

#define MH_STEREO_NONE 0xffffffffffffffffull

// ---- 1. reduced images and census codes
__global__ __launch_bounds__(256) void mh_stereo_reduce_kernel(const uint8_t *__restrict__ gray, int V, int H, int W, int cell,
                                                               int Hc, int Wc, uint8_t *__restrict__ reduced) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)V * Hc * Wc) return;
    const int j = (int)(t % Wc), i = (int)((t / Wc) % Hc), v = (int)(t / ((size_t)Hc * Wc));
    const int r0 = i * cell, c0 = j * cell, r1 = min(r0 + cell, H), c1 = min(c0 + cell, W);
    const uint8_t *img = gray + (size_t)v * H * W;
    int sum = 0;
    for (int r = r0; r < r1; ++r)
        for (int c = c0; c < c1; ++c) sum += img[(size_t)r * W + c];
    const int n = (r1 - r0) * (c1 - c0);
    reduced[t] = (uint8_t)((2 * sum + n) / (2 * n));
}

__global__ __launch_bounds__(256) void mh_stereo_census_kernel(const uint8_t *__restrict__ reduced, int V, int Hc, int Wc,
                                                               int radius, unsigned long long *__restrict__ census) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)V * Hc * Wc) return;
    const int j = (int)(t % Wc), i = (int)((t / Wc) % Hc), v = (int)(t / ((size_t)Hc * Wc));
    const uint8_t *g = reduced + (size_t)v * Hc * Wc;
    const int centre = g[(size_t)i * Wc + j];
    unsigned long long code = 0;
    int b = 0;
    for (int dy = -radius; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const int y = min(max(i + dy, 0), Hc - 1), x = min(max(j + dx, 0), Wc - 1);
            code |= (unsigned long long)(g[(size_t)y * Wc + x] < centre ? 1 : 0) << b;
            ++b;
        }
    census[t] = code;
}

__global__ __launch_bounds__(256) void mh_stereo_fill_kernel(unsigned long long *__restrict__ keys, size_t n) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) keys[t] = MH_STEREO_NONE;
}

// ---- 2. the terms of a (voxel, view) pair, as the carve forms them
struct MhStereoTerm {
    bool seen;       // the view does not abstain
    bool free_;      // ... and the bust does not hide the voxel
    bool takes;      // ... and the pixel is hair: the view takes part
    int cell;        // (row / cell) * Wc + col / cell
    float z255;
};
__device__ __forceinline__ MhStereoTerm mh_stereo_term(const MhViews &vw, const float *__restrict__ bust, int v, float X0, float X1,
                                                       float X2, int cell, int Wc) {
    MhStereoTerm t = {false, false, false, 0, 0.0f};
    const MhCentre s = mh_centre_sample(vw.cams + v * MH_CAM_STRIDE, X0, X1, X2, vw.H, vw.W, false);
    if (s.oob || !((-s.z / 2.0f) > 0.0f)) return t;
    const size_t p = (size_t)v * vw.H * vw.W + (size_t)s.r * vw.W + s.c;
    t.seen = true;
    t.z255 = mh_centre_depth(s);
    t.free_ = t.z255 <= bust[p];
    t.takes = t.free_ && vw.mask[p] > 0.2f;
    t.cell = (s.r / cell) * Wc + s.c / cell;
    return t;
}
// z255 of a voxel in a view, whatever the view decides about it
__device__ __forceinline__ float mh_stereo_z255(const MhViews &vw, int v, const MhVolGrid &gr, unsigned lin) {
    const int z = (int)(lin % gr.Z), y = (int)((lin / gr.Z) % gr.Y), x = (int)(lin / ((unsigned)gr.Y * gr.Z));
    float X0, X1, X2;
    mh_fill_centre(gr, x, y, z, X0, X1, X2);
    return mh_centre_depth(mh_centre_sample(vw.cams + v * MH_CAM_STRIDE, X0, X1, X2, vw.H, vw.W, false));
}
// a cell's key -> is it valid, and the voxel it names
__device__ __forceinline__ bool mh_stereo_valid(unsigned long long key, int max_cost, size_t nvox, unsigned &lin) {
    lin = (unsigned)(key & 0xffffffffull);
    return key != MH_STEREO_NONE && (key >> 32) <= (unsigned long long)max_cost && lin < nvox;
}

// ---- 3. cost and winners
__global__ __launch_bounds__(256) void mh_stereo_winners_kernel(MhViews vw, const float *__restrict__ bust, MhVolGrid gr,
                                                                const int32_t *__restrict__ cand, int n_cand,
                                                                const unsigned long long *__restrict__ census,
                                                                const int32_t *__restrict__ nb, int K, int cell, int Hc,
                                                                int Wc, int B, int keep,
                                                                unsigned long long *__restrict__ keys) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n_cand) return;
    const int32_t lin = cand[t];
    if (lin < 0 || (size_t)lin >= (size_t)gr.X * gr.Y * gr.Z) return;
    const int z = lin % gr.Z, y = (lin / gr.Z) % gr.Y, x = lin / (gr.Y * gr.Z);
    float X0, X1, X2;
    mh_fill_centre(gr, x, y, z, X0, X1, X2);
    const int V = vw.V;
    const size_t plane = (size_t)Hc * Wc;
    for (int r = 0; r < V; ++r) {
        const MhStereoTerm a = mh_stereo_term(vw, bust, r, X0, X1, X2, cell, Wc);
        if (!a.takes) continue;
        const unsigned long long code = census[(size_t)r * plane + a.cell];
        int h[8];      // the smallest distances so far, ascending (static indices only: registers)
#pragma unroll
        for (int q = 0; q < 8; ++q) h[q] = 1 << 20;
        int have = 0;
        for (int k = 0; k < K; ++k) {
            const int n = nb[(size_t)r * K + k];
            if (n < 0 || n >= V || n == r) continue;
            const MhStereoTerm b = mh_stereo_term(vw, bust, n, X0, X1, X2, cell, Wc);
            if (!b.takes) continue;
            int d = __popcll(code ^ census[(size_t)n * plane + b.cell]);
            ++have;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int lo = min(h[q], d);
                d = max(h[q], d);
                h[q] = lo;
            }
        }
        if (have < keep) continue;
        int S = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) S += q < keep ? h[q] : 0;
        const unsigned long long cost = (unsigned long long)((1024 * S) / (B * keep));
        atomicMin(keys + (size_t)r * plane + a.cell, (cost << 32) | (unsigned long long)(unsigned)lin);
    }
}

// ---- 4. agreement
__global__ __launch_bounds__(256) void mh_stereo_agree_kernel(MhViews vw, const float *__restrict__ bust, MhVolGrid gr,
                                                              const uint8_t *__restrict__ flags,
                                                              const unsigned long long *__restrict__ keys, int cell, int Hc,
                                                              int Wc, int max_cost, float m255, int32_t *__restrict__ agree) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nvox = (size_t)gr.X * gr.Y * gr.Z;
    if (i >= nvox) return;
    int count = 0;
    if (flags[i] != 0) {
        const int z = (int)(i % gr.Z), y = (int)((i / gr.Z) % gr.Y), x = (int)(i / ((size_t)gr.Y * gr.Z));
        float X0, X1, X2;
        mh_fill_centre(gr, x, y, z, X0, X1, X2);
        const size_t plane = (size_t)Hc * Wc;
        for (int r = 0; r < vw.V; ++r) {
            const MhStereoTerm a = mh_stereo_term(vw, bust, r, X0, X1, X2, cell, Wc);
            if (!a.takes) continue;
            unsigned win;
            if (!mh_stereo_valid(keys[(size_t)r * plane + a.cell], max_cost, nvox, win)) continue;
            count += fabsf(a.z255 - mh_stereo_z255(vw, r, gr, win)) <= m255 ? 1 : 0;
        }
    }
    agree[i] = count;
}

// ---- 5. refinement
__global__ __launch_bounds__(256) void mh_stereo_refine_kernel(MhViews vw, const float *__restrict__ bust, MhVolGrid gr,
                                                               const uint8_t *__restrict__ flags,
                                                               const unsigned long long *__restrict__ keys,
                                                               const int32_t *__restrict__ agree, int cell, int Hc, int Wc,
                                                               int max_cost, float m255, int min_agree, int min_through,
                                                               uint8_t *__restrict__ refined) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nvox = (size_t)gr.X * gr.Y * gr.Z;
    if (i >= nvox) return;
    bool keep = false;
    if (flags[i] != 0) {
        const int z = (int)(i % gr.Z), y = (int)((i / gr.Z) % gr.Y), x = (int)(i / ((size_t)gr.Y * gr.Z));
        float X0, X1, X2;
        mh_fill_centre(gr, x, y, z, X0, X1, X2);
        const size_t plane = (size_t)Hc * Wc;
        int through = 0;
        for (int r = 0; r < vw.V && through < min_through; ++r) {      // (the decision is taken: through only grows)
            const MhStereoTerm a = mh_stereo_term(vw, bust, r, X0, X1, X2, cell, Wc);
            if (!a.free_) continue;
            unsigned win;
            if (!mh_stereo_valid(keys[(size_t)r * plane + a.cell], max_cost, nvox, win)) continue;
            if (agree[win] < min_agree) continue;
            through += (a.z255 + m255) < mh_stereo_z255(vw, r, gr, win) ? 1 : 0;
        }
        keep = through < min_through;
    }
    refined[i] = keep ? 1 : 0;
}

__global__ __launch_bounds__(256) void mh_stereo_depth_kernel(MhViews vw, MhVolGrid gr,
                                                              const unsigned long long *__restrict__ keys,
                                                              const int32_t *__restrict__ agree, int Hc, int Wc, int max_cost,
                                                              int min_agree, float *__restrict__ depth) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t plane = (size_t)Hc * Wc;
    if (t >= (size_t)vw.V * plane) return;
    unsigned win;
    float d = 255.0f;
    if (mh_stereo_valid(keys[t], max_cost, (size_t)gr.X * gr.Y * gr.Z, win) && agree[win] >= min_agree)
        d = mh_stereo_z255(vw, (int)(t / plane), gr, win);
    depth[t] = d;
}

static inline dim3 mh_stereo_blocks(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

extern "C" int mh_launch_stereo_census(const uint8_t *gray, int V, int H, int W, int cell, int radius, uint8_t *reduced,
                                       unsigned long long *census, hipStream_t st) {
    const int Hc = (H + cell - 1) / cell, Wc = (W + cell - 1) / cell;
    const size_t n = (size_t)V * Hc * Wc;
    hipLaunchKernelGGL(mh_stereo_reduce_kernel, mh_stereo_blocks(n), dim3(256), 0, st, gray, V, H, W, cell, Hc, Wc, reduced);
    hipLaunchKernelGGL(mh_stereo_census_kernel, mh_stereo_blocks(n), dim3(256), 0, st, reduced, V, Hc, Wc, radius, census);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_stereo_winners(MhViews vw, const float *bust, MhVolGrid gr, const int32_t *cand, int n_cand,
                                        const unsigned long long *census, const int32_t *nb, int K, int cell, int radius,
                                        int keep, unsigned long long *keys, hipStream_t st) {
    const int Hc = (vw.H + cell - 1) / cell, Wc = (vw.W + cell - 1) / cell;
    const size_t n = (size_t)vw.V * Hc * Wc;
    hipLaunchKernelGGL(mh_stereo_fill_kernel, mh_stereo_blocks(n), dim3(256), 0, st, keys, n);
    if (n_cand > 0)
        hipLaunchKernelGGL(mh_stereo_winners_kernel, mh_stereo_blocks((size_t)n_cand), dim3(256), 0, st, vw, bust, gr, cand,
                           n_cand, census, nb, K, cell, Hc, Wc, (2 * radius + 1) * (2 * radius + 1) - 1, keep, keys);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_stereo_agree(MhViews vw, const float *bust, MhVolGrid gr, const uint8_t *flags,
                                      const unsigned long long *keys, int cell, int max_cost, float m255, int32_t *agree,
                                      hipStream_t st) {
    const int Hc = (vw.H + cell - 1) / cell, Wc = (vw.W + cell - 1) / cell;
    hipLaunchKernelGGL(mh_stereo_agree_kernel, mh_stereo_blocks((size_t)gr.X * gr.Y * gr.Z), dim3(256), 0, st, vw, bust, gr,
                       flags, keys, cell, Hc, Wc, max_cost, m255, agree);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_stereo_refine(MhViews vw, const float *bust, MhVolGrid gr, const uint8_t *flags,
                                       const unsigned long long *keys, const int32_t *agree, int cell, int max_cost,
                                       float m255, int min_agree, int min_through, uint8_t *refined, float *depth,
                                       hipStream_t st) {
    const int Hc = (vw.H + cell - 1) / cell, Wc = (vw.W + cell - 1) / cell;
    hipLaunchKernelGGL(mh_stereo_refine_kernel, mh_stereo_blocks((size_t)gr.X * gr.Y * gr.Z), dim3(256), 0, st, vw, bust, gr,
                       flags, keys, agree, cell, Hc, Wc, max_cost, m255, min_agree, min_through, refined);
    hipLaunchKernelGGL(mh_stereo_depth_kernel, mh_stereo_blocks((size_t)vw.V * Hc * Wc), dim3(256), 0, st, vw, gr, keys, agree,
                       Hc, Wc, max_cost, min_agree, depth);
    return (int)hipGetLastError();
}
