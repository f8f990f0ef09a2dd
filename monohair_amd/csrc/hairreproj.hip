// hairreproj.hip -- a strand set scored against the 2D maps of the capture it was reconstructed from
// (monohair_amd/hairreproj.py), gfx950 only.  The reference has no counterpart: the specification is the rule written out in
// include/mh_pmvo.h ("Capture agreement") and restated in numpy by tests/hair_reproj_np.py.  Vertices, segments and samples
// are the capture rule's (mh_hairwalk.h, the same device functions as csrc/haircapture.hip), the front plane is its pass A;
// every counter is an INTEGER sum, so the atomics below give the same bits whatever order the waves arrive in.
//
//   mh_support_accumulate_kernel   one lane per segment: its samples classed at their centre pixel (5 gathers: zmin, depth0 and
//                                  the three code planes), the lane's counts summed over the lanes of a wave that share a
//                                  strand, one atomic per (strand, non-zero counter) per wave; the wave's total likewise
//   mh_support_silhouette_kernel   one pass over the plane: predicted / observed pixel counts, wave sum, three atomics
//
// Strands are contiguous runs of segments, so the lanes of a wave hold non-decreasing strand numbers: a segmented inclusive
// scan (a lane adds the lane d below it while that one is of the same strand, d = 1, 2, .. 32) leaves a strand's sum in the
// last of its lanes.  The counts are int32 in the lane (a segment has at most 8192 samples: a wave at most 2^19) and are
// widened at the atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_device.h"
#include "mh_hairwalk.h"

#define MH_SUP_MASK_MIN 52      // PMVO's m > 0.2 on the loaders' decode: codes below 50 decode to 0, 50 / 255 and 51 / 255 are <= 0.2

__global__ __launch_bounds__(256) void mh_support_accumulate_kernel(
    const float *__restrict__ vert, const uint8_t *__restrict__ valid, const int64_t *__restrict__ offs, int S, int n_points,
    int H, int W, float tol, const float *__restrict__ depth0, const float *__restrict__ zmin,
    const uint8_t *__restrict__ ori, const uint8_t *__restrict__ conf, const uint8_t *__restrict__ mask, int conf_min,
    MhCapTable tab, MhSupBounds bd, unsigned long long *__restrict__ strand_counts,
    unsigned long long *__restrict__ view_counts) {
    // the table is looked up by a per-lane code: from the kernel arguments into LDS once per block
    __shared__ float T[360];
    for (int t = threadIdx.x; t < 360; t += 256) T[t] = tab.t[t >> 1][t & 1];
    __syncthreads();

    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int ncols = MH_SUP_COLS + bd.n;
    int s = -1;                                   // lanes past the last segment belong to no strand
    int c[MH_SUP_COLS + MH_SUP_MAX_BOUNDS];       // visible, on hair, confident, dropped, agrees[k]
#pragma unroll
    for (int q = 0; q < MH_SUP_COLS + MH_SUP_MAX_BOUNDS; ++q) c[q] = 0;
    if (i + 1 < n_points) {
        s = mh_strand_of(offs, S, i);
        MhCapSeg sg;
        bool too_long;
        if (mh_cap_segment_in(vert, valid, offs, S, s, i, sg, too_long)) {
            const bool has_dir = sqrt(sg.dr * sg.dr + sg.dc * sg.dc) > 0.0;      // len > 0
            const double qc = (double)sg.qc, qs = (double)sg.qs;
            for (int j = 0; j < sg.n; ++j) {
                int cr, cc;
                float zf;
                if (!mh_cap_sample(sg, j, cr, cc, zf)) continue;
                if (cr < 0 || cr >= H || cc < 0 || cc >= W) continue;            // before any address is formed
                const size_t p = (size_t)cr * W + cc;
                if (depth0 && !(zf <= depth0[p])) continue;
                if (!(zf <= zmin[p] + tol)) continue;
                ++c[0];
                if (mask[p] < MH_SUP_MASK_MIN) continue;
                ++c[1];
                const int code = ori[p];
                if ((int)conf[p] < conf_min || code >= 180) continue;
                ++c[2];
                if (!has_dir) continue;
                const double v = qc * (double)T[2 * code] + qs * (double)T[2 * code + 1];
#pragma unroll
                for (int k = 0; k < MH_SUP_MAX_BOUNDS; ++k) c[MH_SUP_COLS + k] += (k < bd.n && v >= bd.b[k]) ? 1 : 0;
            }
        } else if (too_long) {
            c[3] = 1;
        }
        if (s >= S) s = -1;                       // (i beyond the offsets: a caller's error, counted nowhere)
    }

    const int lane = threadIdx.x & 63;
    // the wave's total first: the butterfly leaves it in every lane
    int tot[MH_SUP_COLS + MH_SUP_MAX_BOUNDS];
#pragma unroll
    for (int q = 0; q < MH_SUP_COLS + MH_SUP_MAX_BOUNDS; ++q) {
        int v = s >= 0 ? c[q] : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        tot[q] = v;
    }
    // the segmented scan: lanes of one strand are adjacent, so equal strands d apart are equal all the way
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int so = __shfl_up(s, d, 64);
        const bool take = lane >= d && so == s;
#pragma unroll
        for (int q = 0; q < MH_SUP_COLS + MH_SUP_MAX_BOUNDS; ++q) {
            const int o = __shfl_up(c[q], d, 64);
            if (take) c[q] += o;
        }
    }
    const int sn = __shfl_down(s, 1, 64);
    if (s >= 0 && (lane == 63 || sn != s)) {
        unsigned long long *row = strand_counts + (size_t)s * ncols;
#pragma unroll
        for (int q = 0; q < MH_SUP_COLS + MH_SUP_MAX_BOUNDS; ++q)
            if (q < ncols && c[q]) atomicAdd(row + q, (unsigned long long)c[q]);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < MH_SUP_COLS + MH_SUP_MAX_BOUNDS; ++q)
            if (q < ncols && tot[q]) atomicAdd(view_counts + q, (unsigned long long)tot[q]);
    }
}

// out3 = {predicted and observed, predicted only, observed only}; predicted: zmin finite, observed: mask >= 52
__global__ __launch_bounds__(256) void mh_support_silhouette_kernel(const float *__restrict__ zmin,
                                                                    const uint8_t *__restrict__ mask, size_t npix,
                                                                    unsigned long long *__restrict__ out3) {
    int both = 0, pred = 0, obs = 0;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (size_t)gridDim.x * 256) {
        const bool a = zmin[p] < __builtin_inff(), b = mask[p] >= MH_SUP_MASK_MIN;
        both += a && b;
        pred += a && !b;
        obs += !a && b;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        both += __shfl_xor(both, d, 64);
        pred += __shfl_xor(pred, d, 64);
        obs += __shfl_xor(obs, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (both) atomicAdd(out3, (unsigned long long)both);
        if (pred) atomicAdd(out3 + 1, (unsigned long long)pred);
        if (obs) atomicAdd(out3 + 2, (unsigned long long)obs);
    }
}

// view_counts [MH_SUP_COLS + bd.n] is zeroed first; strand_counts [S, MH_SUP_COLS + bd.n] is added to
extern "C" int mh_launch_support_accum(const float *vert, const uint8_t *valid, const int64_t *offs, int S, int n_points,
                                       int H, int W, float tol, const float *depth0, const float *zmin, const uint8_t *ori,
                                       const uint8_t *conf, const uint8_t *mask, int conf_min, MhCapTable tab, MhSupBounds bd,
                                       unsigned long long *strand_counts, unsigned long long *view_counts, hipStream_t st) {
    hipError_t e = hipMemsetAsync(view_counts, 0, sizeof(unsigned long long) * (MH_SUP_COLS + bd.n), st);
    if (e != hipSuccess) return (int)e;
    if (n_points < 2) return 0;
    hipLaunchKernelGGL(mh_support_accumulate_kernel, dim3((n_points - 1 + 255) / 256), dim3(256), 0, st, vert, valid, offs, S,
                       n_points, H, W, tol, depth0, zmin, ori, conf, mask, conf_min, tab, bd, strand_counts, view_counts);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_support_silhouette(const float *zmin, const uint8_t *mask, int H, int W, unsigned long long *out3,
                                            hipStream_t st) {
    hipError_t e = hipMemsetAsync(out3, 0, 3 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    const size_t npix = (size_t)H * W;
    const size_t blocks = (npix + 1023) / 1024;      // four pixels per lane, at most 2048 blocks
    hipLaunchKernelGGL(mh_support_silhouette_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, zmin,
                       mask, npix, out3);
    return (int)hipGetLastError();
}
