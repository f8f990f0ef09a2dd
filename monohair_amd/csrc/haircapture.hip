// haircapture.hip -- a strand set rendered into the four per-view maps PMVO reads (monohair_amd/synth_hair.py), gfx950 only.
// The reference has no counterpart: the specification is the capture rule written out in include/mh_pmvo.h and restated in
// numpy by tests/hair_capture_np.py.  The projection is PMVO's own float32 one (mh_cam_project, mh_ndc_to_pixel: a strand
// point lands on the pixels it is looked up at); everything after it is float64 on those float32 values with + - * / sqrt in
// one fixed order (-ffp-contract=off: nothing is fused), and every per-pixel sum is an INTEGER sum, so the atomics below give
// the same bits whatever order the fragments arrive in.
//
//   mh_capture_project_kernel   one lane per strand point: unrounded (row, col), z255, valid
//   mh_capture_pass_kernel<0>   pass A, one lane per segment: the nearest fragment of every pixel (atomicMin on the bits of a
//                               positive float32), and the count of the segments dropped as too long
//   mh_capture_pass_kernel<1>   pass B, one lane per segment: cnt / C2 / S2 of the fragments within `tol` of the nearest
//   mh_capture_resolve_kernel   one lane per pixel: depth, orientation code, confidence code, mask code
//
// The photograph rule ("Hair photograph" in the same header, restated by tests/hair_photo_np.py) draws the same strands as
// 8-bit gray images on an S x S supersampled grid, with the vertex step above it and the strand lookup and the segment walk of
// mh_hairwalk.h (shared with csrc/hairreproj.hip):
//   mh_photo_shade_kernel       one lane per segment: the Kajiya-Kay diffuse shade q of the world segment, 0..255
//   mh_photo_front_kernel       one lane per segment: atomicMin of (bits(zf) << 32 | q) on every sub-pixel of its fragments
//   mh_photo_resolve_kernel     one lane per pixel: the S^2 keys of its sub-pixels -> gray, cover
//
// A segment makes n <= MH_CAP_MAXN samples of (2 radius + 1)^2 fragments each: a lane's loop is short (hair segments are a few
// pixels long) and its atomics go to a few neighbouring lines of the pixel planes.  Fragments outside the image are skipped
// before any address is formed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_device.h"
#include "mh_fill.h"
#include "mh_hairwalk.h"      // the segment walk and, with mh_strands.h, the strand lookup

__global__ __launch_bounds__(256) void mh_capture_project_kernel(MhCapCam cam, const float *__restrict__ pts, int n, float Hf,
                                                                 float Wf, float *__restrict__ vert,
                                                                 uint8_t *__restrict__ valid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float u, v, z, row, col;
    mh_cam_project(cam.c, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], u, v, z);
    mh_ndc_to_pixel(u, v, Hf, Wf, row, col);
    vert[3 * (size_t)i] = row;
    vert[3 * (size_t)i + 1] = col;
    vert[3 * (size_t)i + 2] = (-z / 2.0f) * 255.0f;
    // (NaN fails every comparison: an invalid vertex)
    valid[i] = (z < -0.1f && __builtin_fabsf(row) < 1048576.0f && __builtin_fabsf(col) < 1048576.0f) ? 1 : 0;
}

// ACCUM = false: pass A (zmin, dropped); true: pass B (cnt, C2, S2)
template <bool ACCUM>
__global__ __launch_bounds__(256) void mh_capture_pass_kernel(const float *__restrict__ vert,
                                                              const uint8_t *__restrict__ valid,
                                                              const int64_t *__restrict__ offs, int S, int n_points, int H,
                                                              int W, int radius, float tol,
                                                              const float *__restrict__ depth0, uint32_t *__restrict__ zmin,
                                                              int32_t *__restrict__ dropped, int32_t *__restrict__ cnt,
                                                              unsigned long long *__restrict__ C2,
                                                              unsigned long long *__restrict__ S2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i + 1 >= n_points) return;
    MhCapSeg sg;
    bool too_long;
    if (!mh_cap_segment(vert, valid, offs, S, i, sg, too_long)) {
        if (!ACCUM && too_long) atomicAdd(dropped, 1);
        return;
    }
    for (int j = 0; j < sg.n; ++j) {
        int cr, cc;
        float zf;
        if (!mh_cap_sample(sg, j, cr, cc, zf)) continue;
        // (|centre| <= 2^20: the additions below cannot overflow)
        const int ra = max(cr - radius, 0), rb = min(cr + radius, H - 1);
        const int ca = max(cc - radius, 0), cb = min(cc + radius, W - 1);
        for (int r = ra; r <= rb; ++r)
            for (int c = ca; c <= cb; ++c) {
                const size_t p = (size_t)r * W + c;
                if (depth0 && zf > depth0[p]) continue;
                if (!ACCUM) {
                    atomicMin(zmin + p, __float_as_uint(zf));      // zf > 0: the bits order as the values do
                } else if (zf <= __uint_as_float(zmin[p]) + tol) {
                    atomicAdd(cnt + p, 1);
                    atomicAdd(C2 + p, (unsigned long long)sg.qc);  // two's complement: the signed sum
                    atomicAdd(S2 + p, (unsigned long long)sg.qs);
                }
            }
    }
}

__global__ __launch_bounds__(256) void mh_capture_resolve_kernel(const float *__restrict__ zmin,
                                                                 const int32_t *__restrict__ cnt,
                                                                 const long long *__restrict__ C2,
                                                                 const long long *__restrict__ S2,
                                                                 const float *__restrict__ depth0, MhCapTable tab,
                                                                 int n_full, size_t npix, float *__restrict__ depth,
                                                                 uint8_t *__restrict__ ori, uint8_t *__restrict__ conf,
                                                                 uint8_t *__restrict__ mask) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int k = cnt[p];
    if (k <= 0) {
        depth[p] = depth0 ? depth0[p] : 255.0f;
        ori[p] = conf[p] = mask[p] = 0;
        return;
    }
    const double c2 = (double)C2[p], s2 = (double)S2[p];
    int best = 0;
    if (c2 != 0.0 || s2 != 0.0) {
        double bv = c2 * (double)tab.t[0][0] + s2 * (double)tab.t[0][1];
        for (int q = 1; q < 180; ++q) {
            const double v = c2 * (double)tab.t[q][0] + s2 * (double)tab.t[q][1];
            if (v > bv) bv = v, best = q;
        }
    }
    const double coh = sqrt(c2 * c2 + s2 * s2) / (4096.0 * (double)k);
    const double dens = fmin(1.0, (double)k / (double)n_full);
    const double code = fmin(255.0, floor((255.0 * coh) * dens + 0.5));
    depth[p] = zmin[p];
    ori[p] = (uint8_t)best;
    conf[p] = (uint8_t)(int)code;
    mask[p] = 255;
}

extern "C" int mh_launch_capture_project(MhCapCam cam, const float *pts, int n, int H, int W, float *vert, uint8_t *valid,
                                         hipStream_t st) {
    hipLaunchKernelGGL(mh_capture_project_kernel, dim3((n + 255) / 256), dim3(256), 0, st, cam, pts, n, (float)H, (float)W,
                       vert, valid);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_capture_zmin(const float *vert, const uint8_t *valid, const int64_t *offs, int S, int n_points,
                                      int H, int W, int radius, const float *depth0, float *zmin, int32_t *dropped,
                                      hipStream_t st) {
    int rc = mh_fill_u32(zmin, 0x7f800000u /* +inf */, (size_t)H * W, st);
    if (rc) return rc;
    if ((rc = mh_fill_u32(dropped, 0u, 1, st))) return rc;
    if (n_points < 2) return 0;
    hipLaunchKernelGGL(mh_capture_pass_kernel<false>, dim3((n_points - 1 + 255) / 256), dim3(256), 0, st, vert, valid, offs,
                       S, n_points, H, W, radius, 0.0f, depth0, (uint32_t *)zmin, dropped, (int32_t *)nullptr,
                       (unsigned long long *)nullptr, (unsigned long long *)nullptr);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_capture_accum(const float *vert, const uint8_t *valid, const int64_t *offs, int S, int n_points,
                                       int H, int W, int radius, float tol, const float *depth0, const float *zmin,
                                       int32_t *cnt, long long *C2, long long *S2, hipStream_t st) {
    const size_t npix = (size_t)H * W;
    int rc = mh_fill_u32(cnt, 0u, npix, st);
    if (rc) return rc;
    if ((rc = mh_fill_u32(C2, 0u, 2 * npix, st))) return rc;
    if ((rc = mh_fill_u32(S2, 0u, 2 * npix, st))) return rc;
    if (n_points < 2) return 0;
    hipLaunchKernelGGL(mh_capture_pass_kernel<true>, dim3((n_points - 1 + 255) / 256), dim3(256), 0, st, vert, valid, offs, S,
                       n_points, H, W, radius, tol, depth0, (uint32_t *)const_cast<float *>(zmin), (int32_t *)nullptr, cnt,
                       (unsigned long long *)C2, (unsigned long long *)S2);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_capture_resolve(const float *zmin, const int32_t *cnt, const long long *C2, const long long *S2,
                                         const float *depth0, MhCapTable tab, int n_full, int H, int W, float *depth,
                                         uint8_t *ori, uint8_t *conf, uint8_t *mask, hipStream_t st) {
    const size_t npix = (size_t)H * W;
    hipLaunchKernelGGL(mh_capture_resolve_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, zmin, cnt, C2, S2,
                       depth0, tab, n_full, npix, depth, ori, conf, mask);
    return (int)hipGetLastError();
}

// ---- the photograph rule

__global__ __launch_bounds__(256) void mh_photo_shade_kernel(const float *__restrict__ pts, const uint8_t *__restrict__ valid,
                                                             const int64_t *__restrict__ offs, int S, int n_points,
                                                             const float *__restrict__ albedo, double lx, double ly, double lz,
                                                             double ambient, uint8_t *__restrict__ shade) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points) return;
    const int s = mh_strand_of(offs, S, i);
    if (s >= S || i + 1 >= offs[s + 1] || !valid[i] || !valid[i + 1]) {
        shade[i] = 0;
        return;
    }
    // (both ends valid: the world points are finite)
    const double tx = (double)pts[3 * i + 3] - (double)pts[3 * i];
    const double ty = (double)pts[3 * i + 4] - (double)pts[3 * i + 1];
    const double tz = (double)pts[3 * i + 5] - (double)pts[3 * i + 2];
    const double tt = (tx * tx + ty * ty) + tz * tz;
    const double tl = (tx * lx + ty * ly) + tz * lz;
    double sn = 0.0;
    if (tt > 0.0) sn = sqrt(fmax(0.0, 1.0 - (tl * tl) / tt));
    const double v = (255.0 * (double)albedo[s]) * (ambient + (1.0 - ambient) * sn);
    shade[i] = v > 0.0 ? (uint8_t)(int)fmin(255.0, rint(v)) : 0;      // (NaN fails the comparison)
}

// ss: the supersampling factor; H, W: the image; the key plane is [ss H, ss W]
__global__ __launch_bounds__(256) void mh_photo_front_kernel(const float *__restrict__ vert, const uint8_t *__restrict__ valid,
                                                             const int64_t *__restrict__ offs, int S, int n_points,
                                                             const uint8_t *__restrict__ shade, int H, int W, int ss,
                                                             int width, const float *__restrict__ depth0,
                                                             unsigned long long *__restrict__ keys,
                                                             int32_t *__restrict__ dropped) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i + 1 >= n_points) return;
    if (!mh_cap_pair(valid, offs, S, i)) return;
    const double k = (double)ss, h = (double)(ss - 1) / 2.0;
    MhCapSeg sg;
    if (!mh_cap_walk(sg, k * (double)vert[3 * i] + h, k * (double)vert[3 * i + 1] + h, (double)vert[3 * i + 2],
                     k * (double)vert[3 * i + 3] + h, k * (double)vert[3 * i + 4] + h, (double)vert[3 * i + 5])) {
        atomicAdd(dropped, 1);
        return;
    }
    const unsigned long long q = shade[i];
    const int HS = H * ss, WS = W * ss;
    for (int j = 0; j < sg.n; ++j) {
        int cr, cc;
        float zf;
        if (!mh_cap_sample(sg, j, cr, cc, zf)) continue;
        // (|centre| <= 2^23 + 4: the additions below cannot overflow)
        const int ra = max(cr - width, 0), rb = min(cr + width, HS - 1);
        const int ca = max(cc - width, 0), cb = min(cc + width, WS - 1);
        const unsigned long long key = ((unsigned long long)__float_as_uint(zf) << 32) | q;      // zf > 0
        for (int r = ra; r <= rb; ++r)
            for (int c = ca; c <= cb; ++c) {
                if (depth0 && zf > depth0[(size_t)(r / ss) * W + c / ss]) continue;
                atomicMin(keys + ((size_t)r * WS + c), key);
            }
    }
}

__global__ __launch_bounds__(256) void mh_photo_resolve_kernel(const unsigned long long *__restrict__ keys,
                                                               const float *__restrict__ depth0, int H, int W, int ss,
                                                               int bust_code, int background_code,
                                                               uint8_t *__restrict__ gray, int32_t *__restrict__ cover) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)H * W) return;
    const int pr = (int)(p / W), pc = (int)(p % W);
    const int empty = (depth0 && depth0[p] < 255.0f) ? bust_code : background_code;
    const size_t WS = (size_t)W * ss;
    const unsigned long long *row = keys + ((size_t)pr * ss) * WS + (size_t)pc * ss;
    int sum = 0, hair = 0;
    for (int a = 0; a < ss; ++a, row += WS)
        for (int b = 0; b < ss; ++b) {
            const unsigned long long key = row[b];
            if (key != ~0ull) sum += (int)(key & 0xffull), ++hair;
            else sum += empty;
        }
    const int s2 = ss * ss;
    gray[p] = (uint8_t)((2 * sum + s2) / (2 * s2));
    if (cover) cover[p] = hair;
}

extern "C" int mh_launch_photo_shade(const float *pts, const uint8_t *valid, const int64_t *offs, int S, int n_points,
                                     const float *albedo, double lx, double ly, double lz, double ambient, uint8_t *shade,
                                     hipStream_t st) {
    if (n_points < 1) return 0;
    hipLaunchKernelGGL(mh_photo_shade_kernel, dim3((n_points + 255) / 256), dim3(256), 0, st, pts, valid, offs, S, n_points,
                       albedo, lx, ly, lz, ambient, shade);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_photo_front(const float *vert, const uint8_t *valid, const int64_t *offs, int S, int n_points,
                                     const uint8_t *shade, int H, int W, int ss, int width, const float *depth0,
                                     unsigned long long *keys, int32_t *dropped, hipStream_t st) {
    int rc = mh_fill_u32(keys, 0xffffffffu, 2 * ((size_t)H * ss * W * ss), st);      // (the all-ones 64-bit keys)
    if (rc) return rc;
    if ((rc = mh_fill_u32(dropped, 0u, 1, st))) return rc;
    if (n_points < 2) return 0;
    hipLaunchKernelGGL(mh_photo_front_kernel, dim3((n_points - 1 + 255) / 256), dim3(256), 0, st, vert, valid, offs, S,
                       n_points, shade, H, W, ss, width, depth0, keys, dropped);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_photo_resolve(const unsigned long long *keys, const float *depth0, int H, int W, int ss,
                                       int bust_code, int background_code, uint8_t *gray, int32_t *cover, hipStream_t st) {
    const size_t npix = (size_t)H * W;
    hipLaunchKernelGGL(mh_photo_resolve_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, keys, depth0, H, W, ss,
                       bust_code, background_code, gray, cover);
    return (int)hipGetLastError();
}
