// Scalp diffusion (the reference's diffusion_scalp, Utils/PMVO_utils.py:467-593): fills the gap between the scalp and the
// reconstructed hair shell of the volume HairGrow.py reads when `scalp_diffusion` is set.
//
//   mh_diffuse_walk_kernel    one lane per scalp sample: the walk along the normal in steps of one voxel (:494-536), float32
//                             in torch's order.  The walk ends on an occupied voxel whose orientation agrees with the normal
//                             (cosine > 0.5 either way); otherwise the normal is bent towards that orientation and the walk
//                             restarts from the sample, nine times at the most.
//   mh_diffuse_arc_kernel     one lane per emitted row (an accepted walk of `step` steps emits step + 1): the cubic Hermite
//                             arc from the sample to the end point (:545-547) evaluated in float64 the way scipy's PPoly
//                             does (power form: res += c * z, z *= x), its forward-difference tangent (:548), the unit
//                             tangent (:560) and the voxel of the row (:561).
//   mh_diffuse_splat_kernel   one lane per touched voxel: the rows of the voxel added one after another in row order into a
//                             float32 accumulator through a float64 sum (:563-567), then the combination with the volume
//                             (:568-592).  The rows arrive grouped by a stable sort on the voxel (mh_launch_sort_keys,
//                             mh_launch_segment_heads), so the order of the additions is the reference's and no atomic is used.
//
// The volume is occ [Z,Y,X] and ori [3][Z,Y,X] (planar), float32, as the .mat files hold them (no y/z flip).  Every
// expression is evaluated in the order tests/scalp_diffusion_np.py restates it; -ffp-contract=off keeps the compiler from
// fusing, the only fused multiply-adds are the explicit ones of torch.linalg.norm (sqrt of an fma chain, float32 and float64).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_device.h"

#define MH_DF_ACCEPTED 0    // the walk ended on hair that agrees with the normal
#define MH_DF_INSIDE 1      // the sample lies in an occupied voxel (step == 0)
#define MH_DF_STEPS 2       // ten steps without an end
#define MH_DF_RESTARTS 3    // nine restarts without an end
#define MH_DF_LEFT 4        // the walk left the volume (the reference's indexing raises or wraps there)
#define MH_DF_TRACE_STEP 10
#define MH_DF_MAX_FAIL 8

struct MhDfVol {
    int W, H, Z;
    float vmin[3];     // points_to_voxel's float32 voxel_min
    float vs;          // float32(0.005 / 2): what a float32 tensor is multiplied with and divided by
    double vmin64[3];  // the same voxel_min widened: what float64 points are promoted against
    double vs64;
};

// points_to_voxel(p).type(torch.long) on a float32 point: y and z negated, (p - voxel_min) / voxel_size, truncated toward
// zero -- a coordinate in (-1, 0) gives index 0.  false: outside [0, dim) (or not a number).
__device__ __forceinline__ bool mh_df_voxel32(const MhDfVol &g, float p0, float p1, float p2, int &x, int &y, int &z) {
    const float fx = (p0 - g.vmin[0]) / g.vs, fy = (-p1 - g.vmin[1]) / g.vs, fz = (-p2 - g.vmin[2]) / g.vs;
    if (!(fx > -1.0f && fx < (float)g.W && fy > -1.0f && fy < (float)g.H && fz > -1.0f && fz < (float)g.Z)) return false;
    x = (int)fx;
    y = (int)fy;
    z = (int)fz;
    return true;
}

// torch.linalg.norm(x, 2, dim=-1) of three floats: ATen's norm kernel squares and adds with fused multiply-adds
__device__ __forceinline__ float mh_df_norm32(float a, float b, float c) {
    return sqrtf(__builtin_fmaf(c, c, __builtin_fmaf(b, b, a * a)));
}
__device__ __forceinline__ double mh_df_norm64(double a, double b, double c) {
    return sqrt(__builtin_fma(c, c, __builtin_fma(b, b, a * a)));
}

__global__ __launch_bounds__(256) void mh_diffuse_walk_kernel(MhDfVol g, const float *__restrict__ occ,
                                                              const float *__restrict__ ori,
                                                              const float *__restrict__ pts, const float *__restrict__ nrm,
                                                              int n, int32_t *__restrict__ status,
                                                              int32_t *__restrict__ steps, float *__restrict__ end_pt,
                                                              float *__restrict__ first_n, float *__restrict__ last_n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t nvox = (size_t)g.W * g.H * g.Z;
    const float q0 = pts[3 * (size_t)i], q1 = pts[3 * (size_t)i + 1], q2 = pts[3 * (size_t)i + 2];
    float p0 = q0, p1 = q1, p2 = q2;
    float n0 = nrm[3 * (size_t)i], n1 = nrm[3 * (size_t)i + 1], n2 = nrm[3 * (size_t)i + 2];
    float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;      // normal_bias
    float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;      // normal_set[0]
    float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;      // normal_set[-1]
    int step = 0, fail = 0, st;
    for (;;) {
        if (fail > MH_DF_MAX_FAIL) {
            st = MH_DF_RESTARTS;
            break;
        }
        int x, y, z;
        if (!mh_df_voxel32(g, p0, p1, p2, x, y, z)) {
            st = MH_DF_LEFT;
            break;
        }
        const size_t v = ((size_t)z * g.H + y) * g.W + x;
        if (occ[v] == 0.0f && step < MH_DF_TRACE_STEP) {
            const float t0 = 0.8f * n0 + 0.2f * b0, t1 = 0.8f * n1 + 0.2f * b1, t2 = 0.8f * n2 + 0.2f * b2;
            const float len = mh_df_norm32(t0, t1, t2);
            n0 = t0 / len;
            n1 = t1 / len;
            n2 = t2 / len;
            if (step == 0) {
                f0 = n0;
                f1 = n1;
                f2 = n2;
            }
            p0 = p0 + n0 * g.vs;
            p1 = p1 + n1 * g.vs;
            p2 = p2 + n2 * g.vs;
            ++step;
            continue;
        }
        if (step == 0) {
            st = MH_DF_INSIDE;
            break;
        }
        if (step >= MH_DF_TRACE_STEP) {
            st = MH_DF_STEPS;
            break;
        }
        const float g0 = ori[v], g1 = ori[nvox + v], g2 = ori[2 * nvox + v];
        // torch.cosine_similarity: x / max(|x|, 1e-8) . y / max(|y|, 1e-8); of -grow_dir it is the exact negative
        const float na = fmaxf(mh_df_norm32(g0, g1, g2), 1e-8f), nb = fmaxf(mh_df_norm32(n0, n1, n2), 1e-8f);
        const float c = ((g0 / na) * (n0 / nb) + (g1 / na) * (n1 / nb)) + (g2 / na) * (n2 / nb);
        if (c > 0.5f) {
            l0 = g0, l1 = g1, l2 = g2;
            st = MH_DF_ACCEPTED;
            break;
        }
        if (-c > 0.5f) {
            l0 = -g0, l1 = -g1, l2 = -g2;
            st = MH_DF_ACCEPTED;
            break;
        }
        // restart from the sample; normal_copy keeps what the failed walk left in it
        p0 = q0, p1 = q1, p2 = q2;
        if (c < 0.0f) b0 = -g0, b1 = -g1, b2 = -g2;
        else b0 = g0, b1 = g1, b2 = g2;
        step = 0;
        ++fail;
    }
    status[i] = st;
    steps[i] = step;
    end_pt[3 * (size_t)i] = p0, end_pt[3 * (size_t)i + 1] = p1, end_pt[3 * (size_t)i + 2] = p2;
    first_n[3 * (size_t)i] = f0, first_n[3 * (size_t)i + 1] = f1, first_n[3 * (size_t)i + 2] = f2;
    last_n[3 * (size_t)i] = l0, last_n[3 * (size_t)i + 1] = l1, last_n[3 * (size_t)i + 2] = l2;
}

// scipy's CubicHermiteSpline on x = (0, 1) (interpolate/_cubic.py: the coefficients; _ppoly.evaluate: the evaluation)
struct MhDfArc {
    double c0, c1, c2, c3;
};
__device__ __forceinline__ MhDfArc mh_df_arc(float y0, float y1, float d0, float d1) {
    const double a = (double)y0, b = (double)y1, da = (double)d0, db = (double)d1;
    const double slope = (b - a) / 1.0;
    const double t = ((da + db) - 2.0 * slope) / 1.0;
    MhDfArc r;
    r.c0 = t / 1.0;
    r.c1 = (slope - da) / 1.0 - t;
    r.c2 = da;
    r.c3 = a;
    return r;
}
__device__ __forceinline__ double mh_df_eval(const MhDfArc &a, double x) {
    double res = 0.0, z = 1.0;
    res = res + a.c3 * z;
    z = z * x;
    res = res + a.c2 * z;
    z = z * x;
    res = res + a.c1 * z;
    z = z * x;
    res = res + a.c0 * z;
    return res;
}

__global__ __launch_bounds__(256) void mh_diffuse_arc_kernel(MhDfVol g, const float *__restrict__ pts,
                                                             const float *__restrict__ end_pt,
                                                             const float *__restrict__ first_n,
                                                             const float *__restrict__ last_n,
                                                             const int32_t *__restrict__ steps,
                                                             const int64_t *__restrict__ offs, int n, int rows,
                                                             double *__restrict__ sample, double *__restrict__ tangent,
                                                             double *__restrict__ unit, int32_t *__restrict__ voxel,
                                                             unsigned long long *__restrict__ keys) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    int lo = 0, hi = n - 1;   // the sample i with offs[i] <= r < offs[i+1]: offs[n] = rows > r
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offs[mid + 1] > (int64_t)r) hi = mid; else lo = mid + 1;
    }
    const size_t i = lo;
    const int step = steps[i], k = r - (int)offs[i];
    const float fs = (float)step;
    // np.linspace(0, 1, num=step + 1): k * (1 / step), the last one set to 1
    const double h = 1.0 / (double)step;
    const int ka = k < step ? k : step - 1;            // the tangent of the last row repeats the one before
    const double xa = (double)ka * h, xb = (ka + 1 < step) ? (double)(ka + 1) * h : 1.0;
    double s[3], t[3];
    for (int c = 0; c < 3; ++c) {
        const MhDfArc a = mh_df_arc(pts[3 * i + c], end_pt[3 * i + c], (first_n[3 * i + c] * g.vs) * fs,
                                    (last_n[3 * i + c] * g.vs) * fs);
        const double sa = mh_df_eval(a, xa), sb = mh_df_eval(a, xb);
        s[c] = k < step ? sa : sb;
        t[c] = sb - sa;
    }
    const double len = mh_df_norm64(t[0], t[1], t[2]);
    const double fx = (s[0] - g.vmin64[0]) / g.vs64, fy = (-s[1] - g.vmin64[1]) / g.vs64, fz = (-s[2] - g.vmin64[2]) / g.vs64;
    const bool in = fx > -1.0 && fx < (double)g.W && fy > -1.0 && fy < (double)g.H && fz > -1.0 && fz < (double)g.Z;
    const int x = in ? (int)fx : -1, y = in ? (int)fy : -1, z = in ? (int)fz : -1;
    for (int c = 0; c < 3; ++c) {
        sample[3 * (size_t)r + c] = s[c];
        tangent[3 * (size_t)r + c] = t[c];
        unit[3 * (size_t)r + c] = t[c] / len;
    }
    voxel[3 * (size_t)r] = x, voxel[3 * (size_t)r + 1] = y, voxel[3 * (size_t)r + 2] = z;
    // a row outside the volume sorts behind every voxel and is left out of the splat
    keys[r] = in ? (unsigned long long)(((size_t)z * g.H + y) * g.W + x) : (unsigned long long)((size_t)g.W * g.H * g.Z);
}

__global__ __launch_bounds__(256) void mh_diffuse_splat_kernel(const int32_t *__restrict__ seg_start,
                                                               const unsigned long long *__restrict__ head_keys,
                                                               const int32_t *__restrict__ meta,
                                                               const int32_t *__restrict__ order,
                                                               const double *__restrict__ unit, size_t nvox,
                                                               float *__restrict__ occ, float *__restrict__ ori) {
    const int gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= meta[0]) return;
    const unsigned long long v = head_keys[gi];
    if (v >= (unsigned long long)nvox) return;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, cnt = 0.0f;
    for (int j = seg_start[gi]; j < seg_start[gi + 1]; ++j) {   // ascending rows: the sort is stable
        const double *u = unit + 3 * (size_t)order[j];
        a0 = (float)((double)a0 + u[0]);
        a1 = (float)((double)a1 + u[1]);
        a2 = (float)((double)a2 + u[2]);
        cnt = cnt + 1.0f;
    }
    const float den = fmaxf(cnt, 1e-6f);
    const float o = occ[v], w = 1.0f - o;
    ori[v] = ori[v] + w * (a0 / den);
    ori[nvox + v] = ori[nvox + v] + w * (a1 / den);
    ori[2 * nvox + v] = ori[2 * nvox + v] + w * (a2 / den);
    occ[v] = o + w * 1.0f;
}

// ---------------------------------------------------------------------------------------------- launchers
static MhDfVol mh_df_vol(int W, int H, int Z) {
    MhDfVol g;
    g.W = W, g.H = H, g.Z = Z;
    g.vmin[0] = -0.32f, g.vmin[1] = -0.32f, g.vmin[2] = -0.24f;
    g.vs = (float)(0.005 / 2);
    for (int k = 0; k < 3; ++k) g.vmin64[k] = (double)g.vmin[k];
    g.vs64 = 0.005 / 2;
    return g;
}

extern "C" int mh_launch_diffuse_walk(const float *occ, const float *ori, int W, int H, int Z, const float *pts,
                                      const float *nrm, int n, int32_t *status, int32_t *steps, float *end_pt,
                                      float *first_n, float *last_n, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(mh_diffuse_walk_kernel, dim3((n + 255) / 256), dim3(256), 0, st, mh_df_vol(W, H, Z), occ, ori, pts,
                       nrm, n, status, steps, end_pt, first_n, last_n);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_diffuse_arc(const float *pts, const float *end_pt, const float *first_n, const float *last_n,
                                     const int32_t *steps, const int64_t *offs, int n, int rows, int W, int H, int Z,
                                     double *sample, double *tangent, double *unit, int32_t *voxel,
                                     unsigned long long *keys, hipStream_t st) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(mh_diffuse_arc_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, mh_df_vol(W, H, Z), pts, end_pt,
                       first_n, last_n, steps, offs, n, rows, sample, tangent, unit, voxel, keys);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_diffuse_splat(const int32_t *seg_start, const unsigned long long *head_keys, const int32_t *meta,
                                       const int32_t *order, const double *unit, int rows, int W, int H, int Z, float *occ,
                                       float *ori, hipStream_t st) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(mh_diffuse_splat_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, seg_start, head_keys, meta,
                       order, unit, (size_t)W * H * Z, occ, ori);
    return (int)hipGetLastError();
}
