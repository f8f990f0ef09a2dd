// Scalp sampling of HairGrow.py's __main__ (:880-897): Open3D's TriangleMesh::SamplePointsUniformly with interpolated
// vertex normals, and the epilogue that takes the samples to voxel space, in float64.
//
//   mh_tri_area64_kernel    one lane per triangle: half the norm of (b-a) x (c-a)
//   mh_mesh_sample_kernel   one lane per sample: its triangle by binary search on the allocation bounds (the caller's
//                           B[t] = round(n * cdf[t]), B[nf-1] = n: sample i lies in the first t with B[t] > i), the point
//                           and the normal by the weights (1-sqrt(u0), sqrt(u0)(1-u1), sqrt(u0)u1), then
//                           scalp_points += bust_to_origin, points_to_voxel on float64, the normal divided by its 2-norm
//                           with y/z negated, both cast to float32
//
// Every expression is evaluated in the order a numpy restatement evaluates it (tests/test_mesh_sample_gpu.py);
// -ffp-contract=off keeps the compiler from fusing, sqrt and the divisions are correctly rounded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_device.h"

struct MhVec3d {
    double v[3];
};

__global__ __launch_bounds__(256) void mh_tri_area64_kernel(const double *__restrict__ V, const int32_t *__restrict__ F,
                                                            int nf, double *__restrict__ area) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nf) return;
    const double *a = V + 3 * (size_t)F[3 * t], *b = V + 3 * (size_t)F[3 * t + 1], *c = V + 3 * (size_t)F[3 * t + 2];
    const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];
    const double v0 = c[0] - a[0], v1 = c[1] - a[1], v2 = c[2] - a[2];
    const double x = u1 * v2 - u2 * v1, y = u2 * v0 - u0 * v2, z = u0 * v1 - u1 * v0;
    area[t] = 0.5 * sqrt((x * x + y * y) + z * z);
}

__global__ __launch_bounds__(256) void mh_mesh_sample_kernel(const double *__restrict__ V, const double *__restrict__ VN,
                                                             const int32_t *__restrict__ F, int nf,
                                                             const int64_t *__restrict__ B, const double *__restrict__ U,
                                                             int n, MhVec3d bust, MhVec3d vmin, double vs,
                                                             float *__restrict__ out_pts, float *__restrict__ out_nrm,
                                                             int32_t *__restrict__ out_tri) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = nf - 1;   // B[nf-1] = n > i: the answer exists and is at most nf-1
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (B[mid] > (int64_t)i) hi = mid; else lo = mid + 1;
    }
    const int t = lo;
    const size_t ia = F[3 * t], ib = F[3 * t + 1], ic = F[3 * t + 2];
    const double r1 = sqrt(U[2 * (size_t)i]), r2 = U[2 * (size_t)i + 1];
    const double wa = 1.0 - r1, wb = r1 * (1.0 - r2), wc = r1 * r2;
    double p[3], q[3];
    for (int k = 0; k < 3; ++k) {
        p[k] = (wa * V[3 * ia + k] + wb * V[3 * ib + k]) + wc * V[3 * ic + k];
        q[k] = (wa * VN[3 * ia + k] + wb * VN[3 * ib + k]) + wc * VN[3 * ic + k];
        p[k] = p[k] + bust.v[k];
    }
    p[1] = -p[1];
    p[2] = -p[2];
    const double len = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    for (int k = 0; k < 3; ++k) {
        out_pts[3 * (size_t)i + k] = (float)((p[k] - vmin.v[k]) / vs);
        const double d = q[k] / len;
        out_nrm[3 * (size_t)i + k] = (float)(k ? -d : d);
    }
    if (out_tri) out_tri[i] = t;
}

// ---------------------------------------------------------------------------------------------- launchers
extern "C" int mh_launch_tri_area64(const double *verts, const int32_t *faces, int nf, double *area, hipStream_t st) {
    if (nf <= 0) return 0;
    hipLaunchKernelGGL(mh_tri_area64_kernel, dim3((nf + 255) / 256), dim3(256), 0, st, verts, faces, nf, area);
    return (int)hipGetLastError();
}

extern "C" int mh_launch_mesh_sample(const double *verts, const double *normals, const int32_t *faces, int nf,
                                     const int64_t *bounds, const double *uniforms, int n, const double *bust,
                                     const double *vmin, double vs, float *out_pts, float *out_nrm, int32_t *out_tri,
                                     hipStream_t st) {
    if (n <= 0) return 0;
    MhVec3d b, m;
    for (int k = 0; k < 3; ++k) {
        b.v[k] = bust[k];
        m.v[k] = vmin[k];
    }
    hipLaunchKernelGGL(mh_mesh_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, st, verts, normals, faces, nf, bounds,
                       uniforms, n, b, m, vs, out_pts, out_nrm, out_tri);
    return (int)hipGetLastError();
}
