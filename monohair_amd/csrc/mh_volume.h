// mh_volume.h -- what the volume kernels share (hairvolume.hip, hairfill.hip, haircarve.hip; gfx950 only): the principal axis
// of a voxel's symmetric 3x3 tensor and the world centre of a voxel, each stated ONCE.  include/mh_pmvo.h, "Strand volume",
// Resolve: float64, + - * / sqrt in the order written, nothing fused (the files are compiled with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include "mh_launch.h"

// the float32 world centre of voxel (x, y, z): the inverse of p2v, evaluated in float64 and rounded once
__device__ __forceinline__ void mh_fill_centre(const MhVolGrid &gr, int x, int y, int z, float &X0, float &X1, float &X2) {
    X0 = (float)(gr.vmin[0] + (double)x * gr.vs);
    X1 = (float)(-(gr.vmin[1] + (double)y * gr.vs));
    X2 = (float)(-(gr.vmin[2] + (double)z * gr.vs));
}

// M = {xx, yy, zz, xy, xz, yz} with trace = (xx + yy) + zz > 0: v = the column of M with the largest diagonal entry (the first
// on ties), 24 power steps, coh = v.(M v) / trace, the fit's canonical sign (v.y > 0 -> -v).  -> coh; (x, y, z) = v
__device__ __forceinline__ double mh_tensor_axis(double xx, double yy, double zz, double xy, double xz, double yz, double trace,
                                                 double &x, double &y, double &z) {
    if (xx >= yy && xx >= zz) x = xx, y = xy, z = xz;
    else if (yy >= zz) x = xy, y = yy, z = yz;
    else x = xz, y = yz, z = zz;
    for (int it = 0; it < 24; ++it) {
        const double mx = (xx * x + xy * y) + xz * z, my = (xy * x + yy * y) + yz * z, mz = (xz * x + yz * y) + zz * z;
        const double len = sqrt((mx * mx + my * my) + mz * mz);
        x = mx / len, y = my / len, z = mz / len;
    }
    const double mx = (xx * x + xy * y) + xz * z, my = (xy * x + yy * y) + yz * z, mz = (xz * x + yz * y) + zz * z;
    const double coh = ((x * mx + y * my) + z * mz) / trace;
    if (y > 0.0) x = -x, y = -y, z = -z;
    return coh;
}
