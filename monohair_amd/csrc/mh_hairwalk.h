// mh_hairwalk.h -- the segment walk of the capture rule (include/mh_pmvo.h, "Hair capture": Segment, Sample), shared by the
// kernels that walk projected strands: csrc/haircapture.hip (capture, photograph) and csrc/hairreproj.hip (capture agreement).
// One copy of the arithmetic: float64 on the float32 vertices, + - * / sqrt in one fixed order (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_launch.h"
#include "mh_strands.h"      // the strand lookup

// What the passes need of segment (i, i+1), the same arithmetic in all of them.
struct MhCapSeg {
    double r0, c0, z0, dr, dc, dz;
    int n;
    long long qc, qs;
};

// true: points i and i+1 are consecutive points of strand s = mh_strand_of(i) and both valid
__device__ __forceinline__ bool mh_cap_pair_in(const uint8_t *__restrict__ valid, const int64_t *__restrict__ offs, int S,
                                               int s, int64_t i) {
    return s < S && i + 1 < offs[s + 1] && valid[i] && valid[i + 1];                    // (s = S: i beyond the offsets)
}

// true: points i and i+1 are consecutive points of one strand and both valid
__device__ __forceinline__ bool mh_cap_pair(const uint8_t *__restrict__ valid, const int64_t *__restrict__ offs, int S,
                                            int64_t i) {
    return mh_cap_pair_in(valid, offs, S, mh_strand_of(offs, S, i), i);
}

// the walk from (r0, c0, z0) to (r1, c1, z1), in whatever units the caller's grid has: the steps and the sample count.
// false: the segment is dropped (n > MH_CAP_MAXN)
__device__ __forceinline__ bool mh_cap_walk(MhCapSeg &sg, double r0, double c0, double z0, double r1, double c1, double z1) {
    sg.r0 = r0, sg.c0 = c0, sg.z0 = z0;
    sg.dr = r1 - r0;
    sg.dc = c1 - c0;
    sg.dz = z1 - z0;
    const double m = fmax(fabs(sg.dr), fabs(sg.dc));      // < 2^24: both ends are valid
    const double nn = fmax(1.0, ceil(m));
    if (nn > (double)MH_CAP_MAXN) return false;
    sg.n = (int)nn;
    return true;
}

// The segment that starts at point i of strand s = mh_strand_of(i).  false: there is none (last point of its strand, an
// invalid end), or it is dropped (n > MH_CAP_MAXN: *too_long)
__device__ __forceinline__ bool mh_cap_segment_in(const float *__restrict__ vert, const uint8_t *__restrict__ valid,
                                                  const int64_t *__restrict__ offs, int S, int s, int64_t i, MhCapSeg &sg,
                                                  bool &too_long) {
    too_long = false;
    if (!mh_cap_pair_in(valid, offs, S, s, i)) return false;
    if (!mh_cap_walk(sg, (double)vert[3 * i], (double)vert[3 * i + 1], (double)vert[3 * i + 2], (double)vert[3 * i + 3],
                     (double)vert[3 * i + 4], (double)vert[3 * i + 5])) {
        too_long = true;
        return false;
    }
    const double len = sqrt(sg.dr * sg.dr + sg.dc * sg.dc);
    sg.qc = sg.qs = 0;
    if (len > 0.0) {
        const double ur = sg.dr / len, uc = sg.dc / len;
        const double c2 = uc * uc - ur * ur, s2 = -2.0 * (uc * ur);
        sg.qc = (long long)rint(4096.0 * c2);
        sg.qs = (long long)rint(4096.0 * s2);
    }
    return true;
}

__device__ __forceinline__ bool mh_cap_segment(const float *__restrict__ vert, const uint8_t *__restrict__ valid,
                                               const int64_t *__restrict__ offs, int S, int64_t i, MhCapSeg &sg,
                                               bool &too_long) {
    return mh_cap_segment_in(vert, valid, offs, S, mh_strand_of(offs, S, i), i, sg, too_long);
}

// sample j of a segment: centre pixel and depth; false when the depth is not finite (no fragment)
__device__ __forceinline__ bool mh_cap_sample(const MhCapSeg &sg, int j, int &cr, int &cc, float &zf) {
    const double t = ((double)j + 0.5) / (double)sg.n;
    cr = (int)rint(sg.r0 + t * sg.dr);
    cc = (int)rint(sg.c0 + t * sg.dc);
    zf = (float)(sg.z0 + t * sg.dz);
    return zf < __builtin_inff();
}
