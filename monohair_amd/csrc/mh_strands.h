// mh_strands.h -- the strand lookup, stated ONCE for the kernels of the strand evaluation tools: haircapture.hip and
// hairreproj.hip (through mh_hairwalk.h), hairvolume.hip and hairmetrics.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the strand of point i >= 0: the s with offs[s] <= i < offs[s+1] (offs non-decreasing, offs[0] = 0); S when i >= offs[S]
__device__ __forceinline__ int mh_strand_of(const int64_t *__restrict__ offs, int S, int64_t i) {
    int lo = 0, hi = S;      // first s in [0, S] with offs[s] > i, minus one
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
