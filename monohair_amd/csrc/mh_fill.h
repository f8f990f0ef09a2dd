// mh_fill.h -- the 32-bit fill of the strand evaluation tools (haircapture.hip: the planes of a view; hairvolume.hip: the index
// volume).  A file that includes this header carries the kernel; internal linkage, so nothing is added to the exported surface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One lane per 16-byte-aligned chunk of four words: `lead` words of the first chunk lie in front of p (p is 4-byte aligned).
// A chunk wholly inside [p, p + n) is one 16-byte store, the two ends go word by word; nothing outside is touched.
static __global__ __launch_bounds__(256) void mh_fill_u32_kernel(uint32_t *__restrict__ p, uint32_t value, size_t n,
                                                                 size_t lead) {
    const size_t w = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;      // the chunk's first word, counted from p - lead
    if (w >= lead && w + 4 <= lead + n) {
        *(uint4 *)(p + (w - lead)) = make_uint4(value, value, value, value);
        return;
    }
    for (size_t k = w; k < w + 4; ++k)
        if (k >= lead && k < lead + n) p[k - lead] = value;
}

// p[0 .. nwords) = value (nwords < 2^32: the planes and volumes here have fewer than 2^31 cells of at most two words)
static inline int mh_fill_u32(void *p, uint32_t value, size_t nwords, hipStream_t st) {
    const size_t lead = ((uintptr_t)p >> 2) & 3, chunks = (lead + nwords + 3) / 4;
    hipLaunchKernelGGL(mh_fill_u32_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st, (uint32_t *)p, value,
                       nwords, lead);
    return (int)hipGetLastError();
}
