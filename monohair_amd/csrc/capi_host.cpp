// capi_host.cpp -- the part of the C ABI (include/mh_pmvo.h) that never touches the GPU: the error text, the MAT-v5 sparse
// file writer and the host replay of the strand gate.  It includes no HIP header and builds with a plain C++ compiler, so
// that tests/capi_host_main.cpp can run it under sanitizers; keep it that way.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "../../include/mh_pmvo.h"

static thread_local char g_err[512] = "";

// declared in mh_capi.h for the other translation units of the C ABI
__attribute__((visibility("hidden"))) int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *mh_last_error(void) { return g_err; }
extern "C" int mh_version(void) { return 100; }

// The sequential `flag` gate (HairGrow.py:72,144,247,260,292), replayed on the HOST over finished traces: all
// pointers are host pointers.  mode 0: voxel seeds (skip if flag[seed voxel] >= 3 or fewer than 5 points; an accepted
// strand adds 1 to every distinct voxel it touches); mode 1: scalp roots (kept when len > 0; their voxels are set to 1).
extern "C" int mh_strands_accept(int W, int H, int Z, float *flag, const float *pts, const int32_t *first,
                                 const int32_t *len, int stride, const float *seeds, int n, int mode,
                                 uint8_t *accepted) {
    if (!flag || !pts || !first || !len || !seeds || !accepted || n < 0 || stride < 0)
        return fail(MH_ERR_ARG, "mh_strands_accept: bad arguments");
    const size_t nvox = (size_t)W * H * Z;
    int32_t *stamp = new (std::nothrow) int32_t[nvox];
    if (!stamp) return fail(MH_ERR_NOMEM, "mh_strands_accept: out of host memory");
    memset(stamp, 0xff, sizeof(int32_t) * nvox);
    auto clampi = [](int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); };
    for (int i = 0; i < n; ++i) {
        accepted[i] = 0;
        if (mode == 0) {
            const float *s = seeds + 3 * (size_t)i;
            const size_t q = ((size_t)clampi((int)s[2], Z - 1) * H + clampi((int)s[1], H - 1)) * W + clampi((int)s[0], W - 1);
            if (flag[q] >= 3.0f || len[i] < 5) continue;
        } else if (len[i] <= 0) {
            continue;
        }
        accepted[i] = 1;
        const float *p = pts + ((size_t)i * stride + first[i]) * 3;
        for (int k = 0; k < len[i]; ++k) {
            const size_t q = ((size_t)clampi((int)p[3 * k + 2], Z - 1) * H + clampi((int)p[3 * k + 1], H - 1)) * W +
                             clampi((int)p[3 * k], W - 1);
            if (mode == 1) {
                flag[q] = 1.0f;
            } else if (stamp[q] != i) {
                stamp[q] = i;
                flag[q] += 1.0f;
            }
        }
    }
    delete[] stamp;
    return MH_OK;
}

// Host-side IO of the volume files (PMVO.py:753-764 scipy.io.savemat of the dense float64 arrays): the MAT-v5 payload is
// a zero-filled array of which only the occupied voxels are non-zero, so the file is created sparse and the occupied
// elements are scattered into a shared mapping.  What costs time is the first touch of each 4 KB page (allocation +
// zero fill in the page cache); the scatter is therefore split over threads by DESTINATION range, which keeps every
// page with one thread and preserves "later rows win" for duplicate elements (each thread walks the list in order).
extern "C" int mh_mat_write_sparse(const char *path, const void *prefix, size_t prefix_bytes, size_t payload_bytes,
                                   const long long *elem_index, const double *values, size_t n, int threads) {
    if (!path || (!prefix && prefix_bytes) || (payload_bytes & 7) || (n && (!elem_index || !values)))
        return fail(MH_ERR_ARG, "mh_mat_write_sparse: bad arguments");
    const size_t nelem = payload_bytes / 8;
    for (size_t i = 0; i < n; ++i)
        if (elem_index[i] < 0 || (size_t)elem_index[i] >= nelem)
            return fail(MH_ERR_ARG, "mh_mat_write_sparse: element %zu out of range", i);
    const int fd = open(path, O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail(MH_ERR_STATE, "mh_mat_write_sparse: cannot create %s", path);
    const size_t total = prefix_bytes + payload_bytes;
    bool ok = (size_t)write(fd, prefix, prefix_bytes) == prefix_bytes && ftruncate(fd, (off_t)total) == 0;
    if (ok && n) {
        void *m = mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        if (m == MAP_FAILED) {
            ok = false;
        } else {
            char *payload = (char *)m + prefix_bytes;      // (8-byte elements at an 8-byte aligned prefix: MAT v5 pads)
            int T = threads < 1 ? 1 : (threads > 64 ? 64 : threads);
            if (n < 4096) T = 1;
            const size_t span = (nelem + T - 1) / T;
            auto work = [&](int t) {
                const size_t lo = (size_t)t * span, hi = lo + span;
                for (size_t i = 0; i < n; ++i) {
                    const size_t e = (size_t)elem_index[i];
                    if (e >= lo && e < hi) memcpy(payload + e * 8, &values[i], 8);
                }
            };
            if (T == 1) {
                work(0);
            } else {
                std::vector<std::thread> pool;
                for (int t = 0; t < T; ++t) pool.emplace_back(work, t);
                for (auto &th : pool) th.join();
            }
            munmap(m, total);
        }
    }
    close(fd);
    if (!ok) return fail(MH_ERR_STATE, "mh_mat_write_sparse: writing %s failed", path);
    return MH_OK;
}

// The same file in steps, so that the page faults of the zero-filled mapping (4 KB of page cache to clear per touched page:
// 16-19 ms for the two volume files of a pass) can be taken by a background thread while the GPU still works:
//   open  -> creates the file, writes the prefix, maps it;
//   touch -> makes the pages of the given elements resident without changing their contents (reads the element and writes it
//            back: call it BEFORE store, not beside it), each page once -- called early with a superset of the voxels that
//            can become occupied (every candidate point's voxel);
//   store -> the occupied elements, later entries win;   close -> unmap, close.
struct MhMatSparse {
    int fd;
    char *map;
    size_t total, prefix_bytes, nelem;
};

extern "C" int mh_mat_sparse_open(const char *path, const void *prefix, size_t prefix_bytes, size_t payload_bytes,
                                  void **handle) {
    if (handle) *handle = nullptr;      // (whatever fails below: the caller never closes a stale handle)
    if (!path || !handle || (!prefix && prefix_bytes) || (payload_bytes & 7) || (prefix_bytes & 7))
        return fail(MH_ERR_ARG, "mh_mat_sparse_open: bad arguments");
    const int fd = open(path, O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail(MH_ERR_STATE, "mh_mat_sparse_open: cannot create %s", path);
    const size_t total = prefix_bytes + payload_bytes;
    void *m = MAP_FAILED;
    if ((size_t)write(fd, prefix, prefix_bytes) == prefix_bytes && ftruncate(fd, (off_t)total) == 0 && total)
        m = mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    if (m == MAP_FAILED) {
        close(fd);
        return fail(MH_ERR_STATE, "mh_mat_sparse_open: writing %s failed", path);
    }
    *handle = new MhMatSparse{fd, (char *)m, total, prefix_bytes, payload_bytes / 8};
    return MH_OK;
}

extern "C" int mh_mat_sparse_touch(void *handle, const long long *elem_index, size_t n) {
    MhMatSparse *h = (MhMatSparse *)handle;
    if (!h || (n && !elem_index)) return fail(MH_ERR_ARG, "mh_mat_sparse_touch: bad arguments");
    // pages in ASCENDING order, each once (the block allocation of a sparse file is cheaper front to back than in the order
    // the points happen to come in: 3-5 ms instead of 6-11 for the two files of a pass)
    const size_t npage = (h->total >> 12) + 1;
    std::vector<bool> want(npage, false);
    for (size_t i = 0; i < n; ++i) {
        if (elem_index[i] < 0 || (size_t)elem_index[i] >= h->nelem) continue;      // (a hint: out-of-range entries are skipped)
        want[(h->prefix_bytes + (size_t)elem_index[i] * 8) >> 12] = true;
    }
    for (size_t pg = 0; pg < npage; ++pg) {
        if (!want[pg]) continue;
        size_t byte = pg << 12;
        if (byte < h->prefix_bytes) byte = h->prefix_bytes;      // (prefix and total are multiples of 8)
        if (byte + 8 > h->total) continue;
        volatile unsigned long long *q = (volatile unsigned long long *)(h->map + byte);
        *q = *q;      // a WRITE fault (a read would map the shared zero page); the value stays -- touch precedes store
    }
    return MH_OK;
}

extern "C" int mh_mat_sparse_store(void *handle, const long long *elem_index, const double *values, size_t n) {
    MhMatSparse *h = (MhMatSparse *)handle;
    if (!h || (n && (!elem_index || !values))) return fail(MH_ERR_ARG, "mh_mat_sparse_store: bad arguments");
    for (size_t i = 0; i < n; ++i)
        if (elem_index[i] < 0 || (size_t)elem_index[i] >= h->nelem)
            return fail(MH_ERR_ARG, "mh_mat_sparse_store: element %zu out of range", i);
    char *payload = h->map + h->prefix_bytes;
    for (size_t i = 0; i < n; ++i) memcpy(payload + (size_t)elem_index[i] * 8, &values[i], 8);
    return MH_OK;
}

// store straight from the voxel list of the fit: vox [G,3] (x, y, z), element (y + Y*(x + X*z)) [+ c*X*Y*Z for the three
// orientation channels of Ori]; ori == NULL writes 1.0 (Occ).  Later rows win, as the reference's fancy assignments do.
extern "C" int mh_mat_sparse_store_voxels(void *handle, const long long *vox, const void *ori, int ori_is_f64, size_t G, int X,
                                          int Y, int Z) {
    MhMatSparse *h = (MhMatSparse *)handle;
    const size_t plane = (size_t)X * Y * Z;
    if (!h || (G && !vox) || X < 1 || Y < 1 || Z < 1 || h->nelem != plane * (ori ? 3 : 1))
        return fail(MH_ERR_ARG, "mh_mat_sparse_store_voxels: bad arguments");
    for (size_t g = 0; g < G; ++g)
        if (vox[3 * g] < 0 || vox[3 * g] >= X || vox[3 * g + 1] < 0 || vox[3 * g + 1] >= Y || vox[3 * g + 2] < 0 ||
            vox[3 * g + 2] >= Z)
            return fail(MH_ERR_ARG, "mh_mat_sparse_store_voxels: voxel %zu outside the grid", g);
    double *payload = (double *)(h->map + h->prefix_bytes);
    for (size_t g = 0; g < G; ++g) {
        const size_t lin = (size_t)vox[3 * g + 1] + (size_t)Y * ((size_t)vox[3 * g] + (size_t)X * (size_t)vox[3 * g + 2]);
        if (!ori) {
            payload[lin] = 1.0;
        } else {
            for (int c = 0; c < 3; ++c)
                payload[lin + c * plane] = ori_is_f64 ? ((const double *)ori)[3 * g + c] : (double)((const float *)ori)[3 * g + c];
        }
    }
    return MH_OK;
}

extern "C" int mh_mat_sparse_close(void *handle) {
    MhMatSparse *h = (MhMatSparse *)handle;
    if (!h) return MH_OK;
    munmap(h->map, h->total);
    close(h->fd);
    delete h;
    return MH_OK;
}
