// capi_comm.cpp -- RCCL through the C ABI: the ONE exchange of the data path -- every rank has fitted a
// disjoint slab of the orientation/occupancy volume, rank `root` ends up with all of it.  librccl is bound at run time
// (dlopen by its soname: in a torch process that is the copy torch already loaded, so both share one RCCL), so the
// single-GPU path does not depend on it.
#include <dlfcn.h>

#include <cstdlib>
#include <cstring>

#include "mh_capi.h"

namespace {
struct MhNcclId {
    char internal[128];   // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES)
};
typedef void *MhNcclComm;
struct MhRccl {
    void *h = nullptr;
    int (*GetUniqueId)(MhNcclId *) = nullptr;
    int (*CommInitRank)(MhNcclComm *, int, MhNcclId, int) = nullptr;
    int (*CommDestroy)(MhNcclComm) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void *, size_t, int, int, MhNcclComm, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, MhNcclComm, hipStream_t) = nullptr;
    int (*Reduce)(const void *, void *, size_t, int, int, int, MhNcclComm, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
MhRccl g_rccl;
const int MH_NCCL_FLOAT32 = 7, MH_NCCL_SUM = 0;   // rccl.h: ncclFloat32, ncclSum

int rccl_load() {
    if (g_rccl.h) return MH_OK;
    // MH_RCCL_LIB=<path>: bind this library instead (a site's own RCCL build; tests/fake_rccl.cpp -- a stand-in compiled
    // against rccl.h that moves the data between processes sharing ONE GPU, so that the nranks > 1 branches below run on a
    // one-GPU box).  It must be loadable: a wrong path is an error, never a silent fall-through to the system library.
    const char *over = getenv("MH_RCCL_LIB");
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    if (over && *over) {
        h = dlopen(over, RTLD_NOW | RTLD_LOCAL);
        if (!h) return fail(MH_ERR_STATE, "MH_RCCL_LIB=%s cannot be loaded: %s", over, dlerror());
    } else {
        for (const char *n : names)
            if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    }
    if (!h) return fail(MH_ERR_STATE, "librccl.so.1 not found: %s", dlerror());
    MhRccl r;
    r.h = h;
#define MH_SYM(field, name)                                                               \
    *(void **)(&r.field) = dlsym(h, name);                                                \
    if (!r.field) return fail(MH_ERR_STATE, "librccl: symbol %s missing", name)
    MH_SYM(GetUniqueId, "ncclGetUniqueId");
    MH_SYM(CommInitRank, "ncclCommInitRank");
    MH_SYM(CommDestroy, "ncclCommDestroy");
    MH_SYM(GroupStart, "ncclGroupStart");
    MH_SYM(GroupEnd, "ncclGroupEnd");
    MH_SYM(Send, "ncclSend");
    MH_SYM(Recv, "ncclRecv");
    MH_SYM(Reduce, "ncclReduce");
    MH_SYM(GetErrorString, "ncclGetErrorString");
#undef MH_SYM
    g_rccl = r;
    return MH_OK;
}
}   // namespace

#define MH_NCCL(call)                                                                                   \
    do {                                                                                                \
        int e_ = (call);                                                                                \
        if (e_ != 0) return fail(MH_ERR_HIP, "%s: %s", #call, g_rccl.GetErrorString ? g_rccl.GetErrorString(e_) : "?"); \
    } while (0)

// The grouped point-to-point exchange both entry points below issue: every peer sends its slab to the root, the root
// receives each one at its place in the dense volume.  The group is closed on every path (a failed call inside an open
// group would otherwise leave the thread's group depth raised for every later call).
static int slab_exchange(int rank, int nranks, int root, const float *own_slab, float *volume, size_t plane,
                         const int32_t *slab_host, MhNcclComm comm, hipStream_t st) {
    MH_NCCL(g_rccl.GroupStart());
    int e = 0;
    const char *what = "";
    if (rank == root) {
        for (int r = 0; r < nranks && e == 0; ++r) {
            const size_t cnt = (size_t)(slab_host[r + 1] - slab_host[r]) * plane;
            if (r == root || cnt == 0) continue;
            e = g_rccl.Recv(volume + (size_t)slab_host[r] * plane, cnt, MH_NCCL_FLOAT32, r, comm, st);
            what = "ncclRecv";
        }
    } else if (own_slab) {
        const size_t cnt = (size_t)(slab_host[rank + 1] - slab_host[rank]) * plane;
        e = g_rccl.Send(own_slab, cnt, MH_NCCL_FLOAT32, root, comm, st);
        what = "ncclSend";
    }
    const int e2 = g_rccl.GroupEnd();
    if (e == 0 && e2 != 0) {
        e = e2;
        what = "ncclGroupEnd";
    }
    if (e != 0) return fail(MH_ERR_HIP, "%s: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "?");
    return MH_OK;
}

extern "C" int mh_comm_unique_id(void *id_out_host) {
    if (!id_out_host) return fail(MH_ERR_ARG, "mh_comm_unique_id: NULL");
    if (int rc = rccl_load()) return rc;
    MH_NCCL(g_rccl.GetUniqueId((MhNcclId *)id_out_host));
    return MH_OK;
}

extern "C" int mh_comm_init(mh_ctx *ctx, const void *id_host, int nranks, int rank, void **comm_out) {
    if (!ctx || !id_host || !comm_out || nranks < 1 || rank < 0 || rank >= nranks)
        return fail(MH_ERR_ARG, "mh_comm_init: bad arguments");
    if (int rc = rccl_load()) return rc;
    MH_HIP(hipSetDevice(ctx->device));
    MhNcclId id;
    memcpy(&id, id_host, sizeof(id));
    MhNcclComm c = nullptr;
    MH_NCCL(g_rccl.CommInitRank(&c, nranks, id, rank));
    *comm_out = c;
    return MH_OK;
}

extern "C" int mh_comm_destroy(void *comm) {
    if (!comm) return MH_OK;
    if (int rc = rccl_load()) return rc;
    MH_NCCL(g_rccl.CommDestroy((MhNcclComm)comm));
    return MH_OK;
}

extern "C" int mh_volume_reduce(mh_ctx *ctx, void *comm, int rank, int nranks, int root, float *volume, int X, int Y,
                                int Z, int C, const int32_t *slab_host, int mode, void *stream) {
    if (!ctx || !comm || !volume || !slab_host || nranks < 1 || rank < 0 || rank >= nranks || root < 0 ||
        root >= nranks || X < 1 || Y < 1 || Z < 1 || C < 1 || (mode != 0 && mode != 1))
        return fail(MH_ERR_ARG, "mh_volume_reduce: bad arguments");
    if (slab_host[0] != 0 || slab_host[nranks] != X) return fail(MH_ERR_ARG, "mh_volume_reduce: slabs must cover [0, X)");
    for (int r = 0; r < nranks; ++r)
        if (slab_host[r] > slab_host[r + 1]) return fail(MH_ERR_ARG, "mh_volume_reduce: slabs must be ascending");
    if (int rc = rccl_load()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t plane = (size_t)Y * Z * C;   // floats per x index: a slab is one contiguous block
    if (mode == 1) {   // dense sum into root (x + 0 is exact, so this is the same volume; C*X*Y*Z floats over every link)
        MH_NCCL(g_rccl.Reduce(volume, volume, plane * X, MH_NCCL_FLOAT32, MH_NCCL_SUM, root, (MhNcclComm)comm, st));
        return MH_OK;
    }
    // mode 0: slab ownership is disjoint, so nothing has to be added: every peer sends its own slab straight to the
    // root over its own xGMI link and the root receives it in place -- (nranks-1)/nranks of the volume in total, each
    // link carrying one slab
    const size_t own = (size_t)(slab_host[rank + 1] - slab_host[rank]) * plane;
    return slab_exchange(rank, nranks, root, own ? volume + (size_t)slab_host[rank] * plane : nullptr, volume, plane,
                         slab_host, (MhNcclComm)comm, st);
}

// mh_volume_gather: the slab gather with slab-sized buffers on the peers.  `slab` holds this rank's own x-slab
// ([slab_host[rank+1]-slab_host[rank], Y, Z, C], contiguous); only the root has the dense volume.  The root's own slab is
// copied into place on the stream unless it already lives there (slab == volume + offset).  Same wire traffic as mode 0
// of mh_volume_reduce; a peer allocates 1/nranks of the volume instead of all of it (2.15 GB at 512^3).
extern "C" int mh_volume_gather(mh_ctx *ctx, void *comm, int rank, int nranks, int root, const float *slab, float *volume,
                                int X, int Y, int Z, int C, const int32_t *slab_host, void *stream) {
    if (!ctx || !comm || !slab_host || nranks < 1 || rank < 0 || rank >= nranks || root < 0 || root >= nranks || X < 1 ||
        Y < 1 || Z < 1 || C < 1)
        return fail(MH_ERR_ARG, "mh_volume_gather: bad arguments");
    if (slab_host[0] != 0 || slab_host[nranks] != X) return fail(MH_ERR_ARG, "mh_volume_gather: slabs must cover [0, X)");
    for (int r = 0; r < nranks; ++r)
        if (slab_host[r] > slab_host[r + 1]) return fail(MH_ERR_ARG, "mh_volume_gather: slabs must be ascending");
    const size_t plane = (size_t)Y * Z * C;
    const size_t mine = (size_t)(slab_host[rank + 1] - slab_host[rank]) * plane;
    if (mine && !slab) return fail(MH_ERR_ARG, "mh_volume_gather: rank %d owns %zu floats but slab is NULL", rank, mine);
    if (rank == root && !volume) return fail(MH_ERR_ARG, "mh_volume_gather: the root needs the dense volume");
    if (int rc = rccl_load()) return rc;
    hipStream_t st = (hipStream_t)stream;
    MH_HIP(hipSetDevice(ctx->device));
    if (rank == root) {
        float *dst = volume + (size_t)slab_host[root] * plane;
        if (mine && dst != slab) MH_HIP(hipMemcpyAsync(dst, slab, mine * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if (nranks == 1) return MH_OK;
    return slab_exchange(rank, nranks, root, mine ? slab : nullptr, volume, plane, slab_host, (MhNcclComm)comm, st);
}
