// The reduces of the extern "C" shim (include/tungsten_hip.h): the framebuffers of several contexts of one process, or of one context per process,
// summed into the root's by RCCL.  Host code only, like the shim's other units beside tungsten_hip.hip (shim_context.h lists them).
#include "shim_context.h"

#include <cstring>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is loaded with dlopen at the first multi-GPU reduce

namespace {
// RCCL through dlopen: single-GPU users of this library never load it
struct RcclApi {
    std::mutex mutex;
    bool tried = false;
    void *lib = nullptr;
    decltype(&ncclCommInitAll) commInitAll = nullptr;
    decltype(&ncclGetUniqueId) getUniqueId = nullptr;
    decltype(&ncclCommInitRank) commInitRank = nullptr;
    decltype(&ncclCommDestroy) commDestroy = nullptr;
    decltype(&ncclReduce) reduce = nullptr;
    decltype(&ncclGroupStart) groupStart = nullptr;
    decltype(&ncclGroupEnd) groupEnd = nullptr;
    decltype(&ncclGetErrorString) errorString = nullptr;
    std::map<std::vector<int>, std::vector<ncclComm_t>> comms;   // one communicator set per device list, kept for the life of the process
    bool load()
    {
        if (tried) return lib != nullptr;
        tried = true;
        // An RCCL the process already has comes first (RTLD_NOLOAD matches by SONAME): a host program that brought its own -- PyTorch-ROCm ships
        // one next to libtorch -- and this library must not end up with two copies whose exported symbols resolve into each other.
        lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) return false;
        commInitAll = reinterpret_cast<decltype(commInitAll)>(dlsym(lib, "ncclCommInitAll"));
        reduce = reinterpret_cast<decltype(reduce)>(dlsym(lib, "ncclReduce"));
        groupStart = reinterpret_cast<decltype(groupStart)>(dlsym(lib, "ncclGroupStart"));
        groupEnd = reinterpret_cast<decltype(groupEnd)>(dlsym(lib, "ncclGroupEnd"));
        errorString = reinterpret_cast<decltype(errorString)>(dlsym(lib, "ncclGetErrorString"));
        getUniqueId = reinterpret_cast<decltype(getUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
        commInitRank = reinterpret_cast<decltype(commInitRank)>(dlsym(lib, "ncclCommInitRank"));
        commDestroy = reinterpret_cast<decltype(commDestroy)>(dlsym(lib, "ncclCommDestroy"));
        if (!commInitAll || !reduce || !groupStart || !groupEnd || !errorString || !getUniqueId || !commInitRank || !commDestroy) { dlclose(lib); lib = nullptr; }
        return lib != nullptr;
    }
} g_rccl;
} // namespace

void tghipDestroyRankComm(void *comm)
{
    std::lock_guard<std::mutex> lock(g_rccl.mutex);
    if (comm && g_rccl.load()) (void)g_rccl.commDestroy(static_cast<ncclComm_t>(comm));
}

extern "C" {

int tghip_reduce_framebuffers(tghip_ctx *const *ctxs, int n, int root, float *rgb_sum, uint32_t *count, size_t npixels)
{
    if (!ctxs || n < 1 || root < 0 || root >= n) return TGHIP_E_INVALID;
    for (int i = 0; i < n; ++i)
        if (!ctxs[i]) return TGHIP_E_INVALID;
    tghip_ctx *rc = ctxs[root];
    std::vector<int> devices;
    for (int i = 0; i < n; ++i) {
        tghip_ctx *c = ctxs[i];
        if (c->failReduce) { rc->error = "tghip_reduce_framebuffers: forced failure (the \"fail_reduce\" option)"; return TGHIP_E_HIP; }
        if (!c->haveScene) { rc->error = "tghip_reduce_framebuffers: a context has no scene"; return TGHIP_E_NOSCENE; }
        if (c->width != rc->width || c->height != rc->height) { rc->error = "tghip_reduce_framebuffers: the contexts render different images"; return TGHIP_E_INVALID; }
        for (int d : devices)
            if (d == c->device) { rc->error = "tghip_reduce_framebuffers: two contexts on one device (RCCL wants one rank per device; sum on the host instead)"; return TGHIP_E_UNSUPPORTED; }
        devices.push_back(c->device);
        const int w = runOutPass(c);
        if (w != TGHIP_OK) return w;
    }
    if (npixels != size_t(rc->width)*rc->height) { rc->error = "pixel count mismatch"; return TGHIP_E_INVALID; }
    HIP_TRY(rc, hipSetDevice(rc->device));
    int grc;                                     // (the first call, or the context was re-uploaded with a larger image since)
    if ((grc = rc->redSum.grow(rc, npixels*3)) != TGHIP_OK || (grc = rc->redCount.grow(rc, npixels)) != TGHIP_OK) return grc;

    std::lock_guard<std::mutex> lock(g_rccl.mutex);
    if (!g_rccl.load()) { rc->error = "tghip_reduce_framebuffers: librccl.so could not be loaded"; return TGHIP_E_UNSUPPORTED; }
    auto ncclTry = [&](ncclResult_t r, const char *what) {
        if (r == ncclSuccess) return true;
        rc->error = std::string(what) + ": " + g_rccl.errorString(r);
        return false;
    };
    std::vector<ncclComm_t> &comms = g_rccl.comms[devices];
    if (comms.empty()) {
        comms.resize(size_t(n));
        if (!ncclTry(g_rccl.commInitAll(comms.data(), n, devices.data()), "ncclCommInitAll")) { g_rccl.comms.erase(devices); return TGHIP_E_HIP; }
    }
    // two reductions per rank (radiance sums, sample counts) in one group; every rank's calls run on its own stream
    if (!ncclTry(g_rccl.groupStart(), "ncclGroupStart")) { g_rccl.comms.erase(devices); return TGHIP_E_HIP; }
    bool ok = true;
    for (int i = 0; i < n && ok; ++i) {
        tghip_ctx *c = ctxs[i];
        ok = ncclTry(g_rccl.reduce(c->frameSum(), i == root ? rc->redSum.get() : nullptr, npixels*3, ncclFloat32, ncclSum, root, comms[size_t(i)], c->stream), "ncclReduce")
          && ncclTry(g_rccl.reduce(c->frameCount(), i == root ? rc->redCount.get() : nullptr, npixels, ncclUint32, ncclSum, root, comms[size_t(i)], c->stream), "ncclReduce");
    }
    if (!ncclTry(g_rccl.groupEnd(), "ncclGroupEnd") || !ok) { g_rccl.comms.erase(devices); return TGHIP_E_HIP; }   // (a communicator set that failed is not reused)
    for (int i = 0; i < n; ++i) {
        HIP_TRY(rc, hipSetDevice(ctxs[i]->device));
        HIP_TRY(rc, hipStreamSynchronize(ctxs[i]->stream));
    }
    HIP_TRY(rc, hipSetDevice(rc->device));
    if ((grc = copyBack(rc, rgb_sum, rc->redSum.get(), npixels*3*sizeof(float))) != TGHIP_OK || (grc = copyBack(rc, count, rc->redCount.get(), npixels*sizeof(uint32_t))) != TGHIP_OK) return grc;
    HIP_TRY(rc, hipStreamSynchronize(rc->stream));
    return TGHIP_OK;
}

// ---- the same reduce between PROCESSES (one process per GPU, SURVEY.md 8e: torch.distributed.run, mpirun, ...) ----
int tghip_comm_unique_id(void *id, size_t bytes)
{
    static_assert(sizeof(ncclUniqueId) == TGHIP_COMM_ID_BYTES, "TGHIP_COMM_ID_BYTES");
    if (!id || bytes < sizeof(ncclUniqueId)) return TGHIP_E_INVALID;
    std::lock_guard<std::mutex> lock(g_rccl.mutex);
    if (!g_rccl.load()) return TGHIP_E_UNSUPPORTED;
    ncclUniqueId u;
    if (g_rccl.getUniqueId(&u) != ncclSuccess) return TGHIP_E_HIP;
    std::memcpy(id, &u, sizeof(u));
    return TGHIP_OK;
}

int tghip_comm_init_rank(tghip_ctx *ctx, const void *id, size_t bytes, int nranks, int rank)
{
    if (!ctx || !id || bytes < sizeof(ncclUniqueId) || nranks < 1 || rank < 0 || rank >= nranks) return TGHIP_E_INVALID;
    if (ctx->failReduce) { ctx->error = "tghip_comm_init_rank: forced failure (the \"fail_reduce\" option)"; return TGHIP_E_HIP; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lock(g_rccl.mutex);
    if (!g_rccl.load()) { ctx->error = "tghip_comm_init_rank: librccl.so could not be loaded"; return TGHIP_E_UNSUPPORTED; }
    if (ctx->rankComm) { (void)g_rccl.commDestroy(static_cast<ncclComm_t>(ctx->rankComm)); ctx->rankComm = nullptr; }
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    ncclComm_t comm = nullptr;
    const ncclResult_t r = g_rccl.commInitRank(&comm, nranks, u, rank);
    if (r != ncclSuccess) { ctx->error = std::string("ncclCommInitRank: ") + g_rccl.errorString(r); return TGHIP_E_HIP; }
    ctx->rankComm = comm; ctx->rankCount = nranks; ctx->rankIndex = rank;
    return TGHIP_OK;
}

int tghip_reduce_framebuffer_rank(tghip_ctx *ctx, int root, float *rgb_sum, uint32_t *count, size_t npixels)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!ctx->haveScene) return TGHIP_E_NOSCENE;
    if (!ctx->rankComm) { ctx->error = "tghip_reduce_framebuffer_rank: no communicator (tghip_comm_init_rank)"; return TGHIP_E_INVALID; }
    if (root < 0 || root >= ctx->rankCount || npixels != size_t(ctx->width)*ctx->height) { ctx->error = "tghip_reduce_framebuffer_rank: root / pixel count mismatch"; return TGHIP_E_INVALID; }
    if (ctx->failReduce) { ctx->error = "tghip_reduce_framebuffer_rank: forced failure (the \"fail_reduce\" option)"; return TGHIP_E_HIP; }
    const int w = runOutPass(ctx);
    if (w != TGHIP_OK) return w;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool isRoot = ctx->rankIndex == root;
    int grc;
    if (isRoot && ((grc = ctx->redSum.grow(ctx, npixels*3)) != TGHIP_OK || (grc = ctx->redCount.grow(ctx, npixels)) != TGHIP_OK)) return grc;
    ncclComm_t comm = static_cast<ncclComm_t>(ctx->rankComm);
    ncclResult_t r;
    {
        std::lock_guard<std::mutex> lock(g_rccl.mutex);
        r = g_rccl.groupStart();
        if (r == ncclSuccess) r = g_rccl.reduce(ctx->frameSum(), isRoot ? ctx->redSum.get() : nullptr, npixels*3, ncclFloat32, ncclSum, root, comm, ctx->stream);
        if (r == ncclSuccess) r = g_rccl.reduce(ctx->frameCount(), isRoot ? ctx->redCount.get() : nullptr, npixels, ncclUint32, ncclSum, root, comm, ctx->stream);
        const ncclResult_t e = g_rccl.groupEnd();
        if (r == ncclSuccess) r = e;
    }
    if (r != ncclSuccess) { ctx->error = std::string("ncclReduce: ") + g_rccl.errorString(r); return TGHIP_E_HIP; }
    if (isRoot && ((grc = copyBack(ctx, rgb_sum, ctx->redSum.get(), npixels*3*sizeof(float))) != TGHIP_OK || (grc = copyBack(ctx, count, ctx->redCount.get(), npixels*sizeof(uint32_t))) != TGHIP_OK)) return grc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TGHIP_OK;
}

} // extern "C"
