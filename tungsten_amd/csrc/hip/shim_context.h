// The shim's private header: the context behind the tghip_ctx handle of include/tungsten_hip.h, the small types it is made of and the helpers more
// than one unit of the shim uses.  Shared by the translation units that implement the extern "C" entry points: tungsten_hip.hip (the kernels' unit:
// context, options, upload, launch plan, render pass, tghip_trace_rays, tghip_debug_libm, counters) and the host-only ones -- shim_queries.hip
// (tghip_query_*), shim_images.hip (the transfers, tghip_develop, tghip_nlmeans), shim_debug.hip (tghip_debug_bsdf / _light / _medium), reduce.hip (the RCCL reduces).
#pragma once
#include "pt_kernels.h"
#include "device_array.h"
#include "../host/SceneCheck.hpp"
#include "../host/LaunchChoice.hpp"
#include "../host/PassPlan.hpp"

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

// The streams of a context, kept per device for the life of the process and handed from a destroyed context to the next one created:
// HIP binds a stream to one of a few hardware queues when it is created (GPU_MAX_HW_QUEUES, 4 by default), and the streams of a context
// created after another one was destroyed came out with a binding on which the four parts of the wavefront loop no longer ran side by
// side (materialtest 1280x720x256: 840 Msamples/s in a process's first context, 675 in every later one; the 16-spp passes of the
// as-shipped scene 24 ms against 35 ms).  A renderer that is opened once per frame or per scene keeps its first context's streams this way.
constexpr int TGHIP_MAX_PARTS = 8;        // parts of the pool the wavefront loop may run as ("streams" option, LaunchChoice::parts)
struct StreamSet {
    hipStream_t main = nullptr, part[TGHIP_MAX_PARTS - 1] = {}, abort = nullptr;
};

// The arrays of one upload -- the scene's, the pool's, the per-resolution pass arrays --, freed together
struct DeviceBuffers {
    std::vector<void *> allocs;
    ~DeviceBuffers() { release(); }
    void release() { for (void *p : allocs) (void)hipFree(p); allocs.clear(); }
};

// a launch of the plan: the kernel, its workgroup size and dynamic LDS bytes (the grid is the pool's, or a part of it)
struct ResolvedLaunch { const void *fn = nullptr; int threads = 0; size_t lds = 0; };
// what planLaunches made of the choice (csrc/host/LaunchChoice.hpp) on this device
struct LaunchPlan {
    PassKind kind;
    LaunchChoice choice;
    ResolvedLaunch closest, shadow, shade[2 + PT_NUM_CLASSES], tail;
    int thrShade[3] = {192, 128, 256};    // workgroup sizes of the shading launches, by ShadeSize
    bool tailFits = false;                // a workgroup of k_tail fits a CU
};

// Where a pass of the wavefront loop takes what a render pass takes from the context and its description: the framebuffer it resolves into, the tile
// seeds of a Sobol' pass and -- tghip_query_radiance -- the rays that replace the camera's.
struct PassTarget {
    float *sum = nullptr;                 // W*H*3 floats and W*H counts on the device
    uint32_t *count = nullptr;
    const uint32_t *tileSeeds = nullptr;  // TGHIP_PASS_SOBOL: on the device already; nullptr = the description's host array, through ctx->dTileSeeds
    const float4 *rays = nullptr;         // k_query_paths in front of every closest-hit launch (LaunchChoice::queryPaths): the caller's rays on the device ...
    uint32_t numRays = 0;                 // ... and how many: the pixels from there on are padding
    bool rayPaths = false;
};

struct tghip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t partStream[TGHIP_MAX_PARTS - 1] = {};   // streams of parts 1 .. 7 of the split wavefront loop ("streams" option); part 0 runs on `stream`
    hipStream_t streamOfPart(int k) const { return k ? partStream[k - 1] : stream; }
    hipStream_t classStream[TGHIP_MAX_PARTS][2] = {};   // per part: the streams of the shading classes that run beside the part's own ("class_streams" option)
    hipEvent_t evFork[TGHIP_MAX_PARTS] = {}, evJoin[TGHIP_MAX_PARTS][2] = {};
    hipEvent_t evPart[TGHIP_MAX_PARTS - 1] = {}, evMain = nullptr;
    hipDeviceProp_t prop;
    std::string error = "no error";

    // scene
    bool haveScene = false;
    DeviceBuffers sceneMem;
    DeviceScene scene;
    SceneTraits sc;                       // what checkScene decided about it (csrc/host/SceneCheck.hpp): the facts the launch code branches on, the derived tables
    LaunchOptions opt;                    // the options the choice of a pass's kernels reads (csrc/host/LaunchChoice.hpp) ...
    LaunchPlan lp;                        // ... and what the last upload, option or pass of another kind made of them: choice, kernels, workgroup sizes, LDS bytes
    std::map<std::tuple<const void *, int, size_t>, int> occupancy;   // residentBlocks: the runtime's answers, per kernel, workgroup size and LDS bytes
    int instPhaseMin = 24;                // "inst_phase_min" / "inst_refill_at" (PathState::inst_*)
    int instRefillAt = 48;
    bool topTreeOpt = true;               // "top_tree": 0 = ignore TgHipSceneDesc::top_nodes at the next upload (flat lists walked in record order: faster, not the reference's ties)
    long long tailThreshold = 8192;       // "tail_threshold" (LaunchOptions::tailOpt)
    bool failReduce = false;              // "fail_reduce" option (fault injection for the reduce's callers)
    int wideStride = int(PT_WIDE_NODE_BYTES);   // bytes per device node: 80 (TgHipWideNode), or 128 -- a cache line each ("wide_node_stride" option, at the next upload)
    uint32_t width = 0, height = 0;

    // framebuffer
    DeviceArray<float> fbSum;             // W*H*3 sums and W*H counts; released, with dAux and extMem, when an upload changes the resolution
    DeviceArray<uint32_t> fbCount;
    float *extSum = nullptr;              // tghip_bind_framebuffer: the caller's
    uint32_t *extCount = nullptr;
    float *frameSum() const { return extSum ? extSum : fbSum.get(); }             // the framebuffer passes resolve into: the bound one, or the context's
    uint32_t *frameCount() const { return extCount ? extCount : fbCount.get(); }

    // TGHIP_PASS_SOBOL / TGHIP_PASS_RECORDS state
    DeviceBuffers extMem;                 // tile seeds + per-record pass arrays (sized at upload)
    uint32_t *dTileSeeds = nullptr, *dRecIndex = nullptr, *dRecCount = nullptr, *dRecLum = nullptr;
    TgHipSampleRecord *dRecords = nullptr;   // SampleRecords, ceil(W/4) x ceil(H/4)
    DeviceArray<float> lum;               // per-sample luminance of the running pass
    PassPlan plan;                        // what planPass decided about the running pass (csrc/host/PassPlan.hpp); reused from pass to pass, with the shard's tile list
    DeviceArray<uint32_t> dSorted, dChunkStart, dHint;   // gap-free item enumeration of record passes

    // path pool
    DeviceBuffers poolMem;
    PathState pool;
    uint32_t poolSlots = 0;
    uint32_t poolGrid = 0;                // persistent workgroups the pool is laid out for
    uint32_t poolWalkArrays = 0;          // walk arrays the pool carries behind the A_* ones (0: walks are never suspended)
    uint32_t poolWalkWanted = 0;          // ... and how many the scene it was laid out for asked for (more than fit the 32-bit offsets: none)
    uint32_t *hostLive = nullptr;         // pinned mirror of PathState::live for the loop condition
    unsigned long long walkStats[2][PT_WALK_STATS] = {{0}, {0}};   // BlockStats::walk summed over workgroups and folds (tghip_get_walk_stats)
    std::vector<BlockCtl> hostCtl;        // scratch for tghip_get_counters
    std::vector<BlockStats> hostStats;

    // options
    // path pool size.  Every kernel of an iteration costs a fixed 140-180 us on top of the time that grows with its rays -- the
    // longest walks / the latency of one shading turn, measured by doubling the pool: materialtest closest-hit 246 -> 348 us, shadow
    // 347 -> 518 us, k_shade 421 -> 665 us per launch for twice the rays -- so the pool is as large as the 32-bit slot offsets allow
    // (8 M slots x 272 B = 2.2 GB of the 288 GB): 1280x720x256 669 -> 745 (4 M) -> 818 (8 M) Msamples/s, mesh1m 404 -> 472 -> 507
    long long maxSlots = 1ll << 23;
    bool maxSlotsSet = false;             // "max_slots" was given explicitly
    long long maxItems = 1ll << 26;       // work items per batch (partial-sum buffer = 16 B each)
    int chunkSamples = 0;                 // "chunk_samples": samples per work item; 0 = 4, or one when the pass is short (csrc/host/PassPlan.cpp)
    DeviceArray<float4> partial;

    // shading classes of the uploaded scene (rec_class) and the kernel variants chosen for them
    DeviceArray<TgHipAuxPixel> dAux;      // auxiliary output buffers (allocated by the first TGHIP_PASS_AUX pass)
    DeviceArray<float> dSamples;          // TGHIP_PASS_SAMPLES: per-sample radiance of the last such pass, samplesFloats of them
    size_t samplesFloats = 0;
    // tghip_develop: where the kernels write when the caller's outputs are host memory (grown on demand), the depth output's maximum, the option
    // that hands the work back to the caller's host code, the kernels' time
    DeviceArray<float> developHdr;
    DeviceArray<uint8_t> developLdr;
    DeviceArray<uint32_t> developMax;
    bool developHost = false;             // "develop_host"
    double developMs = 0.0;
    // tghip_nlmeans: the three input planes and the result on the device when they are not the caller's device memory (grown on demand), the
    // "nlmeans_batch" option (0: the launcher's choice)
    DeviceArray<float> nlmBuf[4];
    uint32_t nlmBatch = 0;
    double nlmMs = 0.0;
    // What tghip_query_rays, _surface, _transmittance and _direct share (no two run at once: each drains the stream before it returns): the counter
    // words the walks claim rays from and the dense launches count survivors in (reset in-stream before every launch that reads them); the rays, the
    // start media and the answers on the device when they are the caller's host memory (grown on demand; a query writes all n of its answers); the
    // "query_blocks" / "query_refill_at" options (0: the measured defaults, RAY_QUERY_BLOCKS_PER_CU / RAY_QUERY_REFILL_AT); tghip_query_rays' time
    DeviceArray<uint32_t> queryCounter;
    DeviceArray<float4> queryRays, queryOut;
    DeviceArray<int> queryMedia;
    int queryBlocks = 0, queryRefillAt = 0;
    double queryMs = 0.0;
    // tghip_query_radiance: the plan of the query's pass (kept like `plan`), the framebuffer of its virtual image and that image's tile seeds -- all
    // equal to radTileSeed where radTileSeedsSet entries are --, the rays on the device when they are the caller's host memory (all grown on demand),
    // the time of the pass and the copy of its answers
    PassPlan radPlan;
    DeviceArray<float> radSum;
    DeviceArray<uint32_t> radCount, radTileSeeds;
    DeviceArray<float4> radRays;
    size_t radTileSeedsSet = 0;
    uint32_t radTileSeed = 0;
    double radMs = 0.0;
    // tghip_query_surface: per ray the hit its walk left and -- instanced scenes -- the instance it was reached through (grown on demand), the event
    // between the two launches, their time and the dense launch's share of it, the "surface_time_stage" option (1: the getter answers with the share)
    DeviceArray<float4> surfHits;
    DeviceArray<int> surfInst;
    hipEvent_t evSurfMid = nullptr;
    double surfMs = 0.0, surfDenseMs = 0.0;
    bool surfTimeDense = false;
    // tghip_query_transmittance: the rays' state between the rounds of its wavefront (csrc/hip/transmittance_query.h: TransmittanceState), the two
    // index lists the rounds alternate between (all grown on demand), the time of the last call's rounds and how many it ran
    DeviceArray<float4> trO, trD, trT, trHits;
    DeviceArray<uint2> trB;
    DeviceArray<int> trInst;
    DeviceArray<uint32_t> trList[2];
    double trMs = 0.0;
    uint32_t trRounds = 0;
    // tghip_query_direct: the items and shadow segments of the chunk under way (csrc/hip/direct_query.h: DirectState), the hits of the chunk's rays,
    // the two index lists the rounds alternate between (all grown on demand, the state to at most DIRECT_QUERY_CHUNK items), the time of the last
    // call's launches
    DeviceArray<float4> dqOrigin, dqO, dqD, dqHits, dqT, dqC, dqE, dqRes, dqRayHits;
    DeviceArray<uint4> dqB;
    DeviceArray<float> dqWeight;
    DeviceArray<int> dqInst, dqRayInst;
    DeviceArray<uint32_t> dqStatus, dqList[2];
    double dqMs = 0.0;
    // tghip_query_vertex: the states on the device when they are the caller's host memory, per live path of the part under way its ray for the walk,
    // the walk's hit and instance and what the front stage leaves the back stage (csrc/hip/vertex_query.h: VertexState), the two index lists the turns
    // alternate between (all grown on demand, to at most VERTEX_QUERY_CHUNK paths); the shadow segments are tghip_query_direct's scratch above.  The
    // time of the last call's launches
    DeviceArray<float4> vqPaths, vqWalkRays, vqHits, vqW, vqP;
    DeviceArray<int> vqInst;
    DeviceArray<uint32_t> vqList[2];
    double vqMs = 0.0;
    void *rankComm = nullptr;             // tghip_comm_init_rank: this process's ncclComm_t (one process per GPU); destroyed with the context (tghipDestroyRankComm)
    int rankCount = 0, rankIndex = 0;
    DeviceArray<float> redSum;            // the reduces (reduce.hip): where the reduced image lands when this context is the root (grown: a re-upload
    DeviceArray<uint32_t> redCount;       // may change the resolution)
    // the tiles of the shard the last pass rendered (plan.ownedList), on the device
    DeviceArray<uint32_t> dOwnedTiles;
    bool hoistOpt = true;                 // "hoist_quad": the scene's one quad tested before the decoupled walks instead of inside them (at the next upload)
                                          // (scene.hoisted_rec and scene.env_tex are sc.hoisted.record / sc.env_tex unless "hoist_quad" / "env_lds" = 0 say -1)
    bool countTraversal = false;
    int checkInterval = 0;                // "check_interval": wavefront iterations between host-side liveness checks; 0 = 16 for batches that refill
                                          // the pool several times (every check drains all streams: materialtest 825 / 835 / 845 Msamples/s for
                                          // 4 / 8 / 16), 4 for short ones (the iterations after the last path ended are wasted)
    int gridRounds = 1;                   // "grid_rounds": launch this many times the resident workgroups (each owns 1/rounds of the slots);
                                          // the dispatcher starts the later ones as the first finish, filling the drain tail of a launch
    // "suspend_lanes" / "suspend_turns" / "suspend_min_queue" (PathState::suspend_*): walk time-slicing of the wide traversal kernels
    int suspendLanes = 12, suspendTurns = 16, suspendMinQueue = 1024;   // (measured, profiles/README.md: materialtest +0.5 %, mesh1m +4 % over none; round 5 on the final kernels, r5_sweep_final_kernels.txt: 12 lanes +0.5 % / +1 % over 16, 8 lanes +0.8 % / -3 %)
    uint32_t numWideNodes = 0;
    int leafBatch = 1;                    // "leaf_batch" (PathState::leaf_batch)
    int leafBatchBvh2 = 0;                // "leaf_batch_bvh2" (PathState::leaf_batch_bvh2); 0 = leaf_batch, or the measured value for two-level scenes
    long long poolPad = 9472;             // bytes between the per-slot arrays of the pool (multiple of 16)
    bool timeKernels = false;             // HIP events around every launch of the wavefront loop (bench.py roofline)
    std::vector<hipEvent_t> evPool;       // ... in pairs, a run of pairs per class of launches (tungsten_hip.hip: Batch::timed)

    // abort (PathTraceIntegrator::abortRender): a host-side request flag, mirrored into one device word the kernels poll.
    // The word is allocated once per context (never with the reallocatable pool), so tghip_abort may write it from any
    // thread at any time; the request is cleared by tghip_render_pass only, so one that lands before the pass's kernels
    // have started is not lost.
    std::atomic<bool> abortRequested{false};
    DeviceArray<uint32_t> abortFlagDev;
    hipStream_t abortStream = nullptr;
    std::mutex abortMutex;                // serialises tghip_abort callers (they share abortStream)

    // async pass state
    bool passPending = false;
    int passResult = TGHIP_OK;
    TgHipPassDesc pendingPass;

    // counters
    TgHipCounters counters;
    hipEvent_t evA = nullptr, evB = nullptr;

    // (the device arrays free themselves: tghip_destroy deletes the context last, with its device current and its streams idle)
    ~tghip_ctx() { if (hostLive) (void)hipHostFree(hostLive); }
};

// reduce.hip: destroys the communicator of tghip_comm_init_rank (tghip_destroy)
void tghipDestroyRankComm(void *comm);
// tungsten_hip.hip: the planned pass `plan` of `pass` over a w x h image, into `target` (tghip_wait's render pass, tghip_query_radiance's query)
int tghipRunPass(tghip_ctx *ctx, const TgHipPassDesc &pass, uint32_t w, uint32_t h, PassPlan &plan, const PassTarget &target);

// What planPass reads of the context's options, for work items of `chunkSamples` samples ("chunk_samples"; tghip_query_radiance: always 1)
inline PassPlanOptions passPlanOptions(const tghip_ctx *ctx, int chunkSamples) { return {uint64_t(std::max<long long>(ctx->maxItems, 256)), uint64_t(ctx->maxSlots), uint32_t(std::max(chunkSamples, 0))}; }
// The pass under way run out, before a call reads or writes what it renders into: one that was aborted is no error of that call's
inline int runOutPass(tghip_ctx *ctx) { const int rc = tghip_wait(ctx); return rc == TGHIP_E_ABORTED ? TGHIP_OK : rc; }

// The launches of `launch` between the context's two timing events, `after` -- the copies back into host memory -- behind them and, once the stream
// has run dry, the launches' milliseconds in `ms`.
template<typename Launch, typename After>
static int timedLaunches(tghip_ctx *ctx, double &ms, Launch launch, After after)
{
    HIP_TRY(ctx, hipEventRecord(ctx->evA, ctx->stream));
    int rc = launch();
    if (rc != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->evB, ctx->stream));
    if ((rc = after()) != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float elapsed = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&elapsed, ctx->evA, ctx->evB));
    ms = elapsed;
    return TGHIP_OK;
}
// ... and what the tghip_*_kernel_time functions answer: the milliseconds the last such call stored
inline int kernelTime(const tghip_ctx *ctx, double tghip_ctx::*stored, double *ms)
{
    if (!ctx || !ms) return TGHIP_E_INVALID;
    *ms = ctx->*stored;
    return TGHIP_OK;
}

// ---- "The caller's pointer, host or device" as a device pointer, with an array of the context as the scratch of host memory ----
// An input of `bytes` bytes: the caller's device memory itself, or `scratch` -- grown to hold them -- behind a copy queued on the context's stream.
template<typename T>
static int stageInput(tghip_ctx *ctx, bool device, const void *user, size_t bytes, DeviceArray<T> &scratch, const T *&dev)
{
    dev = static_cast<const T *>(user);
    if (device) return TGHIP_OK;
    const int rc = scratch.grow(ctx, (bytes + sizeof(T) - 1)/sizeof(T));
    if (rc != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(scratch.get(), user, bytes, hipMemcpyHostToDevice, ctx->stream));
    dev = scratch.get();
    return TGHIP_OK;
}
// An output of `bytes` bytes: the caller's device memory itself, or `scratch`, grown to hold them.  (`user` == nullptr: an output the caller does
// not ask for -- nullptr.)
template<typename T>
static int stageOutput(tghip_ctx *ctx, bool device, void *user, size_t bytes, DeviceArray<T> &scratch, T *&dev)
{
    dev = static_cast<T *>(user);
    if (device || !user) return TGHIP_OK;
    const int rc = scratch.grow(ctx, (bytes + sizeof(T) - 1)/sizeof(T));
    dev = scratch.get();
    return rc;
}
// ... and its way back, queued behind the launches that wrote `dev`: nothing where they wrote the caller's memory, or where the caller asked for nothing
inline int copyBack(tghip_ctx *ctx, void *user, const void *dev, size_t bytes)
{
    if (user && user != dev) HIP_TRY(ctx, hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return TGHIP_OK;
}
