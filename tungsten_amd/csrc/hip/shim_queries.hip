// The ray queries of the extern "C" shim (include/tungsten_hip.h): tghip_query_rays, _radiance, _surface, _transmittance, _direct and _vertex with
// their getters.  Host code only: the kernels are behind the launchers of the six *_query.h headers, the pass of tghip_query_radiance is
// tungsten_hip.hip's (tghipRunPass), the context and what the shim's units share are shim_context.h's.
#include "shim_context.h"
#include "ray_query.h"
#include "radiance_query.h"
#include "surface_query.h"
#include "transmittance_query.h"
#include "direct_query.h"
#include "vertex_query.h"
#include "../host/RayQuery.hpp"
#include "../host/RadianceQuery.hpp"
#include "../host/SurfaceQuery.hpp"
#include "../host/TransmittanceQuery.hpp"
#include "../host/DirectQuery.hpp"
#include "../host/VertexQuery.hpp"

// Idle lanes of a wave at which the wide walk of tghip_query_rays claims new rays, and its workgroups per CU (swept: profiles/ray_query_ab.txt)
#define RAY_QUERY_REFILL_AT 48
#define RAY_QUERY_BLOCKS_PER_CU 2

// How tghip_query_rays, _surface, _transmittance and _direct walk on the uploaded scene: the walk tghip_trace_rays answers with, its stack in LDS,
// the refill threshold, whether hits are reached through instances, and the workgroups of a launch over `live` rays -- "query_blocks", or as many as
// stay resident, no more than there are waves for (a workgroup without a ray only reads the counter).
struct QueryWalk {
    RayQueryWalk walk;
    size_t lds;
    uint32_t refillAt, fixedBlocks, residentBlocks;
    bool inst;
    uint32_t blocks(size_t live) const { return fixedBlocks ? fixedBlocks : uint32_t(std::min<size_t>(residentBlocks, ((live + 63)/64 + 3)/4)); }
};
static QueryWalk queryWalk(const tghip_ctx *ctx)
{
    const LaunchChoice &choice = ctx->lp.choice;
    const bool wide = choice.rayWalk == LaunchChoice::RAYS_WIDE;
    QueryWalk q;
    q.inst = choice.rayWalk == LaunchChoice::RAYS_INST;
    q.walk = wide ? RAY_QUERY_WIDE : q.inst ? RAY_QUERY_INST : choice.rayWalk == LaunchChoice::RAYS_FLAT ? RAY_QUERY_FLAT : RAY_QUERY_BVH2;
    q.lds = wide ? size_t(std::max(ctx->sc.wideDepth, 1))*RAY_QUERY_THREADS*sizeof(uint2)
                 : std::max<size_t>(ldsBytes(ctx->sc, choice, LDS_TRACE, RAY_QUERY_THREADS), sizeof(int));
    q.refillAt = uint32_t(ctx->queryRefillAt > 0 ? ctx->queryRefillAt : RAY_QUERY_REFILL_AT);
    q.fixedBlocks = uint32_t(std::max(ctx->queryBlocks, 0));
    q.residentBlocks = uint32_t(ctx->prop.multiProcessorCount)*RAY_QUERY_BLOCKS_PER_CU;
    return q;
}

// A query needs a scene ...
static int queryScene(tghip_ctx *ctx, const char *fn)
{
    if (!ctx->haveScene) ctx->error = std::string(fn) + " before tghip_upload_scene";
    return ctx->haveScene ? TGHIP_OK : TGHIP_E_NOSCENE;
}
// ... and, behind its own argument check, begins like this: the scene; for a batch that is not empty -- the caller answers an empty one -- the pass
// under way run out (one that was aborted is no error of the query's), the device, the counter words.
static int queryBegin(tghip_ctx *ctx, const char *fn, size_t n)
{
    int rc = queryScene(ctx, fn);
    if (rc != TGHIP_OK || n == 0) return rc;
    if ((rc = runOutPass(ctx)) != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, ctx->queryCounter.once(16));
    return TGHIP_OK;
}

// The start medium of a description: TGHIP_MEDIUM_OF_CAMERA is the camera's
template<typename Params>
static void queryStartMedium(const tghip_ctx *ctx, int32_t medium, Params &p)
{
    p.cameraMedium = ctx->sc.cameraMedium;
    p.medium = medium == TGHIP_MEDIUM_OF_CAMERA ? p.cameraMedium : medium;
}

extern "C" {

int tghip_query_rays(tghip_ctx *ctx, const TgHipRayQueryDesc *desc, const TgHipRay *rays, void *out, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    int rc = checkRayQuery(desc, rays, out, n, ctx->error);
    if (rc != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_rays", n)) != TGHIP_OK || n == 0) return rc;
    const bool occluded = desc->mode == TGHIP_QUERY_OCCLUDED, device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    const size_t outBytes = occluded ? n : n*sizeof(TgHipHit);
    const float4 *dRays = nullptr;
    float4 *dOut = nullptr;
    if ((rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->queryRays, dRays)) != TGHIP_OK) return rc;
    if ((rc = stageOutput(ctx, device, out, outBytes, ctx->queryOut, dOut)) != TGHIP_OK) return rc;
    const QueryWalk q = queryWalk(ctx);
    HIP_TRY(ctx, hipMemsetAsync(ctx->queryCounter.get(), 0, sizeof(uint32_t), ctx->stream));
    return timedLaunches(ctx, ctx->queryMs, [&]() -> int {
        HIP_TRY(ctx, rayQueryLaunch(ctx->stream, ctx->scene, q.walk, occluded, dRays, dOut, uint32_t(n), ctx->queryCounter.get(), q.blocks(n), q.refillAt, q.lds));
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, out, dOut, outBytes); });
}

int tghip_query_rays_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::queryMs, ms); }

int tghip_query_radiance(tghip_ctx *ctx, const TgHipRadianceQueryDesc *desc, const TgHipRay *rays, float *rgb_sum, uint32_t *count, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_query_radiance: no description"; return TGHIP_E_INVALID; }
    int rc = queryScene(ctx, "tghip_query_radiance");
    if (rc != TGHIP_OK) return rc;
    if ((rc = checkRadianceQuery(desc, rays, rgb_sum, count, n, ctx->scene.sobol != nullptr, ctx->error)) != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_radiance", n)) != TGHIP_OK || n == 0) return rc;
    // the pass over the virtual image (csrc/host/RadianceQuery.cpp).  Its work items hold ONE sample each, whatever "chunk_samples" says, and k_resolve
    // adds them to the ray's sum one by one (tghipRunPass: group 1): the order of the additions is part of the answer, not a matter of options.
    const RadianceQueryImage im = radianceQueryImage(n);
    const TgHipPassDesc pass = radianceQueryPass(*desc);
    PassPlan &plan = ctx->radPlan;
    if ((rc = planRadianceQuery(*desc, n, passPlanOptions(ctx, 1), plan, ctx->error)) != TGHIP_OK) return rc;
    // the scratch: the image's framebuffer (zero: k_resolve adds), its tile seeds, the rays when they are host memory
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    const size_t npix = size_t(im.width)*im.height;
    if ((rc = ctx->radSum.grow(ctx, npix*3)) != TGHIP_OK) return rc;
    if ((rc = ctx->radCount.grow(ctx, npix)) != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->radSum.get(), 0, npix*3*sizeof(float), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->radCount.get(), 0, npix*sizeof(uint32_t), ctx->stream));
    PassTarget target;
    target.sum = ctx->radSum.get(); target.count = ctx->radCount.get();
    target.rayPaths = true;
    target.numRays = uint32_t(n);
    if (pass.flags & TGHIP_PASS_SOBOL) {
        bool fresh = false;
        if ((rc = ctx->radTileSeeds.grow(ctx, size_t(plan.numTiles), &fresh)) != TGHIP_OK) return rc;
        if (fresh) ctx->radTileSeedsSet = 0;
        if (ctx->radTileSeedsSet < plan.numTiles || ctx->radTileSeed != desc->sobol_seed) {
            HIP_TRY(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->radTileSeeds.get()), int(desc->sobol_seed), size_t(plan.numTiles), ctx->stream));
            ctx->radTileSeedsSet = plan.numTiles; ctx->radTileSeed = desc->sobol_seed;
        }
        target.tileSeeds = ctx->radTileSeeds.get();
    }
    if ((rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->radRays, target.rays)) != TGHIP_OK) return rc;
    // what the pass borrows of the context and gets back: the launch plan of the last render pass's kind (so that the next one plans nothing anew).
    // An abort request left over from an earlier pass -- tghip_wait above has honoured it -- is cleared and NOT put back, as tghip_render_pass clears
    // it where a pass begins; an abort DURING the query ends the query like a pass (TGHIP_E_ABORTED) and stays set until the next pass or query.
    const LaunchPlan lpBefore = ctx->lp;
    const double msTotalBefore = ctx->counters.ms_total;
    ctx->abortRequested.store(false, std::memory_order_release);
    rc = tghipRunPass(ctx, pass, im.width, im.height, plan, target);
    ctx->lp = lpBefore;
    ctx->radMs = ctx->counters.ms_total - msTotalBefore;
    if (rc != TGHIP_OK) return rc;
    // the answers: a launch into the caller's device memory, whose time counts with the pass's, or copies of the image's first n pixels -- the n rays
    double msCopy = 0.0;
    rc = timedLaunches(ctx, msCopy, [&]() -> int {
        if (device) HIP_TRY(ctx, radianceQueryLaunchResults(ctx->stream, ctx->radSum.get(), ctx->radCount.get(), rgb_sum, count, uint32_t(n)));
        if (device) return TGHIP_OK;
        const int crc = copyBack(ctx, rgb_sum, ctx->radSum.get(), n*3*sizeof(float));
        return crc != TGHIP_OK ? crc : copyBack(ctx, count, ctx->radCount.get(), n*sizeof(uint32_t));
    }, []() { return TGHIP_OK; });
    if (rc == TGHIP_OK && device) ctx->radMs += msCopy;
    return rc;
}

int tghip_query_radiance_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::radMs, ms); }

int tghip_query_surface(tghip_ctx *ctx, const TgHipSurfaceQueryDesc *desc, const TgHipRay *rays, TgHipSurface *out, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    int rc = checkSurfaceQuery(desc, rays, out, n, ctx->error);
    if (rc != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_surface", n)) != TGHIP_OK || n == 0) return rc;
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    const size_t outBytes = n*sizeof(TgHipSurface);
    const float4 *dRays = nullptr;
    float4 *dOut = nullptr;
    if ((rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->queryRays, dRays)) != TGHIP_OK) return rc;
    if ((rc = stageOutput(ctx, device, out, outBytes, ctx->queryOut, dOut)) != TGHIP_OK) return rc;
    // what the walk leaves for the dense launch
    const QueryWalk q = queryWalk(ctx);
    if ((rc = ctx->surfHits.grow(ctx, n)) != TGHIP_OK) return rc;
    if (q.inst && (rc = ctx->surfInst.grow(ctx, n)) != TGHIP_OK) return rc;
    int *dInst = q.inst ? ctx->surfInst.get() : nullptr;
    HIP_TRY(ctx, hipMemsetAsync(ctx->queryCounter.get(), 0, sizeof(uint32_t), ctx->stream));
    rc = timedLaunches(ctx, ctx->surfMs, [&]() -> int {
        HIP_TRY(ctx, surfaceQueryLaunchWalk(ctx->stream, ctx->scene, q.walk, dRays, ctx->surfHits.get(), dInst, uint32_t(n), ctx->queryCounter.get(), q.blocks(n), q.refillAt, q.lds));
        HIP_TRY(ctx, hipEventRecord(ctx->evSurfMid, ctx->stream));
        HIP_TRY(ctx, surfaceQueryLaunchDescribe(ctx->stream, ctx->scene, dRays, ctx->surfHits.get(), dInst, dOut, uint32_t(n)));
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, out, dOut, outBytes); });
    if (rc != TGHIP_OK) return rc;
    float dense = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&dense, ctx->evSurfMid, ctx->evB));
    ctx->surfDenseMs = dense;
    return TGHIP_OK;
}

int tghip_query_surface_kernel_time(tghip_ctx *ctx, double *ms)
{
    return kernelTime(ctx, ctx && ctx->surfTimeDense ? &tghip_ctx::surfDenseMs : &tghip_ctx::surfMs, ms);
}

int tghip_query_transmittance(tghip_ctx *ctx, const TgHipTransmittanceQueryDesc *desc, const TgHipRay *rays, const int32_t *media, TgHipTransmittance *out, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_query_transmittance: no description"; return TGHIP_E_INVALID; }
    int rc = queryScene(ctx, "tghip_query_transmittance");
    if (rc != TGHIP_OK) return rc;
    const TgHostTransmittanceScene facts = {uint32_t(ctx->sc.mediumOperand.size()), ctx->sc.mediumOperand.data(), uint32_t(ctx->sc.objectType.size()), ctx->sc.objectType.data()};
    if ((rc = checkTransmittanceQuery(desc, rays, media, out, n, &facts, ctx->error)) != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_transmittance", n)) != TGHIP_OK || n == 0) return rc;
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    const size_t outBytes = n*sizeof(TgHipTransmittance);
    const float4 *dRays = nullptr;
    const int *dMedia = nullptr;
    float4 *dOut = nullptr;
    if ((rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->queryRays, dRays)) != TGHIP_OK) return rc;
    if (media && (rc = stageInput(ctx, device, media, n*sizeof(int32_t), ctx->queryMedia, dMedia)) != TGHIP_OK) return rc;
    if ((rc = stageOutput(ctx, device, out, outBytes, ctx->queryOut, dOut)) != TGHIP_OK) return rc;
    const QueryWalk q = queryWalk(ctx);
    // the state between the rounds.  A scene without a forward-lobe BSDF ends every ray in round 0: nothing but the hits is ever stored.
    const bool oneRound = !ctx->sc.haveForwardBsdf;
    if ((rc = ctx->trHits.grow(ctx, n)) != TGHIP_OK) return rc;
    if (q.inst && (rc = ctx->trInst.grow(ctx, n)) != TGHIP_OK) return rc;
    if (!oneRound) {
        if ((rc = ctx->trO.grow(ctx, n)) != TGHIP_OK || (rc = ctx->trD.grow(ctx, n)) != TGHIP_OK || (rc = ctx->trT.grow(ctx, n)) != TGHIP_OK ||
            (rc = ctx->trB.grow(ctx, n)) != TGHIP_OK || (rc = ctx->trList[0].grow(ctx, n)) != TGHIP_OK || (rc = ctx->trList[1].grow(ctx, n)) != TGHIP_OK)
            return rc;
    }
    const TransmittanceState st = {ctx->trO.get(), ctx->trD.get(), ctx->trT.get(), ctx->trB.get(), ctx->trHits.get(), q.inst ? ctx->trInst.get() : nullptr};
    TransmittanceParams p;
    queryStartMedium(ctx, desc->medium, p);
    p.endCap = desc->end_cap;
    p.bounce = desc->bounce;
    p.startsOnSurface = (desc->flags & TGHIP_TRANSMITTANCE_STARTS_ON_SURFACE) ? 1u : 0u;
    p.endsOnSurface = (desc->flags & TGHIP_TRANSMITTANCE_ENDS_ON_SURFACE) ? 1u : 0u;
    // A ray that goes on has crossed a surface: bounce < max_bounces bounds the rounds whatever the rays do
    const long long maxRounds = oneRound ? 1 : std::max<long long>(1, (long long)ctx->scene.settings.max_bounces - (long long)desc->bounce);
    uint32_t *counters = ctx->queryCounter.get();
    ctx->trRounds = 0;
    return timedLaunches(ctx, ctx->trMs, [&]() -> int {
        uint32_t live = uint32_t(n);
        for (long long round = 0; round < maxRounds && live > 0; ++round) {
            const uint32_t *list = round == 0 ? nullptr : ctx->trList[(round - 1) & 1].get();
            uint32_t *next = ctx->trList[round & 1].get();
            HIP_TRY(ctx, hipMemsetAsync(counters, 0, 2*sizeof(uint32_t), ctx->stream));
            HIP_TRY(ctx, transmittanceQueryLaunchWalk(ctx->stream, ctx->scene, q.walk, dRays, st, list, live, counters, q.blocks(live), q.refillAt, q.lds));
            HIP_TRY(ctx, transmittanceQueryLaunchSegment(ctx->stream, ctx->scene, p, dRays, dMedia, st, list, live, dOut, next, counters + 1));
            ctx->trRounds++;
            if (oneRound) break;
            // the one word a round hands back: how many rays the next one has
            HIP_TRY(ctx, hipMemcpyAsync(&live, counters + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, out, dOut, outBytes); });
}

int tghip_query_transmittance_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::trMs, ms); }

int tghip_query_transmittance_rounds(tghip_ctx *ctx, uint32_t *rounds)
{
    if (!ctx || !rounds) return TGHIP_E_INVALID;
    *rounds = ctx->trRounds;
    return TGHIP_OK;
}

// (ray, sample) items of tghip_query_direct that are under way at once: what its scratch grows to at most (about 300 bytes an item); a larger call
// runs in parts, whole rays where a ray's samples fit and runs of one ray's samples where they do not.  A part changes no bit of an answer: a ray's
// samples are added in sample order, a later part going on from the sums the earlier ones stored.
#define DIRECT_QUERY_CHUNK (1u << 20)
// rounds of shadow walks per part, whatever the scene's max_bounces
#define DIRECT_QUERY_MAX_ROUNDS 257

// The scratch of `items` direct estimates under way at once (tghip_query_direct's items, tghip_query_vertex's live paths): st for the dense stages,
// walkState for the shadow walks -- tghip_query_transmittance's, reading segments through a list: of its state they touch o, d, hits and inst
static int directScratch(tghip_ctx *ctx, const QueryWalk &q, size_t items, DirectState &st, TransmittanceState &walkState)
{
    int rc;
    if ((rc = ctx->dqStatus.grow(ctx, items)) != TGHIP_OK || (rc = ctx->dqWeight.grow(ctx, items)) != TGHIP_OK || (rc = ctx->dqOrigin.grow(ctx, items)) != TGHIP_OK ||
        (rc = ctx->dqO.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqD.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqHits.grow(ctx, 2*items)) != TGHIP_OK ||
        (rc = ctx->dqT.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqB.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqC.grow(ctx, 2*items)) != TGHIP_OK ||
        (rc = ctx->dqE.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqRes.grow(ctx, 2*items)) != TGHIP_OK ||
        (rc = ctx->dqList[0].grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqList[1].grow(ctx, 2*items)) != TGHIP_OK)
        return rc;
    if (q.inst && (rc = ctx->dqInst.grow(ctx, 2*items)) != TGHIP_OK) return rc;
    st = {ctx->dqStatus.get(), ctx->dqWeight.get(), ctx->dqOrigin.get(), ctx->dqO.get(), ctx->dqD.get(), ctx->dqHits.get(),
          q.inst ? ctx->dqInst.get() : nullptr, ctx->dqT.get(), ctx->dqB.get(), ctx->dqC.get(), ctx->dqE.get(), ctx->dqRes.get()};
    walkState = {st.o, st.d, nullptr, nullptr, st.hits, st.inst};
    return TGHIP_OK;
}

// The shadow rounds of the `live` segments a setup or front stage left in dqList[1]: per round the walk, k_direct_round and the one word it hands back,
// how many segments the next one has.  A segment that goes on has crossed a surface (bounce++) and bounce >= max_bounces ends it: bounded.  fn: the caller.
static int directShadowRounds(tghip_ctx *ctx, const char *fn, const QueryWalk &q, const DirectState &st, const TransmittanceState &walkState, uint32_t live)
{
    uint32_t *counters = ctx->queryCounter.get();
    for (int round = 0; live > 0; ++round) {
        if (round >= DIRECT_QUERY_MAX_ROUNDS) { ctx->error = std::string(fn) + ": shadow rays still under way after 257 rounds"; return TGHIP_E_UNSUPPORTED; }
        const uint32_t *list = ctx->dqList[(round + 1) & 1].get();
        uint32_t *next = ctx->dqList[round & 1].get();
        HIP_TRY(ctx, hipMemsetAsync(counters, 0, 2*sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, transmittanceQueryLaunchWalk(ctx->stream, ctx->scene, q.walk, nullptr, walkState, list, live, counters, q.blocks(live), q.refillAt, q.lds));
        HIP_TRY(ctx, directQueryLaunchRound(ctx->stream, ctx->scene, st, list, live, next, counters + 1));
        HIP_TRY(ctx, hipMemcpyAsync(&live, counters + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return TGHIP_OK;
}

int tghip_query_direct(tghip_ctx *ctx, const TgHipDirectQueryDesc *desc, const TgHipRay *rays, const int32_t *media, TgHipDirect *out, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_query_direct: no description"; return TGHIP_E_INVALID; }
    int rc = queryScene(ctx, "tghip_query_direct");
    if (rc != TGHIP_OK) return rc;
    const TgHostDirectScene facts = {uint32_t(ctx->sc.mediumOperand.size()), ctx->sc.mediumOperand.data(), ctx->scene.num_lights, ctx->sc.cameraMedium};
    if ((rc = checkDirectQuery(desc, rays, media, out, n, &facts, ctx->error)) != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_direct", n)) != TGHIP_OK || n == 0) return rc;
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0, volume = (desc->flags & TGHIP_DIRECT_VOLUME) != 0;
    const size_t outBytes = n*sizeof(TgHipDirect);
    const float4 *dRays = nullptr;
    const int *dMedia = nullptr;
    float4 *dOut = nullptr;
    if ((rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->queryRays, dRays)) != TGHIP_OK) return rc;
    if (media && (rc = stageInput(ctx, device, media, n*sizeof(int32_t), ctx->queryMedia, dMedia)) != TGHIP_OK) return rc;
    if ((rc = stageOutput(ctx, device, out, outBytes, ctx->queryOut, dOut)) != TGHIP_OK) return rc;
    const QueryWalk q = queryWalk(ctx);
    // the parts: raysPer rays by samplesPer samples, at most DIRECT_QUERY_CHUNK items
    const uint64_t spp = uint64_t(desc->spp_end) - desc->spp_begin;
    const uint64_t samplesPer = std::min<uint64_t>(spp, DIRECT_QUERY_CHUNK);
    const uint64_t raysPer = std::min<uint64_t>(n, std::max<uint64_t>(1, DIRECT_QUERY_CHUNK/samplesPer));
    DirectState st;
    TransmittanceState walkState;
    if ((rc = directScratch(ctx, q, size_t(raysPer*samplesPer), st, walkState)) != TGHIP_OK) return rc;
    if (!volume && (rc = ctx->dqRayHits.grow(ctx, size_t(raysPer))) != TGHIP_OK) return rc;
    if (!volume && q.inst && (rc = ctx->dqRayInst.grow(ctx, size_t(raysPer))) != TGHIP_OK) return rc;
    const float4 *rayHits = volume ? nullptr : ctx->dqRayHits.get();
    int *rayInst = !volume && q.inst ? ctx->dqRayInst.get() : nullptr;
    DirectParams p;
    p.seed = desc->seed; p.skip = desc->skip; p.bounce = desc->bounce; p.light = desc->light;
    queryStartMedium(ctx, desc->medium, p);
    uint32_t *counters = ctx->queryCounter.get();
    return timedLaunches(ctx, ctx->dqMs, [&]() -> int {
        for (uint64_t r0 = 0; r0 < n; r0 += raysPer) {
            for (uint64_t s0 = desc->spp_begin; s0 < desc->spp_end; s0 += samplesPer) {
                p.ray0 = uint32_t(r0); p.rays = uint32_t(std::min<uint64_t>(raysPer, n - r0));
                p.sample0 = uint32_t(s0); p.samples = uint32_t(std::min<uint64_t>(samplesPer, desc->spp_end - s0));
                p.first = s0 == desc->spp_begin ? 1u : 0u;
                HIP_TRY(ctx, hipMemsetAsync(counters, 0, 2*sizeof(uint32_t), ctx->stream));
                if (!volume && p.first)      // the point: tghip_query_surface's walk as it is (the hits stay for the ray's later parts)
                    HIP_TRY(ctx, surfaceQueryLaunchWalk(ctx->stream, ctx->scene, q.walk, dRays + r0*2u, ctx->dqRayHits.get(), rayInst, p.rays, counters, q.blocks(p.rays), q.refillAt, q.lds));
                HIP_TRY(ctx, directQueryLaunchSetup(ctx->stream, ctx->scene, p, volume, dRays, dMedia, rayHits, rayInst, st, ctx->dqList[1].get(), counters + 1));
                uint32_t live = 0;
                HIP_TRY(ctx, hipMemcpyAsync(&live, counters + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                if ((rc = directShadowRounds(ctx, "tghip_query_direct", q, st, walkState, live)) != TGHIP_OK) return rc;
                HIP_TRY(ctx, directQueryLaunchFinish(ctx->stream, p, volume, dMedia, ctx->scene.num_media, rayHits, st, dOut));
            }
        }
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, out, dOut, outBytes); });
}

int tghip_query_direct_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::dqMs, ms); }

// Paths of tghip_query_vertex that are under way at once: what its scratch grows to at most; a larger call runs in parts, each through all its turns.
// A part changes no bit of an answer: a path's turn reads nothing but its own state and the scene.  The shadow segments use tghip_query_direct's
// scratch, one item per live path.
#define VERTEX_QUERY_CHUNK (1u << 20)

int tghip_query_vertex(tghip_ctx *ctx, const TgHipVertexQueryDesc *desc, const TgHipRay *rays, const int32_t *media, TgHipPath *paths, size_t n, uint32_t *alive)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_query_vertex: no description"; return TGHIP_E_INVALID; }
    int rc = queryScene(ctx, "tghip_query_vertex");
    if (rc != TGHIP_OK) return rc;
    const TgHostVertexScene facts = {uint32_t(ctx->sc.mediumOperand.size()), ctx->sc.mediumOperand.data()};
    if ((rc = checkVertexQuery(desc, rays, media, paths, alive, n, &facts, ctx->error)) != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_vertex", n)) != TGHIP_OK) return rc;
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0, start = (desc->flags & TGHIP_VERTEX_START) != 0;
    // *alive, where it is asked for: device memory, or a host word (see the header)
    auto putAlive = [&](uint32_t count) -> int {
        if (alive && device) HIP_TRY(ctx, hipMemcpy(alive, &count, sizeof count, hipMemcpyDefault));
        else if (alive) *alive = count;
        return TGHIP_OK;
    };
    if (n == 0) return putAlive(0);
    const size_t pathBytes = n*sizeof(TgHipPath);
    const float4 *dRays = nullptr;
    const int *dMedia = nullptr;
    float4 *dPaths = nullptr;
    if (start && (rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->queryRays, dRays)) != TGHIP_OK) return rc;
    if (start && media && (rc = stageInput(ctx, device, media, n*sizeof(int32_t), ctx->queryMedia, dMedia)) != TGHIP_OK) return rc;
    if (start || device) {
        if ((rc = stageOutput(ctx, device, paths, pathBytes, ctx->vqPaths, dPaths)) != TGHIP_OK) return rc;
    } else {
        const float4 *staged = nullptr;
        if ((rc = stageInput(ctx, false, paths, pathBytes, ctx->vqPaths, staged)) != TGHIP_OK) return rc;
        dPaths = ctx->vqPaths.get();
    }
    const QueryWalk q = queryWalk(ctx);
    const size_t items = std::min<size_t>(n, VERTEX_QUERY_CHUNK);
    DirectState st;
    TransmittanceState walkState;
    if ((rc = directScratch(ctx, q, items, st, walkState)) != TGHIP_OK ||
        (rc = ctx->vqWalkRays.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->vqHits.grow(ctx, items)) != TGHIP_OK || (rc = ctx->vqW.grow(ctx, items)) != TGHIP_OK ||
        (rc = ctx->vqP.grow(ctx, items)) != TGHIP_OK || (rc = ctx->vqList[0].grow(ctx, items)) != TGHIP_OK || (rc = ctx->vqList[1].grow(ctx, items)) != TGHIP_OK)
        return rc;
    if (q.inst && (rc = ctx->vqInst.grow(ctx, items)) != TGHIP_OK) return rc;
    const VertexState vs = {ctx->vqW.get(), ctx->vqP.get()};
    int *pathInst = q.inst ? ctx->vqInst.get() : nullptr;
    VertexParams p;
    p.seed = desc->seed; p.sample = desc->sample; p.firstIndex = desc->first_index; p.firstNumber = desc->first_number;
    p.start = start ? 1u : 0u;
    queryStartMedium(ctx, desc->medium, p);
    uint32_t *counters = ctx->queryCounter.get();
    uint32_t aliveTotal = 0;
    rc = timedLaunches(ctx, ctx->vqMs, [&]() -> int {
        for (size_t p0 = 0; p0 < n; p0 += VERTEX_QUERY_CHUNK) {
            p.path0 = uint32_t(p0); p.paths = uint32_t(std::min<size_t>(VERTEX_QUERY_CHUNK, n - p0));
            HIP_TRY(ctx, hipMemsetAsync(counters, 0, 3*sizeof(uint32_t), ctx->stream));
            HIP_TRY(ctx, vertexQueryLaunchBegin(ctx->stream, p, ctx->scene.num_media, dRays, dMedia, dPaths, ctx->vqList[0].get(), ctx->vqWalkRays.get(), counters + 2));
            uint32_t live = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&live, counters + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            for (uint32_t turn = 0; turn < desc->turns && live > 0; ++turn) {
                const uint32_t *list = ctx->vqList[turn & 1].get();
                uint32_t *next = ctx->vqList[(turn + 1) & 1].get();
                HIP_TRY(ctx, hipMemsetAsync(counters, 0, 3*sizeof(uint32_t), ctx->stream));
                // the closest hit: tghip_query_surface's walk as it is, over the live paths' rays
                HIP_TRY(ctx, surfaceQueryLaunchWalk(ctx->stream, ctx->scene, q.walk, ctx->vqWalkRays.get(), ctx->vqHits.get(), pathInst, live, counters, q.blocks(live), q.refillAt, q.lds));
                HIP_TRY(ctx, vertexQueryLaunchFront(ctx->stream, ctx->scene, dPaths, list, live, ctx->vqHits.get(), pathInst, st, vs, ctx->dqList[1].get(), counters + 1));
                uint32_t segments = 0;
                HIP_TRY(ctx, hipMemcpyAsync(&segments, counters + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                if ((rc = directShadowRounds(ctx, "tghip_query_vertex", q, st, walkState, segments)) != TGHIP_OK) return rc;   // tghip_query_direct's, as they are
                HIP_TRY(ctx, vertexQueryLaunchBack(ctx->stream, dPaths, list, live, st, vs, next, ctx->vqWalkRays.get(), counters + 2));
                // the one word a turn hands back: how many paths the next one has
                HIP_TRY(ctx, hipMemcpyAsync(&live, counters + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            }
            aliveTotal += live;
        }
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, paths, dPaths, pathBytes); });
    return rc != TGHIP_OK ? rc : putAlive(aliveTotal);
}

int tghip_query_vertex_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::vqMs, ms); }

} // extern "C"
