// How much light gets along caller rays (tghip_query_transmittance): TraceBase::generalizedShadowRayImpl<false> (TraceBase.cpp:62-125) as a small
// wavefront on the context's stream.  Per round two launches:
//   k_transmittance_walk*     the closest-hit walks of tghip_query_rays (the claim and the decoupled loop of the 8-wide BVH: query_walk.h, shared
//                             with ray_query.hip; the per-ray machines: that unit's loop once more) over the rays still under way, read through
//                             the round's index list from the SoA state -- round 0 reads the caller's rays directly --, storing per ray the hit
//                             and, instanced scenes, the instance record.
//   k_transmittance_segment   dense, one lane per ray of the round: the end-cap test with Embree's box cull for a quad, intersectionInfo and the
//                             forward-lobe bsdfEval of a see-through surface under the all-features mask, the segment's medium transmittance AFTER the
//                             transparency (the reference's order), the bounce limits, selectMedium and the step to the hit.  A ray whose walk is
//                             over gets its 16-byte answer; a ray that goes on has its state stored and its index appended to the next round's list:
//                             one atomicAdd per wave (ballot, popcount, rank) and a contiguous store.
// Two launches because the second stage's IntersectionInfo, BSDF, texture and medium code must not share the walk's registers and must not run at the
// occupancy of whichever lanes of a walking wave just finished -- what k_trace_shadow<., FORWARD>, the per-ray loop of the same function, pays.
// (FEAT_QMC cleared as in debug_units.hip: nothing here draws a number.)
#include "transmittance_query.h"
#include "query_walk.h"

#define TRANSMITTANCE_MASK (BSDF_MASK_ALL & ~FEAT_QMC)

namespace {

// Place j of the round: the ray's index in the batch and its current segment.  (The direct case is loadRay's two loads, written out: through
// loadRay every kernel of this unit came out a few instructions different, profiles/query_walk/kernel_resources_diff.txt.)
PT_DEV RayD loadSegment(const float4 *rays, const TransmittanceState &st, const uint32_t *list, uint32_t j, uint32_t &i)
{
    float4 ro, rd;
    if (list) { i = list[j]; ro = st.o[i]; rd = st.d[i]; }
    else      { i = j; ro = rays[(size_t)j*2u + 0u]; rd = rays[(size_t)j*2u + 1u]; }
    RayD ray;
    ray.o = xyz(ro); ray.d = xyz(rd); ray.tmin = ro.w; ray.tmax = rd.w;
    return ray;
}

}  // namespace

// Scenes on the 8-wide BVH: k_query_rays_wide<false>'s loop (query_walk_wide.h) over the round's segments.  (These scenes hold no instance.)
__global__ __launch_bounds__(RAY_QUERY_THREADS) void k_transmittance_walk_wide(DeviceScene s, const float4 *rays, TransmittanceState st, const uint32_t *list, uint32_t n,
                                                                               uint32_t *counter, uint32_t refillAt)
{
#define QUERY_WALK_OCCLUDED false
#define QUERY_WALK_LOAD(j, index) loadSegment(rays, st, list, j, index)
#define QUERY_WALK_STORE(index, hit, found) st.hits[index] = hit
#include "query_walk_wide.h"
}

// Flat-list, BVH2 and instanced scenes: k_query_rays<WALK, false>'s loop, the instanced walk's hitInst kept
template<int WALK>
__global__ __launch_bounds__(RAY_QUERY_THREADS) void k_transmittance_walk(DeviceScene s, const float4 *rays, TransmittanceState st, const uint32_t *list, uint32_t n,
                                                                          uint32_t *counter)
{
    extern __shared__ int ldsStack[];
    int *stack = ldsStack + threadIdx.x;
    const int stride = RAY_QUERY_THREADS;
    bool exhausted = false;
    while (!exhausted) {
        const uint32_t j = claimRays(counter, true, n, exhausted);
        if (j < n) {
            uint32_t i;
            const RayD ray = loadSegment(rays, st, list, j, i);
            uint32_t nodes = 0, prims = 0;
            int hitInst = -1;
            const float4 hit = WALK == RAY_QUERY_INST ? traverseClosestInst<false, KINDS_ALL>(s, ray, stack, stride, nodes, prims, hitInst)
                                                      : traverseClosest<false, WALK == RAY_QUERY_FLAT>(s, ray, stack, stride, nodes, prims);
            st.hits[i] = hit;
            if (WALK == RAY_QUERY_INST) st.inst[i] = hitInst;
        }
    }
}

// One round of generalizedShadowRayImpl<false>'s loop body for one ray, behind its `_scene->intersect` (the walk's launch).  Every lane of a wave gets
// here -- the ones past the round's end with `live` clear -- because the survivors are counted with a ballot.
__global__ __launch_bounds__(TRANSMITTANCE_QUERY_THREADS) void k_transmittance_segment(DeviceScene s, TransmittanceParams p, const float4 *rays, const int *media,
                                                                                      TransmittanceState st, const uint32_t *list, uint32_t n, float4 *out,
                                                                                      uint32_t *next, uint32_t *nextCount)
{
    const uint32_t j = blockIdx.x*TRANSMITTANCE_QUERY_THREADS + threadIdx.x;
    const bool live = j < n;
    bool goesOn = false;
    uint32_t i = 0;
    if (live) {
        RayD ray = loadSegment(rays, st, list, j, i);
        f3 throughput = splat3(1.0f);
        int medium = p.medium;
        uint32_t bounce = p.bounce, crossed = 0u;
        bool startsOnSurface = p.startsOnSurface != 0u;
        if (list) {
            const float4 t = st.t[i];
            const uint2 b = st.b[i];
            throughput = xyz(t); medium = __float_as_int(t.w);
            bounce = b.x; crossed = b.y;
            startsOnSurface = true;
        } else if (media) {
            medium = media[i];
            if (medium == TGHIP_MEDIUM_OF_CAMERA) medium = p.cameraMedium;
            if (medium < 0 || (uint32_t)medium >= s.num_media) medium = -1;    // (out of range: an unspecified answer, no read outside the table)
        }
        const float4 hit = st.hits[i];
        const int hitInst = st.inst ? st.inst[i] : -1;
        const int ri = __float_as_int(hit.w);
        int hitObject = -1;
        if (ri >= 0)          // geometry reached through an instance belongs to the `instances` primitive (never an end cap)
            hitObject = (int)TGHIP_REC_OBJECT(__float_as_uint(at32(s.recs, (uint32_t)(hitInst >= 0 ? hitInst : ri)*3u).w));
        const bool atEndCap = ri >= 0 && hitObject == p.endCap;
        // The quad the ray is aimed at is only FOUND when Embree's slab test lets the ray into its flat box (k_trace_shadow, pt_wavefront.h): culled,
        // the function returns as at the end cap, but ray.farT() was not shortened to the hit
        bool found = ri >= 0;
        if (atEndCap && s.objects[p.endCap].type == TGHIP_OBJ_QUAD) {
            const TgHipObject &lo = s.objects[p.endCap];
            const f3 b = ld3(lo.base), e0 = ld3(lo.edge0), e1 = ld3(lo.edge1);
            const f3 p1 = b + e0, p2 = b + e1, p3 = (b + e0) + e1;
            const f3 bl = mk3(fminf(fminf(b.x, p1.x), fminf(p2.x, p3.x)), fminf(fminf(b.y, p1.y), fminf(p2.y, p3.y)), fminf(fminf(b.z, p1.z), fminf(p2.z, p3.z)));
            const f3 bh = mk3(fmaxf(fmaxf(b.x, p1.x), fmaxf(p2.x, p3.x)), fmaxf(fmaxf(b.y, p1.y), fmaxf(p2.y, p3.y)), fmaxf(fmaxf(b.z, p1.z), fmaxf(p2.z, p3.z)));
            found = embreeBoxVisible(ray.o, ray.d, ray.tmin, ray.tmax, bl, bh);
        }
        bool dark = false;
        Info info;
        if (ri >= 0 && !atEndCap) {                  // didHit (TraceBase.cpp:79-102)
            intersectionInfo<TRANSMITTANCE_MASK>(s, ray, hit, info, hitInst);
            const uint32_t lobes = s.bsdfs[info.bsdf].lobes;
            if (!(lobes & TGHIP_LOBE_FORWARD)) {
                dark = true;
            } else {
                Frame frame = frameFromNormal(info.Ns);
                const bool hitBackside = dot(frame.normal, ray.d) > 0.0f;
                if (s.settings.enable_two_sided_shading && hitBackside && !(lobes & LOBE_TRANSMISSIVE)) {
                    frame.normal = -frame.normal;
                    frame.tangent = -frame.tangent;
                }
                Event fe;
                fe.wi = toLocal(frame, -ray.d); fe.wo = -fe.wi;
                fe.requested = TGHIP_LOBE_FORWARD; fe.u = info.u; fe.v = info.v; fe.rng = nullptr;
                const f3 transparency = bsdfEval<TRANSMITTANCE_MASK>(s, info.bsdf, fe);
                if (isZero(transparency)) {
                    dark = true;
                } else {
                    throughput = throughput*transparency;
                    bounce++; crossed++;
                    if ((int)bounce >= s.settings.max_bounces) dark = true;
                }
            }
        }
        if (!dark && medium >= 0)                    // :104-112; ray.farT() is the hit distance when anything was found
            throughput = throughput*mediumTransmittance(s, medium, ray.o, ray.d, found ? hit.x : ray.tmax, startsOnSurface, p.endsOnSurface != 0u);
        if (dark) {
            out[i] = mk4(splat3(0.0f), __uint_as_float(crossed));
        } else if (ri < 0 || atEndCap) {             // :114-115
            out[i] = mk4((int)bounce >= s.settings.min_bounces ? throughput : splat3(0.0f), __uint_as_float(crossed));
        } else {                                     // :116-122
            if (s.num_media)
                medium = selectMedium(s.objects[info.object], medium, !info.backSide);
            st.o[i] = mk4(ray.o + ray.d*hit.x, 5e-4f);
            st.d[i] = mk4(ray.d, ray.tmax - hit.x);
            st.t[i] = mk4(throughput, __int_as_float(medium));
            st.b[i] = make_uint2(bounce, crossed);
            goesOn = true;
        }
    }
    // the rays of this wave that go on, appended to the next round's list in lane order
    appendLive(goesOn, i, next, nextCount);
}

hipError_t transmittanceQueryLaunchWalk(hipStream_t stream, const DeviceScene &scene, RayQueryWalk walk, const float4 *rays, const TransmittanceState &st,
                                        const uint32_t *list, uint32_t live, uint32_t *counter, uint32_t blocks, uint32_t refillAt, size_t ldsBytes)
{
    const dim3 grid(blocks), block(RAY_QUERY_THREADS);
    switch (walk) {
    case RAY_QUERY_FLAT: hipLaunchKernelGGL((k_transmittance_walk<RAY_QUERY_FLAT>), grid, block, ldsBytes, stream, scene, rays, st, list, live, counter); break;
    case RAY_QUERY_BVH2: hipLaunchKernelGGL((k_transmittance_walk<RAY_QUERY_BVH2>), grid, block, ldsBytes, stream, scene, rays, st, list, live, counter); break;
    case RAY_QUERY_INST: hipLaunchKernelGGL((k_transmittance_walk<RAY_QUERY_INST>), grid, block, ldsBytes, stream, scene, rays, st, list, live, counter); break;
    case RAY_QUERY_WIDE: hipLaunchKernelGGL(k_transmittance_walk_wide, grid, block, ldsBytes, stream, scene, rays, st, list, live, counter, refillAt); break;
    }
    return hipGetLastError();
}

hipError_t transmittanceQueryLaunchSegment(hipStream_t stream, const DeviceScene &scene, const TransmittanceParams &p, const float4 *rays, const int *media,
                                           const TransmittanceState &st, const uint32_t *list, uint32_t live, float4 *out, uint32_t *next, uint32_t *nextCount)
{
    const dim3 grid((live + TRANSMITTANCE_QUERY_THREADS - 1u)/TRANSMITTANCE_QUERY_THREADS), block(TRANSMITTANCE_QUERY_THREADS);
    hipLaunchKernelGGL(k_transmittance_segment, grid, block, 0, stream, scene, p, rays, media, st, list, live, out, next, nextCount);
    return hipGetLastError();
}
