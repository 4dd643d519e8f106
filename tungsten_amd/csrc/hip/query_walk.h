// What the walks of the ray queries share (ray_query.hip, surface_query.hip, transmittance_query.hip): the wave's claim on the one global counter and
// the load of a caller ray; and what the dense stages around them share (transmittance_query.hip, direct_query.hip, vertex_query.hip,
// radiance_query.hip): the ballot-append to the next round's list, a ray's start medium, the far distance of a bounded segment's walk.  The decoupled loop of the 8-wide BVH is shared too, as text: query_walk_wide.h is the body of k_query_rays_wide<OCCLUDED>
// and of k_transmittance_walk_wide, with the load and the store as macros -- the form of the turn's memory part (pt_wavefront.h: PT_WALK_FETCH).
// As a force-inlined function template over a load and a store the same loop did not leave ray_query.hip's kernels instruction for instruction as
// they were (profiles/query_walk/kernel_resources_diff.txt).  A change to a turn of the wide walk is made in that one file.
#ifndef TGAMD_QUERY_WALK_H_
#define TGAMD_QUERY_WALK_H_

#include "ray_query.h"
#include "pt_wavefront.h"

// The wave's claim: every lane with `idle` set gets the index of a ray of the batch (a place of the round's list), or one >= n when the batch has
// been handed out.  `exhausted` (wave-uniform) is set by the claim that reaches n.  Called by all 64 lanes.
PT_DEV uint32_t claimRays(uint32_t *counter, bool idle, uint32_t n, bool &exhausted)
{
    const unsigned long long want = __ballot(idle);
    const uint32_t lane = laneId(), count = (uint32_t)__popcll(want);
    uint32_t base = 0;
    if (lane == 0)
        base = atomicAdd(counter, count);
    base = __shfl(base, 0);
    // (the counter cannot wrap: n < 2^31, and every wave adds at most 64 once it has seen n passed)
    exhausted = base + count >= n;
    return base + (uint32_t)__popcll(want & ((1ull << lane) - 1ull));
}

// The ballot-append: every lane that is `alive` gets its place, counted in *count in lane order with one atomicAdd per wave (ballot, popcount,
// rank), and stores there with put(place).  Called by all 64 lanes.  (A store handed in, not a place handed out: as two functions, place then
// store, k_direct_round did not keep its code.)
template<typename Put>
PT_DEV void appendAt(bool alive, uint32_t *count, Put put)
{
    const unsigned long long on = __ballot(alive);
    if (on != 0ull) {
        const uint32_t lane = laneId();
        uint32_t base = 0;
        if (lane == 0)
            base = atomicAdd(count, (uint32_t)__popcll(on));
        base = __shfl(base, 0);
        if (alive) put(base + (uint32_t)__popcll(on & ((1ull << lane) - 1ull)));
    }
}

// The segments (or rays) of this wave that are alive, appended to a list
PT_DEV void appendLive(bool alive, uint32_t g, uint32_t *list, uint32_t *count)
{
    appendAt(alive, count, [&](uint32_t at) { list[at] = g; });
}

PT_DEV RayD loadRay(const float4 *rays, uint32_t i)
{
    const float4 ro = rays[(size_t)i*2u + 0u], rd = rays[(size_t)i*2u + 1u];
    RayD ray;
    ray.o = xyz(ro); ray.d = xyz(rd); ray.tmin = ro.w; ray.tmax = rd.w;
    return ray;
}

// The medium ray i of a call starts in: the call's (Params::medium), or its own -- TGHIP_MEDIUM_OF_CAMERA resolved; out of range: an unspecified
// answer, no read outside the table.  The device's side of the shim's queryStartMedium.  (k_transmittance_segment keeps these lines written out:
// through this function its code moved.)
template<typename Params>
PT_DEV int rayStartMedium(const Params &p, const int *media, uint32_t numMedia, uint32_t i)
{
    int medium = p.medium;
    if (media) {
        medium = media[i];
        if (medium == TGHIP_MEDIUM_OF_CAMERA) medium = p.cameraMedium;
        if (medium < 0 || (uint32_t)medium >= numMedia) medium = -1;
    }
    return medium;
}

// The far distance the closest-hit walk of a segment [tmin, tmax) starts with (tghip_query_radiance's first segment, a path's of tghip_query_vertex).
// The walks are the reference's: a quad accepts t <= far, and a leaf is skipped by its BOX's entry distance, which lies up to a few ulps to either
// side of the t the primitive's own test reports (TgHipTopNode, include/tungsten_hip.h) -- so a walk that starts with far = tmax answers for hits
// within a few ulps of tmax by its own arithmetic, not by the segment.  It starts 2^-10 further instead, far beyond that slack, and the stage behind
// the walk turns every hit with t >= tmax into the miss it is.  An infinite tmax (the camera's) and the -1 of a padding pixel stay what they are.
PT_DEV float queryWalkFar(float tmax) { return (tmax > 0.0f && tmax < PT_INF) ? tmax*1.0009765625f : tmax; }

#endif
