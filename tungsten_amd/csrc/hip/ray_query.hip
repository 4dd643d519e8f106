// Batched ray queries on caller rays (tghip_query_rays): closest hit -- tghip_trace_rays' answer, bit for bit -- and occlusion, the byte "the closest-hit
// query of this ray has a hit" (TraceBase.cpp:79, 114-115: the closest-hit formulation of the path tracer's shadow rays; geometry only, no light to
// leave out).  Persistent workgroups claim rays from ONE global counter: the idle lanes of a wave are counted with a ballot, one lane adds the count and
// broadcasts the base, each idle lane takes base + its rank.  Nothing waits for another workgroup and nothing spins: a wave leaves once it holds no
// ray and the counter has passed n.  The shim resets the counter in-stream before every launch (shim_queries.hip: tghip_query_rays).
// The closest-hit kernels answer tghip_query_surface's walk on scenes without instances as well (surface_query.hip).  The claim, the ray load and the
// 8-wide loop are query_walk.h's, shared with transmittance_query.hip; the per-ray loop below exists there once more over its list of rays
// (k_transmittance_walk<WALK>), and its instanced form in surface_query.hip with the instance record kept (k_surface_walk<RAY_QUERY_INST>).
#include "query_walk.h"

namespace {

template<bool OCCLUDED>
PT_DEV void storeAnswer(void *out, uint32_t i, float4 hit, bool occluded)
{
    if (OCCLUDED) static_cast<uint8_t *>(out)[i] = occluded ? 1u : 0u;
    else static_cast<float4 *>(out)[i] = hit;
}

}  // namespace

// Scenes on the 8-wide BVH: the decoupled loop (query_walk_wide.h) on the caller's rays in batch order, the answer a hit or the occlusion byte
template<bool OCCLUDED>
__global__ __launch_bounds__(RAY_QUERY_THREADS) void k_query_rays_wide(DeviceScene s, const float4 *rays, void *out, uint32_t n, uint32_t *counter, uint32_t refillAt)
{
#define QUERY_WALK_OCCLUDED OCCLUDED
#define QUERY_WALK_LOAD(j, index) (index = j, loadRay(rays, j))
#define QUERY_WALK_STORE(index, hit, found) storeAnswer<OCCLUDED>(out, index, hit, found)
#include "query_walk_wide.h"
}

// Flat-list, BVH2 and instanced scenes: tghip_trace_rays' per-ray functions inside the same claim loop, claims at ray granularity -- every lane is
// idle after its ray, so a wave claims 64 at a time.  (The 8-wide walk was measured this way too, traverseClosestWide per ray: 7 % slower than the
// decoupled loop on incoherent rays, and occlusion no faster than closest hits -- profiles/ray_query_ab.txt.)
template<int WALK, bool OCCLUDED>
__global__ __launch_bounds__(RAY_QUERY_THREADS) void k_query_rays(DeviceScene s, const float4 *rays, void *out, uint32_t n, uint32_t *counter)
{
    extern __shared__ int ldsStack[];
    int *stack = ldsStack + threadIdx.x;
    const int stride = RAY_QUERY_THREADS;
    bool exhausted = false;
    while (!exhausted) {
        const uint32_t i = claimRays(counter, true, n, exhausted);
        if (i < n) {
            const RayD ray = loadRay(rays, i);
            uint32_t nodes = 0, prims = 0;
            int hitInst;
            float4 hit = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
            bool occluded = false;
            if (OCCLUDED) {
                occluded = WALK == RAY_QUERY_INST ? traverseOccludedInst<false, KINDS_ALL>(s, ray, -1, stack, stride, nodes, prims)
                                                  : traverseOccluded<false, WALK == RAY_QUERY_FLAT>(s, ray, -1, stack, stride, nodes, prims);
            } else {
                hit = WALK == RAY_QUERY_INST ? traverseClosestInst<false, KINDS_ALL>(s, ray, stack, stride, nodes, prims, hitInst)
                                             : traverseClosest<false, WALK == RAY_QUERY_FLAT>(s, ray, stack, stride, nodes, prims);
            }
            storeAnswer<OCCLUDED>(out, i, hit, occluded);
        }
    }
}

hipError_t rayQueryLaunch(hipStream_t stream, const DeviceScene &scene, RayQueryWalk walk, bool occluded, const float4 *rays, void *out, uint32_t n,
                          uint32_t *counter, uint32_t blocks, uint32_t refillAt, size_t ldsBytes)
{
    const dim3 grid(blocks), block(RAY_QUERY_THREADS);
#define QUERY_LAUNCH(W) do { \
        if (occluded) hipLaunchKernelGGL((k_query_rays<W, true>), grid, block, ldsBytes, stream, scene, rays, out, n, counter); \
        else          hipLaunchKernelGGL((k_query_rays<W, false>), grid, block, ldsBytes, stream, scene, rays, out, n, counter); \
    } while (0)
    switch (walk) {
    case RAY_QUERY_FLAT: QUERY_LAUNCH(RAY_QUERY_FLAT); break;
    case RAY_QUERY_BVH2: QUERY_LAUNCH(RAY_QUERY_BVH2); break;
    case RAY_QUERY_INST: QUERY_LAUNCH(RAY_QUERY_INST); break;
    case RAY_QUERY_WIDE:
        if (occluded) hipLaunchKernelGGL((k_query_rays_wide<true>), grid, block, ldsBytes, stream, scene, rays, out, n, counter, refillAt);
        else          hipLaunchKernelGGL((k_query_rays_wide<false>), grid, block, ldsBytes, stream, scene, rays, out, n, counter, refillAt);
        break;
    }
#undef QUERY_LAUNCH
    return hipGetLastError();
}
