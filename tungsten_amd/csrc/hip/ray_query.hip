// Batched ray queries on caller rays (tghip_query_rays): closest hit -- tghip_trace_rays' answer, bit for bit -- and occlusion, the byte "the closest-hit
// query of this ray has a hit" (TraceBase.cpp:79, 114-115: the closest-hit formulation of the path tracer's shadow rays; geometry only, no light to
// leave out).  Persistent workgroups claim rays from ONE global counter: the idle lanes of a wave are counted with a ballot, one lane adds the count and
// broadcasts the base, each idle lane takes base + its rank.  Nothing waits for another workgroup and nothing spins: a wave leaves once it holds no
// ray and the counter has passed n.  The shim resets the counter in-stream before every launch (tungsten_hip.hip: tghip_query_rays).
// The two loops below exist twice more with another load and another store -- surface_query.hip (k_surface_walk*) and transmittance_query.hip
// (k_transmittance_walk*): instantiated there again because as a shared template these kernels did not come out instruction for instruction
// (profiles/surface_query/kernel_resources_diff.txt).  A change to a turn of the walk is made in all three.
#include "ray_query.h"
#include "pt_wavefront.h"

namespace {

// The wave's claim: every lane with `idle` set gets the index of a ray of the batch, or one >= n when the batch has been handed out.
// `exhausted` (wave-uniform) is set by the claim that reaches n.  Called by all 64 lanes.
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

PT_DEV RayD loadRay(const float4 *rays, uint32_t i)
{
    const float4 ro = rays[(size_t)i*2u + 0u], rd = rays[(size_t)i*2u + 1u];
    RayD ray;
    ray.o = xyz(ro); ray.d = xyz(rd); ray.tmin = ro.w; ray.tmax = rd.w;
    return ray;
}

template<bool OCCLUDED>
PT_DEV void storeAnswer(void *out, uint32_t i, float4 hit, bool occluded)
{
    if (OCCLUDED) static_cast<uint8_t *>(out)[i] = occluded ? 1u : 0u;
    else static_cast<float4 *>(out)[i] = hit;
}

}  // namespace

// Scenes on the 8-wide BVH: the decoupled walk of the wavefront kernels (pt_wavefront.h: traceClosestWideBody) on caller rays.  Per turn a lane tests
// at most one pending record and visits at most one node; a lane whose walk is over stores its answer and is idle; the wave claims once `refillAt`
// of its lanes are.  A lane's walk is a pure function of its ray -- records are tested in the order traverseClosestWide tests them, and a node visited
// before an earlier node's records have shortened the ray only reports children that begin behind the hit --, so the closest hit is
// traverseClosestWide's whatever the turn order.  OCCLUDED: the same loop, ended at the first accepted record, the ray's tmax never shortened.
// (No hoisted quad here: the record order is the sequential walk's.)
template<bool OCCLUDED>
__global__ __launch_bounds__(RAY_QUERY_THREADS) void k_query_rays_wide(DeviceScene s, const float4 *rays, void *out, uint32_t n, uint32_t *counter, uint32_t refillAt)
{
    extern __shared__ int ldsStack[];
    uint2 *stack = reinterpret_cast<uint2 *>(ldsStack) + threadIdx.x;
    const int stride = RAY_QUERY_THREADS;
    bool busy = false, exhausted = false;
    uint32_t index = 0;
    RayD ray; ray.o = splat3(0.0f); ray.d = splat3(1.0f); ray.tmin = 0.0f; ray.tmax = 0.0f;
    WideRay wr; wr.idir = splat3(1.0f); wr.octInv = 0u;
    WideState w;
    wideStart(w);
    float tmax = 0.0f;
    float4 hit = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    for (;;) {
        unsigned long long busyMask = __ballot(busy);
        if (!exhausted && 64u - (uint32_t)__popcll(busyMask) >= refillAt) {
            const uint32_t i = claimRays(counter, !busy, n, exhausted);
            if (!busy && i < n) {
                index = i;
                ray = loadRay(rays, i);
                wr = wideRaySetup(ray);
                wideStart(w);
                tmax = ray.tmax;
                hit = make_float4(tmax, 0.0f, 0.0f, __int_as_float(-1));
                busy = true;
            }
            busyMask = __ballot(busy);
        }
        if (busyMask == 0ull)
            break;                               // (an idle wave has claimed above, refillAt <= 64: the counter has passed n)
        uint32_t recIdx = 0, nodeIdx = 0;
        bool hasRec = false, hasNode = false;
        if (busy) {
            if (w.triMask == 0u && w.tri2Mask != 0u) { w.triBase = w.tri2Base; w.triMask = w.tri2Mask; w.triValid = w.tri2Valid; w.tri2Mask = 0u; }
            if (w.triMask) {
                const uint32_t b = (uint32_t)__ffs((int)w.triMask) - 1u;
                recIdx = w.triBase + (uint32_t)__popc(w.triValid & ((1u << b) - 1u));
                w.triMask &= w.triMask - 1u;
                hasRec = true;
            }
            if (w.tri2Mask == 0u)                // (room for the records of the node visited now)
                hasNode = wideNextNode(w, wr.octInv, stack, stride, nodeIdx);
        }
        float4 r0, r1, r2;
        WideNodeRegs nd;
        PT_WALK_FETCH(s, r0, r1, r2, nd, hasRec, recIdx, hasNode, nodeIdx);
        bool found = false;
        if (hasRec) {
            uint32_t meta;
            if (OCCLUDED) {
                float t = ray.tmax;
                found = testRecordLoaded<false, KINDS_ALL>(s, recIdx, r0, r1, r2, ray, t, hit, meta);
            } else {
                (void)testRecordLoaded<false, KINDS_ALL>(s, recIdx, r0, r1, r2, ray, tmax, hit, meta);
            }
        }
        if (hasNode) {
            const uint32_t ob = w.triBase, om = w.triMask, ov = w.triValid;
            wideVisit(w, nd, ray.o, wr, ray.tmin, OCCLUDED ? ray.tmax : tmax);
            if (om) { w.tri2Base = w.triBase; w.tri2Mask = w.triMask; w.tri2Valid = w.triValid; w.triBase = ob; w.triMask = om; w.triValid = ov; }
        }
        if (busy && (found || wideWalkOver(w))) {    // (in the turn that looked at the walk's last record / node)
            storeAnswer<OCCLUDED>(out, index, hit, found);
            busy = false;
        }
    }
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
