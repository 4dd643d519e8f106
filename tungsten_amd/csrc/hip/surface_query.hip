// What is at the closest hit of caller rays (tghip_query_surface), in two launches on the context's stream.
//   the walk            tghip_query_rays' closest-hit kernels themselves (ray_query.hip, through rayQueryLaunch), the hits left in scratch; on
//                       instanced scenes k_surface_walk<RAY_QUERY_INST>, that unit's per-ray loop storing the record of the instance a hit was
//                       reached through as well, which k_query_rays computes and drops (the claim and the ray load: query_walk.h).
//   k_surface_describe  dense, one lane per ray in ray order: IntersectionInfo of the hit (pt_scene.h: intersectionInfo, all seven record kinds and
//                       through instances), the material's albedo and the primitive's emission as the path tracer's output buffers take them
//                       (PathTracer.cpp:83-88), or for a miss the infinite emitter along the ray (TraceableScene.hpp:194-209), and the 96 bytes, staged
//                       in LDS and written out contiguously.
// Two launches because the description is gathers, one or two texture lookups and lightEvalDirect: inside the walk's loop it would run at the
// occupancy of whichever lanes just finished and add its registers to the walk's; behind it every lane of every wave has a ray.
// One instantiation, under the all-features family's mask: every record kind, every texture type, cubeSurface with the reference's tie rule -- an
// answer never depends on which shading family the scene's passes use.  (FEAT_QMC cleared as in debug_units.hip: nothing here draws a number.)
#include "surface_query.h"
#include "query_walk.h"

#define SURFACE_MASK (BSDF_MASK_ALL & ~FEAT_QMC)

// Instanced scenes: k_query_rays<RAY_QUERY_INST, false>'s loop (ray_query.hip) -- tghip_trace_rays' per-ray function, claims at ray granularity -- with
// the walk's hitInst, which that kernel drops, kept.  (WALK stays a parameter for the kernel's name; the other walks are ray_query.hip's kernels.)
template<int WALK>
__global__ __launch_bounds__(RAY_QUERY_THREADS) void k_surface_walk(DeviceScene s, const float4 *rays, float4 *hits, int *inst, uint32_t n, uint32_t *counter)
{
    static_assert(WALK == RAY_QUERY_INST, "the walks without instances are rayQueryLaunch's");
    extern __shared__ int ldsStack[];
    int *stack = ldsStack + threadIdx.x;
    const int stride = RAY_QUERY_THREADS;
    bool exhausted = false;
    while (!exhausted) {
        const uint32_t i = claimRays(counter, true, n, exhausted);
        if (i < n) {
            const RayD ray = loadRay(rays, i);
            uint32_t nodes = 0, prims = 0;
            int hitInst = -1;
            hits[i] = traverseClosestInst<false, KINDS_ALL>(s, ray, stack, stride, nodes, prims, hitInst);
            inst[i] = hitInst;
        }
    }
}

// The answer of one ray as the six 16-byte vectors of a TgHipSurface
struct SurfaceWords { float4 v[6]; };

template<uint32_t M>
PT_DEV SurfaceWords describeSurface(const DeviceScene &s, const RayD &ray, float4 hit, int hitInst)
{
    SurfaceWords w;
    const float minusOne = __int_as_float(-1);
    if (__float_as_int(hit.w) >= 0) {
        Info info;
        intersectionInfo<M>(s, ray, hit, info, hitInst);
        // the ray's hit point (TraceableScene.hpp:184): not Instance::intersectionInfo's second transform of it, which info.p carries for the path tracer
        const f3 p = ray.o + ray.d*hit.x;
        int ab = info.bsdf;                              // TransparencyBsdf: its base's albedo (PathTracer.cpp:83-88)
        if (s.bsdfs[ab].type == TGHIP_BSDF_TRANSPARENCY) ab = s.bsdfs[ab].sub0;
        const f3 albedo = textureEval<M>(s, s.bsdfs[ab].albedo, info.u, info.v);
        const bool emissive = s.objects[info.object].emission >= 0;     // Primitive::isEmissive
        const f3 emission = emissive ? lightEvalDirect<M>(s, info.object, info.u, info.v, info.backSide) : splat3(0.0f);
        const uint32_t flags = TGHIP_SURFACE_HIT | (info.backSide ? TGHIP_SURFACE_BACK_SIDE : 0u) | (emissive ? TGHIP_SURFACE_EMISSIVE : 0u);
        w.v[0] = mk4(p, hit.x);
        w.v[1] = mk4(info.Ng, hit.w);
        w.v[2] = mk4(info.Ns, __int_as_float(hitInst));
        w.v[3] = make_float4(info.u, info.v, __int_as_float(info.object), __int_as_float(info.bsdf));
        w.v[4] = mk4(albedo, __uint_as_float(flags));
        w.v[5] = mk4(emission, 0.0f);
        return w;
    }
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    w.v[0] = zero;
    w.v[1] = make_float4(0.0f, 0.0f, 0.0f, minusOne);
    w.v[2] = make_float4(0.0f, 0.0f, 0.0f, minusOne);
    w.v[3] = make_float4(0.0f, 0.0f, minusOne, minusOne);
    w.v[4] = zero;
    w.v[5] = zero;
    // TraceableScene::intersectInfinites (TraceableScene.hpp:194-209): every infinite emitter is asked, the last one found stays; a cap is found
    // inside its angle only (auxPostLoop's loop, pt_wavefront.h)
    int objIdx = -1;
    for (uint32_t li = 0; li < s.num_infinite_lights; ++li) {
        const TgHipObject &c = s.objects[s.infinite_lights[li]];
        if (c.type != TGHIP_OBJ_INFINITE_SPHERE_CAP || dot(ray.d, ld3(c.normal)) >= c.scale[0])
            objIdx = s.infinite_lights[li];
    }
    if (objIdx >= 0) {
        const TgHipObject &o = s.objects[objIdx];
        float u = 0.0f, v = 0.0f, sinTheta;
        if (o.type == TGHIP_OBJ_INFINITE_SPHERE) infDirectionToUV(o, ray.d, u, v, sinTheta);
        const f3 e = textureEval<M>(s, o.emission, u, v);
        w.v[3] = make_float4(u, v, __int_as_float(objIdx), minusOne);
        w.v[4].w = __uint_as_float(TGHIP_SURFACE_INFINITE);
        w.v[5] = mk4(e, 0.0f);
    }
    return w;
}

// A lane's answer is 96 bytes, so six 16-byte stores of a wave would each scatter 64 pieces 96 bytes apart over 48 of the 128-byte lines.  The
// workgroup stages its answers in LDS instead (24 KiB) and writes them out in order: every store instruction of a wave covers 1024 contiguous bytes,
// eight whole lines.  Measured against the plain stores on materialtest at 1280 x 720, alternated three times: the launch 0.029 against 0.039 ms on
// camera rays, 0.053 against 0.060 ms on random rays (profiles/surface_query/bench.txt); the plain form is not in the tree.
__global__ __launch_bounds__(SURFACE_QUERY_THREADS) void k_surface_describe(DeviceScene s, const float4 *rays, const float4 *hits, const int *inst, float4 *out, uint32_t n)
{
    __shared__ float4 stage[SURFACE_QUERY_THREADS*6];
    const uint32_t i = blockIdx.x*SURFACE_QUERY_THREADS + threadIdx.x;
    if (i < n) {
        const SurfaceWords w = describeSurface<SURFACE_MASK>(s, loadRay(rays, i), hits[i], inst ? inst[i] : -1);
        for (int k = 0; k < 6; ++k) stage[threadIdx.x*6u + k] = w.v[k];
    }
    __syncthreads();
    // the workgroup's answers are contiguous in `out`: vector j of the workgroup goes to out[first*6 + j]
    const size_t first = (size_t)blockIdx.x*SURFACE_QUERY_THREADS;
    const uint32_t live = min((uint32_t)SURFACE_QUERY_THREADS, n - blockIdx.x*SURFACE_QUERY_THREADS)*6u;
    for (uint32_t j = threadIdx.x; j < live; j += SURFACE_QUERY_THREADS)
        out[first*6u + j] = stage[j];
}

hipError_t surfaceQueryLaunchWalk(hipStream_t stream, const DeviceScene &scene, RayQueryWalk walk, const float4 *rays, float4 *hits, int *inst, uint32_t n,
                                  uint32_t *counter, uint32_t blocks, uint32_t refillAt, size_t ldsBytes)
{
    // no instance in the scene: the hit is all the walk leaves, and tghip_query_rays' closest-hit kernels leave it
    if (walk != RAY_QUERY_INST)
        return rayQueryLaunch(stream, scene, walk, false, rays, hits, n, counter, blocks, refillAt, ldsBytes);
    hipLaunchKernelGGL((k_surface_walk<RAY_QUERY_INST>), dim3(blocks), dim3(RAY_QUERY_THREADS), ldsBytes, stream, scene, rays, hits, inst, n, counter);
    return hipGetLastError();
}

hipError_t surfaceQueryLaunchDescribe(hipStream_t stream, const DeviceScene &scene, const float4 *rays, const float4 *hits, const int *inst, float4 *out,
                                      uint32_t n)
{
    const dim3 grid((n + SURFACE_QUERY_THREADS - 1u)/SURFACE_QUERY_THREADS), block(SURFACE_QUERY_THREADS);
    hipLaunchKernelGGL(k_surface_describe, grid, block, 0, stream, scene, rays, hits, inst, out, n);
    return hipGetLastError();
}
