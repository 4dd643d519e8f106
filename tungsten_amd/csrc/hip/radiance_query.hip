// tghip_query_radiance (include/tungsten_hip.h): the kernels that make a pass of the wavefront loop estimate radiance along the caller's rays.
// gfx950 (MI355X) only.  The pass itself is the one tghip_wait drives -- k_start, the walks, the shading launches, k_finish, k_resolve, untouched --
// over a virtual image whose row-major pixel index is the ray index (csrc/host/RadianceQuery.cpp); what is new is here.
#include "radiance_query.h"
#include "query_walk.h"      // queryWalkFar: the far distance the walk of the first segment starts with; k_query_clip below ends the segment exactly

// The ray source.  nextPath has written every fresh path with the pinhole ray of its virtual pixel and left the path's stream behind the two numbers
// a pinhole camera spends on its pixel filter (Sobol': at dimension 2), throughput 1, bounce 0, wasSpecular, the camera's medium: the state of
// PathTracer::traceSample (PathTracer.cpp:14-41) behind Camera::sampleDirection.  Here the ray is replaced, for the slots of the workgroup's Q_EXTP
// (the freshly generated paths), in a launch in front of every closest-hit launch -- where and how k_camera_rays (tungsten_hip.hip) replaces the
// direction for the equirectangular and cubemap cameras, which does not run in a query's pass.  Memory-bound: per fresh path one word of A_MISC and
// the ray's 32 bytes in, two 16-byte slot words out, the slots of a wave ascending.  Idempotent.
__global__ __launch_bounds__(256) void k_query_paths(PathState st, const float4 *__restrict__ rays, uint32_t n)
{
    const uint32_t W = st.slots_per_block >> 5;
    const uint32_t first = blockIdx.x*st.slots_per_block;
    for (uint32_t local = threadIdx.x; local < st.slots_per_block; local += blockDim.x) {
        const uint32_t word = st.bm[(uint32_t)Q_EXTP*st.bmStride + blockIdx.x*W + (local >> 5)];
        if (!((word >> (local & 31u)) & 1u))
            continue;
        const uint32_t slot = first + local;
        const uint32_t ray = slotUW(st, A_MISC, slot, 2u);       // the path's pixel index
        if (ray < n) {
            const float4 o = rays[(size_t)ray*2u];
            float4 d = rays[(size_t)ray*2u + 1u];
            d.w = queryWalkFar(d.w);             // (the walk looks a little further than the segment reaches: k_query_clip ends the segment exactly)
            slotF4(st, A_RAY_O, slot) = o;
            slotF4(st, A_RAY_D, slot) = d;
        } else {                                 // as nextPath leaves a failed camera sample: a ray that can hit nothing, no throughput
            slotW(st, A_RAY_D, slot, 3u) = -1.0f;
            const float flags = slotW(st, A_THR, slot, 3u);
            slotF4(st, A_THR, slot) = make_float4(0.0f, 0.0f, 0.0f, flags);
        }
    }
}

// The end of the first segment, behind every closest-hit launch: a path that is still on the caller's ray -- bounce 0, origin and direction the ray's
// own bits -- and whose walk found a hit at t >= rays[i].tmax has hit nothing inside [tmin, tmax): its hit record becomes the walk's miss record
// (tmax, 0, 0, -1) and its slot moves from the shading queue of the hit's class to Q_MISS, where the escaped paths are shaded.  A_RAY_D gets the
// caller's tmax back for every such path, hit or not, so that what the shading kernels read as the ray's far distance (a medium's last distance) is
// the segment's.  One thread per slot over the workgroup's four shading-queue bitmaps; moves are rare (atomics on the workgroup's own words).
// Idempotent; a finite tmax only (the camera's own rays have none and cost one flag word per hit here).
__global__ __launch_bounds__(256) void k_query_clip(PathState st, const float4 *__restrict__ rays, uint32_t n)
{
    const uint32_t W = st.slots_per_block >> 5;
    const uint32_t first = blockIdx.x*st.slots_per_block;
    const int queues[5] = {Q_SHADE0, Q_SHADE1, Q_SHADE2, Q_SHADE3, Q_MISS};
    for (uint32_t local = threadIdx.x; local < st.slots_per_block; local += blockDim.x) {
        const uint32_t wordIndex = blockIdx.x*W + (local >> 5), bit = 1u << (local & 31u);
        int q = -1;
        for (int k = 0; k < 5; ++k)
            if (st.bm[(uint32_t)queues[k]*st.bmStride + wordIndex] & bit) q = queues[k];
        if (q < 0)
            continue;
        const uint32_t slot = first + local;
        if (FLAG_BOUNCE(slotUW(st, A_THR, slot, 3u)) != 0u)
            continue;
        const uint32_t ray = slotUW(st, A_MISC, slot, 2u);
        if (ray >= n)
            continue;
        const float4 o = rays[(size_t)ray*2u], d = rays[(size_t)ray*2u + 1u];
        if (!(d.w > 0.0f && d.w < PT_INF))
            continue;
        const float4 so = slotF4(st, A_RAY_O, slot), sd = slotF4(st, A_RAY_D, slot);
        const bool own = __float_as_uint(so.x) == __float_as_uint(o.x) && __float_as_uint(so.y) == __float_as_uint(o.y) && __float_as_uint(so.z) == __float_as_uint(o.z) &&
                         __float_as_uint(sd.x) == __float_as_uint(d.x) && __float_as_uint(sd.y) == __float_as_uint(d.y) && __float_as_uint(sd.z) == __float_as_uint(d.z);
        if (!own)
            continue;
        slotW(st, A_RAY_D, slot, 3u) = d.w;
        const float4 hit = slotF4(st, A_HIT, slot);
        if (q == Q_MISS) {
            slotW(st, A_HIT, slot, 0u) = d.w;
        } else if (!(hit.x < d.w)) {
            slotF4(st, A_HIT, slot) = make_float4(d.w, 0.0f, 0.0f, __int_as_float(-1));
            atomicAnd(&st.bm[(uint32_t)q*st.bmStride + wordIndex], ~bit);
            atomicOr(&st.bm[(uint32_t)Q_MISS*st.bmStride + wordIndex], bit);
        }
    }
}

// The first n pixels of the pass's framebuffer are the n rays' answers: copied word by word (the caller's arrays are 4-byte aligned), grid-stride
__global__ __launch_bounds__(256) void k_query_results(const float *__restrict__ sum, const uint32_t *__restrict__ count, float *__restrict__ outSum,
                                                       uint32_t *__restrict__ outCount, uint32_t n)
{
    const size_t stride = (size_t)gridDim.x*blockDim.x, start = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
    for (size_t i = start; i < (size_t)n*3u; i += stride)
        outSum[i] = sum[i];
    if (outCount)
        for (size_t i = start; i < (size_t)n; i += stride)
            outCount[i] = count[i];
}

void radianceQueryLaunchPaths(hipStream_t stream, int grid, const PathState &st, const float4 *rays, uint32_t n)
{
    hipLaunchKernelGGL(k_query_paths, dim3(grid), dim3(256), 0, stream, st, rays, n);
}

void radianceQueryLaunchClip(hipStream_t stream, int grid, const PathState &st, const float4 *rays, uint32_t n)
{
    hipLaunchKernelGGL(k_query_clip, dim3(grid), dim3(256), 0, stream, st, rays, n);
}

hipError_t radianceQueryLaunchResults(hipStream_t stream, const float *sum, const uint32_t *count, float *outSum, uint32_t *outCount, uint32_t n)
{
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<size_t>(((size_t)n*3u + 255u)/256u, 2048u);
    hipLaunchKernelGGL(k_query_results, dim3(blocks), dim3(256), 0, stream, sum, count, outSum, outCount, n);
    return hipGetLastError();
}
