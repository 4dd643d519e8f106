// Launcher of ray_query.hip: batched closest-hit and occlusion queries on caller rays (tghip_query_rays, include/tungsten_hip.h).  The shim in
// shim_queries.hip holds the context, checks the arguments (csrc/host/RayQuery.cpp), stages host memory and resets the work counter in-stream; this
// enqueues the kernel on `stream` and returns.
#ifndef TGAMD_RAY_QUERY_H_
#define TGAMD_RAY_QUERY_H_

#include "pt_scene.h"

// which walk answers: the scene's flat record list, its BVH2, the BVH2 with the reference's tree over the instances, the 8-wide BVH
enum RayQueryWalk { RAY_QUERY_FLAT = 0, RAY_QUERY_BVH2 = 1, RAY_QUERY_INST = 2, RAY_QUERY_WIDE = 3 };
#define RAY_QUERY_THREADS 256

// rays: n x two float4 (o, tmin | d, tmax), 16-byte aligned device memory; out: n float4 hits (t, u, v, rec), or with `occluded` n bytes;
// counter: one device word of the context, zero when the kernel starts; blocks >= 1 workgroups of RAY_QUERY_THREADS lanes; refillAt 1..64: the idle lanes of a wave at which it
// claims new rays (the wide walk; the others claim per ray); ldsBytes: a stack of the walk's depth per lane
hipError_t rayQueryLaunch(hipStream_t stream, const DeviceScene &scene, RayQueryWalk walk, bool occluded, const float4 *rays, void *out, uint32_t n,
                          uint32_t *counter, uint32_t blocks, uint32_t refillAt, size_t ldsBytes);

#endif
