// Launchers of surface_query.hip: what is at the closest hit of caller rays (tghip_query_surface, include/tungsten_hip.h).  The shim in
// shim_queries.hip holds the context, checks the arguments (csrc/host/SurfaceQuery.cpp), stages host memory and resets the work counter in-stream; these
// enqueue the two stages on `stream` and return.
#ifndef TGAMD_SURFACE_QUERY_H_
#define TGAMD_SURFACE_QUERY_H_

#include "ray_query.h"

// workgroup size of the dense stage: four waves, one per SIMD of a CU, staging 256 x 96 B = 24 KiB of answers in LDS -- six workgroups, 24 waves,
// fit a CU's 160 KiB, enough to hide the gathers of a kernel of 52 VGPRs
#define SURFACE_QUERY_THREADS 256

// Stage 1, the walk: tghip_query_rays' closest-hit walk (`walk`, `blocks`, `refillAt`, `ldsBytes`, `counter` as rayQueryLaunch's) that leaves per ray
// hits[i] = the float4 of a TgHipHit and -- RAY_QUERY_INST only, where `inst` must hold n words; unused otherwise -- inst[i] = the record index of the
// instance the hit was reached through, -1 = none.
hipError_t surfaceQueryLaunchWalk(hipStream_t stream, const DeviceScene &scene, RayQueryWalk walk, const float4 *rays, float4 *hits, int *inst, uint32_t n,
                                  uint32_t *counter, uint32_t blocks, uint32_t refillAt, size_t ldsBytes);
// Stage 2, dense: one lane per ray in ray order describes hits[i] (inst == nullptr: no hit was reached through an instance) and writes out[i], a
// TgHipSurface as six float4, 16-byte aligned device memory.
hipError_t surfaceQueryLaunchDescribe(hipStream_t stream, const DeviceScene &scene, const float4 *rays, const float4 *hits, const int *inst, float4 *out,
                                      uint32_t n);

#endif
