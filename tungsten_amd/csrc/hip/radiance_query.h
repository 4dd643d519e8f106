// Launchers of radiance_query.hip: the two small kernels tghip_query_radiance (include/tungsten_hip.h) adds to a pass of the wavefront loop -- the
// ray source in front of every closest-hit launch, and the copy of the pass's sums and counts into the caller's arrays.  The shim in shim_queries.hip
// holds the context, checks the arguments and plans the pass (csrc/host/RadianceQuery.cpp) and stages host memory, tungsten_hip.hip drives the loop
// (tghipRunPass; runBatch launches the ray source); these enqueue on `stream` and return.
#ifndef TGAMD_RADIANCE_QUERY_H_
#define TGAMD_RADIANCE_QUERY_H_

#include "pt_kernels.h"

// k_query_paths over the `grid` workgroups of `st` (the pool, or one part of it): for every slot of a workgroup's Q_EXTP bitmap -- the paths nextPath
// has just generated -- the ray of the path's "pixel" i replaces the camera ray: origin and tmin into A_RAY_O, direction and tmax into A_RAY_D from
// rays[2 i], rays[2 i + 1]; a padding pixel i >= n gets tmax = -1 and no throughput.  rays: 16-byte aligned device memory of n rays.
void radianceQueryLaunchPaths(hipStream_t stream, int grid, const PathState &st, const float4 *rays, uint32_t n);
// k_query_clip over the same workgroups, behind every closest-hit launch: a path on its first segment whose hit lies at t >= rays[i].tmax has hit
// nothing inside [tmin, tmax) and joins the escaped paths (k_query_paths lets the walk look a little further than tmax; this ends the segment exactly)
void radianceQueryLaunchClip(hipStream_t stream, int grid, const PathState &st, const float4 *rays, uint32_t n);
// outSum[0, 3 n) = sum[0, 3 n), outCount[0, n) = count[0, n) (outCount may be NULL): the first n pixels of the pass's framebuffer, word by word
hipError_t radianceQueryLaunchResults(hipStream_t stream, const float *sum, const uint32_t *count, float *outSum, uint32_t *outCount, uint32_t n);

#endif
