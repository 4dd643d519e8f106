// Launchers of vertex_query.hip: one turn of PathTracer::traceSample's loop (integrators/path_tracer/PathTracer.cpp:50-131) on paths whose state the
// caller holds (tghip_query_vertex, include/tungsten_hip.h) as a small wavefront.  The shim in shim_queries.hip holds the context, checks the arguments
// (csrc/host/VertexQuery.cpp), stages host memory, cuts a large call into parts, runs the closest-hit walk of tghip_query_surface (surface_query.h)
// over the live paths' rays and the shadow walks and rounds of tghip_query_direct (transmittance_query.h, direct_query.h) as they are, and reads the
// one-word counts back; these enqueue the three dense stages and return.
#ifndef TGAMD_VERTEX_QUERY_H_
#define TGAMD_VERTEX_QUERY_H_

#include "direct_query.h"

// workgroup size of the dense stages: four waves, one per SIMD of a CU
#define VERTEX_QUERY_THREADS 256
// a TgHipPath as 16-byte vectors
#define VERTEX_PATH_VECTORS 7u

// What is the same for every path of a part
struct VertexParams {
    uint32_t seed, sample, firstIndex, firstNumber;   // TGHIP_VERTEX_START: the stream's key and the numbers thrown away first
    int medium;           // TGHIP_VERTEX_START: start medium when `media` is nullptr: index or -1 (the shim has resolved TGHIP_MEDIUM_OF_CAMERA)
    int cameraMedium;     // what a per-ray TGHIP_MEDIUM_OF_CAMERA stands for
    uint32_t path0;       // the part's first path: paths, rays and media below are the whole call's, indexed by path0 + local path
    uint32_t paths;       // ... and how many it covers
    uint32_t start;       // 1: TGHIP_VERTEX_START
};

// What the front stage leaves for the back stage, per live path of the turn (indexed by the path's place in the turn's list, as the DirectState
// whose item it is): the factors the direct term is multiplied with and the emissive hit's term, apart.
struct VertexState {
    float4 *w;            // the throughput estimateDirect's result is multiplied with, chooseLight's weight
    float4 *p;            // the emissive hit's term; VERTEX_ADD_* bits
};
#define VERTEX_ADD_PENDING 1u   // handleSurface got as far as its emission term (zero or not): it is added

// The stage in front of a call's first turn: one lane per path of the part.  TGHIP_VERTEX_START makes state i from ray i first.  The paths that are
// alive are appended to `list` (the path's index in the call), counted in *count (zero when the launch starts), and their rays -- the walk's far
// distance in place of tmax -- written to `walkRays` at the same place.
hipError_t vertexQueryLaunchBegin(hipStream_t stream, const VertexParams &p, uint32_t numMedia, const float4 *rays, const int *media, float4 *paths,
                                  uint32_t *list, float4 *walkRays, uint32_t *count);
// The front stage, behind the closest-hit walk over walkRays (hits / inst, indexed like `list`): one lane per live path does everything of the turn
// that needs no shadow walk and writes the path's new state but for the terms the back stage adds; item j of `st` is path list[j]'s direct estimate
// (direct_estimate.h's bodies, as k_direct_setup calls them, but without the segment of a light sample whose emission is zero),
// its live segments appended to segList, counted in *segCount (zero when the launch starts; segList holds two words per path).
hipError_t vertexQueryLaunchFront(hipStream_t stream, const DeviceScene &scene, float4 *paths, const uint32_t *list, uint32_t live, const float4 *hits,
                                  const int *inst, const DirectState &st, const VertexState &vs, uint32_t *segList, uint32_t *segCount);
// The back stage, behind the rounds of the shadow segments: one lane per live path adds the finished terms in the reference's order, runs the guards,
// writes emission and status, and appends the survivors to `next` with their rays in walkRays, counted in *nextCount (zero when the launch starts).
hipError_t vertexQueryLaunchBack(hipStream_t stream, float4 *paths, const uint32_t *list, uint32_t live, const DirectState &st, const VertexState &vs,
                                 uint32_t *next, float4 *walkRays, uint32_t *nextCount);

#endif
