// Launchers of transmittance_query.hip: TraceBase::generalizedShadowRay on caller rays (tghip_query_transmittance, include/tungsten_hip.h) as a small
// wavefront.  The shim in shim_queries.hip holds the context, checks the arguments (csrc/host/TransmittanceQuery.cpp), stages host memory, resets the
// two counter words in-stream before every round and reads the survivors' count back behind it; these enqueue one round's two stages and return.
#ifndef TGAMD_TRANSMITTANCE_QUERY_H_
#define TGAMD_TRANSMITTANCE_QUERY_H_

#include "ray_query.h"

// workgroup size of the dense stage: four waves, one per SIMD of a CU
#define TRANSMITTANCE_QUERY_THREADS 256

// The rays of a query between its rounds, one entry per ray of the batch (indexed by the ray's index, not by its place in a round's list), and what
// a round hands to the next: 16-byte vectors, each array read and written with one access per ray.
struct TransmittanceState {
    float4 *o;            // origin of the current segment, its tmin
    float4 *d;            // direction, the distance that remains (the segment's tmax)
    float4 *t;            // throughput, the medium the ray is in (bits of an int, -1 = none)
    uint2 *b;             // bounce, crossed
    float4 *hits;         // the walk's answer for the current segment: a TgHipHit
    int *inst;            // RAY_QUERY_INST: the instance record the hit was reached through, -1 = none; nullptr otherwise
};

// What is the same for every ray of a call
struct TransmittanceParams {
    int medium;           // start medium when `media` is nullptr: index or -1 (the shim has resolved TGHIP_MEDIUM_OF_CAMERA)
    int cameraMedium;     // what a per-ray TGHIP_MEDIUM_OF_CAMERA stands for
    int endCap;           // object index, -1 = none
    uint32_t bounce;
    uint32_t startsOnSurface, endsOnSurface;
};

// Stage 1 of a round, the walk: tghip_query_rays' closest-hit walk (`walk`, `blocks`, `refillAt`, `ldsBytes`, `counter` as rayQueryLaunch's) over `live`
// rays.  list == nullptr (round 0): ray j of the launch is ray j of the batch, read from `rays`; else it is ray list[j], read from st.o / st.d.
// Leaves st.hits[i] and -- RAY_QUERY_INST -- st.inst[i] for every such ray i.
hipError_t transmittanceQueryLaunchWalk(hipStream_t stream, const DeviceScene &scene, RayQueryWalk walk, const float4 *rays, const TransmittanceState &st,
                                        const uint32_t *list, uint32_t live, uint32_t *counter, uint32_t blocks, uint32_t refillAt, size_t ldsBytes);
// Stage 2, dense: one lane per ray of the round (list as above; round 0 takes the start state from `p` and `media`, n words or nullptr) does the
// round's steps of generalizedShadowRay and either writes out[i] -- a TgHipTransmittance as a float4, 16-byte aligned device memory -- or stores the
// ray's state and appends i to `next`, counting in *nextCount (zero when the launch starts).  `next` holds at least `live` words.
hipError_t transmittanceQueryLaunchSegment(hipStream_t stream, const DeviceScene &scene, const TransmittanceParams &p, const float4 *rays, const int *media,
                                           const TransmittanceState &st, const uint32_t *list, uint32_t live, float4 *out, uint32_t *next, uint32_t *nextCount);

#endif
