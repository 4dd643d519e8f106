// Launchers of direct_query.hip: TraceBase::estimateDirect / volumeEstimateDirect at the hit (or start) of caller rays (tghip_query_direct,
// include/tungsten_hip.h) as a small wavefront.  The shim in shim_queries.hip holds the context, checks the arguments (csrc/host/DirectQuery.cpp),
// stages host memory, cuts a large call into chunks of items, runs the hit walk of tghip_query_surface (surface_query.h) and the shadow walks of
// tghip_query_transmittance (transmittance_query.h) as they are, and reads the survivors' count back behind every round; these enqueue the three
// dense stages and return.
#ifndef TGAMD_DIRECT_QUERY_H_
#define TGAMD_DIRECT_QUERY_H_

#include "ray_query.h"

// workgroup size of the dense stages: four waves, one per SIMD of a CU
#define DIRECT_QUERY_THREADS 256

// An ITEM is one (ray, sample) of the chunk under way: item k = (ray - ray0)*samples + (sample - sample0).  It owns two shadow SEGMENTS, 2k the light
// sample's and 2k + 1 the BSDF's (or phase function's).  16-byte vectors, each array read and written with one access per segment and stage.
struct DirectState {
    // per item
    uint32_t *status;     // DIRECT_ITEM_* bits
    float *weight;        // chooseLight's weight
    float4 *origin;       // where the shadow rays start (the mesh emitter's directPdf needs it after the walk has moved on)
    // per segment: the walk's view of it (TransmittanceState's o, d, hits, inst: transmittance_query.hip's walks read and write these) ...
    float4 *o;            // origin of the current stretch, its tmin
    float4 *d;            // direction, the distance that remains (the stretch's tmax)
    float4 *hits;         // the walk's answer for the current stretch: a TgHipHit
    int *inst;            // RAY_QUERY_INST: the instance record the hit was reached through; nullptr otherwise
    // ... and what the round stage carries
    float4 *t;            // transmittance so far, the medium the stretch is in (bits of an int, -1 = none)
    uint4 *b;             // bounce, end cap (the light's object), distance travelled (float bits), the power heuristic's weight (float bits)
    float4 *c;            // f or the sample's weight; mesh emitters: the sampled distance (light sample) / the BSDF's pdf
    float4 *e;            // the emission of an analytic or infinite light at the end; the light sample's pdf
    float4 *res;          // the finished term; its shadow ray's transmittance.avg(), or a NaN when attenuatedEmission never got to the shadow ray
};
#define DIRECT_ITEM_ESTIMATE 1u   // sampleDirect got past its early returns: the terms below count
#define DIRECT_ITEM_DIRAC    2u   // ... of a Dirac light: no BSDF term is added
#define DIRECT_ITEM_SEG0     4u   // the light sample queued a shadow segment
#define DIRECT_ITEM_SEG1     8u   // the BSDF / phase sample did

// What is the same for every item of a chunk
struct DirectParams {
    uint32_t seed, skip, bounce;
    int light;            // -1: chooseLight; else a slot of the scene's lights
    int medium;           // start medium when `media` is nullptr: index or -1 (the shim has resolved TGHIP_MEDIUM_OF_CAMERA)
    int cameraMedium;     // what a per-ray TGHIP_MEDIUM_OF_CAMERA stands for
    uint32_t ray0;        // the chunk's first ray: rays, media, hits and answers below are the whole call's, indexed by ray0 + local ray
    uint32_t rays;        // ... and how many it covers
    uint32_t sample0;     // first sample index of the chunk (an absolute one: the stream's key)
    uint32_t samples;     // ... and how many per ray
    uint32_t first;       // 1: the chunk holds the first samples of its rays (the sums start from zero); 0: they go on from the answers so far
};

// Surface mode (volume == false): hits / inst hold the closest hit of the chunk's rays, indexed by local ray (surfaceQueryLaunchWalk).  One lane per
// item: the event, chooseLight, the light's and the BSDF's sample with everything about an analytic light that needs no walk; the live segments are
// appended to `list`, counted in *count (zero when the launch starts; `list` holds two words per item).
hipError_t directQueryLaunchSetup(hipStream_t stream, const DeviceScene &scene, const DirectParams &p, bool volume, const float4 *rays, const int *media,
                                  const float4 *hits, const int *inst, const DirectState &st, uint32_t *list, uint32_t *count);
// One round of the shadow segments in `list` behind their walk (transmittanceQueryLaunchWalk over st.o / st.d): a segment that ends gets its term in
// st.res, one that goes on is appended to `next`, counted in *nextCount
hipError_t directQueryLaunchRound(hipStream_t stream, const DeviceScene &scene, const DirectState &st, const uint32_t *list, uint32_t live, uint32_t *next,
                                  uint32_t *nextCount);
// One lane per ray of the chunk: its items' estimates added in sample order into out[ray0 + .] (a TgHipDirect as two float4)
hipError_t directQueryLaunchFinish(hipStream_t stream, const DirectParams &p, bool volume, const int *media, uint32_t numMedia, const float4 *hits,
                                   const DirectState &st, float4 *out);

#endif
