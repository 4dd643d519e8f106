// Direct lighting at the hit of caller rays (tghip_query_direct): TraceBase::estimateDirect (TraceBase.cpp:483-494) and its volume twin
// volumeEstimateDirect (:470-481) as a small wavefront on the context's stream.  Around the walks of its siblings, which it launches as they are --
// tghip_query_surface's closest-hit walk for the point, tghip_query_transmittance's walk over an index list for the shadow rays -- three dense stages:
//   k_direct_setup<VOLUME>  one lane per (ray, sample): the keyed stream, makeLocalScatterEvent, chooseLight, sampleDirect's early returns, lightSample
//                           and bsdfSample (volumeLightSample / volumePhaseSample) as far as they get without a walk -- sampleDirect, isConsistent,
//                           selectMedium, bsdfEval / bsdfPdf / bsdfSample, and for every light but a triangle mesh the light's own intersect, the
//                           distance test, evalDirect and directPdf.  A term that still needs its shadow ray is stored as a SEGMENT with its factors
//                           apart, as k_shade leaves them for k_trace_shadow under nee_factors, and appended to the first round's list: one atomicAdd
//                           per wave and term (ballot, popcount, rank).
//   k_direct_round          one lane per live segment behind its walk: one turn of generalizedShadowRay's loop (TraceBase.cpp:78-123) with the
//                           segment's own end cap -- k_transmittance_segment's steps in the reference's order -- and, where the loop ends, the rest of
//                           attenuatedEmission and of the sample: a mesh emitter's intersectionInfo, distance test, evalDirect and directPdf at the hit
//                           the walk found (what k_trace_shadow does for mesh lights), shadow*e, (f*e)/pdf, the power heuristic.
//   k_direct_finish         one lane per ray: (0 + lightSample) + bsdfSample, times chooseLight's weight, added to the ray's sum sample by sample in
//                           sample order; the shadow ray's transmittance.avg() of the samples that recorded one; 32 bytes as two 16-byte stores.
// Separate launches because the setup carries BSDF, texture, light and medium code at once and must not share registers with a walk, because a round's
// lanes are the segments still alive and not the items they came from, and because the order of a ray's float additions is part of the answer: the
// finish adds in sample order whatever order the segments ended in.
// The setup's two bodies -- the estimate at one point -- and the helpers around them are direct_estimate.h's, shared with vertex_query.hip's front
// stage (the direct estimate of a caller-held path's vertex); here with KEEP_BLACK set, for the visibility output.
#include "direct_estimate.h"

template<bool VOLUME>
__global__ __launch_bounds__(DIRECT_QUERY_THREADS) void k_direct_setup(DeviceScene s, DirectParams p, const float4 *rays, const int *media, const float4 *hits,
                                                                      const int *inst, DirectState st, uint32_t *list, uint32_t *count)
{
    const uint32_t k = blockIdx.x*DIRECT_QUERY_THREADS + threadIdx.x;
    uint32_t status = 0u;
    if (k < p.rays*p.samples) {
        const uint32_t lr = k/p.samples, ls = k - lr*p.samples;
        const uint32_t i = p.ray0 + lr;
        const int medium = rayStartMedium(p, media, s.num_media, i);
        const RayD ray = loadRay(rays, i);
        const float4 hit = VOLUME ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : hits[lr];
        if (VOLUME ? medium >= 0 : __float_as_int(hit.w) >= 0) {
            float lightWeight = 1.0f;
            Rng rng = rngStart(p.seed, i, p.sample0 + ls);
            for (uint32_t j = 0; j < p.skip; ++j) (void)rngNextI(rng);
            if (VOLUME) {
                // at mediumSample.p = ray.o with parentRay.dir() = ray.d
                status = estimateDirectVolume(s, st, k, rng, ray.o, ray.d, medium, p.bounce, p.light, lightWeight);
            } else {
                ScatterPoint pt;
                Event ev;
                makeScatterPoint(s, ray, hit, inst ? inst[lr] : -1, rng, pt, ev);
                status = estimateDirectSurface<true>(s, st, k, rng, pt, ev, medium, p.bounce, p.light, lightWeight);
            }
            st.status[k] = status;
            st.weight[k] = lightWeight;
        }
    }
    appendLive((status & DIRECT_ITEM_SEG0) != 0u, k*2u, list, count);
    appendLive((status & DIRECT_ITEM_SEG1) != 0u, k*2u + 1u, list, count);
}

// One turn of generalizedShadowRayImpl<false>'s loop for one segment, behind its `_scene->intersect` (the walk's launch), with endsOnSurface = true:
// k_transmittance_segment's steps, the end cap the segment's own; where the loop ends, what is left of attenuatedEmission and of lightSample / bsdfSample.
// Every lane of a wave gets here -- the ones past the round's end with `live` clear -- because the survivors are counted with a ballot.
__global__ __launch_bounds__(DIRECT_QUERY_THREADS) void k_direct_round(DeviceScene s, DirectState st, const uint32_t *list, uint32_t n, uint32_t *next, uint32_t *nextCount)
{
    constexpr uint32_t M = DIRECT_MASK;
    const uint32_t j = blockIdx.x*DIRECT_QUERY_THREADS + threadIdx.x;
    bool goesOn = false;
    uint32_t g = 0;
    if (j < n) {
        g = list[j];
        const float4 ro = st.o[g], rd = st.d[g], tm = st.t[g];
        const uint4 b = st.b[g];
        RayD ray;
        ray.o = xyz(ro); ray.d = xyz(rd); ray.tmin = ro.w; ray.tmax = rd.w;
        f3 transmittance = xyz(tm);
        int medium = __float_as_int(tm.w);
        uint32_t bounce = b.x;
        const int endCap = (int)b.y;
        const float travelled = __uint_as_float(b.z);
        const bool startsOnSurface = ray.tmin != 0.0f;       // the shadow rays of a volume vertex start at tmin = 0; every later stretch starts on a surface
        const bool lightTerm = (g & 1u) == 0u;
        const TgHipObject &lo = s.objects[endCap];
        const bool meshLight = lo.type == TGHIP_OBJ_MESH;
        const float4 hit = st.hits[g];
        const int hitInst = st.inst ? st.inst[g] : -1;
        const int ri = __float_as_int(hit.w);
        int hitObject = -1;
        if (ri >= 0)          // geometry reached through an instance belongs to the `instances` primitive (never a light)
            hitObject = (int)TGHIP_REC_OBJECT(__float_as_uint(at32(s.recs, (uint32_t)(hitInst >= 0 ? hitInst : ri)*3u).w));
        bool ended = false, visValid = true;
        f3 meshE = splat3(0.0f);
        float meshMis = 1.0f;
        if (meshLight && ri < 0) {                           // the ray never reaches the mesh: attenuatedEmission returns before its shadow ray
            transmittance = splat3(0.0f); visValid = false; ended = true;
        } else if (ri < 0 || hitObject == endCap) {
            // The quad the ray is aimed at is only FOUND when Embree's slab test lets the ray into its flat box (k_trace_shadow, pt_wavefront.h): culled,
            // the function returns as at the end cap, but ray.farT() was not shortened to the hit
            bool found = ri >= 0;
            if (found && lo.type == TGHIP_OBJ_QUAD) {
                const f3 q = ld3(lo.base), e0 = ld3(lo.edge0), e1 = ld3(lo.edge1);
                const f3 p1 = q + e0, p2 = q + e1, p3 = (q + e0) + e1;
                const f3 bl = mk3(fminf(fminf(q.x, p1.x), fminf(p2.x, p3.x)), fminf(fminf(q.y, p1.y), fminf(p2.y, p3.y)), fminf(fminf(q.z, p1.z), fminf(p2.z, p3.z)));
                const f3 bh = mk3(fmaxf(fmaxf(q.x, p1.x), fmaxf(p2.x, p3.x)), fmaxf(fmaxf(q.y, p1.y), fmaxf(p2.y, p3.y)), fmaxf(fmaxf(q.z, p1.z), fmaxf(p2.z, p3.z)));
                found = embreeBoxVisible(ray.o, ray.d, ray.tmin, ray.tmax, bl, bh);
            }
            if (medium >= 0)                                 // TraceBase.cpp:104-112; ray.farT() is the hit distance when anything was found
                transmittance = transmittance*mediumTransmittance(s, medium, ray.o, ray.d, found ? hit.x : ray.tmax, startsOnSurface, true);
            if ((int)bounce < s.settings.min_bounces) transmittance = splat3(0.0f);   // :114-115
            if (meshLight) {
                // attenuatedEmission on a mesh light (TraceBase.cpp:144-174, TriangleMesh.cpp:344-355, 469-473, 493-496) at the hit the walk found
                Info li;
                intersectionInfo<M>(s, ray, hit, li);
                f3 e = lightEvalDirect<M>(s, endCap, li.u, li.v, li.backSide);
                const float total = travelled + hit.x;
                const float4 c = st.c[g];
                if (lightTerm) {
                    if (total*(1.0f + 1e-3f) < c.w) { e = splat3(0.0f); visValid = false; }   // a nearer part of the mesh than the sampled point
                } else {
                    const float directPdf = lengthSq(xyz(st.origin[g >> 1]) - li.p)/(-dot(ray.d, li.Ng)*lo.area);
                    meshMis = powerHeuristic(c.w, directPdf);
                }
                meshE = e;
            }
            ended = true;
        } else {                                             // didHit (TraceBase.cpp:79-102)
            Info info;
            intersectionInfo<M>(s, ray, hit, info, hitInst);
            const uint32_t lobes = s.bsdfs[info.bsdf].lobes;
            if (!(lobes & TGHIP_LOBE_FORWARD)) {
                transmittance = splat3(0.0f); ended = true;
            } else {
                Frame frame = frameFromNormal(info.Ns);
                const bool hitBackside = dot(frame.normal, ray.d) > 0.0f;
                if (s.settings.enable_two_sided_shading && hitBackside && !(lobes & LOBE_TRANSMISSIVE)) {
                    frame.normal = -frame.normal;
                    frame.tangent = -frame.tangent;
                }
                Event fe;
                fe.wi = toLocal(frame, -ray.d); fe.wo = -fe.wi;
                fe.requested = TGHIP_LOBE_FORWARD; fe.u = info.u; fe.v = info.v; fe.rng = nullptr;
                const f3 transparency = bsdfEval<M>(s, info.bsdf, fe);
                if (isZero(transparency)) {
                    transmittance = splat3(0.0f); ended = true;
                } else {
                    transmittance = transmittance*transparency;
                    bounce++;
                    if ((int)bounce >= s.settings.max_bounces) {
                        transmittance = splat3(0.0f); ended = true;
                    } else {
                        if (medium >= 0)                     // the medium AFTER the transparency: the reference's order (:97, 104-112)
                            transmittance = transmittance*mediumTransmittance(s, medium, ray.o, ray.d, hit.x, startsOnSurface, true);
                        if (s.num_media)                     // :116
                            medium = selectMedium(s.objects[info.object], medium, !info.backSide);
                        st.o[g] = mk4(ray.o + ray.d*hit.x, 5e-4f);
                        st.d[g] = mk4(ray.d, ray.tmax - hit.x);
                        st.t[g] = mk4(transmittance, __int_as_float(medium));
                        st.b[g] = make_uint4(bounce, b.y, __float_as_uint(travelled + hit.x), b.w);
                        goesOn = true;
                    }
                }
            }
        }
        if (ended) {
            // attenuatedEmission returns shadow*light.evalDirect (TraceBase.cpp:173); lightSample (f*e)/pdf, then *= the power heuristic unless the light is
            // a Dirac one (:277-282; its weight is stored as 1); bsdfSample (e*weight), then *= the power heuristic (:316-318); the volume pair likewise
            const f3 shadowT = transmittance;
            const bool dark = isZero(transmittance);         // `if (shadow == 0.0f) return Vec3f(0.0f)` (:170-171)
            const float4 c = st.c[g], le = st.e[g];
            const f3 e = transmittance*(meshLight ? meshE : xyz(le));
            f3 term;
            if (lightTerm) term = (xyz(c)*e)/le.w*__uint_as_float(b.w);
            else           term = (e*xyz(c))*(meshLight ? meshMis : __uint_as_float(b.w));
            if (dark || isZero(e)) term = splat3(0.0f);      // `if (e == 0.0f) return Vec3f(0.0f)` (:273-274, 311-312)
            st.res[g] = mk4(term, visValid ? avg3(shadowT) : __uint_as_float(0x7FC00000u));
        }
    }
    appendLive(goesOn, g, next, nextCount);
}

// The estimates of one ray's items in sample order.  sampleDirect: result(0) += lightSample, += bsdfSample unless the light is a Dirac one
// (TraceBase.cpp:390-399), times chooseLight's weight (:493); the visibility output takes the light sample's transmittance.avg() where
// attenuatedEmission reported one (PathTracer.cpp:70, 93-94).  An item whose sampleDirect returned early, or that found no light, adds a zero.
__global__ __launch_bounds__(DIRECT_QUERY_THREADS) void k_direct_finish(DirectParams p, bool volume, const int *media, uint32_t numMedia, const float4 *hits,
                                                                       DirectState st, float4 *out)
{
    const uint32_t lr = blockIdx.x*DIRECT_QUERY_THREADS + threadIdx.x;
    if (lr >= p.rays) return;
    const uint32_t i = p.ray0 + lr;
    int rec = -1;
    bool active;
    if (volume) {
        active = rayStartMedium(p, media, numMedia, i) >= 0;
    } else {
        rec = __float_as_int(hits[lr].w);
        active = rec >= 0;
        if (!active) rec = -1;
    }
    f3 rgb = splat3(0.0f);
    float visibility = 0.0f;
    uint32_t count = 0u, visibilityCount = 0u;
    if (!p.first) {
        const float4 a = out[(size_t)i*2u + 0u], b = out[(size_t)i*2u + 1u];
        rgb = xyz(a); visibility = a.w;
        count = __float_as_uint(b.x); visibilityCount = __float_as_uint(b.y);
    }
    if (active) {
        for (uint32_t ls = 0; ls < p.samples; ++ls) {
            const uint32_t k = lr*p.samples + ls;
            const uint32_t status = st.status[k];
            count++;
            if (!(status & DIRECT_ITEM_ESTIMATE)) continue;
            float shadowT;
            const f3 result = directItemResult(st, k, status, shadowT);
            rgb = rgb + result*st.weight[k];
            if (!volume && !isnan(shadowT)) { visibility += shadowT; visibilityCount++; }
        }
    }
    out[(size_t)i*2u + 0u] = mk4(rgb, visibility);
    out[(size_t)i*2u + 1u] = make_float4(__uint_as_float(count), __uint_as_float(visibilityCount), __int_as_float(rec), __uint_as_float(0u));
}

hipError_t directQueryLaunchSetup(hipStream_t stream, const DeviceScene &scene, const DirectParams &p, bool volume, const float4 *rays, const int *media,
                                  const float4 *hits, const int *inst, const DirectState &st, uint32_t *list, uint32_t *count)
{
    const uint32_t items = p.rays*p.samples;
    const dim3 grid((items + DIRECT_QUERY_THREADS - 1u)/DIRECT_QUERY_THREADS), block(DIRECT_QUERY_THREADS);
    if (volume) hipLaunchKernelGGL(k_direct_setup<true>, grid, block, 0, stream, scene, p, rays, media, hits, inst, st, list, count);
    else        hipLaunchKernelGGL(k_direct_setup<false>, grid, block, 0, stream, scene, p, rays, media, hits, inst, st, list, count);
    return hipGetLastError();
}

hipError_t directQueryLaunchRound(hipStream_t stream, const DeviceScene &scene, const DirectState &st, const uint32_t *list, uint32_t live, uint32_t *next,
                                  uint32_t *nextCount)
{
    const dim3 grid((live + DIRECT_QUERY_THREADS - 1u)/DIRECT_QUERY_THREADS), block(DIRECT_QUERY_THREADS);
    hipLaunchKernelGGL(k_direct_round, grid, block, 0, stream, scene, st, list, live, next, nextCount);
    return hipGetLastError();
}

hipError_t directQueryLaunchFinish(hipStream_t stream, const DirectParams &p, bool volume, const int *media, uint32_t numMedia, const float4 *hits,
                                   const DirectState &st, float4 *out)
{
    const dim3 grid((p.rays + DIRECT_QUERY_THREADS - 1u)/DIRECT_QUERY_THREADS), block(DIRECT_QUERY_THREADS);
    hipLaunchKernelGGL(k_direct_finish, grid, block, 0, stream, p, volume, media, numMedia, hits, st, out);
    return hipGetLastError();
}
