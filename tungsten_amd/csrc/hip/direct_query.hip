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
// One instantiation, under the all-features family's mask, so an answer never depends on which shading family the scene's passes use (FEAT_QMC
// cleared: the stream is the keyed PCG one, there is no Sobol' form).
// k_direct_setup's two bodies are restated in vertex_query.hip (k_vertex_front: the direct estimate of a caller-held path's vertex, on the path's own
// stream, medium and bounce + 1).  One difference is meant: that copy queues no light-sample segment for an emitter's black side, as k_shade does
// without the visibility output.  Whatever else changes here changes there; tests/test_gpu_vertex_query.py holds the two to each other on the camera
// vertex of three scenes.
#include "direct_query.h"
#include "pt_wavefront.h"

#define DIRECT_MASK (BSDF_MASK_ALL & ~FEAT_QMC)

namespace {

PT_DEV RayD loadRay(const float4 *rays, uint32_t i)
{
    const float4 ro = rays[(size_t)i*2u + 0u], rd = rays[(size_t)i*2u + 1u];
    RayD ray;
    ray.o = xyz(ro); ray.d = xyz(rd); ray.tmin = ro.w; ray.tmax = rd.w;
    return ray;
}

// The medium ray i starts in: the call's, or its own (out of range: an unspecified answer, no read outside the table)
PT_DEV int startMedium(const DirectParams &p, const int *media, uint32_t numMedia, uint32_t i)
{
    int medium = p.medium;
    if (media) {
        medium = media[i];
        if (medium == TGHIP_MEDIUM_OF_CAMERA) medium = p.cameraMedium;
        if (medium < 0 || (uint32_t)medium >= numMedia) medium = -1;
    }
    return medium;
}

// The segments of this wave that are alive, appended in lane order.  Called by all 64 lanes.
PT_DEV void appendLive(bool alive, uint32_t g, uint32_t *list, uint32_t *count)
{
    const unsigned long long on = __ballot(alive);
    if (on != 0ull) {
        const uint32_t lane = laneId();
        uint32_t base = 0;
        if (lane == 0)
            base = atomicAdd(count, (uint32_t)__popcll(on));
        base = __shfl(base, 0);
        if (alive) list[base + (uint32_t)__popcll(on & ((1ull << lane) - 1ull))] = g;
    }
}

PT_DEV void putSegment(const DirectState &st, uint32_t g, f3 o, float tmin, f3 d, float tmax, int medium, uint32_t bounce, int endCap, float mis,
                       f3 c, float cw, f3 e, float ew)
{
    st.o[g] = mk4(o, tmin);
    st.d[g] = mk4(d, tmax);
    st.t[g] = mk4(splat3(1.0f), __int_as_float(medium));
    st.b[g] = make_uint4(bounce, (uint32_t)endCap, __float_as_uint(0.0f), __float_as_uint(mis));
    st.c[g] = mk4(c, cw);
    st.e[g] = mk4(e, ew);
}

}  // namespace

template<bool VOLUME>
__global__ __launch_bounds__(DIRECT_QUERY_THREADS) void k_direct_setup(DeviceScene s, DirectParams p, const float4 *rays, const int *media, const float4 *hits,
                                                                      const int *inst, DirectState st, uint32_t *list, uint32_t *count)
{
    constexpr uint32_t M = DIRECT_MASK;
    const uint32_t k = blockIdx.x*DIRECT_QUERY_THREADS + threadIdx.x;
    bool q0 = false, q1 = false;
    if (k < p.rays*p.samples) {
        const uint32_t lr = k/p.samples, ls = k - lr*p.samples;
        const uint32_t i = p.ray0 + lr;
        const int medium = startMedium(p, media, s.num_media, i);
        const RayD ray = loadRay(rays, i);
        const float4 hit = VOLUME ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : hits[lr];
        if (VOLUME ? medium >= 0 : __float_as_int(hit.w) >= 0) {
            uint32_t status = 0u;
            float lightWeight = 1.0f;
            Rng rng = rngStart(p.seed, i, p.sample0 + ls);
            for (uint32_t j = 0; j < p.skip; ++j) (void)rngNextI(rng);
            if (VOLUME) {
                // volumeEstimateDirect / volumeSampleDirect / volumeLightSample / volumePhaseSample (TraceBase.cpp:323-381, 402-414, 470-481) at
                // mediumSample.p = ray.o with parentRay.dir() = ray.d: shadow rays start at tmin = 0, the medium is not re-selected
                const TgHipMedium &mm = s.media[medium];
                const f3 volP = ray.o;
                const int light = p.light >= 0 ? s.lights[p.light] : chooseLight<M>(s, rng, volP, lightWeight);
                if (light >= 0) {
                    status |= DIRECT_ITEM_ESTIMATE;
                    const bool meshLight = s.objects[light].type == TGHIP_OBJ_MESH;
                    const bool diracLight = s.objects[light].type == TGHIP_OBJ_POINT;
                    if (diracLight) status |= DIRECT_ITEM_DIRAC;
                    {
                        f3 d; float dist, pdf;
                        if (lightSampleDirect<M>(s, light, volP, rng, d, dist, pdf)) {
                            const float f = phaseEval(mm, ray.d, d);
                            if (f != 0.0f && meshLight) {
                                putSegment(st, k*2u, volP, 0.0f, d, PT_INF, medium, p.bounce, light, powerHeuristic(pdf, f), splat3(f), dist, splat3(0.0f), pdf);
                                q0 = true;
                            } else if (f != 0.0f) {
                                RayD sr; sr.o = volP; sr.d = d; sr.tmin = 0.0f; sr.tmax = PT_INF;   // parentRay.scatter(p, d, 0.0f)
                                LightHit lh;
                                bool reached;
                                if (diracLight) { lh.t = dist; lh.u = 0.0f; lh.v = 0.0f; lh.backSide = false; lh.n = splat3(0.0f); reached = true; }
                                else reached = lightIntersect<M>(s, light, sr, lh) && !(lh.t*(1.0f + 1e-3f) < dist);
                                if (reached) {
                                    const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                                    if (!isZero(e)) {      // (no transmittance is reported here: a black side needs no shadow ray)
                                        putSegment(st, k*2u, volP, 0.0f, d, lh.t, medium, p.bounce, light, diracLight ? 1.0f : powerHeuristic(pdf, f), splat3(f), 0.0f, e, pdf);
                                        q0 = true;
                                    }
                                }
                            }
                        }
                    }
                    if (!diracLight) {
                        f3 w; float ppdf;
                        phaseSample<M>(mm, rng, ray.d, w, ppdf);
                        if (meshLight) {
                            putSegment(st, k*2u + 1u, volP, 0.0f, w, PT_INF, medium, p.bounce, light, 1.0f, splat3(1.0f), ppdf, splat3(0.0f), 0.0f);   // directPdf needs the hit
                            q1 = true;
                        } else {
                            RayD sr; sr.o = volP; sr.d = w; sr.tmin = 0.0f; sr.tmax = PT_INF;
                            LightHit lh;
                            if (lightIntersect<M>(s, light, sr, lh)) {
                                const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                                if (!isZero(e)) {
                                    const float mis1 = powerHeuristic(ppdf, lightDirectPdf<M>(s, light, w, volP, lh));
                                    putSegment(st, k*2u + 1u, volP, 0.0f, w, lh.t, medium, p.bounce, light, mis1, splat3(1.0f), 0.0f, e, 0.0f);   // phaseSample.weight = 1
                                    q1 = true;
                                }
                            }
                        }
                    }
                    st.origin[k] = mk4(volP, 0.0f);
                }
            } else {
                Info info;
                intersectionInfo<M>(s, ray, hit, info, inst ? inst[lr] : -1);
                const uint32_t lobes = s.bsdfs[info.bsdf].lobes;
                // TraceBase::makeLocalScatterEvent (TraceBase.cpp:24-51)
                Frame frame = shadingFrame<M>(s, info);
                const bool hitBackside = dot(frame.normal, ray.d) > 0.0f;
                const bool flipped = s.settings.enable_two_sided_shading && hitBackside && !(lobes & LOBE_TRANSMISSIVE);
                if (flipped) {
                    frame.normal = -frame.normal;
                    frame.tangent = -frame.tangent;
                }
                Event ev;
                ev.wi = toLocal(frame, -ray.d);
                ev.u = info.u; ev.v = info.v; ev.rng = &rng;
                const bool consistency = s.settings.enable_consistency_checks != 0;
                auto isConsistent = [&](f3 woLocal, f3 w) {      // TraceBase.cpp:53-60
                    if (!consistency) return true;
                    const bool geometricBackside = dot(w, info.Ng) < 0.0f;
                    const bool shadingBackside = (woLocal.z < 0.0f) != flipped;
                    return geometricBackside == shadingBackside;
                };
                // each shadow ray starts in the medium on its side of the surface (TraceBase.cpp:260-261, 302-303)
                auto sideMedium = [&](f3 dir) {
                    return s.num_media ? selectMedium(s.objects[info.object], medium, dot(dir, info.Ng) < 0.0f) : medium;
                };
                // estimateDirect (TraceBase.cpp:483-494): chooseLight draws whatever sampleDirect then does
                const int light = p.light >= 0 ? s.lights[p.light] : chooseLight<M>(s, rng, info.p, lightWeight);
                const bool pureSpecular = lobes != 0 && (lobes & ~(uint32_t)LOBE_SPECULAR) == 0;
                if (light >= 0 && !pureSpecular && lobes != TGHIP_LOBE_FORWARD) {
                    status |= DIRECT_ITEM_ESTIMATE;
                    const bool meshLight = s.objects[light].type == TGHIP_OBJ_MESH;
                    const bool diracLight = s.objects[light].type == TGHIP_OBJ_POINT;
                    if (diracLight) status |= DIRECT_ITEM_DIRAC;
                    // lightSample (TraceBase.cpp:246-285)
                    {
                        f3 d; float dist, pdf;
                        if (lightSampleDirect<M>(s, light, info.p, rng, d, dist, pdf)) {
                            ev.wo = toLocal(frame, d);
                            ev.requested = LOBE_ALL_BUT_SPECULAR;
                            if (isConsistent(ev.wo, d)) {
                                const f3 f = bsdfEval<M>(s, info.bsdf, ev);
                                if (!isZero(f) && meshLight) {
                                    // whether the ray reaches a mesh emitter, and with which emission, is known after the walk (TriangleMesh::intersect
                                    // is a tree query): the round stage completes the term
                                    putSegment(st, k*2u, info.p, 5e-4f, d, PT_INF, sideMedium(d), p.bounce, light, powerHeuristic(pdf, bsdfPdf<M>(s, info.bsdf, ev)), f, dist,
                                               splat3(0.0f), pdf);
                                    q0 = true;
                                } else if (!isZero(f)) {
                                    RayD sr; sr.o = info.p; sr.d = d; sr.tmin = 5e-4f; sr.tmax = PT_INF;
                                    LightHit lh;
                                    // attenuatedEmission's own hit and distance test (TraceBase.cpp:155-162); a Dirac light is not intersected: the
                                    // shadow ray ends at the sampled distance
                                    bool reached;
                                    if (diracLight) { lh.t = dist; lh.u = 0.0f; lh.v = 0.0f; lh.backSide = false; lh.n = splat3(0.0f); reached = true; }
                                    else reached = lightIntersect<M>(s, light, sr, lh) && !(lh.t*(1.0f + 1e-3f) < dist);
                                    if (reached) {
                                        // (a black side too: attenuatedEmission reports the shadow ray's transmittance before it looks at the emission, :167-171)
                                        const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                                        const float mis0 = diracLight ? 1.0f : powerHeuristic(pdf, bsdfPdf<M>(s, info.bsdf, ev));   // no MIS against a Dirac light (:281-282)
                                        putSegment(st, k*2u, info.p, 5e-4f, d, lh.t, sideMedium(d), p.bounce, light, mis0, f, 0.0f, e, pdf);
                                        q0 = true;
                                    }
                                }
                            }
                        }
                    }
                    // bsdfSample (TraceBase.cpp:287-321); not for Dirac lights (:396-397)
                    if (!diracLight) {
                        ev.requested = LOBE_ALL_BUT_SPECULAR;
                        ev.weight = splat3(1.0f); ev.pdf = 1.0f;
                        if (bsdfSample<M>(s, info.bsdf, ev) && !isZero(ev.weight)) {
                            const f3 wog = toGlobal(frame, ev.wo);
                            if (isConsistent(ev.wo, wog)) {
                                if (meshLight) {
                                    putSegment(st, k*2u + 1u, info.p, 5e-4f, wog, PT_INF, sideMedium(wog), p.bounce, light, 1.0f, ev.weight, ev.pdf, splat3(0.0f), 0.0f);   // directPdf needs the hit
                                    q1 = true;
                                } else {
                                    RayD sr; sr.o = info.p; sr.d = wog; sr.tmin = 5e-4f; sr.tmax = PT_INF;
                                    LightHit lh;
                                    if (lightIntersect<M>(s, light, sr, lh)) {
                                        const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                                        if (!isZero(e)) {
                                            const float mis1 = powerHeuristic(ev.pdf, lightDirectPdf<M>(s, light, wog, info.p, lh));
                                            putSegment(st, k*2u + 1u, info.p, 5e-4f, wog, lh.t, sideMedium(wog), p.bounce, light, mis1, ev.weight, 0.0f, e, 0.0f);
                                            q1 = true;
                                        }
                                    }
                                }
                            }
                        }
                    }
                    st.origin[k] = mk4(info.p, 0.0f);
                }
            }
            st.status[k] = status | (q0 ? DIRECT_ITEM_SEG0 : 0u) | (q1 ? DIRECT_ITEM_SEG1 : 0u);
            st.weight[k] = lightWeight;
        }
    }
    appendLive(q0, k*2u, list, count);
    appendLive(q1, k*2u + 1u, list, count);
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
        active = startMedium(p, media, numMedia, i) >= 0;
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
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7FC00000u));
            const float4 r0 = (status & DIRECT_ITEM_SEG0) ? st.res[k*2u] : zero;
            f3 result = splat3(0.0f) + xyz(r0);
            if (!(status & DIRECT_ITEM_DIRAC)) {
                const float4 r1 = (status & DIRECT_ITEM_SEG1) ? st.res[k*2u + 1u] : zero;
                result = result + xyz(r1);
            }
            rgb = rgb + result*st.weight[k];
            if (!volume && !isnan(r0.w)) { visibility += r0.w; visibilityCount++; }
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
