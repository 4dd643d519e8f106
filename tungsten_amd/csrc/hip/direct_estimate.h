// The direct estimate at one point, once: TraceBase::estimateDirect (TraceBase.cpp:483-494) with sampleDirect / lightSample / bsdfSample (:246-321,
// 383-400) and the volume twin volumeEstimateDirect (:470-481) with volumeSampleDirect / volumeLightSample / volumePhaseSample (:323-381, 402-414), as
// far as they get without a shadow walk.  k_direct_setup (direct_query.hip: the hit or start of a caller ray) and k_vertex_front (vertex_query.hip: the
// vertex of a caller-held path, on the path's own stream, medium and bounce + 1) both call it; what it leaves -- SEGMENTS with their factors apart, as
// k_shade leaves them for k_trace_shadow under nee_factors -- k_direct_round completes behind the walks.  With it the helpers both units need: a segment's
// store and an item's sum (the ballot-append, the start medium and the walk's far distance are query_walk.h's: other units use them too).
// Form: force-inlined function templates (PT_DEV) under DIRECT_MASK, the one mask of both units.  The three kernels that inline the bodies stay within
// their occupancy steps this way (profiles/direct_estimate/kernel_resources_diff.txt), so the textual form of query_walk_wide.h was not needed.
// The bodies differ between the callers in one place, a compile-time switch: KEEP_BLACK, see estimateDirectSurface.
#ifndef TGAMD_DIRECT_ESTIMATE_H_
#define TGAMD_DIRECT_ESTIMATE_H_

#include "direct_query.h"
#include "query_walk.h"

// One instantiation, under the all-features family's mask, so an answer never depends on which shading family the scene's passes use (FEAT_QMC
// cleared: the stream is the keyed PCG one, there is no Sobol' form)
#define DIRECT_MASK (BSDF_MASK_ALL & ~FEAT_QMC)

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

// sampleDirect's sum for item k behind the rounds: result(0) += lightSample, += bsdfSample unless the light is a Dirac one (TraceBase.cpp:390-399).
// shadowT: the light sample's transmittance.avg(), a NaN where attenuatedEmission reported none.
PT_DEV f3 directItemResult(const DirectState &st, uint32_t k, uint32_t status, float &shadowT)
{
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7FC00000u));
    const float4 r0 = (status & DIRECT_ITEM_SEG0) ? st.res[k*2u] : zero;
    f3 result = splat3(0.0f) + xyz(r0);
    if (!(status & DIRECT_ITEM_DIRAC)) {
        const float4 r1 = (status & DIRECT_ITEM_SEG1) ? st.res[k*2u + 1u] : zero;
        result = result + xyz(r1);
    }
    shadowT = r0.w;
    return result;
}

// TraceBase::makeLocalScatterEvent (TraceBase.cpp:24-51) at the hit of `ray`: the point, its frame -- flipped where two-sided shading says so --
// and the event with wi, u, v and the stream set
struct ScatterPoint {
    Info info;
    Frame frame;
    uint32_t lobes;
    bool flipped;
};

PT_DEV void makeScatterPoint(const DeviceScene &s, const RayD &ray, float4 hit, int hitInst, Rng &rng, ScatterPoint &pt, Event &ev)
{
    constexpr uint32_t M = DIRECT_MASK;
    intersectionInfo<M>(s, ray, hit, pt.info, hitInst);
    pt.lobes = s.bsdfs[pt.info.bsdf].lobes;
    pt.frame = shadingFrame<M>(s, pt.info);
    const bool hitBackside = dot(pt.frame.normal, ray.d) > 0.0f;
    pt.flipped = s.settings.enable_two_sided_shading && hitBackside && !(pt.lobes & LOBE_TRANSMISSIVE);
    if (pt.flipped) {
        pt.frame.normal = -pt.frame.normal;
        pt.frame.tangent = -pt.frame.tangent;
    }
    ev.wi = toLocal(pt.frame, -ray.d);
    ev.u = pt.info.u; ev.v = pt.info.v; ev.rng = &rng;
}

PT_DEV bool isConsistent(const DeviceScene &s, const ScatterPoint &pt, f3 woLocal, f3 w)      // TraceBase.cpp:53-60
{
    if (!s.settings.enable_consistency_checks) return true;
    const bool geometricBackside = dot(w, pt.info.Ng) < 0.0f;
    const bool shadingBackside = (woLocal.z < 0.0f) != pt.flipped;
    return geometricBackside == shadingBackside;
}

// a ray that leaves the point along `dir` starts in the medium on its side of the surface (TraceBase.cpp:260-261, 302-303, 561-563)
PT_DEV int sideMedium(const DeviceScene &s, const ScatterPoint &pt, int medium, f3 dir)
{
    return s.num_media ? selectMedium(s.objects[pt.info.object], medium, dot(dir, pt.info.Ng) < 0.0f) : medium;
}

// estimateDirect at `pt`, which lies in `medium`: item k of `st`, its segments 2k (the light sample's) and 2k + 1 (the BSDF sample's) stored with
// `bounce`; lightSlot: a slot of the scene's lights, or -1 for chooseLight, whose weight goes to lightWeight.  Returns the item's DIRECT_ITEM_* bits.
// KEEP_BLACK: the light sample's segment is queued even where evalDirect is zero at the sampled point -- attenuatedEmission reports the shadow ray's
// transmittance before it looks at the emission (TraceBase.cpp:167-171), which tghip_query_direct's visibility output needs; a path's vertex, like
// k_shade, needs no shadow ray there.
template<bool KEEP_BLACK>
PT_DEV uint32_t estimateDirectSurface(const DeviceScene &s, const DirectState &st, uint32_t k, Rng &rng, const ScatterPoint &pt, Event &ev, int medium,
                                      uint32_t bounce, int lightSlot, float &lightWeight)
{
    constexpr uint32_t M = DIRECT_MASK;
    const Info &info = pt.info;
    uint32_t status = 0u;
    // chooseLight draws whatever sampleDirect then does
    const int light = lightSlot >= 0 ? s.lights[lightSlot] : chooseLight<M>(s, rng, info.p, lightWeight);
    const bool pureSpecular = pt.lobes != 0 && (pt.lobes & ~(uint32_t)LOBE_SPECULAR) == 0;
    if (light < 0 || pureSpecular || pt.lobes == TGHIP_LOBE_FORWARD) return status;
    status |= DIRECT_ITEM_ESTIMATE;
    const bool meshLight = s.objects[light].type == TGHIP_OBJ_MESH;
    const bool diracLight = s.objects[light].type == TGHIP_OBJ_POINT;
    if (diracLight) status |= DIRECT_ITEM_DIRAC;
    // lightSample (TraceBase.cpp:246-285)
    {
        f3 d; float dist, pdf;
        if (lightSampleDirect<M>(s, light, info.p, rng, d, dist, pdf)) {
            ev.wo = toLocal(pt.frame, d);
            ev.requested = LOBE_ALL_BUT_SPECULAR;
            if (isConsistent(s, pt, ev.wo, d)) {
                const f3 f = bsdfEval<M>(s, info.bsdf, ev);
                if (!isZero(f) && meshLight) {
                    // whether the ray reaches a mesh emitter, and with which emission, is known after the walk (TriangleMesh::intersect is a tree
                    // query): the round stage completes the term
                    putSegment(st, k*2u, info.p, 5e-4f, d, PT_INF, sideMedium(s, pt, medium, d), bounce, light, powerHeuristic(pdf, bsdfPdf<M>(s, info.bsdf, ev)), f, dist,
                               splat3(0.0f), pdf);
                    status |= DIRECT_ITEM_SEG0;
                } else if (!isZero(f)) {
                    RayD sr; sr.o = info.p; sr.d = d; sr.tmin = 5e-4f; sr.tmax = PT_INF;
                    LightHit lh;
                    // attenuatedEmission's own hit and distance test (TraceBase.cpp:155-162); a Dirac light is not intersected: the shadow ray ends
                    // at the sampled distance
                    bool reached;
                    if (diracLight) { lh.t = dist; lh.u = 0.0f; lh.v = 0.0f; lh.backSide = false; lh.n = splat3(0.0f); reached = true; }
                    else reached = lightIntersect<M>(s, light, sr, lh) && !(lh.t*(1.0f + 1e-3f) < dist);
                    if (reached) {
                        const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                        if (KEEP_BLACK || !isZero(e)) {
                            const float mis0 = diracLight ? 1.0f : powerHeuristic(pdf, bsdfPdf<M>(s, info.bsdf, ev));   // no MIS against a Dirac light (:281-282)
                            putSegment(st, k*2u, info.p, 5e-4f, d, lh.t, sideMedium(s, pt, medium, d), bounce, light, mis0, f, 0.0f, e, pdf);
                            status |= DIRECT_ITEM_SEG0;
                        }
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
            const f3 wog = toGlobal(pt.frame, ev.wo);
            if (isConsistent(s, pt, ev.wo, wog)) {
                if (meshLight) {
                    putSegment(st, k*2u + 1u, info.p, 5e-4f, wog, PT_INF, sideMedium(s, pt, medium, wog), bounce, light, 1.0f, ev.weight, ev.pdf, splat3(0.0f), 0.0f);   // directPdf needs the hit
                    status |= DIRECT_ITEM_SEG1;
                } else {
                    RayD sr; sr.o = info.p; sr.d = wog; sr.tmin = 5e-4f; sr.tmax = PT_INF;
                    LightHit lh;
                    if (lightIntersect<M>(s, light, sr, lh)) {
                        const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                        if (!isZero(e)) {
                            const float mis1 = powerHeuristic(ev.pdf, lightDirectPdf<M>(s, light, wog, info.p, lh));
                            putSegment(st, k*2u + 1u, info.p, 5e-4f, wog, lh.t, sideMedium(s, pt, medium, wog), bounce, light, mis1, ev.weight, 0.0f, e, 0.0f);
                            status |= DIRECT_ITEM_SEG1;
                        }
                    }
                }
            }
        }
    }
    st.origin[k] = mk4(info.p, 0.0f);
    return status;
}

// volumeEstimateDirect at volP in `medium` (mediumSample.p), the path having come along dirIn (parentRay.dir()): shadow rays start at tmin = 0, the
// medium is not re-selected; no transmittance is reported here, so a black side needs no shadow ray for either caller.  Otherwise as above.
PT_DEV uint32_t estimateDirectVolume(const DeviceScene &s, const DirectState &st, uint32_t k, Rng &rng, f3 volP, f3 dirIn, int medium, uint32_t bounce,
                                     int lightSlot, float &lightWeight)
{
    constexpr uint32_t M = DIRECT_MASK;
    const TgHipMedium &mm = s.media[medium];
    uint32_t status = 0u;
    const int light = lightSlot >= 0 ? s.lights[lightSlot] : chooseLight<M>(s, rng, volP, lightWeight);
    if (light < 0) return status;
    status |= DIRECT_ITEM_ESTIMATE;
    const bool meshLight = s.objects[light].type == TGHIP_OBJ_MESH;
    const bool diracLight = s.objects[light].type == TGHIP_OBJ_POINT;
    if (diracLight) status |= DIRECT_ITEM_DIRAC;
    {
        f3 d; float dist, pdf;
        if (lightSampleDirect<M>(s, light, volP, rng, d, dist, pdf)) {
            const float f = phaseEval(mm, dirIn, d);
            if (f != 0.0f && meshLight) {
                putSegment(st, k*2u, volP, 0.0f, d, PT_INF, medium, bounce, light, powerHeuristic(pdf, f), splat3(f), dist, splat3(0.0f), pdf);
                status |= DIRECT_ITEM_SEG0;
            } else if (f != 0.0f) {
                RayD sr; sr.o = volP; sr.d = d; sr.tmin = 0.0f; sr.tmax = PT_INF;   // parentRay.scatter(p, d, 0.0f)
                LightHit lh;
                bool reached;
                if (diracLight) { lh.t = dist; lh.u = 0.0f; lh.v = 0.0f; lh.backSide = false; lh.n = splat3(0.0f); reached = true; }
                else reached = lightIntersect<M>(s, light, sr, lh) && !(lh.t*(1.0f + 1e-3f) < dist);
                if (reached) {
                    const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                    if (!isZero(e)) {
                        putSegment(st, k*2u, volP, 0.0f, d, lh.t, medium, bounce, light, diracLight ? 1.0f : powerHeuristic(pdf, f), splat3(f), 0.0f, e, pdf);
                        status |= DIRECT_ITEM_SEG0;
                    }
                }
            }
        }
    }
    if (!diracLight) {
        f3 w; float ppdf;
        phaseSample<M>(mm, rng, dirIn, w, ppdf);
        if (meshLight) {
            putSegment(st, k*2u + 1u, volP, 0.0f, w, PT_INF, medium, bounce, light, 1.0f, splat3(1.0f), ppdf, splat3(0.0f), 0.0f);   // directPdf needs the hit
            status |= DIRECT_ITEM_SEG1;
        } else {
            RayD sr; sr.o = volP; sr.d = w; sr.tmin = 0.0f; sr.tmax = PT_INF;
            LightHit lh;
            if (lightIntersect<M>(s, light, sr, lh)) {
                const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                if (!isZero(e)) {
                    const float mis1 = powerHeuristic(ppdf, lightDirectPdf<M>(s, light, w, volP, lh));
                    putSegment(st, k*2u + 1u, volP, 0.0f, w, lh.t, medium, bounce, light, mis1, splat3(1.0f), 0.0f, e, 0.0f);   // phaseSample.weight = 1
                    status |= DIRECT_ITEM_SEG1;
                }
            }
        }
    }
    st.origin[k] = mk4(volP, 0.0f);
    return status;
}

#endif
