// One turn of PathTracer::traceSample's loop on caller-held paths (tghip_query_vertex): PathTracer.cpp:50-131 with TraceBase::handleSurface
// (TraceBase.cpp:516-568), handleVolume (:496-514), Medium::sampleDistance, the roulette, the NaN guards and handleInfiniteLights (:570-578), as a small
// wavefront on the context's stream.  Around the walks and the shadow rounds of its siblings, which it launches as they are -- tghip_query_surface's
// closest-hit walk over the live paths' rays, tghip_query_transmittance's walk and tghip_query_direct's k_direct_round over the shadow segments --
// three dense stages:
//   k_vertex_begin   one lane per path, once per call and part: TGHIP_VERTEX_START makes the state from the ray; the live paths are appended to the
//                    first turn's list, their rays written next to it for the walk.
//   k_vertex_front   one lane per live path behind the walk: the medium's distance sample, the transparency boolean, makeLocalScatterEvent, the
//                    direct estimate's draws with everything that needs no shadow walk (k_direct_setup's surface and volume bodies, restated here on
//                    the path's own stream, medium and bounce + 1: a second copy, so that k_direct_setup, k_direct_round and k_direct_finish keep
//                    their code), the emissive term, the BSDF or phase sample, the roulette draw and the next ray.  The direct term's factors and
//                    the emissive term stay apart; the rest of the new state is written.
//   k_vertex_back    one lane per live path behind the shadow rounds: emission += estimateDirect*throughput, then the emissive hit's term
//                    (TraceBase.cpp:537-543), the NaN guards on the emission after both, the status; 16-byte accesses.  The survivors are appended to
//                    the next turn's list with their rays: one atomicAdd per wave (ballot, popcount, rank).
// Separate launches for the reasons direct_query.hip gives: the front stage carries BSDF, texture, light and medium code at once and must not share
// registers with a walk, and a round's lanes are the segments still alive.
// One instantiation, under the all-features family's mask with FEAT_QMC cleared: the keyed PCG stream only, and an answer never depends on which
// shading family the scene's passes use.
#include "vertex_query.h"
#include "pt_wavefront.h"

#define VERTEX_MASK (BSDF_MASK_ALL & ~FEAT_QMC)

namespace {

// where a lane that is `alive` appends, counted in *count: one atomicAdd per wave.  Called by all 64 lanes.
PT_DEV uint32_t appendPlace(bool alive, uint32_t *count)
{
    const unsigned long long on = __ballot(alive);
    uint32_t base = 0;
    if (on != 0ull) {
        const uint32_t lane = laneId();
        if (lane == 0)
            base = atomicAdd(count, (uint32_t)__popcll(on));
        base = __shfl(base, 0) + (uint32_t)__popcll(on & ((1ull << lane) - 1ull));
    }
    return base;
}

PT_DEV void appendLive(bool alive, uint32_t g, uint32_t *list, uint32_t *count)
{
    const uint32_t at = appendPlace(alive, count);
    if (alive) list[at] = g;
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

// The far distance the walk of a segment [tmin, tmax) starts with (radiance_query.hip: queryWalkFar): 2^-10 further than a finite tmax, so that the
// front stage ends the segment exactly -- a hit counts when t < tmax -- whatever the walk's own arithmetic does within a few ulps of its far distance
PT_DEV float walkFar(float tmax) { return (tmax > 0.0f && tmax < PT_INF) ? tmax*1.0009765625f : tmax; }

PT_DEV void putWalkRay(float4 *walkRays, uint32_t at, float4 ro, float4 rd)
{
    rd.w = walkFar(rd.w);
    walkRays[(size_t)at*2u + 0u] = ro;
    walkRays[(size_t)at*2u + 1u] = rd;
}

}  // namespace

__global__ __launch_bounds__(VERTEX_QUERY_THREADS) void k_vertex_begin(VertexParams p, uint32_t numMedia, const float4 *rays, const int *media, float4 *paths,
                                                                      uint32_t *list, float4 *walkRays, uint32_t *count)
{
    const uint32_t l = blockIdx.x*VERTEX_QUERY_THREADS + threadIdx.x;
    bool alive = false;
    uint32_t i = 0;
    float4 ro = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rd = ro;
    if (l < p.paths) {
        i = p.path0 + l;
        float4 *P = paths + (size_t)i*VERTEX_PATH_VECTORS;
        if (p.start) {
            ro = rays[(size_t)i*2u + 0u]; rd = rays[(size_t)i*2u + 1u];
            int medium = p.medium;
            if (media) {
                medium = media[i];
                if (medium == TGHIP_MEDIUM_OF_CAMERA) medium = p.cameraMedium;
                if (medium < 0 || (uint32_t)medium >= numMedia) medium = -1;
            }
            const uint32_t key = p.firstIndex + i;
            Rng rng = rngStart(p.seed, key, p.sample);          // PathSampleGenerator::startPath
            for (uint32_t k = 0; k < p.firstNumber; ++k) (void)rngNextI(rng);
            // throughput 1, emission 0, bounce 0, wasSpecular, the medium's state reset (PathTracer.cpp:30-48)
            P[0] = ro;
            P[1] = rd;
            P[2] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
            P[3] = make_float4(0.0f, 0.0f, __uint_as_float(0u), __int_as_float(medium));
            P[4] = make_float4(__uint_as_float(0u), __uint_as_float(0u), __uint_as_float(TGHIP_PATH_WAS_SPECULAR), __int_as_float(-1));
            P[5] = make_float4(0.0f, __uint_as_float((uint32_t)rng.state), __uint_as_float((uint32_t)(rng.state >> 32)), __uint_as_float(key));
            P[6] = make_float4(__uint_as_float(p.firstNumber), __uint_as_float(0u), __uint_as_float(0u), __uint_as_float(0u));
            alive = true;
        } else {
            alive = __float_as_uint(P[3].z) == 0u;
            if (alive) { ro = P[0]; rd = P[1]; }
        }
    }
    const uint32_t at = appendPlace(alive, count);
    if (alive) {
        list[at] = i;
        putWalkRay(walkRays, at, ro, rd);
    }
}

__global__ __launch_bounds__(VERTEX_QUERY_THREADS) void k_vertex_front(DeviceScene s, float4 *paths, const uint32_t *list, uint32_t live, const float4 *hits,
                                                                      const int *inst, DirectState st, VertexState vs, uint32_t *segList, uint32_t *segCount)
{
    constexpr uint32_t M = VERTEX_MASK;
    const uint32_t j = blockIdx.x*VERTEX_QUERY_THREADS + threadIdx.x;
    bool q0 = false, q1 = false;
    if (j < live) {
        float4 *P = paths + (size_t)list[j]*VERTEX_PATH_VECTORS;
        const float4 c0 = P[0], c1 = P[1], c2 = P[2], c3 = P[3], c4 = P[4], c5 = P[5], c6 = P[6];
        RayD ray;
        ray.o = xyz(c0); ray.d = xyz(c1); ray.tmin = c0.w; ray.tmax = c1.w;
        f3 throughput = xyz(c2);
        f3 em = mk3(c2.w, c3.x, c3.y);
        int med = __float_as_int(c3.w);
        if (med < 0 || (uint32_t)med >= s.num_media) med = -1;   // (out of range: an unspecified answer, no read outside the table)
        uint32_t medBounce = __float_as_uint(c4.x);
        int bounce = (int)__float_as_uint(c4.y);
        bool wasSpecular = (__float_as_uint(c4.z) & TGHIP_PATH_WAS_SPECULAR) != 0u;
        Rng rng;
        rng.state = ((uint64_t)__float_as_uint(c5.z) << 32) | __float_as_uint(c5.y);
        rng.inc = ((uint64_t)__float_as_uint(c5.w) << 1) | 1u;
        rng.sobol = nullptr;
        rng.scramble = rng.index = rng.dim = 0u;
        const uint64_t stateBefore = rng.state;
        // the end of the segment [tmin, tmax): a hit counts when t < tmax
        float4 hit = hits[j];
        if (__float_as_int(hit.w) >= 0 && !(hit.x < ray.tmax)) hit = make_float4(ray.tmax, 0.0f, 0.0f, __int_as_float(-1));
        const bool didHit = __float_as_int(hit.w) >= 0;
        const int hitInst = inst ? inst[j] : -1;
        const int maxBounces = s.settings.max_bounces, minBounces = s.settings.min_bounces;
        const bool nee = s.settings.enable_light_sampling != 0;
        uint32_t end = 0u, status = 0u, add = 0u;
        float lightWeight = 1.0f;
        f3 directThroughput = splat3(0.0f), pending = splat3(0.0f);

        // the loop's end (PathTracer.cpp:108-126) for a path that goes on from `o` in direction `d`; the guard on the emission is the back stage's
        auto continuePath = [&](f3 o, f3 d, float tmin) {
            ray.o = o; ray.d = d; ray.tmin = tmin; ray.tmax = PT_INF;
            if (max3(throughput) == 0.0f) {
                end = TGHIP_PATH_END_ZERO_THROUGHPUT;
            } else {
                const float roulettePdf = fmaxf(fabsf(throughput.x), fmaxf(fabsf(throughput.y), fabsf(throughput.z)));
                bool killed = false;
                if (bounce > 2 && roulettePdf < 0.1f) {
                    if (rngNextBoolean(rng, roulettePdf))
                        throughput = throughput/roulettePdf;
                    else
                        killed = true;
                }
                if (killed) {
                    end = TGHIP_PATH_END_ROULETTE;
                } else if (isnan(sum3(ray.d) + sum3(ray.o))) {
                    end = TGHIP_PATH_END_NAN;
                } else {
                    bounce++;
                    if (bounce >= maxBounces) end = TGHIP_PATH_END_MAX_BOUNCES;
                }
            }
        };

        // participating media (PathTracer.cpp:48-61): a path inside a medium samples a distance along the segment first
        bool volumeEvent = false, mediumEnd = false;
        f3 volP = splat3(0.0f);
        // a ray with a non-finite component or a zero direction: an unspecified answer -- the path ends here, before any of its numbers becomes an index
        const bool badRay = !(isfinite(ray.o.x) && isfinite(ray.o.y) && isfinite(ray.o.z) && isfinite(ray.d.x) && isfinite(ray.d.y) && isfinite(ray.d.z) &&
                              isfinite(ray.tmin)) || isnan(ray.tmax) || (ray.d.x == 0.0f && ray.d.y == 0.0f && ray.d.z == 0.0f);
        if (!badRay && med >= 0) {
            f3 w; float t; bool exited;
            if (!mediumSampleDistance<M>(s, med, rng, ray.o, ray.d, didHit ? hit.x : ray.tmax, medBounce, w, t, exited)) {
                mediumEnd = true;                    // "return emission"
            } else {
                throughput = throughput*w;           // mediumSample.emission = 0
                volumeEvent = !exited;
                volP = ray.o + ray.d*t;
            }
        }

        if (badRay) {
            end = TGHIP_PATH_END_NAN;
        } else if (mediumEnd) {
            end = TGHIP_PATH_END_ABSORBED;
        } else if (volumeEvent) {
            // TraceBase::handleVolume (TraceBase.cpp:496-514) with volumeEstimateDirect / volumeSampleDirect / volumeLightSample / volumePhaseSample
            // (:323-381, 402-414, 470-481): k_direct_setup<true>'s body at mediumSample.p
            const TgHipMedium &mm = s.media[med];
            const bool volumeNee = s.settings.enable_volume_light_sampling != 0;
            wasSpecular = !volumeNee;
            if (volumeNee && bounce < maxBounces - 1) {
                const uint32_t segBounce = (uint32_t)(bounce + 1);
                const int light = chooseLight<M>(s, rng, volP, lightWeight);
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
                                putSegment(st, j*2u, volP, 0.0f, d, PT_INF, med, segBounce, light, powerHeuristic(pdf, f), splat3(f), dist, splat3(0.0f), pdf);
                                q0 = true;
                            } else if (f != 0.0f) {
                                RayD sr; sr.o = volP; sr.d = d; sr.tmin = 0.0f; sr.tmax = PT_INF;   // parentRay.scatter(p, d, 0.0f)
                                LightHit lh;
                                bool reached;
                                if (diracLight) { lh.t = dist; lh.u = 0.0f; lh.v = 0.0f; lh.backSide = false; lh.n = splat3(0.0f); reached = true; }
                                else reached = lightIntersect<M>(s, light, sr, lh) && !(lh.t*(1.0f + 1e-3f) < dist);
                                if (reached) {
                                    const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                                    if (!isZero(e)) {
                                        putSegment(st, j*2u, volP, 0.0f, d, lh.t, med, segBounce, light, diracLight ? 1.0f : powerHeuristic(pdf, f), splat3(f), 0.0f, e, pdf);
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
                            putSegment(st, j*2u + 1u, volP, 0.0f, w, PT_INF, med, segBounce, light, 1.0f, splat3(1.0f), ppdf, splat3(0.0f), 0.0f);   // directPdf needs the hit
                            q1 = true;
                        } else {
                            RayD sr; sr.o = volP; sr.d = w; sr.tmin = 0.0f; sr.tmax = PT_INF;
                            LightHit lh;
                            if (lightIntersect<M>(s, light, sr, lh)) {
                                const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                                if (!isZero(e)) {
                                    const float mis1 = powerHeuristic(ppdf, lightDirectPdf<M>(s, light, w, volP, lh));
                                    putSegment(st, j*2u + 1u, volP, 0.0f, w, lh.t, med, segBounce, light, mis1, splat3(1.0f), 0.0f, e, 0.0f);   // phaseSample.weight = 1
                                    q1 = true;
                                }
                            }
                        }
                    }
                    st.origin[j] = mk4(volP, 0.0f);
                    directThroughput = throughput;
                    if (q0 || q1) add |= VERTEX_ADD_PENDING;   // (the pending term of a volume vertex is zero)
                }
            }
            f3 w; float ppdf;
            phaseSample<M>(mm, rng, ray.d, w, ppdf);         // the continuation; throughput *= 1
            continuePath(volP, w, 0.0f);
        } else if (!didHit) {
            // the path escaped (the loop's condition failed, or PathTracer.cpp:59-60): the epilogue below
            end = TGHIP_PATH_END_ESCAPED;
        } else {
            Info info;
            intersectionInfo<M>(s, ray, hit, info, hitInst);
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
                return s.num_media ? selectMedium(s.objects[info.object], med, dot(dir, info.Ng) < 0.0f) : med;
            };

            f3 transparency = splat3(0.0f);
            if (lobes & TGHIP_LOBE_FORWARD) {
                ev.wo = -ev.wi; ev.requested = TGHIP_LOBE_FORWARD;
                transparency = bsdfEval<M>(s, info.bsdf, ev);
            }
            const float transparencyScalar = avg3(transparency);
            f3 wo;
            bool alive = true;
            if (rngNextBoolean(rng, transparencyScalar)) {
                wo = ray.d;
                throughput = throughput*(transparency/transparencyScalar);
            } else {
                // estimateDirect (TraceBase.cpp:483-494) as k_direct_setup<false> computes it, with bounce + 1, the path's medium and stream
                if (nee && bounce < maxBounces - 1) {
                    const uint32_t segBounce = (uint32_t)(bounce + 1);
                    const int light = chooseLight<M>(s, rng, info.p, lightWeight);
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
                                        // whether the ray reaches a mesh emitter, and with which emission, is known after the walk: the round completes the term
                                        putSegment(st, j*2u, info.p, 5e-4f, d, PT_INF, sideMedium(d), segBounce, light, powerHeuristic(pdf, bsdfPdf<M>(s, info.bsdf, ev)), f, dist,
                                                   splat3(0.0f), pdf);
                                        q0 = true;
                                    } else if (!isZero(f)) {
                                        RayD sr; sr.o = info.p; sr.d = d; sr.tmin = 5e-4f; sr.tmax = PT_INF;
                                        LightHit lh;
                                        // attenuatedEmission's own hit and distance test (TraceBase.cpp:155-162); a Dirac light's shadow ray ends at the sampled distance
                                        bool reached;
                                        if (diracLight) { lh.t = dist; lh.u = 0.0f; lh.v = 0.0f; lh.backSide = false; lh.n = splat3(0.0f); reached = true; }
                                        else reached = lightIntersect<M>(s, light, sr, lh) && !(lh.t*(1.0f + 1e-3f) < dist);
                                        if (reached) {
                                            const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                                            if (!isZero(e)) {          // (no visibility output here: a black side needs no shadow ray)
                                                const float mis0 = diracLight ? 1.0f : powerHeuristic(pdf, bsdfPdf<M>(s, info.bsdf, ev));   // no MIS against a Dirac light (:281-282)
                                                putSegment(st, j*2u, info.p, 5e-4f, d, lh.t, sideMedium(d), segBounce, light, mis0, f, 0.0f, e, pdf);
                                                q0 = true;
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
                                const f3 wog = toGlobal(frame, ev.wo);
                                if (isConsistent(ev.wo, wog)) {
                                    if (meshLight) {
                                        putSegment(st, j*2u + 1u, info.p, 5e-4f, wog, PT_INF, sideMedium(wog), segBounce, light, 1.0f, ev.weight, ev.pdf, splat3(0.0f), 0.0f);   // directPdf needs the hit
                                        q1 = true;
                                    } else {
                                        RayD sr; sr.o = info.p; sr.d = wog; sr.tmin = 5e-4f; sr.tmax = PT_INF;
                                        LightHit lh;
                                        if (lightIntersect<M>(s, light, sr, lh)) {
                                            const f3 e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
                                            if (!isZero(e)) {
                                                const float mis1 = powerHeuristic(ev.pdf, lightDirectPdf<M>(s, light, wog, info.p, lh));
                                                putSegment(st, j*2u + 1u, info.p, 5e-4f, wog, lh.t, sideMedium(wog), segBounce, light, mis1, ev.weight, 0.0f, e, 0.0f);
                                                q1 = true;
                                            }
                                        }
                                    }
                                }
                            }
                        }
                        st.origin[j] = mk4(info.p, 0.0f);
                        directThroughput = throughput;
                    }
                }
                // emission of the surface itself (TraceBase.cpp:540-543): added behind the direct term, by the back stage
                {
                    const TgHipObject &o = s.objects[info.object];
                    if (o.emission >= 0 && bounce >= minBounces && (!nee || wasSpecular || o.light < 0))
                        pending = lightEvalDirect<M>(s, info.object, info.u, info.v, info.backSide)*throughput;
                }
                add |= VERTEX_ADD_PENDING;

                // the continuation: bsdf.sample(event, adjoint = false) with all lobes (TraceBase.cpp:546-558)
                ev.requested = LOBE_ALL;
                ev.weight = splat3(1.0f); ev.pdf = 1.0f;
                if (!bsdfSample<M>(s, info.bsdf, ev)) {
                    alive = false;
                } else {
                    wo = toGlobal(frame, ev.wo);
                    if (!isConsistent(ev.wo, wo)) {
                        alive = false;
                    } else {
                        throughput = throughput*ev.weight;
                        wasSpecular = (ev.sampled & LOBE_SPECULAR) != 0;
                    }
                }
            }
            if (!alive) {
                end = TGHIP_PATH_END_ABSORBED;
            } else {
                const f3 hp = ray.o + ray.d*hit.x;           // ray.hitpoint()
                if (s.num_media)                             // TraceBase.cpp:561-563
                    med = selectMedium(s.objects[info.object], med, dot(wo, info.Ng) < 0.0f);
                medBounce = 0;                               // state.reset()
                continuePath(hp, wo, 5e-4f);
            }
        }

        // The epilogue (PathTracer.cpp:128-129) of a path that left the loop -- escaped, or by `break` with no throughput left (:108-109), then along its
        // NEW ray and with the bounce it had --: TraceBase::handleInfiniteLights (TraceBase.cpp:570-578); the last infinite light wins.  The reference adds
        // this term behind the turn's direct and emissive terms, which the back stage adds; here it comes first.  Only a path without throughput has both,
        // and its term is a zero or a NaN: the sum has the same bits either way.  The guard behind it (:130-131) is the back stage's.
        if ((end == TGHIP_PATH_END_ESCAPED || end == TGHIP_PATH_END_ZERO_THROUGHPUT) && bounce >= minBounces && bounce < maxBounces && s.num_infinite_lights > 0) {
            int objIdx = -1;                             // intersectInfinites (TraceableScene.hpp:194-209): every one is asked, the last hit stays
            for (uint32_t li = 0; li < s.num_infinite_lights; ++li) {
                const TgHipObject &c = s.objects[s.infinite_lights[li]];
                if (c.type != TGHIP_OBJ_INFINITE_SPHERE_CAP || dot(ray.d, ld3(c.normal)) >= c.scale[0])
                    objIdx = s.infinite_lights[li];
            }
            if (objIdx >= 0) {
                const TgHipObject &o = s.objects[objIdx];
                if (!nee || wasSpecular || !(o.flags & TGHIP_OBJF_SAMPLE)) {
                    float u = 0.0f, v = 0.0f, sinTheta;
                    if (o.type == TGHIP_OBJ_INFINITE_SPHERE) infDirectionToUV(o, ray.d, u, v, sinTheta);
                    em = em + throughput*textureEval<M>(s, o.emission, u, v);
                }
            }
        }

        // The numbers this turn took from the stream: the steps from the state it began with (every draw is one step of the generator).  Counted here
        // and not where they are drawn: rngNextI and its kin (pt_math.h) are the helpers of every kernel of the library, and a counter in Rng would
        // change the code of all of them; a path draws a few dozen numbers a turn (at most a few hundred in a medium), one 64-bit multiply-add each
        uint32_t drawn = __float_as_uint(c6.x);
        for (uint64_t state = stateBefore; state != rng.state && drawn != 0xFFFFFFFFu; ++drawn)
            state = state*6364136223846793005ULL + rng.inc;

        P[0] = mk4(ray.o, ray.tmin);
        P[1] = mk4(ray.d, ray.tmax);
        P[2] = mk4(throughput, em.x);
        P[3] = make_float4(em.y, em.z, __uint_as_float(end), __int_as_float(med));
        P[4] = make_float4(__uint_as_float(medBounce), __uint_as_float((uint32_t)bounce), __uint_as_float(wasSpecular ? TGHIP_PATH_WAS_SPECULAR : 0u), hit.w);
        P[5] = make_float4(didHit ? hit.x : 0.0f, __uint_as_float((uint32_t)rng.state), __uint_as_float((uint32_t)(rng.state >> 32)), c5.w);
        P[6] = make_float4(__uint_as_float(drawn), c6.y, c6.z, c6.w);
        st.status[j] = status | (q0 ? DIRECT_ITEM_SEG0 : 0u) | (q1 ? DIRECT_ITEM_SEG1 : 0u);
        st.weight[j] = lightWeight;
        vs.w[j] = mk4(directThroughput, lightWeight);
        vs.p[j] = mk4(pending, __uint_as_float(add));
    }
    appendLive(q0, j*2u, segList, segCount);
    appendLive(q1, j*2u + 1u, segList, segCount);
}

// sampleDirect: result(0) += lightSample, += bsdfSample unless the light is a Dirac one (TraceBase.cpp:390-399), times chooseLight's weight (:493) as
// k_direct_finish adds a sample; emission += that times the throughput, then the emissive hit's term (:537-543); the guards on the emission behind both
// (PathTracer.cpp:119-122, 130-131).
__global__ __launch_bounds__(VERTEX_QUERY_THREADS) void k_vertex_back(float4 *paths, const uint32_t *list, uint32_t live, DirectState st, VertexState vs,
                                                                     uint32_t *next, float4 *walkRays, uint32_t *nextCount)
{
    const uint32_t j = blockIdx.x*VERTEX_QUERY_THREADS + threadIdx.x;
    bool alive = false;
    uint32_t i = 0;
    float4 *P = nullptr;
    if (j < live) {
        i = list[j];
        P = paths + (size_t)i*VERTEX_PATH_VECTORS;
        float4 c2 = P[2], c3 = P[3];
        f3 em = mk3(c2.w, c3.x, c3.y);
        uint32_t end = __float_as_uint(c3.z);
        const uint32_t status = st.status[j];
        const float4 p = vs.p[j];
        if (status & (DIRECT_ITEM_SEG0 | DIRECT_ITEM_SEG1)) {
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const float4 r0 = (status & DIRECT_ITEM_SEG0) ? st.res[j*2u] : zero;
            f3 result = splat3(0.0f) + xyz(r0);
            if (!(status & DIRECT_ITEM_DIRAC)) {
                const float4 r1 = (status & DIRECT_ITEM_SEG1) ? st.res[j*2u + 1u] : zero;
                result = result + xyz(r1);
            }
            const float4 w = vs.w[j];
            em = em + (result*w.w)*xyz(w);               // emission += estimateDirect(...)*throughput
        }
        if (__float_as_uint(p.w) & VERTEX_ADD_PENDING)
            em = em + xyz(p);
        // the loop's guard where the path goes on or ends at its bounce limit, the one behind the loop where it left it
        if (end == 0u || end == TGHIP_PATH_END_MAX_BOUNCES || end == TGHIP_PATH_END_ESCAPED || end == TGHIP_PATH_END_ZERO_THROUGHPUT) {
            if (isnan(sum3(xyz(c2)) + sum3(em))) end = TGHIP_PATH_END_NAN;
        }
        if (end == TGHIP_PATH_END_NAN) em = splat3(0.0f);    // (the reference returns its NaN colours: the sample is dropped)
        c2.w = em.x; c3.x = em.y; c3.y = em.z; c3.z = __uint_as_float(end);
        P[2] = c2;
        P[3] = c3;
        alive = end == 0u;
    }
    const uint32_t at = appendPlace(alive, nextCount);
    if (alive) {
        next[at] = i;
        putWalkRay(walkRays, at, P[0], P[1]);
    }
}

hipError_t vertexQueryLaunchBegin(hipStream_t stream, const VertexParams &p, uint32_t numMedia, const float4 *rays, const int *media, float4 *paths,
                                  uint32_t *list, float4 *walkRays, uint32_t *count)
{
    const dim3 grid((p.paths + VERTEX_QUERY_THREADS - 1u)/VERTEX_QUERY_THREADS), block(VERTEX_QUERY_THREADS);
    hipLaunchKernelGGL(k_vertex_begin, grid, block, 0, stream, p, numMedia, rays, media, paths, list, walkRays, count);
    return hipGetLastError();
}

hipError_t vertexQueryLaunchFront(hipStream_t stream, const DeviceScene &scene, float4 *paths, const uint32_t *list, uint32_t live, const float4 *hits,
                                  const int *inst, const DirectState &st, const VertexState &vs, uint32_t *segList, uint32_t *segCount)
{
    const dim3 grid((live + VERTEX_QUERY_THREADS - 1u)/VERTEX_QUERY_THREADS), block(VERTEX_QUERY_THREADS);
    hipLaunchKernelGGL(k_vertex_front, grid, block, 0, stream, scene, paths, list, live, hits, inst, st, vs, segList, segCount);
    return hipGetLastError();
}

hipError_t vertexQueryLaunchBack(hipStream_t stream, float4 *paths, const uint32_t *list, uint32_t live, const DirectState &st, const VertexState &vs,
                                 uint32_t *next, float4 *walkRays, uint32_t *nextCount)
{
    const dim3 grid((live + VERTEX_QUERY_THREADS - 1u)/VERTEX_QUERY_THREADS), block(VERTEX_QUERY_THREADS);
    hipLaunchKernelGGL(k_vertex_back, grid, block, 0, stream, paths, list, live, st, vs, next, walkRays, nextCount);
    return hipGetLastError();
}
