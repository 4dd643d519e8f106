// One turn of PathTracer::traceSample's loop on caller-held paths (tghip_query_vertex): PathTracer.cpp:50-131 with TraceBase::handleSurface
// (TraceBase.cpp:516-568), handleVolume (:496-514), Medium::sampleDistance, the roulette, the NaN guards and handleInfiniteLights (:570-578), as a small
// wavefront on the context's stream.  Around the walks and the shadow rounds of its siblings, which it launches as they are -- tghip_query_surface's
// closest-hit walk over the live paths' rays, tghip_query_transmittance's walk and tghip_query_direct's k_direct_round over the shadow segments --
// three dense stages:
//   k_vertex_begin   one lane per path, once per call and part: TGHIP_VERTEX_START makes the state from the ray; the live paths are appended to the
//                    first turn's list, their rays written next to it for the walk.
//   k_vertex_front   one lane per live path behind the walk: the medium's distance sample, the transparency boolean, makeLocalScatterEvent, the
//                    direct estimate's draws with everything that needs no shadow walk (direct_estimate.h's surface and volume bodies, the ones
//                    k_direct_setup calls, here on the path's own stream, medium and bounce + 1 and without the segment of a black light sample),
//                    the emissive term, the BSDF or phase sample, the roulette draw and the next ray.  The direct term's factors and the emissive
//                    term stay apart; the rest of the new state is written.
//   k_vertex_back    one lane per live path behind the shadow rounds: emission += estimateDirect*throughput, then the emissive hit's term
//                    (TraceBase.cpp:537-543), the NaN guards on the emission after both, the status; 16-byte accesses.  The survivors are appended to
//                    the next turn's list with their rays: one atomicAdd per wave (ballot, popcount, rank).
// Separate launches for the reasons direct_query.hip gives: the front stage carries BSDF, texture, light and medium code at once and must not share
// registers with a walk, and a round's lanes are the segments still alive.
// One instantiation, under direct_estimate.h's DIRECT_MASK (the all-features family's mask with FEAT_QMC cleared): the keyed PCG stream only, and an
// answer never depends on which shading family the scene's passes use.
#include "vertex_query.h"
#include "direct_estimate.h"

namespace {

// (the walk looks a little further than the segment reaches, query_walk.h: the front stage ends the segment exactly)
PT_DEV void putWalkRay(float4 *walkRays, uint32_t at, float4 ro, float4 rd)
{
    rd.w = queryWalkFar(rd.w);
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
            const int medium = rayStartMedium(p, media, numMedia, i);
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
    appendAt(alive, count, [&](uint32_t at) {
        list[at] = i;
        putWalkRay(walkRays, at, ro, rd);
    });
}

__global__ __launch_bounds__(VERTEX_QUERY_THREADS) void k_vertex_front(DeviceScene s, float4 *paths, const uint32_t *list, uint32_t live, const float4 *hits,
                                                                      const int *inst, DirectState st, VertexState vs, uint32_t *segList, uint32_t *segCount)
{
    constexpr uint32_t M = DIRECT_MASK;
    const uint32_t j = blockIdx.x*VERTEX_QUERY_THREADS + threadIdx.x;
    uint32_t status = 0u;
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
        uint32_t end = 0u, add = 0u;
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
            // (:323-381, 402-414, 470-481): direct_estimate.h's volume body at mediumSample.p
            const TgHipMedium &mm = s.media[med];
            const bool volumeNee = s.settings.enable_volume_light_sampling != 0;
            wasSpecular = !volumeNee;
            if (volumeNee && bounce < maxBounces - 1) {
                status = estimateDirectVolume(s, st, j, rng, volP, ray.d, med, (uint32_t)(bounce + 1), -1, lightWeight);
                if (status & DIRECT_ITEM_ESTIMATE) directThroughput = throughput;
                if (status & (DIRECT_ITEM_SEG0 | DIRECT_ITEM_SEG1)) add |= VERTEX_ADD_PENDING;   // (the pending term of a volume vertex is zero)
            }
            f3 w; float ppdf;
            phaseSample<M>(mm, rng, ray.d, w, ppdf);         // the continuation; throughput *= 1
            continuePath(volP, w, 0.0f);
        } else if (!didHit) {
            // the path escaped (the loop's condition failed, or PathTracer.cpp:59-60): the epilogue below
            end = TGHIP_PATH_END_ESCAPED;
        } else {
            ScatterPoint pt;
            Event ev;
            makeScatterPoint(s, ray, hit, hitInst, rng, pt, ev);
            const Info &info = pt.info;
            const Frame &frame = pt.frame;

            f3 transparency = splat3(0.0f);
            if (pt.lobes & TGHIP_LOBE_FORWARD) {
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
                // estimateDirect (TraceBase.cpp:483-494): direct_estimate.h's surface body with bounce + 1, the path's medium and stream; no visibility
                // output here, so no segment for a light sample without emission
                if (nee && bounce < maxBounces - 1) {
                    status = estimateDirectSurface<false>(s, st, j, rng, pt, ev, med, (uint32_t)(bounce + 1), -1, lightWeight);
                    if (status & DIRECT_ITEM_ESTIMATE) directThroughput = throughput;
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
                    if (!isConsistent(s, pt, ev.wo, wo)) {
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
                med = sideMedium(s, pt, med, wo);            // TraceBase.cpp:561-563
                medBounce = 0;                              // state.reset()
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
        st.status[j] = status;
        st.weight[j] = lightWeight;
        vs.w[j] = mk4(directThroughput, lightWeight);
        vs.p[j] = mk4(pending, __uint_as_float(add));
    }
    appendLive((status & DIRECT_ITEM_SEG0) != 0u, j*2u, segList, segCount);
    appendLive((status & DIRECT_ITEM_SEG1) != 0u, j*2u + 1u, segList, segCount);
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
            float shadowT;                               // (no visibility output here)
            const f3 result = directItemResult(st, j, status, shadowT);
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
    appendAt(alive, nextCount, [&](uint32_t at) {
        next[at] = i;
        putWalkRay(walkRays, at, P[0], P[1]);
    });
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
