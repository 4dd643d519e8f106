// Kernels of tghip_debug_bsdf (include/tungsten_hip.h): bsdfEval / bsdfPdf / bsdfSample -- the wrappers the shading kernels call (pt_scene.h) --
// on caller-supplied cases, one thread per case, instantiated once per shading family's mask (pt_wavefront.h).  Parity instrumentation
// (tests/test_gpu_bsdf_units.py compares every word with the oracle and the reference's recorded answers); no render launches these.
// Likewise tghip_debug_light: chooseLight / lightSampleDirect / lightApproximateRadiance / lightIntersect / lightEvalDirect / lightDirectPdf in the
// order and with the arguments of k_shade's next-event estimation (tests/test_gpu_light_units.py).
// Likewise tghip_debug_medium: mediumSampleDistance / mediumTransmittance / phaseEval / phaseSample, for the two families that carry the media code
// (tests/test_gpu_medium_units.py).
#include "pt_wavefront.h"
#include "debug_units.h"

// One instantiation per family of PT_FAMILY_VARIANTS (pt_variants.h), the masks familyMask reports (csrc/host/SceneCheck.cpp).
// Every instantiation has FEAT_QMC cleared: the Sobol' twin of the sampler reads generator matrices a debug call does not have.
#define DEBUG_MASK(m) ((m) & ~FEAT_QMC)

template<uint32_t M>
__global__ void __launch_bounds__(64) k_debug_bsdf(DeviceScene s, const TgHipBsdfCase *cases, TgHipBsdfResult *results, uint32_t n, uint32_t variant)
{
    static_assert((M & FEAT_QMC) == 0, "the debug kernels draw from the counter-based stream only");
    const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= n) return;
    const TgHipBsdfCase c = cases[i];
    if (c.variant != variant) return;
    Rng rng = rngStart(c.seed, c.stream, 0u);
    Event e;
    e.wi = mk3(c.wi[0], c.wi[1], c.wi[2]);
    e.wo = mk3(c.wo[0], c.wo[1], c.wo[2]);
    e.weight = splat3(1.0f);
    e.pdf = 1.0f;
    e.requested = c.requested;
    e.sampled = 0u;
    e.u = c.uv[0]; e.v = c.uv[1];
    e.rng = &rng;
    const f3 f = bsdfEval<M>(s, c.bsdf, e);
    const float pdf = bsdfPdf<M>(s, c.bsdf, e);
    Event q = e;
    q.wo = splat3(0.0f);
    const bool ok = bsdfSample<M>(s, c.bsdf, q);
    TgHipBsdfResult r;
    r.f[0] = f.x; r.f[1] = f.y; r.f[2] = f.z;
    r.pdf = pdf;
    r.sample_ok = ok ? 1u : 0u;
    r.sample_wo[0] = q.wo.x; r.sample_wo[1] = q.wo.y; r.sample_wo[2] = q.wo.z;
    r.sample_weight[0] = q.weight.x; r.sample_weight[1] = q.weight.y; r.sample_weight[2] = q.weight.z;
    r.sample_pdf = q.pdf;
    r.sampled = q.sampled;
    r.next = rngNext1D(rng);          // the stream's next number: how many the sample consumed, without a counter in Rng
    r.reserved[0] = r.reserved[1] = 0u;
    results[i] = r;
}

// One light case (TgHipLightCase): the calls of k_shade's estimateDirect block (pt_wavefront.h), each on the unstaged scene in global memory.
template<uint32_t M>
__global__ void __launch_bounds__(64) k_debug_light(DeviceScene s, const TgHipLightCase *cases, TgHipLightResult *results, uint32_t n, uint32_t variant)
{
    static_assert((M & FEAT_QMC) == 0, "the debug kernels draw from the counter-based stream only");
    const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= n) return;
    const TgHipLightCase c = cases[i];
    if (c.variant != variant || c.light < 0 || (uint32_t)c.light >= s.num_lights) return;     // (the shim has refused such a slot already)
    const f3 p = mk3(c.p[0], c.p[1], c.p[2]), w = mk3(c.w[0], c.w[1], c.w[2]);
    const int light = s.lights[c.light];
    TgHipLightResult r;
    // TraceBase::chooseLight on the case's first stream
    Rng rng = rngStart(c.seed, c.stream, 0u);
    float lightWeight = 1.0f;
    r.chosen = chooseLight<M>(s, rng, p, lightWeight);
    r.choose_weight = lightWeight;
    r.choose_next = rngNext1D(rng);
    // lightSample's sampleDirect on the second
    Rng rng2 = rngStart(c.seed, c.stream, 1u);
    f3 d = splat3(0.0f);
    float dist = 0.0f, pdf = 0.0f;
    const bool sampled = lightSampleDirect<M>(s, light, p, rng2, d, dist, pdf);
    r.sample_ok = sampled ? 1u : 0u;
    r.d[0] = d.x; r.d[1] = d.y; r.d[2] = d.z;
    r.dist = dist; r.pdf = pdf;
    r.sample_next = rngNext1D(rng2);
    r.approx = lightApproximateRadiance<M>(s, light, p);
    // bsdfSample's leg: the analytic hit, the emission and the light's pdf for a direction the BSDF chose
    const bool meshLight = (M & FEAT_MESHLIGHT) && s.objects[light].type == TGHIP_OBJ_MESH;
    const bool diracLight = (M & FEAT_SOLIDS) && s.objects[light].type == TGHIP_OBJ_POINT;
    LightHit lh;
    lh.t = 0.0f; lh.u = 0.0f; lh.v = 0.0f; lh.backSide = false; lh.n = splat3(0.0f); lh.sinTheta = 0.0f;
    bool hit = false;
    f3 e = splat3(0.0f);
    float lightPdf = 0.0f;
    if (diracLight) {
        // never intersected: the shadow ray ends at the sampled distance, with this hit record
        lh.t = dist; lh.u = 0.0f; lh.v = 0.0f; lh.backSide = false; lh.n = splat3(0.0f);
        lightPdf = lightDirectPdf<M>(s, light, w, p, lh);
    } else if (!meshLight) {
        RayD sr; sr.o = p; sr.d = w; sr.tmin = 5e-4f; sr.tmax = PT_INF;
        hit = lightIntersect<M>(s, light, sr, lh);
        if (hit) {
            e = lightEvalDirect<M>(s, light, lh.u, lh.v, lh.backSide);
            lightPdf = lightDirectPdf<M>(s, light, w, p, lh);
        }
    }
    r.hit = hit ? 1u : 0u;
    r.t = lh.t; r.u = lh.u; r.v = lh.v;
    r.back_side = lh.backSide ? 1u : 0u;
    r.emission[0] = e.x; r.emission[1] = e.y; r.emission[2] = e.z;
    r.direct_pdf = lightPdf;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = 0u;
    results[i] = r;
}

// One medium case (TgHipMediumCase): the calls k_shade makes on a path inside a medium and the shadow walks make segment by segment (pt_wavefront.h),
// each on the unstaged scene in global memory.
template<uint32_t M>
__global__ void __launch_bounds__(64) k_debug_medium(DeviceScene s, const TgHipMediumCase *cases, TgHipMediumResult *results, uint32_t n, uint32_t variant)
{
    static_assert((M & FEAT_QMC) == 0, "the debug kernels draw from the counter-based stream only");
    static_assert((M & FEAT_MEDIA) != 0, "the medium code is compiled into the FEAT_MEDIA families only");
    const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= n) return;
    const TgHipMediumCase c = cases[i];
    if (c.variant != variant || c.medium < 0 || (uint32_t)c.medium >= s.num_media) return;     // (the shim has refused such an index already)
    const f3 p = mk3(c.p[0], c.p[1], c.p[2]), d = mk3(c.d[0], c.d[1], c.d[2]), wo = mk3(c.wo[0], c.wo[1], c.wo[2]);
    const TgHipMedium &mm = s.media[c.medium];
    TgHipMediumResult r;
    // Medium::sampleDistance on the case's first stream
    Rng rng = rngStart(c.seed, c.stream, 0u);
    uint32_t medBounce = c.state_bounce;
    f3 weight = splat3(0.0f);
    float t = 0.0f;
    bool exited = false;
    const bool ok = mediumSampleDistance<M>(s, c.medium, rng, p, d, c.max_t, medBounce, weight, t, exited);
    r.ok = ok ? 1u : 0u;
    r.t = t;
    r.weight[0] = weight.x; r.weight[1] = weight.y; r.weight[2] = weight.z;
    r.exited = exited ? 1u : 0u;
    r.bounce_after = medBounce;
    r.dist_next = rngNext1D(rng);
    // Medium::transmittance for the four (startOnSurface, endOnSurface) pairs
    for (int k = 0; k < 4; ++k) {
        const f3 tr = mediumTransmittance(s, c.medium, p, d, c.max_t, k < 2, (k & 1) == 0);
        r.tr[k][0] = tr.x; r.tr[k][1] = tr.y; r.tr[k][2] = tr.z;
    }
    // the phase function: eval for the given pair, sample on the second stream
    r.phase_f = phaseEval(mm, d, wo);
    Rng rng2 = rngStart(c.seed, c.stream, 1u);
    f3 w = splat3(0.0f);
    float pdf = 0.0f;
    phaseSample<M>(mm, rng2, d, w, pdf);
    r.w[0] = w.x; r.w[1] = w.y; r.w[2] = w.z;
    r.phase_pdf = pdf;
    r.phase_next = rngNext1D(rng2);
    r.reserved[0] = r.reserved[1] = 0u;
    results[i] = r;
}

hipError_t debugBsdfLaunch(hipStream_t stream, const DeviceScene &scene, const TgHipBsdfCase *cases, TgHipBsdfResult *results, uint32_t n,
                           uint32_t variants)
{
    const dim3 grid((n + 63u)/64u), block(64);
#define DEBUG_LAUNCH(V, MASK) \
    if (variants & (1u << (V))) hipLaunchKernelGGL(k_debug_bsdf<DEBUG_MASK(MASK)>, grid, block, 0, stream, scene, cases, results, n, uint32_t(V));
    PT_FAMILY_VARIANTS(DEBUG_LAUNCH)
#undef DEBUG_LAUNCH
    return hipGetLastError();
}

hipError_t debugLightLaunch(hipStream_t stream, const DeviceScene &scene, const TgHipLightCase *cases, TgHipLightResult *results, uint32_t n,
                            uint32_t variants)
{
    const dim3 grid((n + 63u)/64u), block(64);
#define DEBUG_LAUNCH(V, MASK) \
    if (variants & (1u << (V))) hipLaunchKernelGGL(k_debug_light<DEBUG_MASK(MASK)>, grid, block, 0, stream, scene, cases, results, n, uint32_t(V));
    PT_FAMILY_VARIANTS(DEBUG_LAUNCH)
#undef DEBUG_LAUNCH
    return hipGetLastError();
}

// (only the families whose mask carries FEAT_MEDIA have the medium code: the others are not instantiated, and the shim refuses their cases)
template<uint32_t M>
static void debugMediumLaunchOne(hipStream_t stream, const DeviceScene &scene, const TgHipMediumCase *cases, TgHipMediumResult *results, uint32_t n, uint32_t variant)
{
    if constexpr ((M & FEAT_MEDIA) != 0u)
        hipLaunchKernelGGL(k_debug_medium<M>, dim3((n + 63u)/64u), dim3(64), 0, stream, scene, cases, results, n, variant);
}

hipError_t debugMediumLaunch(hipStream_t stream, const DeviceScene &scene, const TgHipMediumCase *cases, TgHipMediumResult *results, uint32_t n,
                             uint32_t variants)
{
#define DEBUG_LAUNCH(V, MASK) \
    if (variants & (1u << (V))) debugMediumLaunchOne<DEBUG_MASK(MASK)>(stream, scene, cases, results, n, uint32_t(V));
    PT_FAMILY_VARIANTS(DEBUG_LAUNCH)
#undef DEBUG_LAUNCH
    return hipGetLastError();
}
