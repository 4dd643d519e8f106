// Kernels of tghip_debug_bsdf (include/tungsten_hip.h): bsdfEval / bsdfPdf / bsdfSample -- the wrappers the shading kernels call (pt_scene.h) --
// on caller-supplied cases, one thread per case, instantiated once per shading family's mask (pt_wavefront.h).  Parity instrumentation
// (tests/test_gpu_bsdf_units.py compares every word with the oracle and the reference's recorded answers); no render launches these.
#include "pt_wavefront.h"
#include "debug_units.h"

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

uint32_t debugBsdfVariantMask(uint32_t variant)
{
    switch (variant) {
    case TGHIP_BSDF_VARIANT_LEAN:    return DEBUG_MASK(MASK_LEAN);
    case TGHIP_BSDF_VARIANT_SIMPLE:  return DEBUG_MASK(MASK_SIMPLE);
    case TGHIP_BSDF_VARIANT_COAT:    return DEBUG_MASK(MASK_COAT);
    case TGHIP_BSDF_VARIANT_GLASS:   return DEBUG_MASK(MASK_GLASS);
    case TGHIP_BSDF_VARIANT_PLASTIC: return DEBUG_MASK(MASK_PLASTIC);
    case TGHIP_BSDF_VARIANT_MEDIA:   return DEBUG_MASK(MASK_MEDIA);
    case TGHIP_BSDF_VARIANT_TAIL:    return DEBUG_MASK(MASK_TAIL);
    case TGHIP_BSDF_VARIANT_FULL:    return DEBUG_MASK(MASK_FULL);
    case TGHIP_BSDF_VARIANT_ALL:     return DEBUG_MASK(BSDF_MASK_ALL);
    default: return 0u;
    }
}

hipError_t debugBsdfLaunch(hipStream_t stream, const DeviceScene &scene, const TgHipBsdfCase *cases, TgHipBsdfResult *results, uint32_t n,
                           uint32_t variants)
{
    const dim3 grid((n + 63u)/64u), block(64);
#define DEBUG_LAUNCH(V, MASK) \
    if (variants & (1u << (V))) hipLaunchKernelGGL(k_debug_bsdf<DEBUG_MASK(MASK)>, grid, block, 0, stream, scene, cases, results, n, uint32_t(V))
    DEBUG_LAUNCH(TGHIP_BSDF_VARIANT_LEAN, MASK_LEAN);
    DEBUG_LAUNCH(TGHIP_BSDF_VARIANT_SIMPLE, MASK_SIMPLE);
    DEBUG_LAUNCH(TGHIP_BSDF_VARIANT_COAT, MASK_COAT);
    DEBUG_LAUNCH(TGHIP_BSDF_VARIANT_GLASS, MASK_GLASS);
    DEBUG_LAUNCH(TGHIP_BSDF_VARIANT_PLASTIC, MASK_PLASTIC);
    DEBUG_LAUNCH(TGHIP_BSDF_VARIANT_MEDIA, MASK_MEDIA);
    DEBUG_LAUNCH(TGHIP_BSDF_VARIANT_TAIL, MASK_TAIL);
    DEBUG_LAUNCH(TGHIP_BSDF_VARIANT_FULL, MASK_FULL);
    DEBUG_LAUNCH(TGHIP_BSDF_VARIANT_ALL, BSDF_MASK_ALL);
#undef DEBUG_LAUNCH
    return hipGetLastError();
}
