// The debug-case entry points of the extern "C" shim (include/tungsten_hip.h): the product's BSDF, light and medium code called on caller-supplied cases.
// Host code only: the kernels are behind the launchers of debug_units.h, the context is shim_context.h's.  (tghip_debug_libm: tungsten_hip.hip, with its kernels.)
#include "shim_context.h"
#include "debug_units.h"

// What tghip_debug_bsdf, _light and _medium do behind their argument checks: the n cases to the device, the results zeroed, one launch per variant
// in `variants` (debug_units.hip), the results back
template<typename Case, typename Result, typename Launch>
static int runDebugCases(tghip_ctx *ctx, const Case *cases, Result *results, size_t n, uint32_t variants, Launch launch)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    DeviceArray<Case> dc;
    DeviceArray<Result> dr;
    HIP_TRY(ctx, dc.once(n));
    hipError_t e = dr.once(n);
    if (e == hipSuccess) e = hipMemcpyAsync(dc.get(), cases, n*sizeof(Case), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(dr.get(), 0, n*sizeof(Result), ctx->stream);
    if (e == hipSuccess) e = launch(ctx->stream, ctx->scene, dc.get(), dr.get(), uint32_t(n), variants);
    if (e == hipSuccess) e = hipMemcpyAsync(results, dr.get(), n*sizeof(Result), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->error = hipGetErrorString(e); return TGHIP_E_HIP; }
    return TGHIP_OK;
}

extern "C" {

// the BSDF wrappers exactly as the shading kernels call them, per shading family (debug_units.hip)
int tghip_debug_bsdf(tghip_ctx *ctx, const TgHipBsdfCase *cases, TgHipBsdfResult *results, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (n == 0) return TGHIP_OK;
    if (!cases || !results || n > 0x3FFFFFFFu) { ctx->error = "invalid bsdf self-test arguments"; return TGHIP_E_INVALID; }
    if (!ctx->haveScene) { ctx->error = "bsdf self-test without an uploaded scene"; return TGHIP_E_INVALID; }
    uint32_t variants = 0;
    for (size_t i = 0; i < n; ++i) {
        if (cases[i].bsdf < 0 || uint32_t(cases[i].bsdf) >= ctx->scene.num_bsdfs) { ctx->error = "bsdf self-test: bsdf index outside the scene's table"; return TGHIP_E_INVALID; }
        if (cases[i].variant >= TGHIP_BSDF_VARIANT_COUNT) { ctx->error = "bsdf self-test: unknown variant"; return TGHIP_E_INVALID; }
        variants |= 1u << cases[i].variant;
    }
    return runDebugCases(ctx, cases, results, n, variants, debugBsdfLaunch);
}

int tghip_debug_bsdf_info(tghip_ctx *ctx, int variant, uint32_t *type_mask, uint32_t *forward, uint32_t *covered, uint32_t *variant_mask)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!ctx->haveScene) { ctx->error = "bsdf self-test without an uploaded scene"; return TGHIP_E_INVALID; }
    if (variant < 0 || variant >= TGHIP_BSDF_VARIANT_COUNT) { ctx->error = "bsdf self-test: unknown variant"; return TGHIP_E_INVALID; }
    if (variant_mask) *variant_mask = familyMask(uint32_t(variant));
    for (size_t i = 0; i < ctx->sc.bsdfTypes.size(); ++i) {
        if (type_mask) type_mask[i] = ctx->sc.bsdfTypes[i];
        if (forward) forward[i] = ctx->sc.bsdfForward[i];
        if (covered) covered[i] = familyCovers(uint32_t(variant), ctx->sc.bsdfTypes[i], ctx->sc.bsdfForward[i] != 0) ? 1u : 0u;
    }
    return TGHIP_OK;
}

// the light functions exactly as the shading kernels' next-event estimation calls them, per shading family (debug_units.hip)
int tghip_debug_light(tghip_ctx *ctx, const TgHipLightCase *cases, TgHipLightResult *results, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (n == 0) return TGHIP_OK;
    if (!cases || !results || n > 0x3FFFFFFFu) { ctx->error = "invalid light self-test arguments"; return TGHIP_E_INVALID; }
    if (!ctx->haveScene) { ctx->error = "light self-test without an uploaded scene"; return TGHIP_E_INVALID; }
    uint32_t variants = 0;
    for (size_t i = 0; i < n; ++i) {
        if (cases[i].light < 0 || uint32_t(cases[i].light) >= ctx->scene.num_lights) { ctx->error = "light self-test: light slot outside the scene's table"; return TGHIP_E_INVALID; }
        if (cases[i].variant >= TGHIP_BSDF_VARIANT_COUNT) { ctx->error = "light self-test: unknown variant"; return TGHIP_E_INVALID; }
        variants |= 1u << cases[i].variant;
    }
    return runDebugCases(ctx, cases, results, n, variants, debugLightLaunch);
}

int tghip_debug_light_info(tghip_ctx *ctx, int variant, uint32_t *needs, uint32_t *covered, uint32_t *variant_mask)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!ctx->haveScene) { ctx->error = "light self-test without an uploaded scene"; return TGHIP_E_INVALID; }
    if (variant < 0 || variant >= TGHIP_BSDF_VARIANT_COUNT) { ctx->error = "light self-test: unknown variant"; return TGHIP_E_INVALID; }
    const uint32_t mask = familyMask(uint32_t(variant));
    if (variant_mask) *variant_mask = mask;
    for (size_t i = 0; i < ctx->sc.lightNeeds.size(); ++i) {
        if (needs) needs[i] = ctx->sc.lightNeeds[i];
        if (covered) covered[i] = (ctx->sc.lightNeeds[i] & ~mask) == 0u ? 1u : 0u;
    }
    return TGHIP_OK;
}

// the medium functions exactly as k_shade and the shadow walks call them, for the two families that carry them (debug_units.hip); the refusals
// are csrc/host/SceneCheck.cpp's checkMediumCases, made before anything is launched
int tghip_debug_medium(tghip_ctx *ctx, const TgHipMediumCase *cases, TgHipMediumResult *results, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (n == 0) return TGHIP_OK;
    if (!ctx->haveScene) { ctx->error = "medium self-test without an uploaded scene"; return TGHIP_E_INVALID; }
    uint32_t variants = 0;
    const int rc = checkMediumCases(ctx->sc, cases, results, n, variants, ctx->error);
    if (rc != TGHIP_OK) return rc;
    return runDebugCases(ctx, cases, results, n, variants, debugMediumLaunch);
}

} // extern "C"
