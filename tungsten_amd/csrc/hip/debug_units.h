// Launchers of debug_units.hip: the product's BSDF and light code called on caller-supplied cases (tghip_debug_bsdf, tghip_debug_light, tghip_debug_medium, include/tungsten_hip.h).  The shim in
// shim_debug.hip holds the context, checks the arguments and stages the host arrays; this enqueues the kernels on `stream` and returns.
#ifndef TGAMD_DEBUG_UNITS_H_
#define TGAMD_DEBUG_UNITS_H_

#include <hip/hip_runtime.h>
#include "pt_scene.h"

// (the mask of each instantiation: familyMask, csrc/host/SceneCheck.hpp)
// cases / results: n entries in device memory.  One launch per variant in `variants` (bit = 1 << TGHIP_BSDF_VARIANT_*); a launch answers the
// cases that select its variant and leaves the others alone.
hipError_t debugBsdfLaunch(hipStream_t stream, const DeviceScene &scene, const TgHipBsdfCase *cases, TgHipBsdfResult *results, uint32_t n,
                           uint32_t variants);
// The same for the light cases of tghip_debug_light.  Every case's light slot lies inside scene.lights (the shim checks; the kernel skips one that does not).
hipError_t debugLightLaunch(hipStream_t stream, const DeviceScene &scene, const TgHipLightCase *cases, TgHipLightResult *results, uint32_t n,
                            uint32_t variants);
// The same for the medium cases of tghip_debug_medium.  Every case's medium lies inside scene.media and every variant carries FEAT_MEDIA (the shim
// checks; the kernel skips an index that does not, and no kernel exists for a variant that does not).
hipError_t debugMediumLaunch(hipStream_t stream, const DeviceScene &scene, const TgHipMediumCase *cases, TgHipMediumResult *results, uint32_t n,
                             uint32_t variants);

#endif
