// Launcher of debug_units.hip: the product's BSDF code called on caller-supplied cases (tghip_debug_bsdf, include/tungsten_hip.h).  The shim in
// tungsten_hip.hip owns the context, checks the arguments and stages the host arrays; this enqueues the kernels on `stream` and returns.
#ifndef TGAMD_DEBUG_UNITS_H_
#define TGAMD_DEBUG_UNITS_H_

#include <hip/hip_runtime.h>
#include "pt_scene.h"

// The BSDF type / feature set M of family variant `variant` (TGHIP_BSDF_VARIANT_*) as debug_units.hip instantiates it: the shading family's
// mask without FEAT_QMC.  0 for an unknown variant.
uint32_t debugBsdfVariantMask(uint32_t variant);
// cases / results: n entries in device memory.  One launch per variant in `variants` (bit = 1 << TGHIP_BSDF_VARIANT_*); a launch answers the
// cases that select its variant and leaves the others alone.
hipError_t debugBsdfLaunch(hipStream_t stream, const DeviceScene &scene, const TgHipBsdfCase *cases, TgHipBsdfResult *results, uint32_t n,
                           uint32_t variants);

#endif
