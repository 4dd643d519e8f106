// Explicit instantiations of the closest-hit shadow walk of scenes that hold a `disk` or `blade` texture (pt_wavefront.h: k_trace_shadow<., true, ., ., BSDF_MASK_ALL>; the
// extern "C" shim in tungsten_hip.hip launches them): the walk's BSDF and texture code instantiated with BSDF_MASK_ALL, the one mask under which
// those textures are evaluated (pt_scene.h: HAS_PROCTEX).  A translation unit of its own: k_trace_shadow of every other scene stays what it was,
// and this one compiles next to the shim's under make -j.
#include "pt_wavefront.h"

template __global__ void k_trace_shadow<false, true, false, 0, BSDF_MASK_ALL>(DeviceScene, PathState, PassParams, uint32_t);
template __global__ void k_trace_shadow<true, true, false, 0, BSDF_MASK_ALL>(DeviceScene, PathState, PassParams, uint32_t);
template __global__ void k_trace_shadow<false, true, true, 0, BSDF_MASK_ALL>(DeviceScene, PathState, PassParams, uint32_t);
template __global__ void k_trace_shadow<true, true, true, 0, BSDF_MASK_ALL>(DeviceScene, PathState, PassParams, uint32_t);
template __global__ void k_trace_shadow<false, true, false, 1, BSDF_MASK_ALL>(DeviceScene, PathState, PassParams, uint32_t);
template __global__ void k_trace_shadow<true, true, false, 1, BSDF_MASK_ALL>(DeviceScene, PathState, PassParams, uint32_t);
template __global__ void k_trace_shadow<false, true, false, 2, BSDF_MASK_ALL>(DeviceScene, PathState, PassParams, uint32_t);
template __global__ void k_trace_shadow<true, true, false, 2, BSDF_MASK_ALL>(DeviceScene, PathState, PassParams, uint32_t);
