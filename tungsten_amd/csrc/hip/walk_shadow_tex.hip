// Explicit instantiations of the closest-hit shadow walk of scenes that hold a `disk` or `blade` texture (pt_wavefront.h: k_trace_shadow<., true, ., ., BSDF_MASK_ALL>;
// which ones: pt_instances.h; the extern "C" shim in tungsten_hip.hip launches them): the walk's BSDF and texture code instantiated with BSDF_MASK_ALL, the
// one mask under which those textures are evaluated (pt_scene.h: HAS_PROCTEX).  A translation unit of its own: k_trace_shadow of every other scene stays
// what it was, and this one compiles next to the shim's under make -j.
#include "pt_wavefront.h"
#include "pt_instances.h"

#define PT_KERNEL PT_INSTANTIATE_KERNEL
PT_UNIT_walk_shadow_tex
