// Explicit instantiations of the single-level shadow walk (pt_wavefront.h: k_trace_shadow_fast; which ones: pt_instances.h); the extern "C" shim in
// tungsten_hip.hip launches them.  A translation unit of its own so that it compiles next to the shim's (the longest one) under make -j; it was also
// where building without SLP vectorisation was found to pay (119 -> 98 VGPRs, 724 -> 634 us per launch: Makefile, profiles/r5_ab_no_slp.txt) before
// the whole library was built that way.
#include "pt_wavefront.h"
#include "pt_instances.h"

#define PT_KERNEL PT_INSTANTIATE_KERNEL
PT_UNIT_walk_shadow
