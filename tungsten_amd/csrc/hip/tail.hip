// Explicit instantiations of k_tail (see pt_wavefront.h; which ones: pt_instances.h); the extern "C" shim in tungsten_hip.hip launches them.
#include "pt_wavefront.h"
#include "pt_instances.h"

#define PT_KERNEL PT_INSTANTIATE_KERNEL
PT_UNIT_tail
