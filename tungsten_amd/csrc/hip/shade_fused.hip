// Explicit instantiations of k_shade_fused (see pt_wavefront.h; which ones: pt_instances.h): one further class + class 0 in one launch, the pairs the
// shipped scenes need.  The extern "C" shim in tungsten_hip.hip launches them.
#include "pt_wavefront.h"
#include "pt_instances.h"

#define PT_KERNEL PT_INSTANTIATE_KERNEL
PT_UNIT_shade_fused
