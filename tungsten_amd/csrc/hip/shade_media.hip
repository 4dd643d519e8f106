// Explicit instantiation of the lean media shading variant (see pt_wavefront.h: MASK_MEDIA; pt_instances.h); the extern "C" shim in tungsten_hip.hip launches it.
#include "pt_wavefront.h"
#include "pt_instances.h"

#define PT_KERNEL PT_INSTANTIATE_KERNEL
PT_UNIT_shade_media
