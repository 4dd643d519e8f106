// Explicit instantiation of the one k_shade variant that reads the scene's small tables from global memory (see pt_wavefront.h: GLOBAL_TABLES;
// pt_kernels.h: stageSceneTables; pt_instances.h): what shades every class of a scene whose tables do not fit the workgroups' LDS copy.
#include "pt_wavefront.h"
#include "pt_instances.h"

#define PT_KERNEL PT_INSTANTIATE_KERNEL
PT_UNIT_shade_global
