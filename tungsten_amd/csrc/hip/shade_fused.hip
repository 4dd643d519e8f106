// Explicit instantiations of k_shade_fused (see pt_wavefront.h): one further class + class 0 in one launch, the pairs the shipped scenes need.
// The extern "C" shim in tungsten_hip.hip launches them.
#include "pt_wavefront.h"

template __global__ void k_shade_fused<MASK_COAT, MASK_SIMPLE, COAT_WAVES>(DeviceScene, PathState, PassParams, int);
template __global__ void k_shade_fused<(MASK_COAT | FEAT_QMC), (MASK_SIMPLE | FEAT_QMC), COAT_WAVES>(DeviceScene, PathState, PassParams, int);
template __global__ void k_shade_fused<MASK_GLASS, MASK_SIMPLE, 2>(DeviceScene, PathState, PassParams, int);
template __global__ void k_shade_fused<(MASK_GLASS | FEAT_QMC), (MASK_SIMPLE | FEAT_QMC), 2>(DeviceScene, PathState, PassParams, int);
template __global__ void k_shade_fused<MASK_PLASTIC, MASK_SIMPLE, 2>(DeviceScene, PathState, PassParams, int);
template __global__ void k_shade_fused<(MASK_PLASTIC | FEAT_QMC), (MASK_SIMPLE | FEAT_QMC), 2>(DeviceScene, PathState, PassParams, int);
