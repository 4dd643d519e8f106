// Launchers of develop.hip: the frame developed on the device (tghip_develop, include/tungsten_hip.h).  The shim in shim_images.hip holds the
// context, checks the arguments and stages host outputs; these enqueue the kernels on `stream` and return.
#ifndef TGAMD_DEVELOP_H_
#define TGAMD_DEVELOP_H_

#include <hip/hip_runtime.h>
#include "../../../include/tungsten_hip.h"

// sum / count / hdr 16-byte aligned, ldr 4-byte aligned; hdr and ldr may each be NULL
hipError_t developLaunchFrame(hipStream_t stream, const float *sum, const uint32_t *count, size_t npixels, uint32_t tonemap, float *hdr, uint8_t *ldr);
// depthMax: one device word of scratch (the depth output's rescale, found by a reduction launch of its own)
hipError_t developLaunchAux(hipStream_t stream, const TgHipAuxPixel *aux, size_t npixels, uint32_t output, uint32_t part, float *hdr, uint8_t *ldr,
                            uint32_t *depthMax);

#endif
