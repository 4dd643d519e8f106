// Launcher of denoise.hip: the denoiser's NL-means filter on the device (tghip_nlmeans, include/tungsten_hip.h).  The shim in shim_images.hip holds
// the context, checks the arguments, develops an aux source's planes and stages host arrays; this enqueues the kernel on `stream` and returns.
#ifndef TGAMD_DENOISE_H_
#define TGAMD_DENOISE_H_

#include <hip/hip_runtime.h>
#include "../../../include/tungsten_hip.h"

constexpr uint32_t NLMEANS_MAX_F = 8, NLMEANS_MAX_R = 16, NLMEANS_MAX_BATCH = 16;

// image / guide / variance / out: height x width pixels of `channels` (1..4) interleaved floats in device memory, 16-byte aligned when channels == 4.
// batch: the offsets whose distances are box-filtered at once (0: the measured choice, one; denoise.hip).  hipErrorInvalidValue when
// even one offset's planes do not fit the device's LDS.
hipError_t nlMeansLaunch(hipStream_t stream, const float *image, const float *guide, const float *variance, float *out, uint32_t width,
                         uint32_t height, uint32_t channels, uint32_t F, uint32_t R, float k, float varianceScale, uint32_t batch);

#endif
