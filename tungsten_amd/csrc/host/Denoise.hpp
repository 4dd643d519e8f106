// The host's text of the denoiser's NL-means filter (denoiser/NlMeans.hpp:19-157 with denoiser/BoxFilter.hpp) over plain arrays: float32,
// operation for operation in the reference's order, so that the result is the reference's bits.  The device computes the same filter
// (tghip_nlmeans, csrc/hip/denoise.hip); this is its comparator (tests/test_gpu_denoise.py) and what tests/test_denoise_cpu.py holds to results
// recorded from the reference itself (tests/golden/nlmeans.npz).
#ifndef TGAMD_DENOISE_HPP_
#define TGAMD_DENOISE_HPP_

#include <cstdint>

namespace tungsten_amd {
namespace Denoise {

const int TileSize = 32;                  // NlMeans.hpp:103
const uint32_t MaxChannels = 4, MaxF = 8, MaxR = 16;

// image / guide / variance / out: height x width pixels of `channels` interleaved floats.  A C-channel image is C independent scalar filters (the
// weight texel of nlMeans is the image texel).  threads: 0 = one per hardware thread (16 at most); the bits do not depend on it.
void nlMeans(const float *image, const float *guide, const float *variance, uint32_t width, uint32_t height, uint32_t channels,
             int F, int R, float k, float varianceScale, float *out, unsigned threads = 0);

}
}

#endif
