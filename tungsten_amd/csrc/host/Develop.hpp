// The host's text of the frame's development: the two loops that turned a downloaded framebuffer into the images of the output files --
// Integrator::writeBuffers' tone mapping (integrators/Integrator.cpp:56-80 with Camera::getLinear, cameras/Tonemap.hpp) and the images of
// Camera::saveOutputBuffers (cameras/OutputBuffer.hpp:56-86, 134-189) -- as functions over plain arrays.  The device computes the same bytes
// where the framebuffer lives (tghip_develop, csrc/hip/develop.hip); these are its comparator (tests/test_gpu_develop.py) and what renders
// merged from several devices, and contexts with the "develop_host" option, go through.
#ifndef TGAMD_DEVELOP_HPP_
#define TGAMD_DEVELOP_HPP_

#include "../../../include/tungsten_hip.h"

#include <cstddef>
#include <cstdint>
#include <string>

namespace tungsten_amd {
namespace Develop {

// "linear" ... "pbrt" <-> TGHIP_TONEMAP_*; tonemapIndex throws on a name ImageIO::tonemap does not know, tonemapName returns nullptr
uint32_t tonemapIndex(const std::string &op);
const char *tonemapName(uint32_t index);
uint32_t auxChannels(uint32_t output);   // 3, 1, 3, 3, 1

// hdr: 3 floats per pixel, ldr: 3 bytes per pixel; either may be null
void frame(const float *sum, const uint32_t *count, size_t n, const std::string &tonemap, float *hdr, uint8_t *ldr);
// output: TGHIP_AUX_*, part: TGHIP_DEVELOP_*; hdr: auxChannels(output) floats per pixel
void aux(const TgHipAuxPixel *aux, size_t n, uint32_t output, uint32_t part, float *hdr, uint8_t *ldr);

}
}

#endif
