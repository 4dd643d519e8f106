#include "Develop.hpp"
#include "ImageIO.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <vector>

namespace tungsten_amd {
namespace Develop {

static const char *const TonemapNames[5] = {"linear", "gamma", "reinhard", "filmic", "pbrt"};

uint32_t tonemapIndex(const std::string &op)
{
    for (uint32_t i = 0; i < 5; ++i)
        if (op == TonemapNames[i])
            return i;
    throw std::runtime_error("Invalid tonemap operator: '" + op + "'");
}

const char *tonemapName(uint32_t index)
{
    return index < 5 ? TonemapNames[index] : nullptr;
}

uint32_t auxChannels(uint32_t output)
{
    static const uint32_t channels[TGHIP_AUX_OUTPUTS] = {3, 1, 3, 3, 1};
    return output < TGHIP_AUX_OUTPUTS ? channels[output] : 0;
}

void frame(const float *sum, const uint32_t *count, size_t n, const std::string &tonemap, float *hdr, uint8_t *ldr)
{
    std::vector<float> linear;
    if (!hdr) {
        linear.resize(n*3);
        hdr = linear.data();
    }
    for (size_t i = 0; i < n; ++i) {                      // Camera::getLinear
        float inv = count[i] ? 1.0f/float(count[i]) : 0.0f;
        for (int k = 0; k < 3; ++k)
            hdr[i*3 + k] = sum[i*3 + k]*inv;
    }
    if (!ldr)
        return;
    for (size_t i = 0; i < n; ++i) {                      // Integrator::writeBuffers
        Vec3f c(std::max(hdr[i*3], 0.0f), std::max(hdr[i*3 + 1], 0.0f), std::max(hdr[i*3 + 2], 0.0f));
        Vec3f t = ImageIO::tonemap(tonemap, c)*255.0f;
        for (int k = 0; k < 3; ++k)
            ldr[i*3 + k] = uint8_t(std::min(std::max(int(t[k]), 0), 255));
    }
}

// OutputBuffer<T>::save for one image of one output (cameras/OutputBuffer.hpp:146-189, saveLdr :56-86).  The device keeps every output as A / B
// halves + Welford sum; what a buffer without two_buffer_variance would hold in _bufferA is the mean of both halves.
void aux(const TgHipAuxPixel *aux, size_t n, uint32_t output, uint32_t part, float *hdr, uint8_t *ldr)
{
    static const int first[5] = {0, 3, 4, 7, 10};
    const int ch0 = first[output], nch = int(auxChannels(output));
    std::vector<float> own;
    if (!hdr) {
        own.resize(n*nch);
        hdr = own.data();
    }
    float *img = hdr;
    for (size_t i = 0; i < n; ++i) {
        const TgHipAuxPixel &p = aux[i];
        uint32_t cnt = p.count[output], cntA = (cnt + 1)/2, cntB = cnt/2;
        for (int k = 0; k < nch; ++k) {
            float a = p.a[ch0 + k], bb = p.b[ch0 + k];
            switch (part) {
            case TGHIP_DEVELOP_MEAN: img[i*nch + k] = (a*float(cntA) + bb*float(cntB))/float(std::max(cnt, 1u)); break;      // operator[] (:134-144)
            case TGHIP_DEVELOP_A: img[i*nch + k] = a; break;
            case TGHIP_DEVELOP_B: img[i*nch + k] = bb; break;
            default: img[i*nch + k] = p.variance[ch0 + k]/float(cnt*std::max(1u, cnt - 1)); break;                           // save() (:178-181)
            }
        }
    }
    if (!ldr)
        return;
    bool rescale = part != TGHIP_DEVELOP_VARIANCE;                                                    // OutputBuffer::saveLdr
    float minimum = 0.0f, maximum = 0.0f;
    if (output == TGHIP_AUX_DEPTH) {
        for (size_t i = 0; i < n; ++i)
            if (img[i] != std::numeric_limits<float>::infinity()) maximum = std::max(maximum, img[i]);
    } else if (output == TGHIP_AUX_NORMAL) {
        minimum = -1.0f; maximum = 1.0f;
    } else {
        rescale = false;
    }
    for (size_t i = 0; i < n; ++i) {
        bool bad = false;
        float f[3];
        for (int k = 0; k < 3; ++k) {
            f[k] = img[i*nch + (nch == 3 ? k : 0)];
            if (rescale) f[k] = (f[k] - minimum)/(maximum - minimum);
        }
        float avg = nch == 3 ? (f[0] + f[1] + f[2])/3.0f : f[0];
        bad = std::isnan(avg) || std::isinf(avg);
        for (int k = 0; k < 3; ++k)
            ldr[i*3 + k] = bad ? 255 : uint8_t(std::min(std::max(int(f[k]*255.0f), 0), 255));
    }
}

}
}
