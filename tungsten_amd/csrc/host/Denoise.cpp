#include "Denoise.hpp"
#include "../hip/fmath_exp_table.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

namespace tungsten_amd {
namespace Denoise {

namespace {

const uint32_t ExpTable[1024] = { FMATH_EXP_TABLE_VALUES };

inline float bitsToFloat(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
inline uint32_t floatToBits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// fastExp (NlMeans.hpp:19-22): one lane of fmath::exp_ps (thirdparty/fmath/fmath.hpp:320-363) -- the +-88 clamp taken when |x| compares
// above 88 as an integer, cvtps2dq's round to nearest even, the 1024-entry table of 2^(i/1024) mantissas
inline float fmathExp(float x)
{
    if ((floatToBits(x) & 0x7fffffffu) > 0x42b00000u) {
        x = x < 88.0f ? x : 88.0f;        // minps / maxps: the second operand unless the comparison holds
        x = x > -88.0f ? x : -88.0f;
    }
    const float a = 1024.0f/0.693147182464599609375f, b = 0.693147182464599609375f/1024.0f;
    const int r = int(lrintf(x*a));
    const float t = (x - float(r)*b) + 1.0f;
    const uint32_t bits = ((uint32_t(r + (127 << 10)) >> 10) << 23) | ExpTable[r & 1023];
    return t*bitsToFloat(bits);
}

// MathUtil.hpp:11-26
inline float refMin(float a, float b) { return a < b ? a : b; }
inline float refMax(float a, float b) { return a > b ? a : b; }

// one channel plane of an interleaved image: pixel (x, y) at p[(y*w + x)*stride]
struct Plane {
    const float *p;
    int w, stride;
    float operator()(int x, int y) const { return p[(size_t(y)*w + x)*stride]; }
};

// boxFilterSlow (BoxFilter.hpp:10-37) as nlMeansWeights reaches it through boxFilter (:48-51) with src and result the same pixmap (NlMeans.hpp:83):
// in place, so a pixel's sum reads the filtered values of the neighbours before it in raster order and the unfiltered ones after it
void boxFilterSlowInPlace(float *buf, int pitch, int R, int w, int h)
{
    for (int y = 0; y < h; ++y) {
        for (int x = 0; x < w; ++x) {
            float sum = 0.0f;
            int pixelCount = 0;
            for (int dy = -R; dy <= R; ++dy) {
                for (int dx = -R; dx <= R; ++dx) {
                    int xp = x + dx, yp = y + dy;
                    if (xp >= 0 && xp < w && yp >= 0 && yp < h) {
                        sum += buf[yp*pitch + xp];
                        pixelCount++;
                    }
                }
            }
            buf[y*pitch + x] = sum/float(pixelCount);
        }
    }
}

// boxFilter (BoxFilter.hpp:39-90) over the sub-image [0, w) x [0, h) of `buf`, result into `buf`: running sums along each row into tmp, then along
// each column back; the chain of additions and subtractions is the result
void boxFilter(float *buf, float *tmp, int pitch, int R, int w, int h)
{
    if (w < 2*R || h < 2*R) {
        boxFilterSlowInPlace(buf, pitch, R, w, h);
        return;
    }
    const float factor = 1.0f/float(2*R + 1);
    for (int y = 0; y < h; ++y) {
        const float *src = buf + y*pitch;
        float *dst = tmp + y*pitch;
        float sumL = 0.0f, sumR = 0.0f;
        for (int x = 0; x < 2*R; ++x) {
            sumL += src[x];
            sumR += src[w - 1 - x];
            if (x >= R) {
                dst[x - R] = sumL/float(x + 1);
                dst[w - 1 - (x - R)] = sumR/float(x + 1);
            }
        }
        for (int x = R; x < w - R; ++x) {
            sumL += src[x + R];
            dst[x] = sumL*factor;
            sumL -= src[x - R];
        }
    }
    for (int x = 0; x < w; ++x) {
        float sumL = 0.0f, sumR = 0.0f;
        for (int y = 0; y < 2*R; ++y) {
            sumL += tmp[y*pitch + x];
            sumR += tmp[(h - 1 - y)*pitch + x];
            if (y >= R) {
                buf[(y - R)*pitch + x] = sumL/float(y + 1);
                buf[(h - 1 - (y - R))*pitch + x] = sumR/float(y + 1);
            }
        }
        for (int y = R; y < h - R; ++y) {
            sumL += tmp[(y + R)*pitch + x];
            buf[y*pitch + x] = sumL*factor;
            sumL -= tmp[(y - R)*pitch + x];
        }
    }
}

// one tile of one channel: nlMeans' loop over the offsets (NlMeans.hpp:129-148) with nlMeansWeights (:47-93) inside
void filterTile(const Plane &image, const Plane &guide, const Plane &variance, int w, int h, int tileX, int tileY, int F, int R, float k,
                float varianceScale, float *result, float *resultWeights, int outStride, float *distances, float *tmp)
{
    const float Epsilon = 1e-7f, MinCenterWeight = 1e-4f, DistanceClamp = 10000.0f;
    const int pitch = TileSize + 2*F;
    const int tx1 = std::min(tileX + TileSize, w), ty1 = std::min(tileY + TileSize, h);

    for (int dy = -R; dy <= R; ++dy) {
        for (int dx = -R; dx <= R; ++dx) {
            // shiftedRect (:134-135): the tile's pixels p with p + delta inside the image
            const int sx0 = std::max(tileX, -dx), sx1 = std::min(tx1, w - dx);
            const int sy0 = std::max(tileY, -dy), sy1 = std::min(ty1, h - dy);
            if (sx0 >= sx1 || sy0 >= sy1)
                continue;                 // no weight is written and none is read (:85-87, :139-140 range over nothing)
            // paddedClippedSrc (:62-67): grow(F), intersect the image, shift by delta, intersect, shift back
            const int px0 = std::max(std::max(sx0 - F, 0), -dx), px1 = std::min(std::min(sx1 + F, w), w - dx);
            const int py0 = std::max(std::max(sy0 - F, 0), -dy), py1 = std::min(std::min(sy1 + F, h), h - dy);
            const int pw = px1 - px0, ph = py1 - py0;

            for (int y = py0; y < py1; ++y) {
                for (int x = px0; x < px1; ++x) {
                    const float varP = variance(x, y)*varianceScale;
                    const float varQ = variance(x + dx, y + dy)*varianceScale;
                    const float diff = guide(x, y) - guide(x + dx, y + dy);
                    const float squaredDiff = diff*diff - (varP + refMin(varP, varQ));
                    const float dist = squaredDiff/((varP + varQ)*k*k + Epsilon);
                    distances[(y - py0)*pitch + (x - px0)] = refMin(dist, DistanceClamp);
                }
            }

            boxFilter(distances, tmp, pitch, F, pw, ph);

            const bool center = dx == 0 && dy == 0;
            for (int y = sy0; y < sy1; ++y) {
                for (int x = sx0; x < sx1; ++x) {
                    float weight = fmathExp(-refMax(distances[(y - py0)*pitch + (x - px0)], 0.0f));
                    if (center)
                        weight = refMax(weight, MinCenterWeight);
                    const size_t idx = (size_t(y)*w + x)*outStride;
                    result[idx] += weight*image(x + dx, y + dy);
                    resultWeights[idx] += weight;
                }
            }
        }
    }
}

}

void nlMeans(const float *image, const float *guide, const float *variance, uint32_t width, uint32_t height, uint32_t channels,
             int F, int R, float k, float varianceScale, float *out, unsigned threads)
{
    const int w = int(width), h = int(height), C = int(channels);
    const size_t n = size_t(w)*h*C;
    if (n == 0)
        return;
    std::vector<float> weights(n, 0.0f);
    std::fill(out, out + n, 0.0f);
    const int tilesX = (w + TileSize - 1)/TileSize, tilesY = (h + TileSize - 1)/TileSize;
    const int jobs = tilesX*tilesY*C;

    std::atomic<int> next(0);
    auto worker = [&]() {
        const int pitch = TileSize + 2*F;
        std::vector<float> distances(size_t(pitch)*pitch), tmp(size_t(pitch)*pitch);
        for (int job = next++; job < jobs; job = next++) {
            const int c = job % C, tile = job/C;
            const Plane img = {image + c, w, C}, gd = {guide + c, w, C}, var = {variance + c, w, C};
            filterTile(img, gd, var, w, h, (tile % tilesX)*TileSize, (tile/tilesX)*TileSize, F, R, k, varianceScale,
                       out + c, weights.data() + c, C, distances.data(), tmp.data());
        }
    };
    if (threads == 0)
        threads = std::min(std::max(std::thread::hardware_concurrency(), 1u), 16u);
    threads = std::min(threads, unsigned(jobs));
    if (threads <= 1) {
        worker();
    } else {
        std::vector<std::thread> pool;
        for (unsigned i = 0; i < threads; ++i)
            pool.emplace_back(worker);
        for (std::thread &t : pool)
            t.join();
    }
    for (size_t j = 0; j < n; ++j)         // :151-152
        out[j] /= weights[j];
}

}
}
