// The denoiser's NL-means filter on the device (tghip_nlmeans, include/tungsten_hip.h): denoiser/NlMeans.hpp:95-157 (nlMeans), :47-93
// (nlMeansWeights) and denoiser/BoxFilter.hpp restated operation for operation, so that the result is the reference's float32 bits
// (csrc/host/Denoise.cpp is the host's text of the same arithmetic; tests/test_gpu_denoise.py compares, tests/test_denoise_cpu.py holds the host to
// results recorded from the reference).
//
// One workgroup of 256 threads per 32 x 32 tile, like one task of the reference's thread pool.  It walks the (2R+1)^2 offsets in the reference's
// order (dy outer, dx inner); each thread owns four of the tile's pixels -- x = thread % 32, y = thread / 32 + 8 i -- and keeps their `result`
// and `resultWeights` sums of every channel in registers for the whole walk: a pixel's sums are sequential float additions in offset order, and
// that order is the result.  Per offset the distances of the padded rectangle, (32+2F)^2 at most, go to LDS -- one plane per channel, a C-channel
// image being C scalar filters -- and are box-filtered there: the filter's running sums (BoxFilter.hpp:55-89) are sequential chains along each row,
// then each column, one thread per chain; a rectangle narrower or lower than 2F takes the reference's in-place slow filter (:10-37 through :48-51
// with src == result), serial by nature, on one thread per plane.  Those chains are the only serial part, and one offset has only (32+2F) C of
// them; the kernel can take the offsets in batches -- the distances of `batch` offsets computed and filtered at once, then their weights added to
// the accumulators offset by offset -- but one offset at a time, with more workgroups on the CU, measured fastest (nlMeansLaunch below).
#include "denoise.h"
#include "pt_math.h"

constexpr int NLM_THREADS = 256;
constexpr int NLM_TILE = 32;              // NlMeans.hpp:103

struct NlMeansArgs {
    const float *image, *guide, *variance;
    float *out;
    int w, h, F, R, tilesX, batch;
    float k, varianceScale;
};

// an offset's rectangles, tile-uniform: the padded rectangle's origin and size (w == 0: the offset leaves the tile, nothing to do), the
// rectangle of pixels that take a weight, the offset
struct NlmJob { int px0, py0, pw, ph, sx0, sy0, sx1, sy1, dx, dy; };

// MathUtil.hpp:11-26
__device__ __forceinline__ float refMin(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float refMax(float a, float b) { return a > b ? a : b; }

// a pixel's C interleaved floats: one 16-byte load for four channels, whole dwords otherwise (lanes run along the row, so a wave's loads of a
// three-channel image cover its row segment without gaps)
template<int C>
__device__ __forceinline__ void loadTexel(const float *__restrict__ plane, size_t pixel, float *v)
{
    if (C == 4) {
        const float4 t = reinterpret_cast<const float4 *>(plane)[pixel];
        v[0] = t.x; v[1 % C] = t.y; v[2 % C] = t.z; v[3 % C] = t.w;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c)
            v[c] = plane[pixel*C + c];
    }
}

// idx / d for 0 <= idx < 2^16 and 0 < d <= 64, inv = 1.0f/d: the quotient of idx + 0.5 lies at least 0.5/d from every integer, far more than
// float rounding moves it
__device__ __forceinline__ int smallDiv(int idx, float inv) { return int((float(idx) + 0.5f)*inv); }

// boxFilterSlow in place (BoxFilter.hpp:10-37 called with src == result): raster order, so a pixel's sum reads the filtered values of the
// neighbours before it and the unfiltered ones after it
__device__ void boxFilterSlowInPlace(float *buf, int pitch, int R, int w, int h)
{
    for (int y = 0; y < h; ++y) {
        for (int x = 0; x < w; ++x) {
            float sum = 0.0f;
            int pixelCount = 0;
            for (int dy = -R; dy <= R; ++dy) {
                for (int dx = -R; dx <= R; ++dx) {
                    const int xp = x + dx, yp = y + dy;
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

// one chain of boxFilter's fast path (BoxFilter.hpp:55-71 for a row, :73-89 for a column): n elements `step` floats apart from src into dst
__device__ __forceinline__ void boxChain(const float *src, float *dst, int step, int n, int R, float factor)
{
    float sumL = 0.0f, sumR = 0.0f;
    for (int x = 0; x < 2*R; ++x) {
        sumL += src[x*step];
        sumR += src[(n - 1 - x)*step];
        if (x >= R) {
            dst[(x - R)*step] = sumL/float(x + 1);
            dst[(n - 1 - (x - R))*step] = sumR/float(x + 1);
        }
    }
    for (int x = R; x < n - R; ++x) {
        sumL += src[(x + R)*step];
        dst[x*step] = sumL*factor;
        sumL -= src[(x - R)*step];
    }
}

template<int C>
__global__ __launch_bounds__(NLM_THREADS) void k_nlmeans(const NlMeansArgs a)
{
    extern __shared__ float lds[];
    __shared__ NlmJob jobs[NLMEANS_MAX_BATCH];

    const int tid = threadIdx.x;
    const int w = a.w, h = a.h, F = a.F, R = a.R;
    const int pad = NLM_TILE + 2*F, pitch = pad + 1, plane = pad*pitch;   // (odd pitch: the row chains of a wave, one row apart, hit different banks)
    const float invPad = 1.0f/float(pad);
    float *const dist = lds, *const tmp = lds + a.batch*C*plane;
    const int tileX = (int(blockIdx.x) % a.tilesX)*NLM_TILE, tileY = (int(blockIdx.x)/a.tilesX)*NLM_TILE;
    const int tx1 = min(tileX + NLM_TILE, w), ty1 = min(tileY + NLM_TILE, h);
    const int myX = tileX + (tid & 31), myY = tileY + (tid >> 5);
    const float Epsilon = 1e-7f, MinCenterWeight = 1e-4f, DistanceClamp = 10000.0f;
    const float factor = 1.0f/float(2*F + 1);
    const float k = a.k, varianceScale = a.varianceScale;

    float result[4][C], resultWeights[4][C];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c)
            result[i][c] = resultWeights[i][c] = 0.0f;

    const int D = 2*R + 1, total = D*D;
    for (int base = 0; base < total; base += a.batch) {
        const int nb = min(a.batch, total - base);
        if (tid < nb) {
            const int o = base + tid, oy = o/D, dy = oy - R, dx = o - oy*D - R;
            NlmJob j;
            // shiftedRect (NlMeans.hpp:134-135): the tile's pixels p with p + delta inside the image
            j.sx0 = max(tileX, -dx); j.sx1 = min(tx1, w - dx);
            j.sy0 = max(tileY, -dy); j.sy1 = min(ty1, h - dy);
            // paddedClippedSrc (:62-67): grow(F), intersect the image, shift by delta, intersect, shift back
            j.px0 = max(max(j.sx0 - F, 0), -dx); j.py0 = max(max(j.sy0 - F, 0), -dy);
            j.pw = min(min(j.sx1 + F, w), w - dx) - j.px0; j.ph = min(min(j.sy1 + F, h), h - dy) - j.py0;
            if (j.sx0 >= j.sx1 || j.sy0 >= j.sy1)
                j.pw = j.ph = 0;
            j.dx = dx; j.dy = dy;
            jobs[tid] = j;
        }
        __syncthreads();

        // squaredDist over the padded rectangles (:70-81)
        for (int idx = tid; idx < nb*pad*pad; idx += NLM_THREADS) {
            const int row = smallDiv(idx, invPad), x = idx - row*pad, jb = smallDiv(row, invPad), y = row - jb*pad;
            const NlmJob &j = jobs[jb];
            if (x >= j.pw || y >= j.ph)
                continue;
            const size_t p = size_t(j.py0 + y)*w + (j.px0 + x), q = size_t(j.py0 + y + j.dy)*w + (j.px0 + x + j.dx);
            float gP[C], gQ[C], vP[C], vQ[C];
            loadTexel<C>(a.guide, p, gP); loadTexel<C>(a.guide, q, gQ);
            loadTexel<C>(a.variance, p, vP); loadTexel<C>(a.variance, q, vQ);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float varP = vP[c]*varianceScale, varQ = vQ[c]*varianceScale;
                const float diff = gP[c] - gQ[c];
                const float squaredDiff = diff*diff - (varP + refMin(varP, varQ));
                const float d = squaredDiff/((varP + varQ)*k*k + Epsilon);
                dist[(jb*C + c)*plane + y*pitch + x] = refMin(d, DistanceClamp);
            }
        }
        __syncthreads();

        // boxFilter (:83): the rows' chains into tmp -- or, in a rectangle narrower or lower than 2F, the whole in-place slow filter on the plane's first chain
        for (int ci = tid; ci < nb*C*pad; ci += NLM_THREADS) {
            const int pl = smallDiv(ci, invPad), y = ci - pl*pad;
            const NlmJob &j = jobs[pl/C];
            if (y >= j.ph)
                continue;
            if (j.pw < 2*F || j.ph < 2*F) {
                if (y == 0)
                    boxFilterSlowInPlace(dist + pl*plane, pitch, F, j.pw, j.ph);
            } else
                boxChain(dist + pl*plane + y*pitch, tmp + pl*plane + y*pitch, 1, j.pw, F, factor);
        }
        __syncthreads();
        // the columns' chains back into the distances
        for (int ci = tid; ci < nb*C*pad; ci += NLM_THREADS) {
            const int pl = smallDiv(ci, invPad), x = ci - pl*pad;
            const NlmJob &j = jobs[pl/C];
            if (x >= j.pw || j.pw < 2*F || j.ph < 2*F)
                continue;
            boxChain(tmp + pl*plane + x, dist + pl*plane + x, pitch, j.ph, F, factor);
        }
        __syncthreads();

        // the weights (:85-92) and the sums (NlMeans.hpp:139-146), offset by offset
        for (int jb = 0; jb < nb; ++jb) {
            const NlmJob j = jobs[jb];
            if (j.pw == 0)
                continue;
            const bool center = j.dx == 0 && j.dy == 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int y = myY + 8*i;
                if (myX < j.sx0 || myX >= j.sx1 || y < j.sy0 || y >= j.sy1)
                    continue;
                float texel[C];
                loadTexel<C>(a.image, size_t(y + j.dy)*w + (myX + j.dx), texel);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    float weight = fmathExp(-refMax(dist[(jb*C + c)*plane + (y - j.py0)*pitch + (myX - j.px0)], 0.0f));
                    if (center)
                        weight = refMax(weight, MinCenterWeight);
                    result[i][c] += weight*texel[c];
                    resultWeights[i][c] += weight;
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {                         // :151-152
        const int y = myY + 8*i;
        if (myX >= tx1 || y >= ty1)
            continue;
        const size_t p = size_t(y)*w + myX;
        if (C == 4) {
            reinterpret_cast<float4 *>(a.out)[p] = make_float4(result[i][0]/resultWeights[i][0], result[i][1 % C]/resultWeights[i][1 % C],
                                                               result[i][2 % C]/resultWeights[i][2 % C], result[i][3 % C]/resultWeights[i][3 % C]);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c)
                a.out[p*C + c] = result[i][c]/resultWeights[i][c];
        }
    }
}

// The batch is one offset unless the caller asks for more ("nlmeans_batch"): measured, a larger batch is slower -- at 3840 x 2160 with F 3, R 5 and four
// channels 18.2 ms for one offset against 42.6 / 34.1 / 34.1 ms for two / four / eight, with F 1, R 9 and three channels 34.1 against 48.9 / 80.9 /
// 73.4 ms (profiles/r9_denoise.txt).  A batch fills the workgroup's idle threads in the chains, but its planes take LDS from the other workgroups
// of the CU (one offset: 46 KiB and 28 KiB there, three and five workgroups on a CU's 160 KiB), and those hide the chains better: while one
// workgroup is in its chains another computes distances or weights.  A batch above 64 KiB (F >= 7 with four channels, or asked for) needs the
// kernel's dynamic LDS limit raised.
constexpr size_t NLM_LDS_DEVICE = 160u << 10, NLM_LDS_STATIC = sizeof(NlmJob)*NLMEANS_MAX_BATCH;

template<int C>
static hipError_t launchFor(hipStream_t stream, const NlMeansArgs &args, unsigned tiles, size_t ldsBytes)
{
    if (ldsBytes > (64u << 10)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_nlmeans<C>), hipFuncAttributeMaxDynamicSharedMemorySize, int(ldsBytes));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_nlmeans<C>, dim3(tiles), dim3(NLM_THREADS), ldsBytes, stream, args);
    return hipGetLastError();
}

hipError_t nlMeansLaunch(hipStream_t stream, const float *image, const float *guide, const float *variance, float *out, uint32_t width,
                         uint32_t height, uint32_t channels, uint32_t F, uint32_t R, float k, float varianceScale, uint32_t batch)
{
    if (width == 0 || height == 0)
        return hipSuccess;
    if (channels < 1 || channels > 4 || F > NLMEANS_MAX_F || R > NLMEANS_MAX_R)
        return hipErrorInvalidValue;
    const size_t pad = NLM_TILE + 2*F, offsetBytes = 2*pad*(pad + 1)*sizeof(float)*channels;
    const size_t fits = (NLM_LDS_DEVICE - NLM_LDS_STATIC)/offsetBytes;
    if (fits == 0)
        return hipErrorInvalidValue;
    if (batch == 0)
        batch = 1;
    batch = uint32_t(std::min<size_t>(std::min<size_t>(std::max<uint32_t>(batch, 1u), fits), NLMEANS_MAX_BATCH));
    batch = std::min(batch, (2*R + 1)*(2*R + 1));

    NlMeansArgs args;
    args.image = image; args.guide = guide; args.variance = variance; args.out = out;
    args.w = int(width); args.h = int(height); args.F = int(F); args.R = int(R);
    args.tilesX = int((width + NLM_TILE - 1)/NLM_TILE);
    args.batch = int(batch);
    args.k = k; args.varianceScale = varianceScale;
    const unsigned tiles = unsigned(args.tilesX)*unsigned((height + NLM_TILE - 1)/NLM_TILE);
    const size_t ldsBytes = offsetBytes*batch;
    switch (channels) {
    case 1: return launchFor<1>(stream, args, tiles, ldsBytes);
    case 2: return launchFor<2>(stream, args, tiles, ldsBytes);
    case 3: return launchFor<3>(stream, args, tiles, ldsBytes);
    default: return launchFor<4>(stream, args, tiles, ldsBytes);
    }
}
