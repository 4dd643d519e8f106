// The frame developed where it lives (tghip_develop, include/tungsten_hip.h): what Integrator::writeBuffers and Camera::saveOutputBuffers compute on
// the host from a downloaded framebuffer -- the mean, the tone-mapped 8-bit image, the auxiliary outputs' float and 8-bit images -- as kernels
// over the device's own buffers, bit for bit (csrc/host/Develop.cpp is the host's text of the same arithmetic; tests/test_gpu_develop.py compares).
//
// Bandwidth-bound and small: one thread per group of four pixels, so that the framebuffer comes in as 16-byte loads (three for the sums, one for the
// counts) and the twelve output bytes leave as three dwords; the image's last group, when the pixel count is no multiple of four, goes pixel by pixel.
#include "develop.h"
#include "pt_libm.h"

#include <climits>

constexpr int DEVELOP_THREADS = 256;

// std::max(a, b) as the host's loops call it: a < b ? b : a -- a NaN in `a` stays, a NaN in `b` never wins, -0.0f is not below 0.0f
__device__ __forceinline__ float stdMax(float a, float b) { return a < b ? b : a; }

// float -> int as the host's build converts (x86's truncating conversion): NaN and every value outside int32's range give INT_MIN; the device's own
// conversion saturates instead (+inf would be white, the reference's PNG has it black)
__device__ __forceinline__ int toIntX86(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? int(f) : INT_MIN; }
__device__ __forceinline__ uint32_t toByte(float f) { return uint32_t(min(max(toIntX86(f), 0), 255)); }

// IEEE 754 leaves a NaN result's sign and payload to the implementation, and the float images are files: r = a op b as the host's SSE unit returns
// it when it is a NaN -- the first operand that is a NaN, made quiet; none: the default NaN with the sign set (inf * 0, 0 / 0, inf - inf) -- whatever the
// device's unit would have made of it
__device__ __forceinline__ float nanX86(float r, float a, float b)
{
    if (r == r) return r;
    if (a != a) return ptlibm::u2f(ptlibm::f2u(a) | 0x00400000u);
    if (b != b) return ptlibm::u2f(ptlibm::f2u(b) | 0x00400000u);
    return ptlibm::u2f(0xffc00000u);
}

// glibc's powf (e_powf.c) for what tone mapping hands it: y = 1/2.2 or 1/2.4, x = whatever max(c, 0) lets through -- +-0, subnormals, normals,
// +inf, NaN.  y log2(x) stays within +-68, far inside the core's range.
__device__ __forceinline__ float developPowf(float x, float y)
{
    uint32_t ix = ptlibm::f2u(x);
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
        if (2u*ix - 1u >= 2u*0x7f800000u - 1u)
            return x*x;                                   // zero, inf, NaN (y positive and no odd integer)
        if (ix & 0x80000000u)
            return ptlibm::u2f(0x7fc00000u);              // finite x < 0
        ix = (ptlibm::f2u(x*0x1p23f) & 0x7fffffffu) - (23u << 23);   // subnormal: normalised, the exponent below zero
    }
    return ptlibm::powfCoreBits(ix, y);
}

// ImageIO::tonemap (cameras/Tonemap.hpp:25-48), one channel
template<uint32_t OP>
__device__ __forceinline__ float developTonemap(float c)
{
    if (OP == TGHIP_TONEMAP_LINEAR)
        return c;
    if (OP == TGHIP_TONEMAP_GAMMA)
        return developPowf(c, 1.0f/2.2f);
    if (OP == TGHIP_TONEMAP_REINHARD)
        return developPowf(c/(c + 1.0f), 1.0f/2.2f);
    if (OP == TGHIP_TONEMAP_FILMIC) {
        float x = stdMax(0.0f, c - 0.004f);
        return (x*(6.2f*x + 0.5f))/(x*(6.2f*x + 1.7f) + 0.06f);
    }
    return c < 0.0031308f ? 12.92f*c : 1.055f*developPowf(c, 1.0f/2.4f) - 0.055f;   // TGHIP_TONEMAP_PBRT
}

// Integrator::writeBuffers' bytes of a group's twelve channels (the operator is the launch's: one run of code per operator, not per channel)
template<uint32_t OP>
__device__ __forceinline__ void developBytes(const float *m, uint32_t *bytes)
{
#pragma unroll
    for (int i = 0; i < 12; ++i)
        bytes[i] = toByte(developTonemap<OP>(stdMax(m[i], 0.0f))*255.0f);
}

__device__ __forceinline__ uint32_t pack4(const uint32_t *b) { return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24); }

// the twelve bytes of a group: three dwords, or the bytes of its `valid` pixels
__device__ __forceinline__ void storeBytes(uint8_t *ldr, size_t first, int valid, const uint32_t *bytes)
{
    if (valid == 4) {
        uint32_t *out = reinterpret_cast<uint32_t *>(ldr + first*3);
        out[0] = pack4(bytes); out[1] = pack4(bytes + 4); out[2] = pack4(bytes + 8);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)                      // (static indices: `bytes` stays in registers)
            if (i < valid*3)
                ldr[first*3 + i] = uint8_t(bytes[i]);
    }
}

// the same for a group's floats, `per` of them per pixel (3 or 1)
template<int PER>
__device__ __forceinline__ void storeFloats(float *hdr, size_t group, int valid, const float *v)
{
    if (valid == 4) {
        float4 *out = reinterpret_cast<float4 *>(hdr) + group*PER;
#pragma unroll
        for (int q = 0; q < PER; ++q)
            out[q] = make_float4(v[q*4], v[q*4 + 1], v[q*4 + 2], v[q*4 + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4*PER; ++i)
            if (i < valid*PER)
                hdr[group*4*PER + i] = v[i];
    }
}

__global__ __launch_bounds__(DEVELOP_THREADS) void k_develop_frame(const float *__restrict__ sum, const uint32_t *__restrict__ count, size_t npixels,
                                                                   uint32_t op, float *__restrict__ hdr, uint8_t *__restrict__ ldr)
{
    const size_t group = size_t(blockIdx.x)*DEVELOP_THREADS + threadIdx.x, first = group*4;
    if (first >= npixels)
        return;
    const int valid = npixels - first < 4 ? int(npixels - first) : 4;
    float m[12];
    uint32_t cnt[4];
    if (valid == 4) {
        const float4 *s4 = reinterpret_cast<const float4 *>(sum) + group*3;
        const float4 s0 = s4[0], s1 = s4[1], s2 = s4[2];
        const uint4 c4 = reinterpret_cast<const uint4 *>(count)[group];
        m[0] = s0.x; m[1] = s0.y; m[2] = s0.z; m[3] = s0.w; m[4] = s1.x; m[5] = s1.y; m[6] = s1.z; m[7] = s1.w;
        m[8] = s2.x; m[9] = s2.y; m[10] = s2.z; m[11] = s2.w;
        cnt[0] = c4.x; cnt[1] = c4.y; cnt[2] = c4.z; cnt[3] = c4.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            cnt[i] = i < valid ? count[first + i] : 0u;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                m[i*3 + k] = i < valid ? sum[(first + i)*3 + k] : 0.0f;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {                         // PathTraceHipIntegrator::linearImage
        const float inv = cnt[i] ? 1.0f/float(cnt[i]) : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            m[i*3 + k] = nanX86(m[i*3 + k]*inv, m[i*3 + k], inv);
    }
    if (hdr)
        storeFloats<3>(hdr, group, valid, m);
    if (ldr) {                                            // Integrator::writeBuffers
        uint32_t bytes[12];
        switch (op) {
        case TGHIP_TONEMAP_LINEAR: developBytes<TGHIP_TONEMAP_LINEAR>(m, bytes); break;
        case TGHIP_TONEMAP_GAMMA: developBytes<TGHIP_TONEMAP_GAMMA>(m, bytes); break;
        case TGHIP_TONEMAP_REINHARD: developBytes<TGHIP_TONEMAP_REINHARD>(m, bytes); break;
        case TGHIP_TONEMAP_FILMIC: developBytes<TGHIP_TONEMAP_FILMIC>(m, bytes); break;
        default: developBytes<TGHIP_TONEMAP_PBRT>(m, bytes); break;
        }
        storeBytes(ldr, first, valid, bytes);
    }
}

// an output's first channel in TgHipAuxPixel (colour 0-2 | depth 3 | normal 4-6 | albedo 7-9 | visibility 10)
__device__ __forceinline__ uint32_t auxFirstChannel(uint32_t type) { return type == TGHIP_AUX_COLOR ? 0u : type == TGHIP_AUX_DEPTH ? 3u : type == TGHIP_AUX_NORMAL ? 4u : type == TGHIP_AUX_ALBEDO ? 7u : 10u; }

// channel ch (of TGHIP_AUX_CHANNELS) of output `type` as OutputBuffer hands it out: operator[] (cameras/OutputBuffer.hpp:134-144), the two halves, save()'s variance (:178-181)
__device__ __forceinline__ float auxValue(const TgHipAuxPixel &p, uint32_t type, uint32_t part, uint32_t ch)
{
    const uint32_t cnt = p.count[type], cntA = (cnt + 1)/2, cntB = cnt/2;
    switch (part) {
    case TGHIP_DEVELOP_MEAN: {
        const float a = p.a[ch], b = p.b[ch], nA = float(cntA), nB = float(cntB), n = float(max(cnt, 1u));
        // (two NaN halves with different bits -- no render makes them --: the host's build adds b's product in place, so that one is the first operand)
        const float sa = nanX86(a*nA, a, nA), sb = nanX86(b*nB, b, nB), s = nanX86(sa + sb, sb, sa);
        return nanX86(s/n, s, n);
    }
    case TGHIP_DEVELOP_A:
        return p.a[ch];
    case TGHIP_DEVELOP_B:
        return p.b[ch];
    default: {                                            // TGHIP_DEVELOP_VARIANCE
        const float v = p.variance[ch], d = float(cnt*max(1u, cnt - 1));
        return nanX86(v/d, v, d);
    }
    }
}

// OutputBuffer::saveLdr's maximum of the depth image (:64-67): over the entries that are not +inf, from 0.0f, by std::max -- so only entries above
// zero ever win and a NaN never does: whatever the order, the largest positive finite entry, or 0.  Positive floats order like their bit patterns:
// per wave by shuffles, then one atomic maximum per wave into *result (cleared by the launcher).
__global__ __launch_bounds__(DEVELOP_THREADS) void k_develop_depth_max(const TgHipAuxPixel *__restrict__ aux, size_t npixels, uint32_t part, uint32_t *result)
{
    const size_t i = size_t(blockIdx.x)*DEVELOP_THREADS + threadIdx.x;
    uint32_t best = 0u;
    if (i < npixels) {
        const float v = auxValue(aux[i], TGHIP_AUX_DEPTH, part, 3);
        if (v > 0.0f && v != ptlibm::u2f(0x7f800000u))
            best = ptlibm::f2u(v);
    }
    for (int off = 32; off > 0; off >>= 1)
        best = max(best, uint32_t(__shfl_xor(int(best), off, 64)));
    if ((threadIdx.x & 63) == 0 && best != 0u)
        atomicMax(result, best);
}

template<int NCH>                                         // the output's channels: 3, or 1 (replicated to RGB in the 8-bit image)
__global__ __launch_bounds__(DEVELOP_THREADS) void k_develop_aux(const TgHipAuxPixel *__restrict__ aux, size_t npixels, uint32_t type, uint32_t part,
                                                                 float *__restrict__ hdr, uint8_t *__restrict__ ldr, const uint32_t *__restrict__ depthMax)
{
    const size_t group = size_t(blockIdx.x)*DEVELOP_THREADS + threadIdx.x, first = group*4;
    if (first >= npixels)
        return;
    const int valid = npixels - first < 4 ? int(npixels - first) : 4;
    const uint32_t ch0 = auxFirstChannel(type);
    float v[4*NCH];                                       // pixel i, channel k at i*NCH + k
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < NCH; ++k)
            v[i*NCH + k] = i < valid ? auxValue(aux[first + i], type, part, ch0 + k) : 0.0f;
    if (hdr)
        storeFloats<NCH>(hdr, group, valid, v);
    if (ldr) {                                            // OutputBuffer::saveLdr (:56-86)
        float minimum = 0.0f, maximum = 0.0f;
        bool rescale = part != TGHIP_DEVELOP_VARIANCE;
        if (type == TGHIP_AUX_DEPTH) {
            if (rescale) maximum = ptlibm::u2f(*depthMax);
        } else if (type == TGHIP_AUX_NORMAL) {
            minimum = -1.0f; maximum = 1.0f;
        } else
            rescale = false;
        uint32_t bytes[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float f[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                f[k] = v[i*NCH + (NCH == 3 ? k : 0)];
                if (rescale) f[k] = (f[k] - minimum)/(maximum - minimum);
            }
            const float avg = NCH == 3 ? (f[0] + f[1] + f[2])/3.0f : f[0];
            const bool bad = avg != avg || fabsf(avg) == ptlibm::u2f(0x7f800000u);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                bytes[i*3 + k] = bad ? 255u : toByte(f[k]*255.0f);
        }
        storeBytes(ldr, first, valid, bytes);
    }
}

static unsigned blocksFor(size_t items) { return unsigned((items + DEVELOP_THREADS - 1)/DEVELOP_THREADS); }

hipError_t developLaunchFrame(hipStream_t stream, const float *sum, const uint32_t *count, size_t npixels, uint32_t tonemap, float *hdr, uint8_t *ldr)
{
    if (npixels == 0 || (!hdr && !ldr))
        return hipSuccess;
    hipLaunchKernelGGL(k_develop_frame, dim3(blocksFor((npixels + 3)/4)), dim3(DEVELOP_THREADS), 0, stream, sum, count, npixels, tonemap, hdr, ldr);
    return hipGetLastError();
}

hipError_t developLaunchAux(hipStream_t stream, const TgHipAuxPixel *aux, size_t npixels, uint32_t output, uint32_t part, float *hdr, uint8_t *ldr,
                            uint32_t *depthMax)
{
    if (npixels == 0 || (!hdr && !ldr))
        return hipSuccess;
    if (ldr && output == TGHIP_AUX_DEPTH && part != TGHIP_DEVELOP_VARIANCE) {
        hipError_t e = hipMemsetAsync(depthMax, 0, sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_develop_depth_max, dim3(blocksFor(npixels)), dim3(DEVELOP_THREADS), 0, stream, aux, npixels, part, depthMax);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (output == TGHIP_AUX_DEPTH || output == TGHIP_AUX_VISIBILITY)
        hipLaunchKernelGGL(k_develop_aux<1>, dim3(blocksFor((npixels + 3)/4)), dim3(DEVELOP_THREADS), 0, stream, aux, npixels, output, part, hdr, ldr, depthMax);
    else
        hipLaunchKernelGGL(k_develop_aux<3>, dim3(blocksFor((npixels + 3)/4)), dim3(DEVELOP_THREADS), 0, stream, aux, npixels, output, part, hdr, ldr, depthMax);
    return hipGetLastError();
}
