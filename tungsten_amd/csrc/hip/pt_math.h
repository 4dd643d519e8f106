// Device-side math for the path_tracer_hip kernels (gfx950 only).
//
// Constants and operation order follow the reference so that the GPU consumes and produces the
// same numbers as Tungsten's CPU code wherever IEEE arithmetic allows (division and sqrt are
// correctly rounded under hipcc's defaults; sinf / cosf / logf / expf / acosf are glibc's own algorithms
// restated -- pt_libm.h: sinf / cosf / logf / expf / atan2f / powf / cbrtf; acosfExact below -- DESIGN.md "Numerics").
#ifndef TGAMD_PT_MATH_H_
#define TGAMD_PT_MATH_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/tungsten_hip.h"
#include "pt_libm.h"

#define PT_PI          3.1415926536f            /* math/Angle.hpp:8 */
#define PT_TWO_PI      (PT_PI*2.0f)
#define PT_FOUR_PI     (PT_PI*4.0f)
#define PT_INV_PI      (1.0f/PT_PI)
#define PT_INV_TWO_PI  (0.5f*PT_INV_PI)
#define PT_INV_FOUR_PI (0.25f*PT_INV_PI)
#define PT_INF         __builtin_huge_valf()

#define PT_DEV __device__ __forceinline__

// base[idx] with the byte offset computed in 32 bits: lets the compiler address with "SGPR base + 32-bit VGPR
// offset" (one offset register shared by every 16-byte-per-slot array) instead of materialising a 64-bit address
// per array.  Arrays indexed this way must stay below 4 GiB (checked at upload / pool allocation).
template<typename T> PT_DEV T &at32(T *base, uint32_t idx)
{
    return *reinterpret_cast<T *>(reinterpret_cast<char *>(base) + (size_t)(idx*(uint32_t)sizeof(T)));
}
template<typename T> PT_DEV const T &at32(const T *base, uint32_t idx)
{
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + (size_t)(idx*(uint32_t)sizeof(T)));
}

// A float4 table entry read as ONE 16-byte vector load.  Read through `const float4 &` the compiler drops the words a kernel does not use and
// issues global_load_dwordx3 / x2 instead.  In isolation the narrow load costs what the wide one costs (tools/ubench_loads.hip), but the kernels
// built around it are slower -- a three-register destination, the copies behind it, the schedule (measured on the wide nodes' second row: shadow
// launches -2 %; on the slots: -6.5 %, profiles/r5_ab_x4_loads.txt).
typedef float PtLd4v __attribute__((ext_vector_type(4)));
PT_DEV float4 ld4(const float4 *base, uint32_t idx)
{
    const PtLd4v v = *reinterpret_cast<const PtLd4v *>(reinterpret_cast<const char *>(base) + (size_t)(idx*16u));
    return make_float4(v.x, v.y, v.z, v.w);
}

struct f3 { float x, y, z; };

// ---- two library functions restated so that the device computes what the host's libm computes, bit for bit ---------------------
// acosf as glibc 2.35 has it (sysdeps/ieee754/flt-32/e_acosf.c, the fdlibm rational approximation evaluated in float): nothing but
// float +, -, *, / and sqrt, every one of them correctly rounded here as there (-ffp-contract=off).  Quad::approximateRadiance
// (primitives/Quad.cpp:253-281) obtains the solid angle of a light as 2 pi minus four arc cosines; for a millimetre-sized emitter the
// last bit of acosf moves chooseLight's weights by per cents, so "within an ulp of libm" (ocml) is not close enough.
PT_DEV float acosfExact(float x)
{
    const float one = 1.0f, pi = 3.1415925026e+00f, pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f,
                pS0 = 1.6666667163e-01f, pS1 = -3.2556581497e-01f, pS2 = 2.0121252537e-01f, pS3 = -4.0055535734e-02f,
                pS4 = 7.9153501429e-04f, pS5 = 3.4793309169e-05f,
                qS1 = -2.4033949375e+00f, qS2 = 2.0209457874e+00f, qS3 = -6.8828397989e-01f, qS4 = 7.7038154006e-02f;
    const int hx = __float_as_int(x), ix = hx & 0x7fffffff;
    if (ix == 0x3f800000)
        return hx > 0 ? 0.0f : pi + 2.0f*pio2_lo;
    if (ix > 0x3f800000)
        return (x - x)/(x - x);
    if (ix < 0x3f000000) {                       // |x| < 0.5
        if (ix <= 0x32800000) return pio2_hi + pio2_lo;
        const float z = x*x;
        const float p = z*(pS0 + z*(pS1 + z*(pS2 + z*(pS3 + z*(pS4 + z*pS5)))));
        const float q = one + z*(qS1 + z*(qS2 + z*(qS3 + z*qS4)));
        const float r = p/q;
        return pio2_hi - (x - (pio2_lo - x*r));
    } else if (hx < 0) {                         // x < -0.5
        const float z = (one + x)*0.5f;
        const float p = z*(pS0 + z*(pS1 + z*(pS2 + z*(pS3 + z*(pS4 + z*pS5)))));
        const float q = one + z*(qS1 + z*(qS2 + z*(qS3 + z*qS4)));
        const float s = sqrtf(z);
        const float r = p/q;
        const float w = r*s - pio2_lo;
        return pi - 2.0f*(s + w);
    } else {                                     // x > 0.5
        const float z = (one - x)*0.5f;
        const float s = sqrtf(z);
        const float df = __int_as_float(__float_as_int(s) & (int)0xfffff000);
        const float c = (z - df*df)/(s + df);
        const float p = z*(pS0 + z*(pS1 + z*(pS2 + z*(pS3 + z*(pS4 + z*pS5)))));
        const float q = one + z*(qS1 + z*(qS2 + z*(qS3 + z*qS4)));
        const float r = p/q;
        const float w = r*s + c;
        return 2.0f*(df + w);
    }
}
// FastMath::exp -> fmath::exp / exp_ps (math/FastMath.hpp:14-27, thirdparty/fmath/fmath.hpp:221-241, 320-363): what the reference's
// ExponentialTransmittance computes (transmittances/ExponentialTransmittance.cpp:26-41) -- a 1024-entry table of 2^(i/1024) and a
// first-order correction, all in float and integer arithmetic, so it is reproduced exactly instead of approximated by expf.
#include "fmath_exp_table.h"
__device__ const uint32_t g_fmathExpTable[1024] = { FMATH_EXP_TABLE_VALUES };
PT_DEV float fmathExp(float x)
{
    if ((__float_as_int(x) & 0x7fffffff) > 0x42b00000)            // |x| > 88 (compared as integers, like the reference)
        x = fmaxf(fminf(x, 88.0f), -88.0f);
    const float a = 1024.0f/0.693147182464599609375f, b = 0.693147182464599609375f/1024.0f;   // n/logf(2), logf(2)/n as floats
    const int r = __float2int_rn(x*a);                             // cvtss2si: round to nearest even
    const float t = x - (float)r*b;
    const uint32_t bits = ((uint32_t)((r >> 10) + 127) << 23) | g_fmathExpTable[r & 1023];
    return (1.0f + t)*__uint_as_float(bits);
}
// glibc's sinf / cosf / logf / expf (pt_libm.h: matched exhaustively against the host libm).  Outside the ranges those cover -- which no
// call site reaches: every angle here is 2 pi xi, pi v or a blade angle -- sin / cos fold the argument into [-pi, pi] in double first
// (not glibc's Payne-Hanek result bit for bit, and cheap: ocml's large-argument path stays out of the kernels); logf / expf are glibc's for
// every float (special cases included).
PT_DEV float foldAngle(float x) { const double xd = x; return (float)(xd - 6.283185307179586*__builtin_rint(xd*0.15915494309189535)); }
PT_DEV float sinfH(float x) { return ptlibm::sinfCore(ptlibm::sincosInRange(x) ? x : foldAngle(x)); }
PT_DEV float cosfH(float x) { return ptlibm::cosfCore(ptlibm::sincosInRange(x) ? x : foldAngle(x)); }
PT_DEV void sincosfH(float x, float &s, float &c) { ptlibm::sincosfCore(ptlibm::sincosInRange(x) ? x : foldAngle(x), s, c); }
PT_DEV float logfH(float x) { return ptlibm::logfAll(x); }
PT_DEV float expfH(float x) { return ptlibm::expfAll(x); }
// glibc's atan2f / powf / cbrtf (pt_libm.h; round 4: called by the kernels).  atan2f: every float pair, special cases included.  powf: the
// core covers positive normal x, finite non-zero y and results that are normal floats -- every call site's operands (Davis transmittances:
// base >= 1, optical depths) --; outside that (zero / subnormal / negative base, overflow, underflow: exact or saturating results) ocml's.
PT_DEV float atan2fH(float y, float x) { return ptlibm::atan2fCore(y, x); }
PT_DEV float powfH(float x, float y) { return ptlibm::powInRange(x, y) ? ptlibm::powfCore(x, y) : powf(x, y); }
PT_DEV float cbrtfH(float x) { return ptlibm::cbrtfCore(x); }
PT_DEV float tanfH(float x) { return ptlibm::tanfCore(x); }      // |x| < 120 (OrenNayarBsdf: angles in [0, pi/2])
PT_DEV float sinhfH(float x) { return ptlibm::sinhfCore(x); }    // 0 < x <= 10 (RoughWireBcsdf::M: 1/v with v >= 0.1), NaN outside

PT_DEV f3 mk3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
PT_DEV f3 splat3(float s) { return mk3(s, s, s); }
// c ? a : b per component (`c ? a : b` on two f3 LVALUES selects an address: both objects then live in scratch memory)
PT_DEV f3 sel3(bool c, f3 a, f3 b) { return mk3(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }
template<typename P> PT_DEV f3 ld3(P p) { return mk3(p[0], p[1], p[2]); }   // P: pointer to float in any address space

// Pointer into the constant address space: a load through it with a wave-uniform address is a scalar-cache
// (s_load) access instead of a vector memory instruction (used by the flat-list traversal, pt_kernels.h).
#define PT_CONST_AS __attribute__((address_space(4)))
template<typename T> PT_DEV const PT_CONST_AS T *asConst(const T *p) { return (const PT_CONST_AS T *)p; }
PT_DEV f3 xyz(float4 v) { return mk3(v.x, v.y, v.z); }
PT_DEV float4 mk4(f3 v, float w) { return make_float4(v.x, v.y, v.z, w); }
PT_DEV f3 operator+(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
PT_DEV f3 operator-(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
PT_DEV f3 operator*(f3 a, f3 b) { return mk3(a.x*b.x, a.y*b.y, a.z*b.z); }
PT_DEV f3 operator/(f3 a, f3 b) { return mk3(a.x/b.x, a.y/b.y, a.z/b.z); }
PT_DEV f3 operator*(f3 a, float s) { return mk3(a.x*s, a.y*s, a.z*s); }
PT_DEV f3 operator/(f3 a, float s) { return mk3(a.x/s, a.y/s, a.z/s); }
PT_DEV f3 operator-(f3 a) { return mk3(-a.x, -a.y, -a.z); }
PT_DEV float dot(f3 a, f3 b) { return a.x*b.x + a.y*b.y + a.z*b.z; }
PT_DEV f3 cross(f3 a, f3 b) { return mk3(a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x); }
PT_DEV float lengthSq(f3 a) { return a.x*a.x + a.y*a.y + a.z*a.z; }
PT_DEV float length(f3 a) { return sqrtf(lengthSq(a)); }
PT_DEV f3 normalized(f3 a) { float inv = 1.0f/length(a); return mk3(a.x*inv, a.y*inv, a.z*inv); }   /* Vec.hpp:168-175 */
PT_DEV float max3(f3 a) { return fmaxf(a.x, fmaxf(a.y, a.z)); }
PT_DEV float avg3(f3 a) { return (a.x + a.y + a.z)*(1.0f/3.0f); }
PT_DEV float sum3(f3 a) { return a.x + a.y + a.z; }
PT_DEV bool isZero(f3 a) { return a.x == 0.0f && a.y == 0.0f && a.z == 0.0f; }   /* Vec == scalar: all components */
PT_DEV f3 exp3(f3 a) { return mk3(expfH(a.x), expfH(a.y), expfH(a.z)); }
PT_DEV float sqr(float x) { return x*x; }
PT_DEV float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

/* row-major 3x3 times vector and transpose times vector */
template<typename P> PT_DEV f3 mat3Mul(P m, f3 p)
{
    return mk3(m[0]*p.x + m[1]*p.y + m[2]*p.z, m[3]*p.x + m[4]*p.y + m[5]*p.z, m[6]*p.x + m[7]*p.y + m[8]*p.z);
}
template<typename P> PT_DEV f3 mat3TMul(P m, f3 p)
{
    return mk3(m[0]*p.x + m[3]*p.y + m[6]*p.z, m[1]*p.x + m[4]*p.y + m[7]*p.z, m[2]*p.x + m[5]*p.y + m[8]*p.z);
}

/* TangentFrame(n): Duff et al. orthonormal basis (math/TangentFrame.hpp:22-31) */
struct Frame { f3 normal, tangent, bitangent; };
PT_DEV Frame frameFromNormal(f3 n)
{
    Frame f;
    f.normal = n;
    float sign = copysignf(1.0f, n.z);
    const float a = -1.0f/(sign + n.z);
    const float b = n.x*n.y*a;
    f.tangent = mk3(1.0f + sign*n.x*n.x*a, sign*b, -sign*n.x);
    f.bitangent = mk3(b, sign + n.y*n.y*a, -n.y);
    return f;
}
PT_DEV f3 toLocal(const Frame &f, f3 p) { return mk3(dot(f.tangent, p), dot(f.bitangent, p), dot(f.normal, p)); }
PT_DEV f3 toGlobal(const Frame &f, f3 p) { return f.tangent*p.x + f.bitangent*p.y + f.normal*p.z; }

/* ---- random numbers: PCG-XSH-RR 64/32 (sampling/UniformSampler.hpp:40-47) keyed per
 * (seed, pixelIndex, sampleIndex) -- identical to oracle/oracle.c sampler_start ---------------- */
PT_DEV uint32_t hash32(uint32_t x)   /* math/MathUtil.hpp:120-128 */
{
    x = ~x + (x << 15);
    x = x ^ (x >> 12);
    x = x + (x << 2);
    x = x ^ (x >> 4);
    x = x * 2057;
    x = x ^ (x >> 16);
    return x;
}

// PathSampleGenerator state of one path.  state/inc: the counter-based PCG stream (DESIGN.md "RNG").  The other
// fields are SobolPathSampler's (sampling/SobolPathSampler.hpp:14-18) and only live in kernel variants compiled
// with FEAT_QMC; `sobol` == nullptr selects the uniform sampler.
struct Rng {
    uint64_t state, inc;
    const uint32_t *sobol;     // generator matrices, TGHIP_SOBOL_DIMS x TGHIP_SOBOL_BITS words
    uint32_t scramble, index, dim;
};

PT_DEV Rng rngStart(uint32_t seed, uint32_t pixelIndex, uint32_t sampleIndex)
{
    uint32_t a = hash32(seed) ^ pixelIndex;
    uint32_t b = hash32(a) + sampleIndex;
    uint32_t hi = hash32(b), lo = hash32(b ^ 0x9E3779B9u);
    Rng r;
    r.state = ((uint64_t)hi << 32) | lo;
    r.inc = ((uint64_t)pixelIndex << 1) | 1u;
    r.sobol = nullptr;
    r.scramble = r.index = r.dim = 0u;
    return r;
}
PT_DEV uint32_t rngNextI(Rng &r)
{
    uint64_t oldState = r.state;
    r.state = oldState*6364136223846793005ULL + r.inc;
    uint32_t xorShifted = (uint32_t)(((oldState >> 18u) ^ oldState) >> 27u);
    uint32_t rot = (uint32_t)(oldState >> 59u);
    return (xorShifted >> rot) | (xorShifted << ((uint32_t)(-(int32_t)rot) & 31));
}
PT_DEV float rngNext1D(Rng &r)       /* BitManip::normalizedUint (math/BitManip.hpp:47-50) */
{
    return __uint_as_float((rngNextI(r) >> 9u) | 0x3F800000u) - 1.0f;
}
// booleans always come from the PCG stream (UniformPathSampler.hpp:39-42; SobolPathSampler.hpp:54-57 uses its
// supplemental sampler)
PT_DEV bool rngNextBoolean(Rng &r, float pTrue) { return rngNext1D(r) < pTrue; }

// sobol::sample (thirdparty/sobol/sobol.h:39-53): XOR of the generator-matrix columns the index bits select
PT_DEV uint32_t sobolSample(const uint32_t *matrices, uint32_t index, uint32_t dimension, uint32_t scramble)
{
    // The first eight columns of a dimension (index bits 0..7, i.e. all of them up to 256 spp) are fetched with two
    // independent 16-byte loads -- a dimension's 52 words start 208 B apart, so they are 16-byte aligned -- and selected
    // by the index bits; the reference's bit-serial loop, one dependent cache access per set bit with a trip count that
    // differs from lane to lane, cost the Cornell box 44 % of its throughput.  Higher bits take the loop.
    const uint32_t *col = matrices + dimension*TGHIP_SOBOL_BITS;
    const uint4 lo = *reinterpret_cast<const uint4 *>(col), hi = *reinterpret_cast<const uint4 *>(col + 4);
    uint32_t result = scramble;
    result ^= (index & 0x01u) ? lo.x : 0u;
    result ^= (index & 0x02u) ? lo.y : 0u;
    result ^= (index & 0x04u) ? lo.z : 0u;
    result ^= (index & 0x08u) ? lo.w : 0u;
    result ^= (index & 0x10u) ? hi.x : 0u;
    result ^= (index & 0x20u) ? hi.y : 0u;
    result ^= (index & 0x40u) ? hi.z : 0u;
    result ^= (index & 0x80u) ? hi.w : 0u;
    col += 8;
    for (index >>= 8; index; index >>= 1, ++col)
        if (index & 1u)
            result ^= *col;
    return result;
}
// SobolPathSampler::next1D (SobolPathSampler.hpp:64-69) when QMC and the path runs the Sobol' sampler
template<bool QMC>
PT_DEV float rngNext1DT(Rng &r)
{
    if (QMC && r.sobol != nullptr && r.dim < TGHIP_SOBOL_DIMS) {
        uint32_t permuted = (r.index & ~0xFFu) | ((r.index + r.scramble) & 0xFFu);   // permutedIndex() :20-23
        return __uint_as_float((sobolSample(r.sobol, permuted, r.dim++, r.scramble) >> 9u) | 0x3F800000u) - 1.0f;
    }
    return rngNext1D(r);
}

/* ---- sample warps (sampling/SampleWarp.hpp) ---- */
PT_DEV f3 cosineHemisphere(float xi0, float xi1)
{
    float phi = xi0*PT_TWO_PI;
    float r = sqrtf(xi1);
    float sinPhi, cosPhi;
    sincosfH(phi, sinPhi, cosPhi);
    return mk3(cosPhi*r, sinPhi*r, sqrtf(fmaxf(1.0f - xi1, 0.0f)));
}
PT_DEV float cosineHemispherePdf(f3 p) { return fabsf(p.z)*PT_INV_PI; }
PT_DEV f3 uniformHemisphere(float xi0, float xi1)      /* SampleWarp.hpp:25-30 */
{
    float phi = PT_TWO_PI*xi0;
    float r = sqrtf(fmaxf(1.0f - xi1*xi1, 0.0f));
    return mk3(cosfH(phi)*r, sinfH(phi)*r, xi1);
}
PT_DEV f3 uniformSphere(float xi0, float xi1)
{
    float phi = xi0*PT_TWO_PI;
    float z = xi1*2.0f - 1.0f;
    float r = sqrtf(fmaxf(1.0f - z*z, 0.0f));
    float sinPhi, cosPhi;
    sincosfH(phi, sinPhi, cosPhi);
    return mk3(cosPhi*r, sinPhi*r, z);
}
PT_DEV float powerHeuristic(float pdf0, float pdf1) { return (pdf0*pdf0)/(pdf0*pdf0 + pdf1*pdf1); }

#endif
