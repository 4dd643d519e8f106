// The BSDF type / scene feature masks of the kernel variants and the limits the upload decides by: preprocessor arithmetic over the ABI enums of
// include/tungsten_hip.h and one plain function, no HIP types -- read by the kernels (pt_scene.h, pt_kernels.h, pt_wavefront.h) and, compiled
// by the host compiler, by csrc/host/SceneCheck.cpp, which sorts a scene's materials into the families named here.
#ifndef TGAMD_PT_VARIANTS_H_
#define TGAMD_PT_VARIANTS_H_

#include "../../../include/tungsten_hip.h"

#ifdef __HIPCC__
#define PT_HOST_DEVICE __host__ __device__
#else
#define PT_HOST_DEVICE
#endif

#define PT_MAX_BSDF_DEPTH 3

// M is the compile-time set of BSDF types (bit = 1 << TGHIP_BSDF_*) a kernel variant has to handle: cases
// outside M fold away, which is what keeps the Lambert-only shading kernel small (DESIGN.md "Kernels").
#define BSDF_BIT(t) (1u << (t))
#define BSDF_MASK_ALL 0xFFFFFFFFu
// The upper bits of M say which scene FEATURES a shading-kernel variant has to handle (all set in BSDF_MASK_ALL);
// code for absent features folds away like BSDF types do.
#define FEAT_BITMAP     (1u << 24)   /* bitmap textures (incl. environment maps)                      */
#define FEAT_INFINITE   (1u << 25)   /* infinite-sphere emitters                                       */
#define FEAT_MULTILIGHT (1u << 26)   /* more than one sampled light (TraceBase::chooseLight's pdf loop) */
#define FEAT_TRIANGLES  (1u << 27)   /* triangle records (attribute gather, smooth normals)            */
#define FEAT_SOLIDS     (1u << 28)   /* sphere records; sphere / cube emitters as sampled lights       */
#define FEAT_ALL        (FEAT_BITMAP | FEAT_INFINITE | FEAT_MULTILIGHT | FEAT_TRIANGLES | FEAT_SOLIDS)
#define FEAT_MESHLIGHT  (1u << 29)   /* triangle-mesh emitters as sampled lights: only in the MASK_FULL / BSDF_MASK_ALL variants */
#define FEAT_QMC        (1u << 30)   /* TGHIP_PASS_SOBOL / TGHIP_PASS_RECORDS passes: every variant has a twin with this bit (csrc/host/LaunchChoice.cpp) */
#define FEAT_INSTANCES  (1u << 31)   /* hits reached through an instance record (primitives/Instance.cpp): only in MASK_FULL / BSDF_MASK_ALL */
#define FEAT_MEDIA      (1u << 23)   /* participating media (media/HomogeneousMedium.cpp): only in the BSDF_MASK_ALL variant */
#define FEAT_AUX        (1u << 22)   /* TGHIP_PASS_AUX passes (auxiliary output buffers): only in the BSDF_MASK_ALL variant */
#define FEAT_CYLINDER   (1u << 21)   /* cylinder primitives / emitters (primitives/Cylinder.cpp): only in the BSDF_MASK_ALL variant */
#define FEAT_PHONG      (1u << 19)   /* microfacet BSDFs with the Phong distribution (pow(double, double)): only in the MASK_FULL / BSDF_MASK_ALL variants */
#define FEAT_BUMP       (1u << 20)   /* bump-mapped shading frames (Primitive::setupTangentFrame, TgHipBsdf::bump1): only in the BSDF_MASK_ALL variant */
#define MASK_FULL       (BSDF_MASK_ALL & ~(FEAT_QMC | FEAT_MEDIA | FEAT_AUX | FEAT_CYLINDER | FEAT_BUMP))
// The marker of the all-features family: the four feature bits that only BSDF_MASK_ALL (and its FEAT_QMC twin, which it is itself) carries together.
// Code for the procedural `disk` and `blade` textures (TGHIP_TEX_DISK / TGHIP_TEX_BLADE) is compiled only where all four are set -- the mask has no
// bit left for a FEAT_ of their own, and a scene that holds one is shaded by that family throughout (SceneCheck.hpp: haveProcTex).  The closest-hit
// shadow walk of scenes WITHOUT such a texture instantiates its BSDF code with MASK_ALL_NO_PROCTEX: no function it calls looks at FEAT_AUX, so
// its instructions are those of BSDF_MASK_ALL before these textures existed.
#define FEAT_FAMILY_ALL (FEAT_MEDIA | FEAT_AUX | FEAT_CYLINDER | FEAT_BUMP)
#define HAS_PROCTEX(M)  ((((M) & FEAT_FAMILY_ALL)) == FEAT_FAMILY_ALL)
#define MASK_ALL_NO_PROCTEX (BSDF_MASK_ALL & ~FEAT_AUX)
// The two fibre BCSDFs (TGHIP_BSDF_LAMBERTIAN_FIBER = 19, TGHIP_BSDF_ROUGH_WIRE = 20) live by the same rule: bits 19 and 20 of M are FEAT_PHONG and FEAT_BUMP, so
// BSDF_BIT is never formed for them; their code, and the shading frame from a primitive's tangent space that their anisotropic lobes ask for, is compiled
// only where the marker is set, and a scene that holds one is shaded by that family throughout and keeps the loop to the end, as TYPES_LATE scenes do
// (SceneCheck.hpp: haveFibre).  MASK_ALL_NO_PROCTEX has neither.
#define HAS_FIBRE(M)    HAS_PROCTEX(M)

// BSDF type sets of the shading-kernel variants (pt_scene.h BsdfOps<D, M>)
#define TYPES_SIMPLE (BSDF_BIT(TGHIP_BSDF_LAMBERT) | BSDF_BIT(TGHIP_BSDF_NULL) | BSDF_BIT(TGHIP_BSDF_ERROR))
#define MASK_SIMPLE  (TYPES_SIMPLE | FEAT_ALL)
#define MASK_LEAN    TYPES_SIMPLE        /* analytic primitives, constant/checker textures, one area light (Cornell box) */
#define MASK_SIMPLE_INST (MASK_SIMPLE | FEAT_INSTANCES)   /* classes 0 and 2 of scenes with instance records (no mesh emitters) */
#define MASK_COAT    (MASK_SIMPLE | BSDF_BIT(TGHIP_BSDF_ROUGH_CONDUCTOR) | BSDF_BIT(TGHIP_BSDF_SMOOTH_COAT) | \
                      BSDF_BIT(TGHIP_BSDF_MIRROR) | BSDF_BIT(TGHIP_BSDF_CONDUCTOR))
#define MASK_GLASS   (MASK_SIMPLE | BSDF_BIT(TGHIP_BSDF_DIELECTRIC) | BSDF_BIT(TGHIP_BSDF_ROUGH_DIELECTRIC) | \
                      BSDF_BIT(TGHIP_BSDF_MIRROR))
#define MASK_PLASTIC (MASK_SIMPLE | BSDF_BIT(TGHIP_BSDF_PLASTIC) | BSDF_BIT(TGHIP_BSDF_ROUGH_PLASTIC))
/* media scenes whose surfaces are Lambert / null / forward / (smooth) dielectric / mirror -- every media scene the reference ships and the
   fog / smoke goldens: 216 VGPRs without scratch where BSDF_MASK_ALL spills 292 registers to 848 B of scratch.  (Always the FEAT_QMC twin:
   media passes carry PT_PASS_MEDIA in their flags.) */
#define MASK_MEDIA   (MASK_SIMPLE | FEAT_MEDIA | FEAT_QMC | BSDF_BIT(TGHIP_BSDF_FORWARD) | BSDF_BIT(TGHIP_BSDF_DIELECTRIC) | BSDF_BIT(TGHIP_BSDF_MIRROR))
/* the five types added last (ABI 9): only the full variants shade them; scenes that use one keep the loop to the end (no k_tail) */
#define TYPES_LATE   (BSDF_BIT(TGHIP_BSDF_DIFFUSE_TRANSMISSION) | BSDF_BIT(TGHIP_BSDF_PHONG) | BSDF_BIT(TGHIP_BSDF_THINSHEET) | \
                      BSDF_BIT(TGHIP_BSDF_OREN_NAYAR) | BSDF_BIT(TGHIP_BSDF_ROUGH_COAT))
#define MASK_TAIL    (MASK_FULL & ~(FEAT_INSTANCES | FEAT_MESHLIGHT | TYPES_LATE))   /* k_tail: the 14 BSDF types of rounds 1-3, single-level scenes without mesh emitters */
/* the class variants of scenes with instance records (no mesh emitters): hits reached through an instance (FEAT_INSTANCES) */
#define MASK_COAT_INST    (MASK_COAT | FEAT_INSTANCES)
#define MASK_GLASS_INST   (MASK_GLASS | FEAT_INSTANCES)
#define MASK_PLASTIC_INST (MASK_PLASTIC | FEAT_INSTANCES)

// The shading families by their ABI number (TGHIP_BSDF_VARIANT_*) and mask: the ONE table behind familyMask (csrc/host/SceneCheck.cpp) and the
// instantiations of the per-call debug kernels (csrc/hip/debug_units.hip) -- a family added here is in both.
#define PT_FAMILY_VARIANTS(X) \
    X(TGHIP_BSDF_VARIANT_LEAN, MASK_LEAN) X(TGHIP_BSDF_VARIANT_SIMPLE, MASK_SIMPLE) X(TGHIP_BSDF_VARIANT_COAT, MASK_COAT) \
    X(TGHIP_BSDF_VARIANT_GLASS, MASK_GLASS) X(TGHIP_BSDF_VARIANT_PLASTIC, MASK_PLASTIC) X(TGHIP_BSDF_VARIANT_MEDIA, MASK_MEDIA) \
    X(TGHIP_BSDF_VARIANT_TAIL, MASK_TAIL) X(TGHIP_BSDF_VARIANT_FULL, MASK_FULL) X(TGHIP_BSDF_VARIANT_ALL, BSDF_MASK_ALL)

// most media of a scene: the path's medium travels as index + 1 in seven bits of the slot flags (pt_kernels.h: FLAG_MEDIUM)
#define PT_MAX_MEDIA 126u

// Shading classes ("sort by material"): the class of a record's BSDF says which k_shade variant shades a hit on it -- 0: Lambert / null
// (MASK_SIMPLE), 1: the conductor family (MASK_COAT: rough conductor, conductor, mirror, smooth coat over those), 2: the dielectric
// family (MASK_GLASS: dielectric, rough dielectric), 3: everything else (plastics, mixed, transparency, forward: MASK_PLASTIC when that
// covers them, else every type); CLS_MISS: the path's ray left the scene.  One queue and one launch per class that occurs in the scene.
#define PT_NUM_CLASSES 4

// What the host-side launch choice (csrc/host/LaunchChoice.cpp) reads next to the masks above: the queue indices of a k_shade launch, the FUSE bits of
// the flat lists' launches, the waves per SIMD of the shading variants (a template argument, so part of a kernel's name) and the slot limit of a workgroup.
// the shading classes (pt_variants.h: PT_NUM_CLASSES) as queue indices; CLS_MISS: the path's ray left the scene
#define CLS_MISS 4
#define CLS_0_AND_MISS 5   /* a k_shade launch that consumes the queue of class 0 and, behind it, the escaped paths' (same shading variant) */
#define FUSE_TRACE  1
#define FUSE_SHADOW 2
#define FUSE_LOOP   4
// waves per SIMD the shading-kernel variants are bounded for (their BSDF type sets: pt_variants.h)
#ifndef SIMPLE_WAVES
#define SIMPLE_WAVES 3   /* measured: 4 waves/SIMD (128 VGPRs, spills) is 10 % slower on materialtest's k_shade */
#endif
#ifndef COAT_WAVES
#define COAT_WAVES   3   /* round 4, without Phong's pow(double) in the family variants (197 VGPRs at 2 waves/SIMD; 168 + 72 B of scratch at 3):
                            materialtest 968.3 / 969.4 -> 977.8 / 974.5, mesh1m 616.9 / 614.2 -> 622.7 / 621.7 Msamples/s (two libraries alternated
                            twice in one session, profiles/r4_ab_coat_waves.txt); round 3 had measured 3 waves as neutral at 223 VGPRs */
#endif
#ifndef LEAN_WAVES
#define LEAN_WAVES   2   /* measured: 2 waves/SIMD without scratch beats 3 with 108 B of scratch (kernel is VALU-bound) */
#endif
#ifndef PT_MAX_SLOTS_PER_BLOCK
#define PT_MAX_SLOTS_PER_BLOCK 4096u
#endif

// Guide tables (built at upload, SceneCheck.cpp) make the two CDF inversions of Distribution2D::warp short dependent
// chains instead of 9- and 10-step binary searches over L2-resident arrays: for a CDF a[0..n] and B buckets,
// g[b] = upper_bound(a, b/B), so for x in [b/B, (b+1)/B) the answer lies in [g[b], g[b+1]].  B is a power of two
// (x*B is exact), and the final search inside the window is the same upper_bound, so the result is identical.
#define PT_GUIDE_MARGINAL 512
#define PT_GUIDE_ROW      256

// ---- small scene tables in LDS --------------------------------------------------------------------
// The shading kernels chase object -> bsdf -> texture -> light records per lane.  Those tables are tiny, but the
// vector L1 is flushed continuously by the streaming path state, so every dependent lookup pays L2 latency.
// Each workgroup copies them into LDS once and the lookups become LDS reads (the big arrays -- records, attributes,
// texels, CDFs -- stay in global memory).
// Round 5: the copy is UNCONDITIONAL.  With the run-time fallback "too large: keep the global tables" every table pointer was a select
// of an LDS and a global address, so the compiler could not infer the address space and every lookup became a flat_load -- 315 of them in
// the class-0 variant, each behind an `s_waitcnt vmcnt(0) lgkmcnt(0)` that also drains every global load in flight (235 such waits).
// Whether the tables fit is decided by the host at upload (SceneCheck.cpp: tablesFit, by the function below); scenes whose
// tables do not fit shade with the GLOBAL_TABLES instantiation of the all-features variant, which does not stage at all.  The sampled
// environment map's marginal tables come along when env_tex >= 0 (the host clears env_tex when they do not fit next to the rest).
#define PT_LDS_TABLE_BYTES 12288u
struct SceneTableLayout { uint32_t offBsdf, offTex, offLights, offEnv, offEnvG, total; };
PT_HOST_DEVICE inline SceneTableLayout sceneTableLayout(uint32_t numObjects, uint32_t numBsdfs, uint32_t numTextures, uint32_t numLights, uint32_t numInfinite, int envH)
{
    SceneTableLayout l;
    const uint32_t szObj = numObjects*(uint32_t)sizeof(TgHipObject), szBsdf = numBsdfs*(uint32_t)sizeof(TgHipBsdf), szTex = numTextures*(uint32_t)sizeof(TgHipTexture);
    const uint32_t szLights = (numLights + numInfinite)*(uint32_t)sizeof(int32_t);
    l.offBsdf = (szObj + 15u) & ~15u;
    l.offTex = (l.offBsdf + szBsdf + 15u) & ~15u;
    l.offLights = (l.offTex + szTex + 15u) & ~15u;
    // the marginal tables of the sampled environment map (mpdf[h] mcdf[h + 1], then its 513-entry guide): the head of the
    // envmap-sampling chain becomes LDS reads
    l.offEnv = (l.offLights + szLights + 15u) & ~15u;
    const uint32_t szEnvF = envH > 0 ? (2u*(uint32_t)envH + 1u)*4u : 0u, szEnvG = envH > 0 ? (PT_GUIDE_MARGINAL + 1u)*2u : 0u;
    l.offEnvG = (l.offEnv + szEnvF + 3u) & ~3u;
    l.total = envH > 0 ? ((l.offEnvG + szEnvG + 3u) & ~3u) : l.offLights + szLights;
    return l;
}

#endif
