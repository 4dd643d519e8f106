// Stand-alone sanitizer run of the host-side launch choice (tungsten_amd/csrc/host/LaunchChoice.cpp), no device and no Python:
//
//     g++ -std=c++11 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/launch_choice_check.cpp tungsten_amd/csrc/host/LaunchChoice.cpp \
//         tungsten_amd/csrc/host/SceneCheck.cpp -o tools/bin/launch_choice_check
//     tools/bin/launch_choice_check
//
// chooseLaunches over EVERY combination of the boolean scene traits and the kinds of a pass, under every option alone and the pairs of the options that steer
// the same branches, for a handful of depth and class settings.
// Checked per combination: the LDS formula of a walk launch belongs to the kernel's family; a wide kernel runs only on a scene with a wide BVH; the shadow walk
// is a closest-hit walk exactly when the scene has a forward lobe or a mesh emitter; the LDS bytes of every formula are those of a restatement here; k_shade_fused only with exactly one further class that a pair covers; every
// class present has exactly one shading launch, of a family that covers the class's types; k_tail only where the loop's kernels are the ones its body is
// built from.  Exit 0 without a report is the result; the number of combinations is printed.
#include "../tungsten_amd/csrc/host/LaunchChoice.hpp"

#include <cstdio>
#include <cstdlib>

namespace {

long g_cases = 0;

#define REQUIRE(cond)                                                                                         \
    do {                                                                                                      \
        if (!(cond)) {                                                                                        \
            std::fprintf(stderr, "launch_choice_check: case %ld, line %d: %s\n", g_cases, __LINE__, #cond); \
            std::exit(1);                                                                                     \
        }                                                                                                     \
    } while (0)

bool isWide(KernelFamily f)
{
    return f == K_CLOSEST_WIDE || f == K_FINISH_CLOSEST_WIDE || f == K_CLOSEST_INSTW || f == K_SHADOW_WIDE || f == K_SHADOW_FAST || f == K_SHADOW_FAST_INST;
}

LdsFormula formulaOf(KernelFamily f)
{
    switch (f) {
    case K_CLOSEST: case K_SHADOW:                       return LDS_TRACE;
    case K_CLOSEST_DYN: case K_CLOSEST_INST: case K_SHADOW_DYN: return LDS_DYN;
    case K_CLOSEST_INSTW:                                return LDS_INST_WIDE;
    case K_CLOSEST_WIDE: case K_FINISH_CLOSEST_WIDE: case K_SHADOW_WIDE: case K_SHADOW_FAST: case K_SHADOW_FAST_INST: return LDS_WIDE;
    default:                                             return LDS_NONE;
    }
}

// Dynamic LDS bytes of a walk launch of t threads, from the kernels' use of it (csrc/hip/pt_wavefront.h): the expanded queue takes 2 bytes per slot of the
// workgroup; a BVH2 walk keeps one 4-byte stack entry per tree level and thread, a wide walk one 8-byte group entry per level of the wide tree and thread.
size_t restatedLds(const SceneTraits &sc, const LaunchChoice &c, LdsFormula f, size_t t)
{
    const size_t queue = 2u*c.slotCap, bvh = size_t(sc.bvhDepth > 1 ? sc.bvhDepth : 1), wide = size_t(sc.wideDepth > 1 ? sc.wideDepth : 1);
    if (f == LDS_TRACE) {                  // the static-fetch walks read the queue out before they push: stack and queue share the bytes; a flat list has no stack
        const size_t stack = c.flat ? 0u : 4u*bvh*t;
        return stack > queue ? stack : queue;
    }
    if (f == LDS_DYN) return queue + 4u*bvh*t;     // the dynamic-fetch walks fetch while they walk: side by side
    if (f == LDS_WIDE) return queue + 8u*wide*t;
    if (f == LDS_INST_WIDE) {              // half a word per slot + the BVH2 stack of the levels above the masters, rounded up to 8 bytes, + the masters' group stacks
        const int above = sc.bvhDepth - sc.bvhMasterDepth;
        size_t words = c.slotCap/2u + size_t(above > 1 ? above : 1)*t;
        words += words & 1u;
        return 4u*words + 8u*size_t(sc.wideMasterDepth > 1 ? sc.wideMasterDepth : 1)*t;
    }
    return 0;
}

// the type sets of the class settings: what a class's materials hold (bit = 1 << TGHIP_BSDF_*)
struct Classes { bool present[PT_NUM_CLASSES]; uint32_t mask[PT_NUM_CLASSES]; };
const uint32_t T0 = BSDF_BIT(TGHIP_BSDF_LAMBERT), T1 = BSDF_BIT(TGHIP_BSDF_ROUGH_CONDUCTOR), T2 = BSDF_BIT(TGHIP_BSDF_DIELECTRIC),
               T3P = BSDF_BIT(TGHIP_BSDF_PLASTIC), T3F = BSDF_BIT(TGHIP_BSDF_PLASTIC) | BSDF_BIT(TGHIP_BSDF_PHONG);
const Classes CLASS_SETTINGS[] = {
    {{true, false, false, false}, {T0, 0, 0, 0}},     {{true, true, false, false}, {T0, T1, 0, 0}},   {{true, false, true, false}, {T0, 0, T2, 0}},
    {{true, false, false, true}, {T0, 0, 0, T3P}},    {{true, false, false, true}, {T0, 0, 0, T3F}}, {{true, true, true, true}, {T0, T1, T2, T3P}},
    {{false, true, false, true}, {0, T1, 0, T3F}},
};
struct Depths { uint32_t numRecs; int bvh, wide, bvhMaster, wideMaster; uint32_t wideNodes; };
const Depths DEPTH_SETTINGS[] = {{8, 0, 0, 0, 0, 0}, {16, 5, 0, 0, 0, 0}, {17, 6, 0, 0, 0, 0}, {200, 9, 3, 0, 0, 40}, {100000, 24, 7, 0, 0, 40000}, {300, 20, 5, 8, 3, 90}};

int variantOfMask(uint32_t mask)
{
    mask &= ~(FEAT_QMC | FEAT_INSTANCES);
    for (int v = 0; v < TGHIP_BSDF_VARIANT_COUNT; ++v)
        if ((familyMask(uint32_t(v)) & ~FEAT_INSTANCES) == mask) return v;
    return -1;
}

void check(const SceneTraits &sc, const Depths &d, const LaunchOptions &o, const PassKind &pass)
{
    ++g_cases;
    LaunchChoice c;
    chooseLaunches(sc, d.numRecs, d.wideNodes, o, pass, c);
    const bool closestWalk = sc.haveForward || sc.haveMeshLight;
    REQUIRE(c.flat == (d.numRecs <= TGHIP_FLAT_MAX_RECS && !sc.haveInstances));
    REQUIRE(c.blocksPerCu >= 1 && c.blocksPerCu <= 8 && c.parts >= 1 && c.parts <= 8);
    REQUIRE(c.slotCap >= 64 && c.slotCap <= PT_MAX_SLOTS_PER_BLOCK);
    // the walks
    const WalkLaunch *walks[2] = {&c.closest, &c.shadow};
    for (int i = 0; i < 2; ++i) {
        const WalkLaunch &w = *walks[i];
        REQUIRE(!kernelName(w.kernel).empty() && !kernelName(w.size.sizedBy).empty());
        REQUIRE(w.lds == formulaOf(w.kernel.family) && w.size.lds == formulaOf(w.size.sizedBy.family));
        REQUIRE(!isWide(w.kernel.family) || sc.wideDepth > 0);
        REQUIRE(!isWide(w.size.sizedBy.family) || sc.wideDepth > 0);
        REQUIRE(w.kernel.count == pass.countTraversal || (w.kernel.family == K_SHADOW_WIDE && !w.kernel.join));
        REQUIRE(!w.size.sizedBy.count);
        REQUIRE(w.size.fixed == 0 || (w.size.fixed % 64 == 0 && w.size.fixed >= 64 && w.size.fixed <= 512));
        REQUIRE(w.size.maxThreads >= 128 && w.size.maxThreads <= 512);
        if (w.kernel.family == K_CLOSEST || w.kernel.family == K_SHADOW) {
            REQUIRE(w.kernel.flat == c.flat && (w.kernel.inst != 0) == sc.haveInstances);
            REQUIRE(w.kernel.inst == 0 || w.kernel.inst == (sc.haveSolids ? 1 : 2));
        } else {
            REQUIRE(w.kernel.solids == sc.haveSolids || (w.kernel.family == K_SHADOW_WIDE && !w.kernel.join));
        }
    }
    REQUIRE((c.closest.kernel.family == K_CLOSEST_INSTW || c.closest.kernel.family == K_CLOSEST_INST) ? sc.haveInstances : true);
    REQUIRE(c.closest.kernel.family != K_CLOSEST_INSTW || sc.wideMasterDepth > 0);
    // a closest-hit shadow walk exactly when shadow rays pick up transmittance or may end on a mesh emitter
    REQUIRE((c.shadow.kernel.family == K_SHADOW && c.shadow.kernel.forward) == closestWalk);
    REQUIRE(c.neeFactors == closestWalk);
    REQUIRE((c.shadow.kernel.family == K_SHADOW && c.shadow.kernel.mask == BSDF_MASK_ALL) == (closestWalk && (sc.haveProcTex || sc.haveFibre)));
    REQUIRE(!pass.aux || c.shadow.kernel.family == K_SHADOW);
    REQUIRE(c.foldFinish == (c.closest.kernel.family == K_FINISH_CLOSEST_WIDE));
    REQUIRE(!c.foldFinish || !sc.cameraFix);
    // the shape of the loop
    REQUIRE(!c.oneLaunch || (c.fusedFlat && !sc.haveComplex));
    REQUIRE(!c.fusedFlat || (c.flat && !closestWalk && !pass.aux && !sc.allFeaturesShading && c.tablesFit && !sc.cameraFix));
    REQUIRE(!c.paired || (!c.flat && c.wideShadowRays));
    REQUIRE(!c.pairedInst || (c.paired && sc.haveInstances));
    REQUIRE(!c.flat || c.parts == 1);
    // shading
    REQUIRE(c.numShade >= 1 && c.numShade <= 2 + PT_NUM_CLASSES);
    int further = 0, lastFurther = 0;
    for (int k = 1; k < PT_NUM_CLASSES; ++k)
        if (sc.classPresent[k]) { ++further; lastFurther = k; }
    if (c.fusedPair) {
        REQUIRE(further == 1 && c.fusedPair == lastFurther && c.numShade == 1 && c.shade[0].kernel.family == K_SHADE_FUSED && c.shadeLaunches == 1);
        REQUIRE(familyCovers(uint32_t(c.shade[0].variant), sc.classMask[lastFurther], false));
        REQUIRE(c.shade[0].variant == TGHIP_BSDF_VARIANT_COAT || c.shade[0].variant == TGHIP_BSDF_VARIANT_GLASS || c.shade[0].variant == TGHIP_BSDF_VARIANT_PLASTIC);
        REQUIRE(!c.flat && !sc.haveInstances && c.tablesFit && !pass.aux);
    }
    int perClass[PT_NUM_CLASSES] = {0, 0, 0, 0}, miss = 0;
    for (int i = 0; i < c.numShade && !c.fusedPair; ++i) {
        const ShadeLaunch &l = c.shade[i];
        REQUIRE(l.kernel.family == K_SHADE && !kernelName(l.kernel).empty());
        REQUIRE(l.variant == variantOfMask(l.kernel.mask) || (l.kernel.mask == MASK_MEDIA && l.variant == TGHIP_BSDF_VARIANT_MEDIA));
        REQUIRE(l.kernel.globalTables == !c.tablesFit);
        REQUIRE((l.kernel.fuse != 0) == c.fusedFlat && (l.lane == 0 || o.classStreamsOpt != 0) && l.lane >= 0 && l.lane <= 2);
        REQUIRE(((l.kernel.mask & FEAT_QMC) != 0) == pass.qmc || l.variant == TGHIP_BSDF_VARIANT_ALL || l.variant == TGHIP_BSDF_VARIANT_MEDIA);
        if (l.cls == CLS_MISS) ++miss;
        else if (l.cls == CLS_0_AND_MISS) { ++miss; ++perClass[0]; }
        else { REQUIRE(l.cls >= 0 && l.cls < PT_NUM_CLASSES); ++perClass[l.cls]; }
        // the family covers the types of the class it shades (a forward lobe: class 3, or the all-features / media / full families)
        const int cls = l.cls == CLS_0_AND_MISS ? 0 : l.cls;
        if (cls < PT_NUM_CLASSES && sc.classPresent[cls] && l.variant != TGHIP_BSDF_VARIANT_MEDIA && l.variant != TGHIP_BSDF_VARIANT_LEAN)
            REQUIRE(familyCovers(uint32_t(l.variant), sc.classMask[cls], false));
        REQUIRE(!pass.aux || l.variant == TGHIP_BSDF_VARIANT_ALL);
        REQUIRE(!(sc.haveMedia || sc.allFeaturesShading) || l.variant == TGHIP_BSDF_VARIANT_ALL || l.variant == TGHIP_BSDF_VARIANT_MEDIA);
        REQUIRE(!sc.haveMeshLight || l.variant == TGHIP_BSDF_VARIANT_FULL || l.variant == TGHIP_BSDF_VARIANT_ALL);
    }
    if (!c.fusedPair) {
        REQUIRE(perClass[0] == 1 && miss == (c.fusedFlat ? 0 : 1));           // (fused flat lists shade the escaped paths inside the class-0 launch)
        for (int k = 1; k < PT_NUM_CLASSES; ++k)
            REQUIRE(perClass[k] == (sc.classPresent[k] ? 1 : 0));
    }
    // k_tail: where runBatch let it run before the choice was host code
    const bool tailWas = o.tailOpt && !sc.cameraFix && c.tablesFit && !c.flat && !sc.haveInstances && c.wideClosest && c.wideShadowRays && o.decoupleOpt &&
                         familyCovers(TGHIP_BSDF_VARIANT_TAIL, sc.complexMask, sc.haveForward) && !sc.haveMeshLight && !sc.haveMedia && !pass.aux &&
                         !sc.allFeaturesShading && !pass.countTraversal;
    REQUIRE(c.tailEligible == tailWas);
    if (c.tailEligible) {
        REQUIRE(c.closest.kernel.family == K_FINISH_CLOSEST_WIDE || (c.closest.kernel.family == K_CLOSEST_WIDE && c.closest.kernel.decoupled));
        REQUIRE(c.shadow.kernel.family == K_SHADOW_FAST && !closestWalk);
        REQUIRE(!kernelName(c.tail).empty() && !kernelName(c.tailProbe).empty());
        REQUIRE((c.tail.mask & ~FEAT_QMC) == MASK_TAIL || ((c.tail.mask & ~FEAT_QMC) == MASK_COAT && !sc.haveSolids && !sc.classPresent[2] && !sc.classPresent[3]));
    }
    // the ray queries
    REQUIRE((c.rayWalk == LaunchChoice::RAYS_WIDE) == (c.useWide && !sc.haveInstances));
    REQUIRE(c.rayWalk != LaunchChoice::RAYS_WIDE || sc.wideDepth > 0);
    REQUIRE((c.rayWalk == LaunchChoice::RAYS_FLAT) == (c.flat && !c.useWide));
    // the flat record
    TgHipLaunchChoice flat;
    exportLaunchChoice(c, &flat);
    REQUIRE(flat.num_shade == c.numShade && flat.parts == c.parts && (flat.tail[0] != 0) == c.tailEligible);
    // the dynamic LDS of every formula, restated from what the kernels keep there (restatedLds above), at the workgroup sizes the plan may pick
    for (int t = 64; t <= 512; t += 64)
        for (int f = LDS_NONE; f <= LDS_INST_WIDE; ++f)
            REQUIRE(ldsBytes(sc, c, LdsFormula(f), t) == restatedLds(sc, c, LdsFormula(f), size_t(t)));
}

} // namespace

int main()
{
    // boolean traits: instances, solids, forward, mesh light, all-features shading, procedural texture, fibre, media, simple media, lean scene, camera fix, tables fit
    const int NT = 12;
    // options, each against its default: every one alone, and every pair of the first NPAIR -- the ones that steer the same branches (all combinations x
    // traits x passes would be 10^12 cases)
    static const char *const KEYS[] = {"wide_bvh", "wide_closest", "wide_shadow", "dynamic_fetch", "inst_dyn", "inst_wide", "inst_shadow_fast", "decouple",
                                       "fold_finish", "fuse_flat", "shade_fused", "merge_miss", "class_streams", "lds_tables", "streams", "blocks_per_cu",
                                       "inst_shadow_join", "inst_simple", "run_to_completion", "media_lean", "tail_kernel", "tail_family", "slots_per_block"};
    static const long long TOGGLED[] = {0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 4, 0, 0, 0, 0, 0, 0, 128};
    const int NK = int(sizeof KEYS/sizeof KEYS[0]), NPAIR = 16;
    for (const Depths &d : DEPTH_SETTINGS)
        for (const Classes &cl : CLASS_SETTINGS)
            for (int tb = 0; tb < (1 << NT); ++tb) {
                SceneTraits sc;
                sc.haveInstances = tb & 1; sc.haveSolids = tb & 2; sc.haveForward = tb & 4; sc.haveMeshLight = tb & 8; sc.allFeaturesShading = tb & 16;
                sc.haveProcTex = tb & 32; sc.haveFibre = tb & 64; sc.haveMedia = tb & 128; sc.mediaSimple = tb & 256; sc.leanScene = tb & 512;
                sc.cameraFix = tb & 1024; sc.tablesFit = !(tb & 2048);
                // (what checkScene never reports together: instances without a two-level tree or on a flat list, procedural textures / fibres / media without
                // their all-features or forward flag, simple media with instances or mesh emitters, a lean scene with instances, meshes or further features)
                if (sc.haveInstances != (d.bvhMaster > 0)) continue;
                if ((sc.haveProcTex || sc.haveFibre) && !sc.allFeaturesShading) continue;
                if (sc.haveMedia && !sc.haveForward) continue;
                if (sc.mediaSimple && (!sc.haveMedia || sc.haveInstances || sc.haveMeshLight)) continue;
                if (sc.leanScene && (sc.haveInstances || sc.haveMeshLight || sc.haveMedia || sc.allFeaturesShading)) continue;
                sc.bvhDepth = d.bvh; sc.wideDepth = d.wide; sc.bvhMasterDepth = d.bvhMaster; sc.wideMasterDepth = d.wideMaster;
                for (int k = 0; k < PT_NUM_CLASSES; ++k) {
                    sc.classPresent[k] = cl.present[k]; sc.classMask[k] = cl.mask[k];
                    if (k) { sc.haveComplex = sc.haveComplex || cl.present[k]; sc.complexMask |= cl.mask[k]; }
                }
                for (int a = -1; a < NK; ++a)
                    for (int b = a; b < NK; ++b) {
                        if (a >= 0 && (b == a || b >= NPAIR)) continue;          // (a = -1: the defaults, then every option alone; else the pairs)
                        LaunchOptions o;
                        if (a >= 0) REQUIRE(setLaunchOption(o, KEYS[a], TOGGLED[a]));
                        if (b >= 0) REQUIRE(setLaunchOption(o, KEYS[b], TOGGLED[b]));
                        for (int pb = 0; pb < 16; ++pb) {
                            PassKind pass;
                            pass.aux = pb & 1; pass.shortBatch = pb & 2; pass.qmc = (pb & 4) || pass.aux || sc.haveMedia; pass.countTraversal = pb & 8;
                            check(sc, d, o, pass);
                        }
                    }
            }
    LaunchOptions o;
    REQUIRE(!setLaunchOption(o, "max_slots", 1) && !setLaunchOption(o, "", 1));
    std::printf("launch_choice_check: %ld combinations, no report\n", g_cases);
    return 0;
}
