#include "LaunchChoice.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

bool setLaunchOption(LaunchOptions &o, const std::string &k, long long value)
{
    const bool on = value != 0;
    auto clamp = [&](long long lo, long long hi) { return int(std::min(std::max(value, lo), hi)); };
    if (k == "wide_bvh") o.wideOpt = on;
    else if (k == "wide_closest") o.wideClosestOpt = value < 0 ? -1 : on;
    else if (k == "wide_shadow") o.wideShadowOpt = value < 0 ? -1 : on;
    else if (k == "dynamic_fetch") o.dynamicFetch = on;
    else if (k == "inst_dyn") o.instDynOpt = on;
    else if (k == "inst_wide") o.instWideOpt = on;
    else if (k == "inst_shadow_fast") o.instShadowFast = on;
    else if (k == "inst_shadow_join") o.instShadowJoin = on;
    else if (k == "inst_simple") o.instSimpleOpt = on;
    else if (k == "decouple") o.decoupleOpt = on;
    else if (k == "fold_finish") o.foldFinishOpt = on;
    else if (k == "fuse_flat") o.fuseFlatOpt = on;
    else if (k == "run_to_completion") o.loopOpt = on;
    else if (k == "shade_fused") o.shadeFusedOpt = on;
    else if (k == "merge_miss") o.mergeMissOpt = on;
    else if (k == "class_streams") o.classStreamsOpt = on;
    else if (k == "media_lean") o.mediaLeanOpt = on;
    else if (k == "tail_kernel") o.tailOpt = on;
    else if (k == "tail_family") o.tailFamilyOpt = on;
    else if (k == "lds_tables") o.ldsTables = on;
    else if (k == "streams") o.streamsOpt = clamp(0, 8);
    else if (k == "blocks_per_cu") o.blocksPerCuOpt = clamp(0, 8);
    else if (k == "slots_per_block") o.slotsPerBlockOpt = clamp(0, PT_MAX_SLOTS_PER_BLOCK)/64*64;
    else if (k == "threads_closest") o.thrOverride[0] = int(value);
    else if (k == "threads_shadow") o.thrOverride[1] = int(value);
    else if (k == "threads_shade_simple") o.thrOverride[2] = int(value);
    else if (k == "threads_shade_complex") o.thrOverride[3] = int(value);
    else return false;
    return true;
}

std::string kernelName(const KernelId &k)
{
    char b[128];
    const char *c = k.count ? "true" : "false", *s = k.solids ? "true" : "false", *f = k.flat ? "true" : "false";
    auto tf = [](bool v) { return v ? "true" : "false"; };
    switch (k.family) {
    case K_CLOSEST:             std::snprintf(b, sizeof b, "k_trace_closest<%s,%s,%d>", c, f, k.inst); break;
    case K_CLOSEST_DYN:         std::snprintf(b, sizeof b, "k_trace_closest_dyn<%s,%s>", c, s); break;
    case K_CLOSEST_INST:        std::snprintf(b, sizeof b, "k_trace_closest_inst<%s,%s>", c, s); break;
    case K_CLOSEST_INSTW:       std::snprintf(b, sizeof b, "k_trace_closest_instw<%s,%s>", c, s); break;
    case K_CLOSEST_WIDE:        std::snprintf(b, sizeof b, "k_trace_closest_wide<%s,%s,%s,%s>", c, s, tf(k.inst != 0), tf(k.decoupled)); break;
    case K_FINISH_CLOSEST_WIDE: std::snprintf(b, sizeof b, "k_finish_trace_closest_wide<%s,%s>", c, s); break;
    case K_SHADOW:              std::snprintf(b, sizeof b, "k_trace_shadow<%s,%s,%s,%d,%u>", c, tf(k.forward), f, k.inst, k.mask); break;
    case K_SHADOW_DYN:          std::snprintf(b, sizeof b, "k_trace_shadow_dyn<%s,%s>", c, s); break;
    case K_SHADOW_WIDE:         std::snprintf(b, sizeof b, "k_trace_shadow_wide<%s,%s,%s,%s>", c, s, tf(k.inst != 0), tf(k.join)); break;
    case K_SHADOW_FAST:         std::snprintf(b, sizeof b, "k_trace_shadow_fast<%s,%s>", c, s); break;
    case K_SHADOW_FAST_INST:    std::snprintf(b, sizeof b, "k_trace_shadow_fast_inst<%s,%s>", c, s); break;
    case K_SHADE:               std::snprintf(b, sizeof b, "k_shade<%u,%d,%d,%s>", k.mask, k.waves, k.fuse, tf(k.globalTables)); break;
    case K_SHADE_FUSED:         std::snprintf(b, sizeof b, "k_shade_fused<%u,%u,%d>", k.mask, k.mask0, k.waves); break;
    case K_TAIL:                std::snprintf(b, sizeof b, "k_tail<%u,%s>", k.mask, s); break;
    case K_TRACE_RAYS:          std::snprintf(b, sizeof b, "k_trace_rays<%s,%s,%d,%s>", c, f, k.inst, tf(k.decoupled)); break;
    default:                    return std::string();
    }
    return b;
}

namespace {

KernelId walkKernel(KernelFamily family, bool count, bool solids)
{
    KernelId k;
    k.family = family; k.count = count; k.solids = solids;
    return k;
}
// k_trace_closest<COUNT, FLAT, INST> / k_trace_shadow<COUNT, FORWARD, FLAT, INST, MS>: no SOLIDS argument; INST = 1 walks instances of a scene with solids, 2 without
KernelId bvh2Kernel(KernelFamily family, bool count, bool flat, bool inst, bool solids, bool forward = false, uint32_t mask = 0)
{
    KernelId k;
    k.family = family; k.count = count; k.flat = flat; k.inst = inst ? (solids ? 1 : 2) : 0; k.forward = forward; k.mask = mask;
    return k;
}

struct ShadeFamily { int variant; uint32_t mask; int waves; };
const ShadeFamily F_LEAN = {TGHIP_BSDF_VARIANT_LEAN, MASK_LEAN, LEAN_WAVES}, F_SIMPLE = {TGHIP_BSDF_VARIANT_SIMPLE, MASK_SIMPLE, SIMPLE_WAVES},
                  F_SIMPLE_INST = {TGHIP_BSDF_VARIANT_SIMPLE, MASK_SIMPLE_INST, SIMPLE_WAVES}, F_COAT = {TGHIP_BSDF_VARIANT_COAT, MASK_COAT, COAT_WAVES},
                  F_GLASS = {TGHIP_BSDF_VARIANT_GLASS, MASK_GLASS, 2}, F_PLASTIC = {TGHIP_BSDF_VARIANT_PLASTIC, MASK_PLASTIC, 2},
                  F_COAT_INST = {TGHIP_BSDF_VARIANT_COAT, MASK_COAT_INST, 2}, F_GLASS_INST = {TGHIP_BSDF_VARIANT_GLASS, MASK_GLASS_INST, 2},
                  F_PLASTIC_INST = {TGHIP_BSDF_VARIANT_PLASTIC, MASK_PLASTIC_INST, 2}, F_FULL = {TGHIP_BSDF_VARIANT_FULL, MASK_FULL, 2},
                  F_MEDIA = {TGHIP_BSDF_VARIANT_MEDIA, MASK_MEDIA, 2}, F_ALL = {TGHIP_BSDF_VARIANT_ALL, BSDF_MASK_ALL, 2};

KernelId shadeKernel(const ShadeFamily &f, bool qmc, int fuse = 0, bool globalTables = false)
{
    KernelId k;
    k.family = K_SHADE; k.mask = f.mask | (qmc ? FEAT_QMC : 0u); k.waves = f.waves; k.fuse = fuse; k.globalTables = globalTables;
    return k;
}

WorkgroupSize sizedBy(const KernelId &k, int maxThreads, LdsFormula lds)
{
    WorkgroupSize w;
    w.maxThreads = maxThreads; w.sizedBy = k; w.lds = lds;
    return w;
}

} // namespace

void chooseLaunches(const SceneTraits &sc, uint32_t numRecs, uint32_t numWideNodes, const LaunchOptions &o, const PassKind &pass, LaunchChoice &c)
{
    c = LaunchChoice();
    const bool inst = sc.haveInstances, solids = sc.haveSolids, count = pass.countTraversal;
    const bool closestWalk = sc.haveForward || sc.haveMeshLight;   // shadow rays are closest-hit walks, not any-hit queries
    const bool flat = c.flat = numRecs <= TGHIP_FLAT_MAX_RECS && !inst;
    c.tablesFit = sc.tablesFit && o.ldsTables;
    // the single-level traversal kernels walk the 8-wide BVH when the scene carries one
    c.useWide = sc.wideDepth > 0 && o.wideOpt && o.dynamicFetch && !flat;
    c.wideClosest = c.useWide && (o.wideClosestOpt < 0 ? !inst : o.wideClosestOpt != 0);
    c.wideShadowRays = c.useWide && o.wideShadowOpt != 0;
    const bool instWide = inst && o.instWideOpt && sc.wideDepth > 0 && sc.wideMasterDepth > 0 && o.wideOpt;
    const bool instDyn = inst && !c.wideClosest && o.dynamicFetch && o.instDynOpt;   // the three-level walk with dynamic ray fetch
    // a launch of its own rewrites the rays nextPath wrote before they are traced: never nextPath and the walk in one kernel, no k_finish folded into the walk
    const bool cameraFix = sc.cameraFix || pass.rayPaths;
    c.fusedFlat = flat && !closestWalk && o.fuseFlatOpt && !pass.aux && !sc.allFeaturesShading && c.tablesFit && !cameraFix;
    c.oneLaunch = c.fusedFlat && !sc.haveComplex && o.loopOpt;
    c.cameraRays = cameraFix;
    c.queryPaths = pass.rayPaths;
    c.neeFactors = closestWalk;
    c.instTreeDepth = std::max(sc.bvhDepth - sc.bvhMasterDepth, 1);

    // Measured (profiles/README.md).  On one stream BVH scenes run best with every workgroup of every kernel resident at once
    // (4 per CU, workgroup size per kernel = that kernel's occupancy limit / 4: the fallback kernels still run so); flat-list scenes are
    // streaming-bound and prefer 8 small workgroups per CU that the dispatcher load-balances.
    // Scenes on the wide kernels run the loop as PARTS of the pool on streams of their own, each kernel launched with its part
    // of the grid: with 8 workgroups per CU kernels of different parts share every CU, and the issue-bound walk of one part fills the
    // memory waits of the shading of another (materialtest 1280x720x256: 608 -> 657 Msamples/s against 4 per CU).  Instanced scenes with
    // the dynamic-fetch closest-hit kernel: two parts, 8 per CU (instances10k: 141 -> 153 Msamples/s; with the static-fetch kernel parts lost: 127 against 114-120).
    const bool oneStream = o.streamsOpt == 1 || (o.streamsOpt == 0 && pass.shortBatch);
    c.pairedInst = !flat && instDyn && !oneStream && c.wideShadowRays && !closestWalk;
    c.paired = (!flat && !inst && !oneStream && c.wideClosest && c.wideShadowRays) || c.pairedInst;
    c.blocksPerCu = o.blocksPerCuOpt > 0 ? o.blocksPerCuOpt : ((flat || c.paired) ? 8 : 4);
    // (materialtest 1280x720x256 / mesh1m 1920x1080x32: 2 parts 656 / 398 Msamples/s, 4 parts 666 / 412; instanced scenes: four are 5 % faster than two
    // with the walk of the reference's instance tree, profiles/r4_sweep_instances10k.jsonl)
    c.parts = o.streamsOpt >= 2 ? o.streamsOpt : (o.streamsOpt == 1 || pass.shortBatch) ? 1 : (!inst || c.blocksPerCu >= 8) ? 4 : 1;
    if (c.fusedFlat || flat)
        c.parts = 1;

    // Most slots a workgroup owns (the pool is sized by it, and the traversal kernels' LDS queue area): 4096 where both traversal kernels are the
    // wide ones.  The static-fetch BVH2 kernels of flat-list and instanced scenes keep a thread's queue entries in 16 half registers (OrderRegs:
    // <= 16 x threads), and their deep stacks leave less LDS: 2048, as measured (instances10k: 4096 slots with the smaller workgroups that then
    // fit are not faster).
    const bool allWide = !flat && !inst && c.wideClosest && c.wideShadowRays && !closestWalk;
    c.slotCap = allWide ? PT_MAX_SLOTS_PER_BLOCK : 2048u;
    if (o.slotsPerBlockOpt > 0)
        c.slotCap = std::min<uint32_t>(c.slotCap, uint32_t(o.slotsPerBlockOpt));
    c.slotCap = std::max(c.slotCap, 64u);
    c.orderRegsCap = flat || inst;
    // the walk arrays behind the A_* ones (suspended walks of the wide kernels)
    c.walkArrays = c.useWide && !inst ? 4u + uint32_t(sc.wideDepth + 1)/2u : 0u;
    // "fold_finish": k_finish rides in front of the next iteration's closest-hit launch (single-level scenes on the decoupled wide walk)
    c.foldFinish = o.foldFinishOpt && !cameraFix && !flat && !inst && c.wideClosest && o.decoupleOpt;

    // ---- the closest-hit walk ----
    WalkLaunch &cl = c.closest;
    int clMax = 512;
    if (flat)                 { cl.kernel = bvh2Kernel(K_CLOSEST, count, true, false, solids); cl.lds = LDS_TRACE; }
    else if (instDyn)         { cl.kernel = walkKernel(instWide ? K_CLOSEST_INSTW : K_CLOSEST_INST, count, solids); cl.lds = instWide ? LDS_INST_WIDE : LDS_DYN; clMax = 320; }
    else if (inst && !c.wideClosest) { cl.kernel = bvh2Kernel(K_CLOSEST, count, false, true, solids); cl.lds = LDS_TRACE; }
    else if (c.wideClosest) {
        // (128 / 192 / 256 / 320 threads = 505 / 433 / 394 / 469 us per launch on materialtest, but the shading launches behind it run 6 % faster after
        // 192 than after 256: 579 / 571 / 552 Msamples/s for 192 / 256 / 320)
        cl.kernel = walkKernel((!inst && o.decoupleOpt && c.foldFinish) ? K_FINISH_CLOSEST_WIDE : K_CLOSEST_WIDE, count, solids);
        cl.kernel.inst = inst;
        cl.kernel.decoupled = !inst && o.decoupleOpt && !c.foldFinish;
        cl.lds = LDS_WIDE; clMax = 192;
    }
    else if (o.dynamicFetch)  { cl.kernel = walkKernel(K_CLOSEST_DYN, count, solids); cl.lds = LDS_DYN; clMax = 320; }   // 20 waves/CU measured best (profiles/README.md)
    else                      { cl.kernel = bvh2Kernel(K_CLOSEST, count, false, false, solids); cl.lds = LDS_TRACE; }
    cl.size = sizedBy(cl.kernel, clMax, cl.lds);
    cl.size.sizedBy.count = false;
    if (c.wideClosest && !inst) {         // the shipped workgroup sizes were measured with the sequential walk's occupancy, not the launched kernel's
        cl.size.sizedBy = walkKernel(K_CLOSEST_WIDE, false, solids);
    }

    // ---- the shadow walk: what the pass launches, and -- sized as if the pass kept no auxiliary outputs -- what sizes it ----
    auto shadowWalk = [&](bool aux, bool cnt, bool join, WalkLaunch &w) {
        const bool wideShadow = c.wideShadowRays && !closestWalk && !aux;
        int maxThreads = 256;
        if ((sc.haveProcTex || sc.haveFibre) && closestWalk) {   // (closestWalk: never the wide or the dynamic-fetch any-hit kernels; haveFibre: the one family with the fibre BCSDFs)
            w.kernel = bvh2Kernel(K_SHADOW, cnt, !inst && flat, inst, solids, true, BSDF_MASK_ALL); w.lds = LDS_TRACE; maxThreads = 512;
        } else if (inst && !wideShadow) {
            w.kernel = bvh2Kernel(K_SHADOW, cnt, false, true, solids, closestWalk, MASK_ALL_NO_PROCTEX); w.lds = LDS_TRACE; maxThreads = 512;
        } else if (wideShadow) {
            w.lds = LDS_WIDE;
            if (inst && !join && !solids && !cnt) { w.kernel = walkKernel(K_SHADOW_WIDE, false, false); w.kernel.inst = 1; w.kernel.join = false; }
            else if (inst && o.instShadowFast)    w.kernel = walkKernel(K_SHADOW_FAST_INST, cnt, solids);   // the two-level walk inside the fast kernel's slot handling
            else if (inst)                        { w.kernel = walkKernel(K_SHADOW_WIDE, cnt, solids); w.kernel.inst = 1; }
            else if (o.decoupleOpt)               w.kernel = walkKernel(K_SHADOW_FAST, cnt, solids);
            else                                  w.kernel = walkKernel(K_SHADOW_WIDE, cnt, solids);
        } else if (!flat && !closestWalk && o.dynamicFetch && !aux) {   // (the dynamic-fetch kernel does not report transmittances)
            w.kernel = walkKernel(K_SHADOW_DYN, cnt, solids); w.lds = LDS_DYN;   // measured: 192 / 256 / 320 / 384 threads = 525 / 462 / 633 / 619 us per launch
        } else {
            w.kernel = bvh2Kernel(K_SHADOW, cnt, flat, false, solids, closestWalk, MASK_ALL_NO_PROCTEX); w.lds = LDS_TRACE; maxThreads = 512;
        }
        return maxThreads;
    };
    WalkLaunch sizing;
    const int shMax = shadowWalk(false, false, true, sizing);
    shadowWalk(pass.aux, count, o.instShadowJoin, c.shadow);
    c.shadow.size = sizedBy(sizing.kernel, shMax, sizing.lds);
    if (sizing.kernel.family == K_SHADOW_FAST)   // the shipped workgroup sizes were measured with the sequential wide walk's occupancy, not the launched kernel's
        c.shadow.size.sizedBy = walkKernel(K_SHADOW_WIDE, false, solids);

    // ---- shading: the family of every class ----
    const bool qmc = pass.qmc;
    const bool plasticOnly = familyCovers(TGHIP_BSDF_VARIANT_PLASTIC, sc.classMask[3], false);
    // the launch of shading class `cls` (1 .. 3) of a scene without media / auxiliary outputs / cylinders / mesh emitters: the smallest variant
    // that covers the BSDF types of the class's materials
    auto classFamily = [&](int cls, bool instTwin) -> const ShadeFamily & {
        if (cls == 1) return instTwin ? F_COAT_INST : F_COAT;
        if (cls == 2) return instTwin ? F_GLASS_INST : F_GLASS;
        if (plasticOnly) return instTwin ? F_PLASTIC_INST : F_PLASTIC;
        return F_FULL;
    };
    auto addShade = [&](const ShadeFamily &f, bool twin, int fuse, int cls, int lane) {
        ShadeLaunch &l = c.shade[c.numShade++];
        const bool all = f.mask == BSDF_MASK_ALL || f.mask == MASK_MEDIA || !c.tablesFit;
        // tables that do not fit the shading workgroups' LDS copy: every class shades with the all-features variant that reads them from global memory
        l.kernel = c.tablesFit ? shadeKernel(f, twin && qmc, fuse) : shadeKernel(F_ALL, false, 0, true);
        l.variant = c.tablesFit ? f.variant : TGHIP_BSDF_VARIANT_ALL;
        l.cls = cls; l.lane = lane;
        l.size = all ? SIZE_ALL : (cls >= 1 && cls < PT_NUM_CLASSES) ? SIZE_COMPLEX : SIZE_SIMPLE;
    };
    auto shadeClass = [&](int cls, int lane) {
        const bool simple = cls == 0 || cls == CLS_MISS || cls == CLS_0_AND_MISS;
        if (sc.mediaSimple && o.mediaLeanOpt && !pass.aux && !sc.allFeaturesShading && !sc.haveMeshLight)
            addShade(F_MEDIA, false, 0, cls, lane);                      // media scenes with simple surfaces: no scratch
        else if (sc.haveMedia || pass.aux || sc.allFeaturesShading) addShade(F_ALL, false, 0, cls, lane);   // the one variant with FEAT_MEDIA / FEAT_AUX / FEAT_CYLINDER
        else if (sc.haveMeshLight) addShade(F_FULL, true, 0, cls, lane);   // the only variant with mesh-emitter sampling (every BSDF type)
        else if (inst && simple && o.instSimpleOpt) addShade(F_SIMPLE_INST, true, 0, cls, lane);   // Lambert / escaped paths of instanced scenes
        else if (inst && (simple || !o.instSimpleOpt)) addShade(F_FULL, true, 0, cls, lane);
        else if (simple) addShade(sc.leanScene ? F_LEAN : F_SIMPLE, true, 0, cls, lane);   // the escaped paths run the class-0 variant: its surface code never runs there
        else addShade(classFamily(cls, inst), true, 0, cls, lane);
    };
    // The further class (1 .. 3) of a scene whose iterations shade in one launch of k_shade_fused: single-level BVH scenes whose tables fit the LDS
    // copy, with class 0 and exactly ONE further class that one of the instantiated pairs covers, on the launch sequence the pairs were built from
    // (class 0 merged with the escaped paths, one stream per part).
    if (o.shadeFusedOpt && !flat && !inst && !sc.haveMedia && !pass.aux && !sc.allFeaturesShading && !sc.haveMeshLight && !sc.leanScene && c.tablesFit &&
        o.mergeMissOpt && o.classStreamsOpt == 0) {
        int further = 0, n = 0;
        for (int k = 1; k < PT_NUM_CLASSES; ++k)
            if (sc.classPresent[k]) { further = k; ++n; }
        if (n == 1 && (further != 3 || plasticOnly))
            c.fusedPair = further;
    }
    c.shadeLaunches = 1;
    if (!c.fusedPair) {
        c.shadeLaunches = (o.classStreamsOpt != 0 || !o.mergeMissOpt) ? 2 : 1;
        for (int k = 1; k < PT_NUM_CLASSES; ++k)
            if (sc.classPresent[k]) ++c.shadeLaunches;
    }
    if (c.fusedFlat) {
        // flat-list scene: intersection and shadow tests happen inside the shading launches
        addShade(sc.leanScene ? F_LEAN : F_SIMPLE, true, c.oneLaunch ? (FUSE_TRACE | FUSE_SHADOW | FUSE_LOOP) : (FUSE_TRACE | FUSE_SHADOW), 0, 0);
        for (int k = 1; k < PT_NUM_CLASSES; ++k)
            if (sc.classPresent[k]) addShade(classFamily(k, false), true, FUSE_SHADOW, k, 0);
    } else if (c.fusedPair) {
        // (class 0, the escaped paths and the scene's one further class in one launch, at the workgroup size of the further class's launches)
        const ShadeFamily &f = classFamily(c.fusedPair, false);
        ShadeLaunch &l = c.shade[c.numShade++];
        l.kernel.family = K_SHADE_FUSED;
        l.kernel.mask = f.mask | (qmc ? FEAT_QMC : 0u); l.kernel.mask0 = MASK_SIMPLE | (qmc ? FEAT_QMC : 0u); l.kernel.waves = f.waves;
        l.variant = f.variant; l.cls = c.fusedPair; l.size = SIZE_COMPLEX;
    } else if (o.classStreamsOpt != 0) {
        // the escaped paths, and class 0 where further classes exist, beside the part's own stream; the longest launches stay on it
        shadeClass(CLS_MISS, 1);
        shadeClass(0, sc.haveComplex ? 2 : 0);
        for (int k = 1; k < PT_NUM_CLASSES; ++k)
            if (sc.classPresent[k]) shadeClass(k, 0);
    } else {
        // (class 0 and the escaped paths run the same variant: one launch over both queues, "merge_miss" = 0 keeps them apart)
        if (o.mergeMissOpt) shadeClass(CLS_0_AND_MISS, 0);
        else { shadeClass(CLS_MISS, 0); shadeClass(0, 0); }
        for (int k = 1; k < PT_NUM_CLASSES; ++k)
            if (sc.classPresent[k]) shadeClass(k, 0);
    }
    // workgroup sizes of the shading launches: class 0's; one for the launches of classes 1 .. 3, that of the largest variant among them; the all-features family's
    const ShadeFamily &simpleBy = (sc.haveMeshLight || inst) ? F_FULL : sc.leanScene ? F_LEAN : F_SIMPLE;
    const ShadeFamily &complexBy = (sc.haveMeshLight || inst || (sc.classPresent[3] && !plasticOnly)) ? F_FULL
                                 : sc.classPresent[3] ? F_PLASTIC : sc.classPresent[2] ? F_GLASS : F_COAT;
    c.shadeSize[SIZE_SIMPLE] = sizedBy(shadeKernel(sc.haveMedia ? F_ALL : simpleBy, false), 256, LDS_NONE);
    c.shadeSize[SIZE_COMPLEX] = sizedBy(shadeKernel(sc.haveMedia ? F_ALL : complexBy, false), 256, LDS_NONE);
    c.shadeSize[SIZE_ALL] = sizedBy(shadeKernel(F_ALL, false), 256, LDS_NONE);

    // ---- fixed workgroup sizes ----
    if (flat && o.blocksPerCuOpt == 0) {
        cl.size.fixed = c.shadow.size.fixed = c.shadeSize[SIZE_SIMPLE].fixed = c.shadeSize[SIZE_COMPLEX].fixed = c.shadeSize[SIZE_ALL].fixed = 256;
    } else if (c.paired && o.blocksPerCuOpt == 0) {
        // (closest / shadow / shade simple / shade complex, Msamples/s: 256/256/128/128 657, 192/256/128/128 634, 128/256/128/128 623,
        //  320/256/128/128 556, 256/320/128/128 549, 256/256/256/128 646, 256/256/128/64 623; 4 per CU with 192/256/192/128: 608)
        cl.size.fixed = c.pairedInst ? 192 : 256;
        if (!closestWalk) c.shadow.size.fixed = 256;
        // (profiles/r5_sweep_shade_threads.jsonl: materialtest 128/128 965, 192/192 967, 256/256 979 Msamples/s -- k_shade's 26 KB of LDS per workgroup
        // then serve four waves instead of two --, but mesh1m 604 -> 597, materialtest with a rough dielectric 453 -> 451 / 431, with a dielectric
        // 480 -> 480: 256 threads only for what it was measured to help, a small tree with the conductor family as its only other shading class)
        const bool smallCoat = !c.pairedInst && numWideNodes <= 32768u && sc.classPresent[1] && !sc.classPresent[2] && !sc.classPresent[3];
        c.shadeSize[SIZE_SIMPLE].fixed = c.shadeSize[SIZE_COMPLEX].fixed = smallCoat ? 256 : 128;
    }
    WorkgroupSize *dst[4] = {&cl.size, &c.shadow.size, &c.shadeSize[SIZE_SIMPLE], &c.shadeSize[SIZE_COMPLEX]};
    for (int i = 0; i < 4; ++i)
        if (o.thrOverride[i] >= 64) dst[i]->fixed = std::min(o.thrOverride[i]/64*64, i < 2 ? 512 : 256);

    // ---- k_tail runs the wide single-level kernels' bodies: scenes those kernels render, passes without visit counts ----
    c.tailEligible = o.tailOpt && !cameraFix && c.tablesFit && !flat && !inst && c.wideClosest && c.wideShadowRays && o.decoupleOpt &&
                     familyCovers(TGHIP_BSDF_VARIANT_TAIL, sc.complexMask, sc.haveForward) &&
                     !sc.haveMeshLight && !sc.haveMedia && !pass.aux && !sc.allFeaturesShading && !count;
    // scenes of Lambert / null and conductor-family materials only (the metric's): the narrower instantiation, "tail_family" = 0 for the A/B
    const bool tailCoat = o.tailFamilyOpt && !solids && !sc.classPresent[2] && !sc.classPresent[3];
    c.tail.family = c.tailProbe.family = K_TAIL;
    c.tail.mask = (tailCoat ? MASK_COAT : MASK_TAIL) | (qmc ? FEAT_QMC : 0u);
    c.tail.solids = !tailCoat && solids;
    c.tailProbe.mask = MASK_TAIL | (qmc ? FEAT_QMC : 0u);
    c.tailProbe.solids = solids;

    // ---- the walk tghip_trace_rays / tghip_query_rays answer with (closest hits of a scene with `instances` primitives are a matter of the
    // reference's visiting order: the BVH2 walk, never the wide one) ----
    c.rayWalk = (c.useWide && !inst) ? LaunchChoice::RAYS_WIDE : inst ? LaunchChoice::RAYS_INST : flat ? LaunchChoice::RAYS_FLAT : LaunchChoice::RAYS_BVH2;
    c.traceRays.family = K_TRACE_RAYS;
    c.traceRays.count = count;
    c.traceRays.flat = c.rayWalk == LaunchChoice::RAYS_FLAT;
    c.traceRays.inst = c.rayWalk == LaunchChoice::RAYS_INST ? 1 : 0;
    c.traceRays.decoupled = c.rayWalk == LaunchChoice::RAYS_WIDE;
}

size_t ldsBytes(const SceneTraits &sc, const LaunchChoice &c, LdsFormula f, int threads)
{
    const size_t t = size_t(threads), queue = size_t(c.slotCap)*sizeof(unsigned short);
    switch (f) {
    case LDS_TRACE:
        // one node stack of bvhDepth ints per thread (a root-to-leaf walk pushes at most one far child per internal level), aliased with the expanded
        // queue (2 B per slot) that is consumed before traversal starts.  Flat-list scenes need no stack.
        return std::max<size_t>(c.flat ? 0 : size_t(std::max(sc.bvhDepth, 1))*t*sizeof(int), queue);
    case LDS_DYN:        // dynamic-fetch traversal kernels keep the expanded queue next to the stacks
        return queue + size_t(std::max(sc.bvhDepth, 1))*t*sizeof(int);
    case LDS_WIDE:       // the wide kernels: expanded queue + one 8-byte group entry per tree level and thread
        return queue + size_t(std::max(sc.wideDepth, 1))*t*8u;
    case LDS_INST_WIDE: {
        // k_trace_closest_instw: expanded queue + the BVH2 stack of the scene's tree and the reference's tree over the instances (no master on it) + the
        // masters' group stack (8-byte entries, 8-byte aligned)
        const size_t ints = ((size_t(c.slotCap) >> 1) + size_t(c.instTreeDepth)*t + 1u) & ~size_t(1);
        return ints*sizeof(int) + size_t(std::max(sc.wideMasterDepth, 1))*t*8u;
    }
    default:
        return 0;
    }
}

static void setName(char (&dst)[TGHIP_KERNEL_NAME_LEN], const KernelId &k) { std::snprintf(dst, sizeof dst, "%s", kernelName(k).c_str()); }

void exportLaunchChoice(const LaunchChoice &c, TgHipLaunchChoice *out)
{
    std::memset(out, 0, sizeof *out);
    out->flat = c.flat; out->fused_flat = c.fusedFlat; out->one_launch = c.oneLaunch; out->paired = c.paired; out->paired_inst = c.pairedInst;
    out->blocks_per_cu = c.blocksPerCu; out->parts = c.parts;
    out->slot_cap = int32_t(c.slotCap); out->order_regs_cap = c.orderRegsCap; out->walk_arrays = int32_t(c.walkArrays); out->fold_finish = c.foldFinish;
    out->nee_factors = c.neeFactors; out->camera_rays = c.cameraRays; out->tables_fit = c.tablesFit;
    const WalkLaunch *walks[2] = {&c.closest, &c.shadow};
    TgHipWalkLaunch *dst[2] = {&out->closest, &out->shadow};
    for (int i = 0; i < 2 && !c.fusedFlat; ++i) {
        setName(dst[i]->name, walks[i]->kernel); setName(dst[i]->sized_by, walks[i]->size.sizedBy);
        dst[i]->lds_formula = walks[i]->lds; dst[i]->sized_lds_formula = walks[i]->size.lds;
        dst[i]->max_threads = walks[i]->size.maxThreads; dst[i]->fixed_threads = walks[i]->size.fixed;
    }
    out->num_shade = c.numShade; out->fused_pair = c.fusedPair; out->shade_launches = c.shadeLaunches;
    for (int i = 0; i < c.numShade; ++i) {
        const ShadeLaunch &l = c.shade[i];
        setName(out->shade[i].name, l.kernel);
        out->shade[i].cls = l.cls; out->shade[i].variant = l.variant; out->shade[i].mask = l.kernel.mask; out->shade[i].fuse = l.kernel.fuse;
        out->shade[i].global_tables = l.kernel.globalTables; out->shade[i].size = l.size; out->shade[i].lane = l.lane;
    }
    for (int i = 0; i < 3; ++i) {
        setName(out->shade_size[i].sized_by, c.shadeSize[i].sizedBy);
        out->shade_size[i].max_threads = c.shadeSize[i].maxThreads; out->shade_size[i].fixed_threads = c.shadeSize[i].fixed;
    }
    out->tail_eligible = c.tailEligible;
    if (c.tailEligible) { setName(out->tail, c.tail); setName(out->tail_probe, c.tailProbe); }
    if (c.cameraRays) std::snprintf(out->camera_rays_name, sizeof out->camera_rays_name, c.queryPaths ? "k_query_paths" : "k_camera_rays");
    out->ray_walk = c.rayWalk;
    setName(out->trace_rays, c.traceRays);
}

