// Which kernels a pass runs on an uploaded scene, as data: the one statement of the decision that sizes the workgroups, lays out the pool and
// launches the wavefront loop (csrc/hip/tungsten_hip.hip resolves the identities to kernels and reads everything else from here).  Plain host
// arithmetic over SceneTraits and the context's options: no device, no context (include/tungsten_host.h: tgh_launch_choice runs it on its own).
#ifndef TGAMD_LAUNCHCHOICE_HPP_
#define TGAMD_LAUNCHCHOICE_HPP_

#include "SceneCheck.hpp"

#include <cstddef>
#include <cstdint>
#include <string>

// the options of a context the choice reads (tghip_set_option; the measurements behind the defaults: DESIGN.md 4b, profiles/README.md)
struct LaunchOptions {
    bool wideOpt = true;                  // "wide_bvh": use the 8-wide BVH when the scene carries one
    // "wide_closest" / "wide_shadow": which kernels walk it.  -1 = the measured default: both, except that closest-hit rays of instanced
    // scenes stay on the two-level BVH2 kernel (instances10k: 849 us per launch against 1061 us on the wide tree; shadow rays 905 against 517 us)
    int wideClosestOpt = -1, wideShadowOpt = -1;
    bool dynamicFetch = true;             // "dynamic_fetch": BVH scenes' closest-hit kernel fetches rays dynamically (k_trace_closest_dyn)
    int instDynOpt = 1;                   // "inst_dyn": closest-hit rays of instanced scenes on the dynamic-fetch kernel (k_trace_closest_inst) instead of the static one
    int instWideOpt = 1;                  // "inst_wide": ... with the masters' subtrees walked through the wide BVH (k_trace_closest_instw); 0 = the BVH2 walk
    bool instShadowFast = true;           // "inst_shadow_fast": instanced scenes' shadow rays on k_trace_shadow_fast_inst (0: k_trace_shadow_wide<., ., INST>)
    bool instShadowJoin = true;           // "inst_shadow_join": 0 = the instanced wide shadow kernel without PT_TURN_JOIN (the miscompiled variant; repro tool only)
    int instSimpleOpt = 1;                // "inst_simple": classes 0 / 2 of instanced scenes on the MASK_SIMPLE_INST variant instead of MASK_FULL
    int decoupleOpt = 1;                  // "decouple": the wide kernels of single-level scenes test a record AND visit a node per turn
    bool foldFinishOpt = true;            // "fold_finish": k_finish rides in front of the next iteration's closest-hit launch
    bool fuseFlatOpt = true;              // "fuse_flat": flat-list scenes without forward lobes trace + shadow-test inside k_shade
    bool loopOpt = true;                  // "run_to_completion": fused flat-list scenes whose materials are all of class 0 render in ONE launch
    bool shadeFusedOpt = true;            // "shade_fused": scenes with class 0 and one further class shade an iteration in ONE launch (k_shade_fused)
    bool mergeMissOpt = true;             // "merge_miss": class 0 and the escaped paths in one launch
    int classStreamsOpt = 0;              // "class_streams": measured 735-800 Msamples/s against 825-830 with the classes one after the other on the part's stream
    bool mediaLeanOpt = true;             // "media_lean": media scenes whose surface BSDFs MASK_MEDIA covers shade with k_shade<MASK_MEDIA> instead of <BSDF_MASK_ALL>
    // "tail_kernel": once a host check finds at most "tail_threshold" paths alive, the rest of the batch runs in k_tail (one launch per part).  Built for
    // latency, not throughput; Msamples/s for thresholds off / 2 Ki / 8 Ki / 32 Ki / 128 Ki: mesh1m 605 / 625 / 611 / 575 / 514, materialtest
    // 963 / 966 / 964 / 968 / 966, materialtest as shipped 573 / 611 / 630 / 623 / 625
    bool tailOpt = true;
    bool tailFamilyOpt = true;            // "tail_family": k_tail<MASK_COAT> for scenes without class-2 / class-3 materials and without solids
    bool ldsTables = true;                // "lds_tables" = 0: shade as if the small tables did not fit the LDS copy (the GLOBAL_TABLES variant: tests)
    int streamsOpt = 0;                   // "streams": 1 .. 8 parts of the pool on as many streams, 0 = the measured default
    int blocksPerCuOpt = 0;               // "blocks_per_cu"; 0 = the measured default
    int slotsPerBlockOpt = 0;             // "slots_per_block": upper bound on the slots of one workgroup (0 = PT_MAX_SLOTS_PER_BLOCK)
    int thrOverride[4] = {0, 0, 0, 0};    // "threads_closest" / "_shadow" / "_shade_simple" / "_shade_complex"
};
// Stores option `key` (tghip_set_option's spelling and clamping) and returns true, or returns false for a key the choice does not read.
bool setLaunchOption(LaunchOptions &opt, const std::string &key, long long value);

// what differs from pass to pass on one scene
struct PassKind {
    bool aux = false;                     // TGHIP_PASS_AUX: BSDF_MASK_ALL shading, no fused / wide / dynamic-fetch shadow kernels
    bool shortBatch = false;              // the pass does not fill the pool once (PassPlan.cpp): one stream, 4 workgroups per CU
    bool qmc = false;                     // the pass's PassParams::flags are not 0: the FEAT_QMC twin of every shading variant
    bool countTraversal = false;          // "count_traversal": the COUNT instantiations of the walks, no k_tail
    // tghip_query_radiance: the pass's paths start on the caller's rays, which k_query_paths writes in front of every closest-hit launch -- the launch
    // shape of the equirectangular / cubemap cameras (SceneTraits::cameraFix), whatever the scene's camera
    bool rayPaths = false;
    bool operator==(const PassKind &o) const
    {
        return aux == o.aux && shortBatch == o.shortBatch && qmc == o.qmc && countTraversal == o.countTraversal && rayPaths == o.rayPaths;
    }
};
// the host-side choice flag that asks for such a pass where a choice is asked for by pass flags (tgh_launch_choice: TGH_CHOICE_RAY_PATHS, tungsten_host.h).
// Not a flag of TgHipPassDesc: tghip_render_pass refuses it like every unknown bit.
#define LAUNCH_CHOICE_RAY_PATHS 0x40000000u

// the kind of a pass with the public flags `passFlags` (TGHIP_PASS_*) on a scene: thin-lens and media scenes add internal flags to every pass
inline PassKind passKindOf(const SceneTraits &sc, uint32_t passFlags, bool shortBatch, bool countTraversal)
{
    PassKind k;
    k.rayPaths = (passFlags & LAUNCH_CHOICE_RAY_PATHS) != 0;
    passFlags &= ~LAUNCH_CHOICE_RAY_PATHS;
    k.aux = (passFlags & TGHIP_PASS_AUX) != 0; k.shortBatch = shortBatch; k.qmc = passFlags != 0 || sc.thinlens || sc.haveMedia; k.countTraversal = countTraversal;
    return k;
}

enum KernelFamily {
    K_NONE = 0,
    K_CLOSEST, K_CLOSEST_DYN, K_CLOSEST_INST, K_CLOSEST_INSTW, K_CLOSEST_WIDE, K_FINISH_CLOSEST_WIDE,
    K_SHADOW, K_SHADOW_DYN, K_SHADOW_WIDE, K_SHADOW_FAST, K_SHADOW_FAST_INST,
    K_SHADE, K_SHADE_FUSED, K_TAIL, K_TRACE_RAYS
};
// A kernel: family + template arguments, in the order of the kernels' template heads (csrc/hip/pt_wavefront.h).  Flags a family has no argument for stay 0.
struct KernelId {
    KernelFamily family = K_NONE;
    bool count = false, solids = false;   // COUNT, SOLIDS
    bool flat = false, forward = false;   // k_trace_closest / k_trace_shadow / k_trace_rays: FLAT; k_trace_shadow: FORWARD
    int inst = 0;                         // k_trace_closest / k_trace_shadow / k_trace_rays: INST (0, 1 = with solids, 2); the wide kernels: INST (0 / 1)
    bool decoupled = false, join = true;  // k_trace_closest_wide: DECOUPLED; k_trace_shadow_wide: JOIN; k_trace_rays: WIDE (in `decoupled`)
    uint32_t mask = 0, mask0 = 0;         // k_shade / k_tail: M; k_shade_fused: MF, M0; k_trace_shadow: MS
    int waves = 0, fuse = 0;              // k_shade / k_shade_fused: W; k_shade: FUSE
    bool globalTables = false;            // k_shade: GLOBAL_TABLES
};
// The kernel's name in one canonical spelling: every template argument, no blanks, masks as decimal numbers -- k_trace_closest_wide<false,false,false,true>
std::string kernelName(const KernelId &k);

// the dynamic LDS of a walk launch at `threads` threads (ldsBytes below)
enum LdsFormula { LDS_NONE = 0, LDS_TRACE, LDS_DYN, LDS_WIDE, LDS_INST_WIDE };

// How a launch's workgroup size is found: `fixed`, or, when that is 0, the largest multiple of 64 from maxThreads down to 128 at which blocksPerCu
// workgroups of `sizedBy` with its dynamic LDS are resident on a CU.
struct WorkgroupSize {
    int fixed = 0, maxThreads = 0;
    KernelId sizedBy;
    LdsFormula lds = LDS_NONE;
};
struct WalkLaunch {
    KernelId kernel;
    LdsFormula lds = LDS_NONE;
    WorkgroupSize size;
};
enum ShadeSize { SIZE_SIMPLE = 0, SIZE_COMPLEX = 1, SIZE_ALL = 2 };
struct ShadeLaunch {
    KernelId kernel;
    int cls = 0;                          // the launch's class argument (0 .. 3, CLS_MISS, CLS_0_AND_MISS; k_shade_fused: the further class)
    int variant = 0;                      // TGHIP_BSDF_VARIANT_* of the family (the _INST twins stand under the family they add FEAT_INSTANCES to)
    ShadeSize size = SIZE_SIMPLE;
    int lane = 0;                         // "class_streams": 0 = the part's own stream, 1 / 2 = the class streams beside it
};

struct LaunchChoice {
    // shape of the loop
    bool flat = false;                    // a flat list of <= TGHIP_FLAT_MAX_RECS records, no instances
    bool fusedFlat = false, oneLaunch = false;   // ... that traces and shadow-tests inside k_shade; ... in ONE launch per batch
    bool useWide = false, wideClosest = false, wideShadowRays = false;
    bool paired = false, pairedInst = false;     // the loop runs as parts of the pool on streams of their own, kernels of different parts sharing every CU
    int blocksPerCu = 4;
    int parts = 1;                        // parts wanted (runBatch still asks whether the grid and the batch's items can be split so)
    uint32_t slotCap = 2048;              // most slots a workgroup owns ...
    bool orderRegsCap = false;            // ... further limited to 16 x threads of the smaller walk workgroup (OrderRegs: static-fetch BVH2 kernels)
    uint32_t walkArrays = 0;              // walk arrays the pool should carry behind the A_* ones
    bool foldFinish = false;              // no k_finish launch per iteration: it rides in the next closest-hit launch
    bool neeFactors = false;              // PathState::nee_factors: the shadow walk is a closest-hit walk
    bool cameraRays = false;              // a launch that rewrites the fresh paths' rays in front of every closest-hit launch: k_camera_rays, or ...
    bool queryPaths = false;              // ... k_query_paths (PassKind::rayPaths) in its place
    bool tablesFit = true;
    int instTreeDepth = 1;
    // the walks of an iteration (unused by fused flat lists)
    WalkLaunch closest, shadow;
    // the shading launches of an iteration, in launch order
    ShadeLaunch shade[2 + PT_NUM_CLASSES];
    int numShade = 0;
    int fusedPair = 0;                    // != 0: shade[0] is k_shade_fused over class 0, the escaped paths and this class
    int shadeLaunches = 1;                // launches the per-kernel counters book per iteration
    WorkgroupSize shadeSize[3];           // by ShadeSize
    // k_tail
    bool tailEligible = false;            // before the occupancy probe
    KernelId tail, tailProbe;             // the launch; the kernel the probe asks about (the all-types tail needs no less than the conductor-family one)
    // tghip_trace_rays / tghip_query_rays
    enum RayWalk { RAYS_FLAT = 0, RAYS_BVH2, RAYS_INST, RAYS_WIDE } rayWalk = RAYS_BVH2;
    KernelId traceRays;
};

void chooseLaunches(const SceneTraits &sc, uint32_t numRecs, uint32_t numWideNodes, const LaunchOptions &opt, const PassKind &pass, LaunchChoice &out);

// dynamic LDS bytes of a walk launch of `threads` threads under choice `c`
size_t ldsBytes(const SceneTraits &sc, const LaunchChoice &c, LdsFormula f, int threads);
// the choice as the flat record of the C interface (include/tungsten_hip.h)
void exportLaunchChoice(const LaunchChoice &c, TgHipLaunchChoice *out);

#endif
