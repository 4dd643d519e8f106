// What tghip_upload_scene decides about a scene description before anything touches the device: every refusal of a malformed or unsupported
// description, the facts the launch code later branches on, and the tables derived from the description that are uploaded next to it.  Plain
// host arithmetic over TgHipSceneDesc: no device, no context (include/tungsten_host.h: tgh_scene_check runs it on its own).
#ifndef TGAMD_SCENECHECK_HPP_
#define TGAMD_SCENECHECK_HPP_

#include "../hip/pt_variants.h"

#include <cstdint>
#include <string>
#include <vector>

// the options of a context that change what an upload derives (tghip_set_option, at the next upload)
struct SceneCheckOptions {
    bool top_tree = true;              // "top_tree": 0 = TgHipSceneDesc::top_nodes is ignored (and not checked)
    uint32_t wide_node_stride = 80;    // "wide_node_stride": bytes per device node; decides whether nodes + records stay below 2^32 bytes
};

struct SceneTraits {
    int bvhDepth = 0;                     // stack words the BVH2 traversal needs (bvhDepthOf)
    int wideDepth = 0;                    // levels of the 8-wide BVH (0: the scene has none -- or nodes and records do not fit one 32-bit offset --, the kernels walk the BVH2)
    int bvhMasterDepth = 0;               // instanced scenes: the part of bvhDepth that is the deepest master's BVH2 subtree, and the wide walk's levels inside a master
    int wideMasterDepth = 0;

    // shading classes of the scene (recClass) and what the kernel variants are chosen by
    bool haveComplex = false;             // some primitive record uses a BSDF of class 1, 2 or 3
    uint32_t complexMask = 0;             // union of the BSDF types inside those materials
    bool classPresent[PT_NUM_CLASSES] = {false, false, false, false};   // shading classes (pt_variants.h: PT_NUM_CLASSES) that occur among the records
    uint32_t classMask[PT_NUM_CLASSES] = {0, 0, 0, 0};                  // ... and the BSDF types inside each
    bool haveForward = false;             // some BSDF has a forward lobe (shadow rays attenuate instead of stop) -- or the scene has media: shadow rays pick up
                                          // transmittance segment by segment (the closest-hit shadow walk)
    std::vector<uint32_t> bsdfTypes;      // per bsdf: bsdfTypeMask, plus FEAT_BITMAP when a texture inside is a bitmap and FEAT_FAMILY_ALL when haveProcTex or haveFibre (tghip_debug_bsdf_info)
    std::vector<uint8_t> bsdfForward;     // ... and whether it has a forward lobe
    std::vector<uint8_t> mediumOperand;   // per entry of media[]: 1 = an operand of the interpolated transmittance in front of it, no medium of its own (tghip_debug_medium)
    // what tghip_query_transmittance reads: whether some BSDF has a forward lobe (haveForward without the media's share of it), per object its
    // TGHIP_OBJ_* type, the medium the camera is in
    bool haveForwardBsdf = false;
    std::vector<int32_t> objectType;
    int32_t cameraMedium = -1;
    std::vector<uint32_t> lightNeeds;     // per slot of lights[]: the feature bits its light code needs (lightNeeds below; tghip_debug_light_info)
    bool haveMeshLight = false;           // a triangle mesh is a sampled light: closest-hit shadow walk, MASK_FULL shading
    bool thinlens = false;                // thin-lens camera: passes run the EXT kernel variants (PT_PASS_THINLENS)
    // equirectangular / cubemap camera: k_camera_rays rewrites the fresh camera rays before they are traced, in a launch of its own in front of every
    // closest-hit launch: the kernels that generate a camera ray and trace it in one go -- the folded finish, the flat lists' fused launches, k_tail --
    // are not used for such scenes
    bool cameraFix = false;
    bool haveSolids = false;              // cube / sphere / disk records: the dynamic-fetch kernels' SOLIDS variants
    bool allFeaturesShading = false;      // cylinder primitives -- or a bump-mapped bsdf (TgHipBsdf::bump1), or a disk / blade texture: BSDF_MASK_ALL shading (the only
                                          // FEAT_CYLINDER / FEAT_BUMP variant), never fused
    bool haveProcTex = false;             // a `disk` or `blade` texture (TGHIP_TEX_DISK / _BLADE), or a sampled infinite sphere whose emission is a checker (its sample / pdf):
                                          // evaluated by the all-features family only -- sets allFeaturesShading (BSDF_MASK_ALL
                                          // shading, never fused, no k_tail) and sends a closest-hit shadow walk to k_trace_shadow<., true, ., ., BSDF_MASK_ALL>
    bool haveFibre = false;               // a fibre BCSDF (TGHIP_BSDF_LAMBERTIAN_FIBER / _ROUGH_WIRE) in the bsdf table: compiled where disk's and blade's code is, so it steers
                                          // exactly where haveProcTex steers (allFeaturesShading, the closest-hit shadow walk's BSDF_MASK_ALL instantiation)
    bool haveMedia = false;               // participating media: BSDF_MASK_ALL shading (the only FEAT_MEDIA variant), closest-hit shadow walk, never fused
    bool mediaSimple = false;             // a media scene whose surface BSDFs MASK_MEDIA covers (no instances, no mesh emitters)
    bool haveInstances = false;           // instance records: two-level traversal kernels (INST), MASK_FULL shading, never the flat list
    bool leanScene = false;               // no bitmap texture, no infinite light, <= 1 sampled light, no triangles: k_shade<MASK_LEAN>
    bool tablesFit = true;                // objects + bsdfs + textures + light lists fit the shading workgroups' LDS copy (pt_kernels.h: stageSceneTables)
    bool topTree = false;                 // the description's top_nodes are used: flatBoxes holds the records' leaf boxes

    // derived tables, uploaded next to the description's own arrays
    std::vector<uint8_t> recClass;        // shading class of each primitive record's bsdf (DeviceScene::rec_class)
    std::vector<uint16_t> guide;          // CDF guide tables of the samplable bitmaps (pt_scene.h: upperBoundGuided) ...
    std::vector<int32_t> texGuide;        // ... per texture the offset of its tables in `guide`, -1 = none
    std::vector<float> rows;              // the conditional tables of those bitmaps once more as interleaved (cdf, pdf) pairs (pt_scene.h: upperBoundGuidedPairs) ...
    std::vector<int32_t> texRows;         // ... per texture its first PAIR in `rows`, -1 = none
    std::vector<uint16_t> envGuide;       // the marginal guide of env_tex, padded to whole 32-bit words
    std::vector<float> flatBoxes;         // topTree: per record the box of its leaf in top_nodes, (lo, 0, hi, 0)
    // The scene's one quad, hoisted out of the decoupled walks (pt_scene.h: DeviceScene::hoisted_rec): a single-level scene of triangles and
    // exactly ONE quad whose wide nodes leave `reserved` zero.  The wide node `node` that holds the quad as a leaf record gets bit `bit` -- the
    // record's bit of leaf_valid -- in its `reserved` word, on the device copy only.  record = -1: nothing is hoisted.
    struct { int32_t record; uint32_t node, bit; } hoisted = {-1, 0u, 0u};
    // the first sampled environment map whose marginal tables fit the shading kernels' LDS copy next to the small tables (-1 / 0: none; then
    // it is sampled through the texture's own tables in global memory, like any other bitmap)
    int32_t env_tex = -1, env_h = 0;
};

// Refuses (TGHIP_E_INVALID / TGHIP_E_UNSUPPORTED, the reason in `error`) or fills `out` and returns TGHIP_OK.  Reads nothing through an index or
// an offset of the description before it has checked it.
int checkScene(const TgHipSceneDesc *sd, const SceneCheckOptions &opt, SceneTraits &out, std::string &error);

int bsdfDepth(const TgHipSceneDesc *s, int bi, int depth);
// set of BSDF types (bit = 1 << type) in the subtree of bsdf `bi`
uint32_t bsdfTypeMask(const TgHipSceneDesc *s, int bi, int depth);
// does a texture inside bsdf `bi` (nested ones included) hold a bitmap?
bool bsdfUsesBitmap(const TgHipSceneDesc *s, int bi, int depth);
bool bsdfHasFibre(const TgHipSceneDesc *s, int bi, int depth);   // a fibre BCSDF inside the material (bsdfTypeMask has no bit for the two types)
// May shading family `variant` (TGHIP_BSDF_VARIANT_*) be given a material with type set `tm` (bsdfTypeMask) and forward lobe `fwd`?  The one
// statement of the rules the upload and the launch plan apply to type sets (they call it on a material's set or on the union over a class / the scene):
// the shading classes 0 / 1 / 2 (SIMPLE / COAT / GLASS) take materials without a forward lobe whose types their mask covers, in that order; what is left
// is class 3, shaded by PLASTIC when all of it fits that mask and by FULL / ALL otherwise; MEDIA takes a media scene whose surface types it covers; TAIL
// finishes scenes without forward lobes and without the five late types.  LEAN is the exception: the product picks it per SCENE (checkScene's
// leanScene: no bitmap texture anywhere, one quad light, quads and cubes only), so for LEAN this is tghip_debug_bsdf_info's per-material reading of that
// rule -- SIMPLE's types and no bitmap inside the material (FEAT_BITMAP in tm, set for that entry only) -- and not a site the product calls.
bool familyCovers(uint32_t variant, uint32_t tm, bool fwd);
// The type / feature mask of shading family `variant` (TGHIP_BSDF_VARIANT_*) without the Sobol' sampler's bit; 0 for an unknown variant.
uint32_t familyMask(uint32_t variant);
// The feature bits the light code needs for the sampled light in slot `slot` of s->lights: the bits the branches of its emitter type are compiled
// behind in chooseLight / lightSampleDirect / lightApproximateRadiance / lightIntersect / lightEvalDirect / lightDirectPdf (csrc/hip/pt_scene.h) and in
// k_shade's next-event estimation (pt_wavefront.h: diracLight, meshLight).  A family may shade a scene only if its mask holds the needs of every
// light: a branch that folds away leaves the light to the next one that compiles -- a cube sampled as a quad --, silently.  FEAT_FAMILY_ALL stands for
// "all four bits" (HAS_PROCTEX): a disk or blade emission, a sampled checker environment.  FEAT_MULTILIGHT whenever the scene has a second light.
uint32_t lightNeeds(const TgHipSceneDesc *s, uint32_t slot);
// What tghip_debug_medium decides about a call before anything touches the device: TGHIP_OK with the set of variants to launch (bit = 1 << variant;
// none for n == 0), or TGHIP_E_INVALID with the refusal in `error` -- null pointers, a scene without media, a medium index outside media[] or one that
// names an operand entry, a variant that is unknown or whose mask lacks FEAT_MEDIA.  t: checkScene's answer for the uploaded scene.
int checkMediumCases(const SceneTraits &t, const TgHipMediumCase *cases, const TgHipMediumResult *results, size_t n, uint32_t &variants, std::string &error);
// Depth of the subtree under `root` (also validates child references).  `level`: 0 = the scene's tree (leaves: non-instance records and
// instance-set records, which are collected in `found`), 1 = the reference's tree behind a set record (leaves: one or two slots of
// inst_prims; the instance records behind them are collected in `found`), 2 = a master's subtree (triangles and the like only).
int subtreeDepth(const TgHipSceneDesc *s, int32_t root, size_t &visited, int level, std::vector<uint32_t> *found);
// Stack words the BVH2 traversal needs: the scene's tree; with `instances` primitives, above it the reference's tree over the instances
// and the deepest master subtree (pt_kernels.h: instanceSetIntersect).  -1 when malformed.
int bvhDepthOf(const TgHipSceneDesc *s, int *masterDepthOut = nullptr);
// Validates the wide BVH -- the top-level tree from node 0 and, with instances, the masters' subtrees behind it (roots in the
// instance records): children behind their parent, every node in one tree, record runs inside the record array -- and returns
// the stack depth the walk needs (-1 when malformed).
int wideDepthOf(const TgHipSceneDesc *s, int *masterDepthOut = nullptr);

#endif
