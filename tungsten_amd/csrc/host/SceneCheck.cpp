#include "SceneCheck.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

static bool isFibre(int32_t type) { return type == TGHIP_BSDF_LAMBERTIAN_FIBER || type == TGHIP_BSDF_ROUGH_WIRE; }
static bool nestsOne(int32_t type) { return type == TGHIP_BSDF_SMOOTH_COAT || type == TGHIP_BSDF_ROUGH_COAT || type == TGHIP_BSDF_TRANSPARENCY; }

int bsdfDepth(const TgHipSceneDesc *s, int bi, int depth)
{
    if (bi < 0 || depth > 16) return depth;
    const TgHipBsdf &b = s->bsdfs[bi];
    int d = depth + 1;
    if (nestsOne(b.type))
        return bsdfDepth(s, b.sub0, d);
    if (b.type == TGHIP_BSDF_MIXED)
        return std::max(bsdfDepth(s, b.sub0, d), bsdfDepth(s, b.sub1, d));
    return d;
}

uint32_t bsdfTypeMask(const TgHipSceneDesc *s, int bi, int depth)
{
    if (bi < 0 || uint32_t(bi) >= s->num_bsdfs || depth > 16) return 0;
    const TgHipBsdf &b = s->bsdfs[bi];
    // (a type no word has a bit for is a type no kernel shades -- but for the two fibre BCSDFs, types 19 and 20, whose bits are FEAT_PHONG and FEAT_BUMP:
    // they leave no bit here, and checkScene marks every material of a scene that holds one with FEAT_FAMILY_ALL, bsdfHasFibre)
    uint32_t m = b.type >= 0 && b.type < 32 && !isFibre(b.type) ? BSDF_BIT(uint32_t(b.type)) : 0u;
    if ((b.type == TGHIP_BSDF_ROUGH_CONDUCTOR || b.type == TGHIP_BSDF_ROUGH_DIELECTRIC || b.type == TGHIP_BSDF_ROUGH_PLASTIC || b.type == TGHIP_BSDF_ROUGH_COAT) &&
        b.distribution == TGHIP_DIST_PHONG)
        m |= FEAT_PHONG;                     // outside every family mask: such a material is shaded by the full variant (pt_scene.h: mfDist)
    if (nestsOne(b.type))
        m |= bsdfTypeMask(s, b.sub0, depth + 1);
    if (b.type == TGHIP_BSDF_MIXED)
        m |= bsdfTypeMask(s, b.sub0, depth + 1) | bsdfTypeMask(s, b.sub1, depth + 1);
    return m;
}

bool bsdfHasFibre(const TgHipSceneDesc *s, int bi, int depth)
{
    if (bi < 0 || uint32_t(bi) >= s->num_bsdfs || depth > 16) return false;
    const TgHipBsdf &b = s->bsdfs[bi];
    if (isFibre(b.type)) return true;
    if (nestsOne(b.type))
        return bsdfHasFibre(s, b.sub0, depth + 1);
    if (b.type == TGHIP_BSDF_MIXED)
        return bsdfHasFibre(s, b.sub0, depth + 1) || bsdfHasFibre(s, b.sub1, depth + 1);
    return false;
}

bool familyCovers(uint32_t variant, uint32_t tm, bool fwd)
{
    switch (variant) {
    case TGHIP_BSDF_VARIANT_LEAN:    return !fwd && (tm & ~MASK_LEAN) == 0;
    case TGHIP_BSDF_VARIANT_SIMPLE:  return !fwd && (tm & ~MASK_SIMPLE) == 0;
    case TGHIP_BSDF_VARIANT_COAT:    return !fwd && (tm & ~MASK_COAT) == 0;
    case TGHIP_BSDF_VARIANT_GLASS:   return !fwd && (tm & ~MASK_GLASS) == 0;
    case TGHIP_BSDF_VARIANT_PLASTIC: return (tm & ~MASK_PLASTIC) == 0;
    case TGHIP_BSDF_VARIANT_MEDIA:   return (tm & ~MASK_MEDIA & 0x7FFFFu) == 0 && !HAS_PROCTEX(tm);   // (bits 0 .. 18: the BSDF types; tghip_debug_bsdf_info's marker of a scene with a disk / blade texture or a sampled checker environment)
    case TGHIP_BSDF_VARIANT_TAIL:    return !fwd && (tm & ~MASK_TAIL) == 0;
    case TGHIP_BSDF_VARIANT_FULL:    return (tm & ~MASK_FULL) == 0;
    case TGHIP_BSDF_VARIANT_ALL:     return true;
    default: return false;
    }
}

uint32_t familyMask(uint32_t variant)
{
    switch (variant) {
#define FAMILY_CASE(V, MASK) case V: return (MASK) & ~FEAT_QMC;
    PT_FAMILY_VARIANTS(FAMILY_CASE)
#undef FAMILY_CASE
    default: return 0u;
    }
}

int checkMediumCases(const SceneTraits &t, const TgHipMediumCase *cases, const TgHipMediumResult *results, size_t n, uint32_t &variants, std::string &error)
{
    variants = 0u;
    if (n == 0) return TGHIP_OK;
    if (!cases || !results || n > 0x3FFFFFFFu) { error = "invalid medium self-test arguments"; return TGHIP_E_INVALID; }
    if (!t.haveMedia || t.mediumOperand.empty()) { error = "medium self-test: the scene has no media"; return TGHIP_E_INVALID; }
    for (size_t i = 0; i < n; ++i) {
        if (cases[i].medium < 0 || size_t(cases[i].medium) >= t.mediumOperand.size()) { error = "medium self-test: medium index outside the scene's table"; return TGHIP_E_INVALID; }
        if (t.mediumOperand[size_t(cases[i].medium)]) { error = "medium self-test: the entry is an operand of an interpolated transmittance, not a medium"; return TGHIP_E_INVALID; }
        if (cases[i].variant >= TGHIP_BSDF_VARIANT_COUNT) { error = "medium self-test: unknown variant"; return TGHIP_E_INVALID; }
        if (!(familyMask(cases[i].variant) & FEAT_MEDIA)) { error = "medium self-test: the variant's kernels carry no medium code"; return TGHIP_E_INVALID; }
        variants |= 1u << cases[i].variant;
    }
    return TGHIP_OK;
}

uint32_t lightNeeds(const TgHipSceneDesc *s, uint32_t slot)
{
    if (slot >= s->num_lights || s->lights[slot] < 0 || uint32_t(s->lights[slot]) >= s->num_objects) return 0u;
    const TgHipObject &o = s->objects[s->lights[slot]];
    const int32_t tex = o.emission >= 0 && uint32_t(o.emission) < s->num_textures ? s->textures[o.emission].type : -1;
    // chooseLight: without the bit it answers lights[0] with weight one
    uint32_t needs = s->num_lights > 1 ? FEAT_MULTILIGHT : 0u;
    switch (o.type) {
    case TGHIP_OBJ_QUAD:                    // the branch every function falls into when no other is compiled
        break;
    case TGHIP_OBJ_CUBE: case TGHIP_OBJ_SPHERE: case TGHIP_OBJ_DISK:
        needs |= FEAT_SOLIDS;
        break;
    case TGHIP_OBJ_POINT:                   // its branches of lightSampleDirect / lightApproximateRadiance sit behind the quad's, which a mask without
        needs |= FEAT_INFINITE | FEAT_SOLIDS;   // FEAT_INFINITE takes for every light; k_shade's diracLight asks for FEAT_SOLIDS
        break;
    case TGHIP_OBJ_INFINITE_SPHERE_CAP:     // (lightSampleDirect / lightApproximateRadiance again; lightIntersect and lightDirectPdf settle for either bit)
        needs |= FEAT_INFINITE;
        break;
    case TGHIP_OBJ_INFINITE_SPHERE:         // a skydome is one whose emission is the baked sky image
        needs |= FEAT_INFINITE;
        // sampled through the texture's own sample / pdf: a bitmap's tables behind FEAT_BITMAP (without it: uniform), a checker's, a disk's and a
        // blade's where all of FEAT_FAMILY_ALL is set (HAS_PROCTEX)
        if (tex == TGHIP_TEX_CHECKER) needs |= FEAT_FAMILY_ALL;
        break;
    case TGHIP_OBJ_MESH:
        needs |= FEAT_MESHLIGHT;
        break;
    case TGHIP_OBJ_CYLINDER:
        needs |= FEAT_CYLINDER;
        break;
    default:
        break;
    }
    // lightEvalDirect looks the emission up with textureEval<M>: black for a bitmap without FEAT_BITMAP, a disk or a blade only under HAS_PROCTEX
    if (tex == TGHIP_TEX_BITMAP) needs |= FEAT_BITMAP;
    if (tex == TGHIP_TEX_DISK || tex == TGHIP_TEX_BLADE) needs |= FEAT_FAMILY_ALL;
    return needs;
}

bool bsdfUsesBitmap(const TgHipSceneDesc *s, int bi, int depth)
{
    if (bi < 0 || uint32_t(bi) >= s->num_bsdfs || depth > 16) return false;
    const TgHipBsdf &b = s->bsdfs[bi];
    const int32_t tex[3] = {b.albedo, b.roughness, b.tex1};
    for (int32_t t : tex)
        if (t >= 0 && uint32_t(t) < s->num_textures && s->textures[t].type == TGHIP_TEX_BITMAP) return true;
    if (nestsOne(b.type))
        return bsdfUsesBitmap(s, b.sub0, depth + 1);
    if (b.type == TGHIP_BSDF_MIXED)
        return bsdfUsesBitmap(s, b.sub0, depth + 1) || bsdfUsesBitmap(s, b.sub1, depth + 1);
    return false;
}

int subtreeDepth(const TgHipSceneDesc *s, int32_t root, size_t &visited, int level, std::vector<uint32_t> *found)
{
    std::vector<std::pair<int32_t, int>> stack;
    stack.emplace_back(root, 1);
    int depth = 0;
    while (!stack.empty()) {
        auto cur = stack.back();
        stack.pop_back();
        if (cur.first < 0) {
            uint32_t first = TGHIP_LEAF_FIRST(cur.first), count = TGHIP_LEAF_COUNT(cur.first);
            if (level == 1) {
                if (count < 1 || count > 2 || first + count > s->num_inst_prims) return -1;
                for (uint32_t k = first; k < first + count; ++k) {
                    const uint32_t ri = s->inst_prims[k];
                    if (ri >= s->num_top_recs || TGHIP_REC_KIND(s->recs[ri].meta) != TGHIP_REC_INSTANCE) return -1;
                    found->push_back(ri);
                }
                continue;
            }
            if (first + count > s->num_recs) return -1;
            for (uint32_t i = first; i < first + count; ++i) {
                const uint32_t kind = TGHIP_REC_KIND(s->recs[i].meta);
                if (kind == TGHIP_REC_INSTANCE) return -1;           // instance records are reached through their set's tree only
                if (kind == TGHIP_REC_INSTANCE_SET) {
                    if (level != 0 || count != 1) return -1;
                    found->push_back(i);
                }
            }
            continue;
        }
        if (uint32_t(cur.first) >= s->num_nodes || ++visited > s->num_nodes) return -1;
        depth = std::max(depth, cur.second);
        stack.emplace_back(s->nodes[cur.first].child0, cur.second + 1);
        stack.emplace_back(s->nodes[cur.first].child1, cur.second + 1);
    }
    return depth;
}

int bvhDepthOf(const TgHipSceneDesc *s, int *masterDepthOut)
{
    if (masterDepthOut) *masterDepthOut = 0;
    size_t visited = 0;
    std::vector<uint32_t> sets;
    int depth = subtreeDepth(s, 0, visited, 0, &sets);
    if (depth < 0 || (sets.empty() != (s->num_instances == 0))) return -1;
    if (sets.empty()) return depth;
    if (!s->inst_prims || !s->inst_leaf_boxes) return -1;
    std::vector<uint32_t> inst;
    int ref = 0;
    for (uint32_t set : sets) {
        int32_t root;
        std::memcpy(&root, &s->recs[set].c[0], 4);
        if (root == 0) return -1;
        int d = subtreeDepth(s, root, visited, 1, &inst);
        if (d < 0) return -1;
        ref = std::max(ref, d);
    }
    if (inst.size() != s->num_instances) return -1;
    std::vector<uint32_t> roots;
    for (uint32_t i : inst) {
        uint32_t root, leaf;
        std::memcpy(&root, &s->recs[i].c[0], 4);
        std::memcpy(&leaf, &s->recs[i].c[1], 4);
        if (root == 0 || root >= s->num_nodes || leaf >= s->num_inst_prims) return -1;
        roots.push_back(root);
    }
    std::sort(roots.begin(), roots.end());
    roots.erase(std::unique(roots.begin(), roots.end()), roots.end());
    int master = 0;
    for (uint32_t root : roots) {
        int d = subtreeDepth(s, int32_t(root), visited, 2, nullptr);
        if (d < 0) return -1;
        master = std::max(master, d);
    }
    if (masterDepthOut) *masterDepthOut = master;
    return depth + ref + master + 3;
}

int wideDepthOf(const TgHipSceneDesc *s, int *masterDepthOut)
{
    if (masterDepthOut) *masterDepthOut = 0;
    const uint32_t n = s->num_wide_nodes;
    std::vector<uint8_t> depth(n, 0);
    depth[0] = 1;
    uint32_t firstMaster = n;
    for (uint32_t i = 0; i < s->num_recs && s->num_instances; ++i) {
        if (TGHIP_REC_KIND(s->recs[i].meta) != TGHIP_REC_INSTANCE) continue;
        uint32_t root;
        std::memcpy(&root, &s->recs[i].c[2], 4);
        if (root == 0 || root >= n) return -1;
        depth[root] = 1;
        firstMaster = std::min(firstMaster, root);
    }
    int topDepth = 1, masterDepth = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const TgHipWideNode &w = s->wide_nodes[i];
        if (depth[i] == 0) return -1;                        // unreachable node: not a forest in breadth-first order
        const uint32_t kids = uint32_t(__builtin_popcount(w.imask));
        if (kids && (w.child_base <= i || uint64_t(w.child_base) + kids > n)) return -1;
        if (kids && i < firstMaster && w.child_base + kids > firstMaster) return -1;   // the top level does not reach into a master
        for (uint32_t k = 0; k < kids; ++k) {
            if (depth[w.child_base + k] != 0) return -1;     // two parents
            depth[w.child_base + k] = uint8_t(depth[i] + 1);
        }
        if (i < firstMaster) topDepth = std::max(topDepth, int(depth[i]) + (kids ? 1 : 0));
        else masterDepth = std::max(masterDepth, int(depth[i]) + (kids ? 1 : 0));
        if (topDepth > TGHIP_MAX_WIDE_DEPTH || masterDepth > TGHIP_MAX_WIDE_DEPTH) return -1;
        for (int sl = 0; sl < 8; ++sl) {
            const uint32_t bits = (w.leaf_valid >> (4*sl)) & 15u;
            if ((bits & (bits + 1u)) != 0u || (bits && (w.imask & (1u << sl)))) return -1;   // records 0 .. count-1 of a leaf slot
        }
        const uint32_t recLimit = i < firstMaster ? (s->num_top_recs ? s->num_top_recs : s->num_recs) : s->num_recs;
        if (w.leaf_valid && uint64_t(w.rec_base) + uint32_t(__builtin_popcount(w.leaf_valid)) > recLimit) return -1;
        for (int a = 0; a < 3; ++a)
            if (w.exp[a] == 0 || w.exp[a] == 255) return -1;
    }
    const int total = s->num_instances ? topDepth + masterDepth + 3 : topDepth;   // + what entering an instance parks on the stack
    if (masterDepthOut) *masterDepthOut = masterDepth;
    return total > TGHIP_MAX_WIDE_DEPTH ? -1 : total;
}

// floats of a Distribution2D over w x h cells: marginalPdf[h] marginalCdf[h + 1] pdf[w h] cdf[(w + 1) h]
static uint64_t dist2dFloats(int32_t w, int32_t h)
{
    const uint64_t uw = uint64_t(std::max(w, 0)), uh = uint64_t(std::max(h, 0));
    return uh + uh + 1 + uw*uh + (uw + 1)*uh;
}

// g[b] = upper_bound(a[0..n], b/buckets), appended to `guide`
static void appendGuide(std::vector<uint16_t> &guide, const float *a, int n, int buckets)
{
    int idx = 0;
    for (int b = 0; b <= buckets; ++b) {
        float x = float(b)/float(buckets);
        while (idx <= n && a[idx] <= x) ++idx;
        guide.push_back(uint16_t(std::min(idx, n + 1)));
    }
}

// TgHipSceneDesc::top_nodes, the reference's top-level Embree tree (TgHipTopNode): flat lists only, every record exactly one leaf, children behind
// their parents (preorder: no cycles), no deeper than the walk's stack allows (pt_kernels.h: flatOrderedWalk).  Fills `boxes` with the leaf boxes.
static bool topTreeBoxes(const TgHipSceneDesc *sd, std::vector<float> &boxes)
{
    const uint32_t nn = sd->num_top_nodes;
    if (!(sd->num_recs >= 2 && sd->num_recs <= TGHIP_FLAT_MAX_RECS && !sd->num_instances && nn < sd->num_recs)) return false;
    boxes.assign(size_t(sd->num_recs)*8, 0.0f);
    std::vector<int> leafOf(sd->num_recs, 0), depth(nn, 0), parents(nn, 0);
    depth[0] = 1;
    for (uint32_t n = 0; n < nn; ++n) {
        if (!(depth[n] >= 1 && depth[n] <= TGHIP_TOP_MAX_DEPTH && (n == 0 || parents[n] == 1))) return false;
        const TgHipTopNode &t = sd->top_nodes[n];
        for (int i = 0; i < 4; ++i) {
            const int32_t c = t.child[i];
            if (c == TGHIP_TOP_EMPTY) continue;
            if (c >= 0) {
                if (!(uint32_t(c) > n && uint32_t(c) < nn)) return false;
                depth[c] = depth[n] + 1; parents[c]++;
            } else {
                const uint32_t r = uint32_t(~c);
                if (!(r < sd->num_recs && leafOf[r]++ == 0)) return false;
                for (int a = 0; a < 3; ++a) { boxes[8*r + a] = t.lower[i][a]; boxes[8*r + 4 + a] = t.upper[i][a]; }
            }
        }
    }
    for (uint32_t r = 0; r < sd->num_recs; ++r) {
        const uint32_t kind = TGHIP_REC_KIND(sd->recs[r].meta);
        if (!(leafOf[r] == 1 && (kind == TGHIP_REC_QUAD || kind == TGHIP_REC_CUBE || kind == TGHIP_REC_SPHERE || kind == TGHIP_REC_DISK || kind == TGHIP_REC_CYLINDER))) return false;
    }
    return true;
}

int checkScene(const TgHipSceneDesc *sd, const SceneCheckOptions &opt, SceneTraits &out, std::string &error)
{
    if (!sd) { error = "no scene description"; return TGHIP_E_INVALID; }
    auto fail = [&](int code, const char *what) { error = what; return code; };
    auto bad = [&](const char *what) { error = std::string("malformed scene description: ") + what; return int(TGHIP_E_INVALID); };
    SceneTraits t;

    if (sd->abi_version != TGHIP_ABI_VERSION) return fail(TGHIP_E_INVALID, "scene description ABI version mismatch");
    if (sd->num_nodes == 0 || !sd->nodes) return fail(TGHIP_E_INVALID, "scene has no BVH");
    if (sd->camera.res_x <= 0 || sd->camera.res_y <= 0) return fail(TGHIP_E_INVALID, "invalid camera resolution");
    if (sd->num_lights > 16) return fail(TGHIP_E_UNSUPPORTED, "more than 16 sampled lights are not supported");
    // a path's bounce lives in 8 bits of its slot's flags, in 8 bits of a media scene's shadow tag, and bounds the 8 bits of the medium's own count
    // (pt_kernels.h: FLAG_BOUNCE, SHADOW_TAG_MEDIA, FLAG_MEDIUM_BOUNCE): bounce 256 would read as bounce 0 with the specular flag set
    if (sd->settings.max_bounces > 255) return fail(TGHIP_E_UNSUPPORTED, "integrator max_bounces above 255 are not supported");
    if (sd->num_objects >= (1u << 24)) return fail(TGHIP_E_UNSUPPORTED, "too many objects");
    if (sd->num_recs >= (1u << 26) || sd->num_nodes >= (1u << 26))   // 64-B attribute / node records behind 32-bit byte offsets (at32)
        return fail(TGHIP_E_UNSUPPORTED, "more than 2^26 primitive records or BVH nodes are not supported");
    // every index the upload (or a kernel) dereferences on the caller's word: refuse a malformed description instead of
    // reading out of bounds
    if ((sd->num_recs && (!sd->recs || !sd->tri_attrs)) || (sd->num_objects && !sd->objects) || (sd->num_bsdfs && !sd->bsdfs) ||
        (sd->num_textures && !sd->textures) || (sd->num_lights && !sd->lights) || (sd->num_infinite_lights && !sd->infinite_lights))
        return bad("a non-empty array is NULL");
    for (uint32_t i = 0; i < sd->num_lights; ++i)
        if (sd->lights[i] < 0 || uint32_t(sd->lights[i]) >= sd->num_objects) return bad("lights[] entry out of range");
    for (uint32_t i = 0; i < sd->num_infinite_lights; ++i)
        if (sd->infinite_lights[i] < 0 || uint32_t(sd->infinite_lights[i]) >= sd->num_objects) return bad("infinite_lights[] entry out of range");
    for (uint32_t i = 0; i < sd->num_recs; ++i)   // (the kind's three bits: every value is a kind, TGHIP_REC_*)
        if (TGHIP_REC_OBJECT(sd->recs[i].meta) >= sd->num_objects) return bad("primitive record refers to an object out of range");
    for (uint32_t i = 0; i < sd->num_objects; ++i) {
        const TgHipObject &o = sd->objects[i];
        if (o.bsdf < -1 || o.bsdf >= int32_t(sd->num_bsdfs)) return bad("object bsdf out of range");
        if (o.emission < -1 || o.emission >= int32_t(sd->num_textures)) return bad("object emission texture out of range");
        if (o.light < -1 || o.light >= int32_t(sd->num_lights)) return bad("object light index out of range");
        if (o.int_medium < -1 || o.ext_medium < -1 || o.int_medium >= int32_t(sd->num_media) || o.ext_medium >= int32_t(sd->num_media))
            return bad("primitive medium out of range");
        if (o.type == TGHIP_OBJ_CYLINDER) t.allFeaturesShading = true;
    }
    for (uint32_t i = 0; i < sd->num_bsdfs; ++i) {
        const TgHipBsdf &b = sd->bsdfs[i];
        const int32_t nt = int32_t(sd->num_textures), nb = int32_t(sd->num_bsdfs);
        if (b.albedo < -1 || b.albedo >= nt || b.roughness < -1 || b.roughness >= nt || b.tex1 < -1 || b.tex1 >= nt)
            return bad("bsdf texture out of range");
        if (b.sub0 < -1 || b.sub0 >= nb || b.sub1 < -1 || b.sub1 >= nb) return bad("nested bsdf out of range");
    }
    if (sd->camera.medium < -1 || sd->camera.medium >= int32_t(sd->num_media)) return bad("camera medium out of range");
    // instanced scenes: bvhDepthOf (level 1) and the tight-box upload index recs[] / inst_tight_boxes[] by num_top_recs
    t.haveInstances = sd->num_instances > 0;
    if (t.haveInstances) {
        if (sd->num_top_recs == 0 || sd->num_top_recs > sd->num_recs) return bad("num_top_recs out of range for a scene with instances");
        if (!sd->inst_tight_boxes) return bad("scene with instances without inst_tight_boxes");
        if (sd->num_inst_prims && !sd->inst_prims) return bad("scene with instances without inst_prims");
    }
    for (uint32_t i = 0; i < sd->num_textures; ++i) {
        const TgHipTexture &x = sd->textures[i];
        if (x.type < TGHIP_TEX_CONSTANT || x.type > TGHIP_TEX_BLADE) return fail(TGHIP_E_UNSUPPORTED, "unknown texture type");
        // a blade's sampling picks one of res_u sectors and its lookups divide by the sector's angle
        if (x.type == TGHIP_TEX_BLADE && (x.res_u < 1 || !(x.on_color[0] > 0.0f))) return fail(TGHIP_E_INVALID, "blade texture without blades");
        if (x.type == TGHIP_TEX_DISK || x.type == TGHIP_TEX_BLADE) t.haveProcTex = true;
        if (x.type != TGHIP_TEX_BITMAP) continue;
        // what the guide tables below and the kernels read through the two offsets
        const uint64_t texelFloats = uint64_t(std::max(x.w, 0))*uint64_t(std::max(x.h, 0))*((x.flags & TGHIP_TEXF_RGB) ? 3u : 1u);
        if (x.texel_offset < 0 || uint64_t(x.texel_offset) > sd->num_texel_floats || texelFloats > sd->num_texel_floats - uint64_t(x.texel_offset) ||
            (texelFloats && !sd->texels))
            return bad("a bitmap's texels lie outside texels[]");
        if (x.dist_offset >= 0 && (!sd->dist || uint64_t(x.dist_offset) > sd->num_dist_floats || dist2dFloats(x.w, x.h) > sd->num_dist_floats - uint64_t(x.dist_offset)))
            return bad("a bitmap's distribution lies outside dist[]");
    }
    t.bvhDepth = bvhDepthOf(sd, &t.bvhMasterDepth);
    if (t.bvhDepth < 0 || t.bvhDepth > TGHIP_MAX_BVH_DEPTH) return fail(TGHIP_E_INVALID, "malformed or too deep BVH");
    for (uint32_t i = 0; i < sd->num_bsdfs; ++i)
        if (bsdfDepth(sd, int(i), 0) > PT_MAX_BSDF_DEPTH) return fail(TGHIP_E_UNSUPPORTED, "BSDF nesting deeper than 3 is not supported");
    for (uint32_t i = 0; i < sd->num_lights; ++i) {
        const TgHipObject &lo = sd->objects[sd->lights[i]];
        const int ty = lo.type;
        if (ty == TGHIP_OBJ_MESH) {
            if (lo.first_light_tri < 0 || lo.num_light_tris <= 0 || !sd->light_tris ||
                uint64_t(lo.first_light_tri) + uint64_t(lo.num_light_tris)*10u + 1u > sd->num_light_tri_floats)
                return fail(TGHIP_E_INVALID, "sampled mesh emitter without a valid light_tris block");
            t.haveMeshLight = true;
        } else if (ty != TGHIP_OBJ_QUAD && ty != TGHIP_OBJ_INFINITE_SPHERE && ty != TGHIP_OBJ_CUBE && ty != TGHIP_OBJ_SPHERE && ty != TGHIP_OBJ_DISK &&
                   ty != TGHIP_OBJ_INFINITE_SPHERE_CAP && ty != TGHIP_OBJ_POINT && ty != TGHIP_OBJ_CYLINDER) {
            return fail(TGHIP_E_UNSUPPORTED, "unknown emitter type");
        }
        // a SAMPLED infinite sphere samples its emission through the texture's own sample / pdf: a checker's are compiled where disk's and blade's are
        // (an unsampled one, and a checker that is only looked up, keep the scene where it is)
        if (ty == TGHIP_OBJ_INFINITE_SPHERE && lo.emission >= 0 && sd->textures[lo.emission].type == TGHIP_TEX_CHECKER) t.haveProcTex = true;
    }
    t.lightNeeds.assign(sd->num_lights, 0u);
    for (uint32_t i = 0; i < sd->num_lights; ++i) t.lightNeeds[i] = lightNeeds(sd, i);
    if (sd->wide_nodes && sd->num_wide_nodes) {
        // the wide nodes and the primitive records share ONE allocation, so that a lane of the wide kernels addresses
        // "a node or a record" with one base pointer and one 32-bit offset: without room for both below 2^32 the scene walks its BVH2
        const int wd = wideDepthOf(sd, &t.wideMasterDepth);
        if (wd < 0) return fail(TGHIP_E_INVALID, "malformed wide BVH");
        const uint64_t nodeBytes = (uint64_t(sd->num_wide_nodes)*opt.wide_node_stride + 127u) & ~uint64_t(127);
        const uint64_t recBytes = uint64_t(std::max<uint32_t>(sd->num_recs, 1))*sizeof(TgHipPrimRec);
        if (nodeBytes + recBytes < (1ull << 32)) t.wideDepth = wd;
    }
    for (uint32_t i = 0; i < sd->num_bsdfs; ++i) {
        if (sd->bsdfs[i].bump1 < 0 || uint32_t(sd->bsdfs[i].bump1) > sd->num_textures) return fail(TGHIP_E_INVALID, "bsdf bump map index out of range");
        if (sd->bsdfs[i].bump1 > 0) t.allFeaturesShading = true;      // (shaded by the same one variant)
        // a fibre BCSDF anywhere, nested or not referred to at all: the table is what the kernels index
        if (isFibre(sd->bsdfs[i].type)) t.haveFibre = true;
    }
    if (t.haveProcTex || t.haveFibre) t.allFeaturesShading = true;     // (that variant again: the only one that evaluates them, pt_variants.h HAS_PROCTEX)
    t.haveMedia = sd->num_media > 0;
    if (t.haveMedia) {
        if (!sd->media || sd->num_media > PT_MAX_MEDIA) return fail(TGHIP_E_UNSUPPORTED, "more than 126 media are not supported");
        if (sd->num_objects >= (1u << 16)) return fail(TGHIP_E_UNSUPPORTED, "media scenes support at most 65535 primitives");
        t.mediumOperand.assign(sd->num_media, 0);
        for (uint32_t i = 0; i < sd->num_media; ++i) {
            const TgHipMedium &m = sd->media[i];
            if (m.phase_type < TGHIP_PHASE_ISOTROPIC || m.phase_type > TGHIP_PHASE_RAYLEIGH) return fail(TGHIP_E_UNSUPPORTED, "unknown phase function");
            if (m.medium_type < TGHIP_MEDIUM_HOMOGENEOUS || m.medium_type > TGHIP_MEDIUM_ATMOSPHERE) return fail(TGHIP_E_UNSUPPORTED, "unknown medium type");
            if (m.medium_type != TGHIP_MEDIUM_HOMOGENEOUS && m.trans_type != TGHIP_TRANS_EXPONENTIAL)
                return fail(TGHIP_E_UNSUPPORTED, "an exponential or atmospheric medium with a non-exponential transmittance is not supported");
            if (m.medium_type == TGHIP_MEDIUM_ATMOSPHERE && !(m.falloff_scale > 0.0f && m.falloff_dir[0] > 0.0f))
                return fail(TGHIP_E_INVALID, "an atmospheric medium needs a positive falloff scale and radius");
            if (m.trans_type < TGHIP_TRANS_EXPONENTIAL || m.trans_type > TGHIP_TRANS_INTERPOLATED) return fail(TGHIP_E_UNSUPPORTED, "unknown transmittance");
            if (m.trans_type == TGHIP_TRANS_INTERPOLATED &&
                (i + 2 >= sd->num_media || sd->media[i + 1].trans_type == TGHIP_TRANS_INTERPOLATED || sd->media[i + 2].trans_type == TGHIP_TRANS_INTERPOLATED))
                return fail(TGHIP_E_INVALID, "an interpolated transmittance needs its two (non-interpolated) operands in the media entries behind it");
            if (m.trans_type == TGHIP_TRANS_INTERPOLATED) t.mediumOperand[i + 1] = t.mediumOperand[i + 2] = 1;
        }
    }
    const TgHipCamera &cam = sd->camera;
    if (cam.type == TGHIP_CAMERA_CUBEMAP && (cam.blade_count < 0 || cam.blade_count > 3)) return fail(TGHIP_E_INVALID, "unknown cubemap projection mode");
    if (cam.type < TGHIP_CAMERA_PINHOLE || cam.type > TGHIP_CAMERA_CUBEMAP) return fail(TGHIP_E_UNSUPPORTED, "unknown camera type");
    t.thinlens = cam.type == TGHIP_CAMERA_THINLENS;
    t.cameraFix = cam.type == TGHIP_CAMERA_EQUIRECTANGULAR || cam.type == TGHIP_CAMERA_CUBEMAP;
    if (t.thinlens && cam.aperture_type == TGHIP_APERTURE_BITMAP) {
        // the aperture's Distribution2D inside dist[]
        const uint64_t ah = uint64_t(std::max(cam.aperture_h, 0));
        if (cam.aperture_w <= 0 || ah == 0 || !sd->dist || uint64_t(cam.aperture_dist) + dist2dFloats(cam.aperture_w, cam.aperture_h) > sd->num_dist_floats)
            return fail(TGHIP_E_INVALID, "the bitmap aperture's distribution lies outside dist[]");
        // a table that cannot be inverted (an all-black aperture: 0/0 in the marginal CDF) would send every lens sample outside it
        const float *mcdf = sd->dist + cam.aperture_dist + ah;
        bool usable = mcdf[0] == 0.0f && mcdf[ah] > 0.0f;
        for (uint64_t i = 0; usable && i < ah; ++i)
            usable = std::isfinite(mcdf[i + 1]) && mcdf[i + 1] >= mcdf[i];
        if (!usable) return fail(TGHIP_E_INVALID, "the bitmap aperture's distribution is not a CDF (zero total weight or non-finite entries)");
    } else if (t.thinlens && cam.aperture_type == TGHIP_APERTURE_CHECKER) {
        // CheckerTexture::sample scales by the resolutions, divides by res_v and by the sum of the two weights (TgHipCamera: blade_edge)
        const float on = cam.blade_edge[0], off = cam.blade_edge[1];
        if (cam.aperture_w <= 0 || cam.aperture_h <= 0) return fail(TGHIP_E_INVALID, "the checker aperture needs positive resolutions");
        if (!std::isfinite(on) || !std::isfinite(off) || on < 0.0f || off < 0.0f || !std::isfinite(on + off) || on + off == 0.0f)
            return fail(TGHIP_E_INVALID, "the checker aperture's weights must be finite, not negative and not both zero");
    } else if (t.thinlens && cam.aperture_type != TGHIP_APERTURE_DISK && cam.aperture_type != TGHIP_APERTURE_BLADE && cam.aperture_type != TGHIP_APERTURE_CONSTANT) {
        return fail(TGHIP_E_UNSUPPORTED, "unknown aperture type");
    }

    // shading classes ("sort by material", pt_variants.h: PT_NUM_CLASSES): 0 = BSDFs made of lambert / null only, 1 = conductor family, 2 = dielectric family, 3 = the rest
    std::vector<uint32_t> typeMask(sd->num_bsdfs, 0u);
    t.bsdfTypes.assign(sd->num_bsdfs, 0u);
    t.bsdfForward.assign(sd->num_bsdfs, 0);
    for (uint32_t i = 0; i < sd->num_bsdfs; ++i) {
        typeMask[i] = bsdfTypeMask(sd, int(i), 0);
        // (FEAT_FAMILY_ALL: the scene holds a `disk` or `blade` texture -- or samples a checkered environment --, so every material of it is shaded by the all-features family -- no other
        // family covers the entry)
        // (the same marker for a scene that holds a fibre BCSDF: types 19 and 20 have no bit in the word)
        t.bsdfTypes[i] = typeMask[i] | (bsdfUsesBitmap(sd, int(i), 0) ? FEAT_BITMAP : 0u) | ((t.haveProcTex || t.haveFibre) ? FEAT_FAMILY_ALL : 0u);
        t.bsdfForward[i] = (sd->bsdfs[i].lobes & TGHIP_LOBE_FORWARD) ? 1 : 0;
        if (t.bsdfForward[i]) t.haveForward = true;
    }
    t.recClass.assign(std::max<uint32_t>(sd->num_recs, 1u), 0);
    uint32_t allTypes = 0;
    for (uint32_t i = 0; i < sd->num_recs; ++i) {
        const uint32_t meta = sd->recs[i].meta, kind = TGHIP_REC_KIND(meta);
        if (kind == TGHIP_REC_INSTANCE || kind == TGHIP_REC_INSTANCE_SET)
            continue;                    // never a hit record itself: hits are the master's triangles
        if (kind != TGHIP_REC_TRIANGLE && kind != TGHIP_REC_QUAD) t.haveSolids = true;
        const int bi = kind == TGHIP_REC_TRIANGLE ? sd->tri_attrs[i].bsdf : sd->objects[TGHIP_REC_OBJECT(meta)].bsdf;
        if (bi < 0 || uint32_t(bi) >= sd->num_bsdfs) return fail(TGHIP_E_INVALID, "primitive record without a valid bsdf");
        // the smallest family that covers every type inside the material (nested ones included); forward lobes -> "everything else"
        // (a material with a fibre BCSDF inside carries the all-features marker instead of a type bit: no smaller family covers it -- class 3)
        const uint32_t tm = typeMask[size_t(bi)] | (t.haveFibre && bsdfHasFibre(sd, bi, 0) ? FEAT_FAMILY_ALL : 0u);
        const bool fwd = t.bsdfForward[size_t(bi)] != 0;
        const int c = familyCovers(TGHIP_BSDF_VARIANT_SIMPLE, tm, fwd) ? 0 : familyCovers(TGHIP_BSDF_VARIANT_COAT, tm, fwd) ? 1 :
                      familyCovers(TGHIP_BSDF_VARIANT_GLASS, tm, fwd) ? 2 : 3;
        t.recClass[i] = uint8_t(c);
        t.classPresent[c] = true;
        t.classMask[c] |= tm;
        allTypes |= tm;
        if (c != 0) { t.haveComplex = true; t.complexMask |= tm; }
    }
    t.haveForwardBsdf = t.haveForward;
    t.objectType.assign(sd->num_objects, 0);
    for (uint32_t i = 0; i < sd->num_objects; ++i) t.objectType[i] = sd->objects[i].type;
    t.cameraMedium = sd->camera.medium;
    t.mediaSimple = t.haveMedia && !t.haveInstances && familyCovers(TGHIP_BSDF_VARIANT_MEDIA, allTypes, false);
    if (t.haveMedia) t.haveForward = true;   // shadow rays pick up transmittance segment by segment: the closest-hit walk
    t.leanScene = sd->num_infinite_lights == 0 && sd->num_lights <= 1;
    for (uint32_t i = 0; i < sd->num_textures && t.leanScene; ++i) t.leanScene = sd->textures[i].type != TGHIP_TEX_BITMAP;
    for (uint32_t i = 0; i < sd->num_recs && t.leanScene; ++i)
        t.leanScene = TGHIP_REC_KIND(sd->recs[i].meta) == TGHIP_REC_QUAD || TGHIP_REC_KIND(sd->recs[i].meta) == TGHIP_REC_CUBE;
    for (uint32_t i = 0; i < sd->num_lights && t.leanScene; ++i) t.leanScene = sd->objects[sd->lights[i]].type == TGHIP_OBJ_QUAD;

    if (sd->top_nodes && sd->num_top_nodes && opt.top_tree) {
        if (!topTreeBoxes(sd, t.flatBoxes))
            return fail(TGHIP_E_INVALID, "top_nodes: not the tree of a flat list (every record one leaf, preorder, depth <= TGHIP_TOP_MAX_DEPTH)");
        t.topTree = true;
    }
    if (sd->sobol_matrices && sd->num_sobol_words != uint64_t(TGHIP_SOBOL_DIMS)*TGHIP_SOBOL_BITS)
        return fail(TGHIP_E_INVALID, "sobol_matrices must hold 1024 x 52 words");

    // CDF guide tables for the samplable bitmaps (pt_scene.h: upperBoundGuided)
    t.texGuide.assign(std::max<uint32_t>(sd->num_textures, 1u), -1);
    t.texRows.assign(std::max<uint32_t>(sd->num_textures, 1u), -1);
    for (uint32_t i = 0; i < sd->num_textures; ++i) {
        const TgHipTexture &x = sd->textures[i];
        if (x.type != TGHIP_TEX_BITMAP || x.dist_offset < 0 || x.w <= 0 || x.h <= 0 || x.w >= 65535 || x.h >= 65535)
            continue;
        if (t.guide.size() + size_t(PT_GUIDE_MARGINAL + 1) + size_t(x.h)*(PT_GUIDE_ROW + 1) >= (1u << 31))
            continue;
        t.texGuide[i] = int32_t(t.guide.size());
        const float *mcdf = sd->dist + x.dist_offset + x.h;
        const float *pdf = mcdf + (x.h + 1), *cdf = pdf + size_t(x.w)*x.h;
        appendGuide(t.guide, mcdf, x.h, PT_GUIDE_MARGINAL);
        for (int y = 0; y < x.h; ++y)
            appendGuide(t.guide, cdf + size_t(y)*(x.w + 1), x.w, PT_GUIDE_ROW);
        // ... and its conditional tables as interleaved (cdf, pdf) pairs
        if (t.rows.size()/2 + size_t(x.w + 1)*size_t(x.h) >= (1u << 28))
            continue;
        t.texRows[i] = int32_t(t.rows.size()/2);
        for (int y = 0; y < x.h; ++y)
            for (int xx = 0; xx <= x.w; ++xx) {
                t.rows.push_back(cdf[size_t(y)*(x.w + 1) + xx]);
                t.rows.push_back(xx < x.w ? pdf[size_t(y)*x.w + xx] : 0.0f);
            }
    }
    if (t.guide.empty()) t.guide.push_back(0);
    if (t.rows.empty()) t.rows.assign(2, 0.0f);
    // the marginal tables of the first sampled environment map, for the shading kernels' LDS copy (stageSceneTables)
    for (uint32_t li = 0; li < sd->num_lights && t.env_tex < 0; ++li) {
        const TgHipObject &o = sd->objects[sd->lights[li]];
        if (o.type != TGHIP_OBJ_INFINITE_SPHERE || o.emission < 0 || t.texGuide[size_t(o.emission)] < 0) continue;
        t.env_tex = o.emission;
        t.env_h = sd->textures[o.emission].h;
    }
    // do the small tables fit the shading workgroups' LDS copy (pt_kernels.h: stageSceneTables)?  Without the environment map's marginal
    // tables they must, or the scene shades with the GLOBAL_TABLES variant; the marginal tables come along only when there is room
    t.tablesFit = sceneTableLayout(sd->num_objects, sd->num_bsdfs, sd->num_textures, sd->num_lights, sd->num_infinite_lights, 0).total <= PT_LDS_TABLE_BYTES;
    if (t.env_tex >= 0 && sceneTableLayout(sd->num_objects, sd->num_bsdfs, sd->num_textures, sd->num_lights, sd->num_infinite_lights, t.env_h).total > PT_LDS_TABLE_BYTES) {
        t.env_tex = -1; t.env_h = 0;
    }
    if (t.env_tex >= 0) {
        const auto first = t.guide.begin() + t.texGuide[size_t(t.env_tex)];
        t.envGuide.assign(first, first + PT_GUIDE_MARGINAL + 1);
        t.envGuide.push_back(0);                              // padded to whole 32-bit words
    } else {
        t.envGuide.assign(2, 0);
    }

    // the scene's one quad (SceneTraits::hoisted): only where the wide BVH is walked
    if (t.wideDepth > 0 && !t.haveInstances) {
        int64_t quad = -1, node = -1;
        uint32_t bit = 0;
        bool ok = true;
        for (uint32_t i = 0; i < sd->num_recs && ok; ++i) {
            const uint32_t kind = TGHIP_REC_KIND(sd->recs[i].meta);
            if (kind == TGHIP_REC_QUAD) { ok = quad < 0; quad = i; }
            else if (kind != TGHIP_REC_TRIANGLE) ok = false;
        }
        for (uint32_t i = 0; i < sd->num_wide_nodes && ok && quad >= 0; ++i) {
            const TgHipWideNode &n = sd->wide_nodes[i];
            if (n.reserved != 0u) ok = false;
            uint32_t rank = 0;
            for (uint32_t b = 0; b < 32u; ++b)
                if ((n.leaf_valid >> b) & 1u) {
                    if (int64_t(n.rec_base) + rank == quad) { ok = ok && node < 0; node = i; bit = b; }
                    ++rank;
                }
        }
        if (ok && quad >= 0 && node >= 0) { t.hoisted.record = int32_t(quad); t.hoisted.node = uint32_t(node); t.hoisted.bit = bit; }
    }
    out = std::move(t);
    return TGHIP_OK;
}
