// Stand-alone sanitizer run of the upload's host-side check (tungsten_amd/csrc/host/SceneCheck.cpp), no device and no Python:
//
//     g++ -std=c++11 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/scene_check_fuzz.cpp tungsten_amd/csrc/host/SceneCheck.cpp -o tools/bin/scene_check_fuzz
//     tools/bin/scene_check_fuzz
//
// Two small valid descriptions built in code -- (a) one BVH2 node over two triangles and a quad, one wide node, a bitmap texture with its
// distribution, a medium, a mesh emitter, a thin lens with a bitmap aperture; (b) a flat list of two quads under a top-level tree -- get a
// fixed-seed sequence of single- and double-field mutations: indices, offsets and type tags go to the boundary values -2, -1, 0, n - 1, n,
// n + 1, INT32_MAX, array pointers to NULL with their counts left standing.  Every array is a heap block of exactly its size, so a read
// through an unchecked index is a sanitizer report.  checkScene must return (accept or refuse) on every one; exit 0 without a report is the result.
#include "../tungsten_amd/csrc/host/SceneCheck.hpp"

#include <cstdio>
#include <cstring>
#include <functional>

namespace {

struct Scene {
    TgHipSceneDesc d;
    std::vector<TgHipBvhNode> nodes;
    std::vector<TgHipPrimRec> recs;
    std::vector<TgHipTriAttr> attrs;
    std::vector<TgHipObject> objects;
    std::vector<int32_t> lights;
    std::vector<TgHipBsdf> bsdfs;
    std::vector<TgHipTexture> textures;
    std::vector<float> texels, dist, lightTris;
    std::vector<TgHipMedium> media;
    std::vector<TgHipWideNode> wide;
    std::vector<TgHipTopNode> top;

    // (vectors of exactly the counts: shrink_to_fit is not binding, so the blocks are allocated at their size)
    template<typename T> static const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
    void fix()
    {
        d.nodes = ptr(nodes); d.num_nodes = uint32_t(nodes.size());
        d.recs = ptr(recs); d.tri_attrs = ptr(attrs); d.num_recs = uint32_t(recs.size());
        d.objects = ptr(objects); d.num_objects = uint32_t(objects.size());
        d.lights = ptr(lights); d.num_lights = uint32_t(lights.size());
        d.bsdfs = ptr(bsdfs); d.num_bsdfs = uint32_t(bsdfs.size());
        d.textures = ptr(textures); d.num_textures = uint32_t(textures.size());
        d.texels = ptr(texels); d.num_texel_floats = texels.size();
        d.dist = ptr(dist); d.num_dist_floats = dist.size();
        d.light_tris = ptr(lightTris); d.num_light_tri_floats = lightTris.size();
        d.media = ptr(media); d.num_media = uint32_t(media.size());
        d.wide_nodes = ptr(wide); d.num_wide_nodes = uint32_t(wide.size());
        d.top_nodes = ptr(top); d.num_top_nodes = uint32_t(top.size());
    }
    Scene() { std::memset(&d, 0, sizeof(d)); }
    Scene(const Scene &o) = default;
};

template<typename T> T zeroed() { T t; std::memset(&t, 0, sizeof(t)); return t; }

TgHipObject object(int type, int bsdf)
{
    TgHipObject o = zeroed<TgHipObject>();
    o.type = type; o.bsdf = bsdf; o.emission = -1; o.light = -1; o.first_light_tri = -1; o.int_medium = -1; o.ext_medium = -1;
    return o;
}

TgHipBsdf bsdf(int type)
{
    TgHipBsdf b = zeroed<TgHipBsdf>();
    b.type = type; b.albedo = 0; b.roughness = -1; b.sub0 = -1; b.sub1 = -1; b.tex1 = -1; b.lobes = TGHIP_LOBE_DIFFUSE_R;
    return b;
}

void common(Scene &s)
{
    s.d.abi_version = TGHIP_ABI_VERSION;
    s.d.camera.res_x = 4; s.d.camera.res_y = 4; s.d.camera.medium = -1;
    TgHipTexture c = zeroed<TgHipTexture>();
    c.type = TGHIP_TEX_CONSTANT; c.texel_offset = -1; c.dist_offset = -1;
    s.textures.push_back(c);
}

Scene meshScene()
{
    Scene s;
    common(s);
    TgHipBvhNode n = zeroed<TgHipBvhNode>();
    n.child0 = TGHIP_MAKE_LEAF(0, 2); n.child1 = TGHIP_MAKE_LEAF(2, 1);
    s.nodes.push_back(n);
    for (int i = 0; i < 3; ++i) {
        TgHipPrimRec r = zeroed<TgHipPrimRec>();
        r.meta = (uint32_t(i < 2 ? TGHIP_REC_TRIANGLE : TGHIP_REC_QUAD) << 29) | uint32_t(i < 2 ? 0 : 1);
        s.recs.push_back(r);
        TgHipTriAttr a = zeroed<TgHipTriAttr>();
        a.bsdf = i == 0 ? 1 : 0;
        s.attrs.push_back(a);
    }
    TgHipObject mesh = object(TGHIP_OBJ_MESH, 0);
    mesh.emission = 0; mesh.light = 0; mesh.first_light_tri = 0; mesh.num_light_tris = 2; mesh.int_medium = 0;
    s.objects.push_back(mesh);
    s.objects.push_back(object(TGHIP_OBJ_QUAD, 0));
    s.lights.push_back(0);
    s.lightTris.assign(2*10 + 1, 0.5f);
    s.bsdfs.push_back(bsdf(TGHIP_BSDF_LAMBERT));
    s.bsdfs[0].albedo = 1;
    s.bsdfs.push_back(bsdf(TGHIP_BSDF_SMOOTH_COAT));
    s.bsdfs[1].sub0 = 0;
    TgHipTexture b = zeroed<TgHipTexture>();
    b.type = TGHIP_TEX_BITMAP; b.flags = TGHIP_TEXF_RGB | TGHIP_TEXF_VALID; b.w = 2; b.h = 2; b.texel_offset = 0; b.dist_offset = 0;
    s.textures.push_back(b);
    s.texels.assign(2*2*3, 0.5f);
    const float tables[15] = {1.0f, 1.0f,  0.0f, 0.5f, 1.0f,  1.0f, 1.0f, 1.0f, 1.0f,  0.0f, 0.5f, 1.0f, 0.0f, 0.5f, 1.0f};   // mpdf[2] mcdf[3] pdf[4] cdf[6]
    s.dist.assign(tables, tables + 15);
    TgHipMedium m = zeroed<TgHipMedium>();
    m.phase_type = TGHIP_PHASE_ISOTROPIC; m.trans_type = TGHIP_TRANS_EXPONENTIAL; m.medium_type = TGHIP_MEDIUM_HOMOGENEOUS;
    s.media.push_back(m);
    TgHipWideNode w = zeroed<TgHipWideNode>();
    w.exp[0] = w.exp[1] = w.exp[2] = 127; w.leaf_valid = 0x13u;   // slot 0: the two triangles, slot 1: the quad
    s.wide.push_back(w);
    s.d.camera.type = TGHIP_CAMERA_THINLENS; s.d.camera.aperture_type = TGHIP_APERTURE_BITMAP;
    s.d.camera.aperture_w = 2; s.d.camera.aperture_h = 2; s.d.camera.aperture_dist = 0; s.d.camera.medium = 0;
    s.fix();
    return s;
}

Scene flatScene()
{
    Scene s;
    common(s);
    TgHipBvhNode n = zeroed<TgHipBvhNode>();
    n.child0 = TGHIP_MAKE_LEAF(0, 1); n.child1 = TGHIP_MAKE_LEAF(1, 1);
    s.nodes.push_back(n);
    for (int i = 0; i < 2; ++i) {
        TgHipPrimRec r = zeroed<TgHipPrimRec>();
        r.meta = (uint32_t(TGHIP_REC_QUAD) << 29) | uint32_t(i);
        s.recs.push_back(r);
        s.attrs.push_back(zeroed<TgHipTriAttr>());
        s.objects.push_back(object(TGHIP_OBJ_QUAD, 0));
    }
    s.objects[1].emission = 0; s.objects[1].light = 0;
    s.lights.push_back(1);
    s.bsdfs.push_back(bsdf(TGHIP_BSDF_LAMBERT));
    TgHipTopNode t = zeroed<TgHipTopNode>();
    t.child[0] = ~0; t.child[1] = ~1; t.child[2] = t.child[3] = TGHIP_TOP_EMPTY;
    s.top.push_back(t);
    s.fix();
    return s;
}

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) { g_state = g_state*6364136223846793005ull + 1442695040888963407ull; return uint32_t((g_state >> 33) % n); }

int64_t boundary(int64_t n)
{
    const int64_t v[7] = {-2, -1, 0, n - 1, n, n + 1, INT32_MAX};
    return v[rnd(7)];
}

typedef std::function<void(Scene &)> Mutation;

// every field checkScene follows or switches on, with the size of what it indexes
std::vector<Mutation> mutations(const Scene &base)
{
    std::vector<Mutation> m;
#define FIELD(expr, n) m.push_back([](Scene &s) { typedef decltype(expr) F; (expr) = F(boundary(int64_t(n))); })
    for (size_t k = 0; k < base.objects.size(); ++k) {
        m.push_back([k](Scene &s) { s.objects[k].type = int32_t(boundary(10)); });
        m.push_back([k](Scene &s) { s.objects[k].bsdf = int32_t(boundary(s.d.num_bsdfs)); });
        m.push_back([k](Scene &s) { s.objects[k].emission = int32_t(boundary(s.d.num_textures)); });
        m.push_back([k](Scene &s) { s.objects[k].light = int32_t(boundary(s.d.num_lights)); });
        m.push_back([k](Scene &s) { s.objects[k].int_medium = int32_t(boundary(s.d.num_media)); });
        m.push_back([k](Scene &s) { s.objects[k].ext_medium = int32_t(boundary(s.d.num_media)); });
        m.push_back([k](Scene &s) { s.objects[k].first_light_tri = int32_t(boundary(int64_t(s.d.num_light_tri_floats))); });
        m.push_back([k](Scene &s) { s.objects[k].num_light_tris = int32_t(boundary(2)); });
    }
    for (size_t k = 0; k < base.bsdfs.size(); ++k) {
        m.push_back([k](Scene &s) { s.bsdfs[k].type = int32_t(boundary(19)); });
        m.push_back([k](Scene &s) { s.bsdfs[k].type = int32_t(rnd(19)); });
        m.push_back([k](Scene &s) { s.bsdfs[k].distribution = int32_t(boundary(3)); });
        m.push_back([k](Scene &s) { s.bsdfs[k].albedo = int32_t(boundary(s.d.num_textures)); });
        m.push_back([k](Scene &s) { s.bsdfs[k].roughness = int32_t(boundary(s.d.num_textures)); });
        m.push_back([k](Scene &s) { s.bsdfs[k].tex1 = int32_t(boundary(s.d.num_textures)); });
        m.push_back([k](Scene &s) { s.bsdfs[k].bump1 = int32_t(boundary(s.d.num_textures + 1)); });
        m.push_back([k](Scene &s) { s.bsdfs[k].sub0 = int32_t(boundary(s.d.num_bsdfs)); });
        m.push_back([k](Scene &s) { s.bsdfs[k].sub1 = int32_t(boundary(s.d.num_bsdfs)); });
        m.push_back([k](Scene &s) { s.bsdfs[k].lobes ^= TGHIP_LOBE_FORWARD; });
    }
    for (size_t k = 0; k < base.textures.size(); ++k) {
        m.push_back([k](Scene &s) { s.textures[k].type = int32_t(boundary(5)); });
        m.push_back([k](Scene &s) { s.textures[k].w = int32_t(boundary(2)); });
        m.push_back([k](Scene &s) { s.textures[k].h = int32_t(boundary(2)); });
        m.push_back([k](Scene &s) { s.textures[k].w = 65534 + int32_t(rnd(3)); });
        m.push_back([k](Scene &s) { s.textures[k].res_u = int32_t(boundary(1)); });
        m.push_back([k](Scene &s) { s.textures[k].flags ^= TGHIP_TEXF_RGB; });
        m.push_back([k](Scene &s) { s.textures[k].texel_offset = boundary(int64_t(s.d.num_texel_floats)); });
        m.push_back([k](Scene &s) { s.textures[k].dist_offset = boundary(int64_t(s.d.num_dist_floats)); });
        m.push_back([k](Scene &s) { s.textures[k].texel_offset = INT64_MAX - int64_t(rnd(3)); });
        m.push_back([k](Scene &s) { s.textures[k].dist_offset = INT64_MAX - int64_t(rnd(3)); });
    }
    for (size_t k = 0; k < base.recs.size(); ++k) {
        m.push_back([k](Scene &s) { s.recs[k].meta = (rnd(8) << 29) | (uint32_t(boundary(s.d.num_objects)) & 0x1FFFFFFFu); });
        m.push_back([k](Scene &s) { s.recs[k].meta = (s.recs[k].meta & 0x1FFFFFFFu) | (rnd(8) << 29); });
        m.push_back([k](Scene &s) { s.attrs[k].bsdf = int32_t(boundary(s.d.num_bsdfs)); });
        m.push_back([k](Scene &s) { const uint32_t v = uint32_t(boundary(rnd(2) ? s.d.num_nodes : s.d.num_wide_nodes)); std::memcpy(&s.recs[k].c[rnd(3)], &v, 4); });
    }
    for (int c = 0; c < 2; ++c) {
        m.push_back([c](Scene &s) { (c ? s.nodes[0].child1 : s.nodes[0].child0) = int32_t(boundary(s.d.num_nodes)); });
        m.push_back([c](Scene &s) { (c ? s.nodes[0].child1 : s.nodes[0].child0) = TGHIP_MAKE_LEAF(uint32_t(boundary(s.d.num_recs)) & 0x07FFFFFFu, rnd(16)); });
    }
    if (!base.wide.empty()) {
        FIELD(s.wide[0].child_base, s.d.num_wide_nodes);
        FIELD(s.wide[0].rec_base, s.d.num_recs);
        FIELD(s.wide[0].reserved, 1);
        m.push_back([](Scene &s) { s.wide[0].leaf_valid = rnd(2) ? rnd(0xFFFFu) : 0xFFFFFFFFu; });
        m.push_back([](Scene &s) { s.wide[0].imask = uint8_t(rnd(256)); });
        m.push_back([](Scene &s) { s.wide[0].exp[rnd(3)] = uint8_t(rnd(2) ? 0 : 255); });
    }
    if (!base.media.empty()) {
        FIELD(s.media[0].phase_type, 3);
        FIELD(s.media[0].medium_type, 3);
        FIELD(s.media[0].trans_type, 9);
        m.push_back([](Scene &s) { s.media[0].trans_type = TGHIP_TRANS_INTERPOLATED; });
    }
    if (!base.top.empty()) {
        m.push_back([](Scene &s) { s.top[0].child[rnd(4)] = int32_t(boundary(s.d.num_top_nodes)); });
        m.push_back([](Scene &s) { s.top[0].child[rnd(4)] = ~int32_t(boundary(s.d.num_recs)); });
    }
    m.push_back([](Scene &s) { if (!s.lights.empty()) s.lights[0] = int32_t(boundary(s.d.num_objects)); });
    FIELD(s.d.camera.type, 4);
    FIELD(s.d.camera.medium, s.d.num_media);
    FIELD(s.d.camera.aperture_type, 3);
    FIELD(s.d.camera.aperture_w, 2);
    FIELD(s.d.camera.aperture_h, 2);
    FIELD(s.d.camera.aperture_dist, s.d.num_dist_floats);
    FIELD(s.d.camera.blade_count, 4);
    FIELD(s.d.camera.res_x, 4);
    FIELD(s.d.abi_version, TGHIP_ABI_VERSION);
    // counts: down to zero (arrays stay), or up from zero where the array is NULL
    m.push_back([](Scene &s) { uint32_t *c[7] = {&s.d.num_nodes, &s.d.num_recs, &s.d.num_objects, &s.d.num_lights, &s.d.num_bsdfs, &s.d.num_textures, &s.d.num_media}; *c[rnd(7)] = 0; });
    m.push_back([](Scene &s) { uint64_t *c[3] = {&s.d.num_texel_floats, &s.d.num_dist_floats, &s.d.num_light_tri_floats}; *c[rnd(3)] = 0; });
    m.push_back([](Scene &s) {
        static uint32_t prims[2];
        static const float boxes[2*8] = {0.0f};
        s.d.num_instances = 1 + rnd(2); s.d.num_top_recs = uint32_t(boundary(s.d.num_recs)); s.d.num_inst_prims = rnd(3);
        prims[0] = uint32_t(boundary(s.d.num_recs)); prims[1] = uint32_t(boundary(s.d.num_recs));
        if (rnd(4)) s.d.inst_prims = prims;
        if (rnd(4)) s.d.inst_leaf_boxes = boxes;
        if (rnd(4)) s.d.inst_tight_boxes = boxes;
    });
    m.push_back([](Scene &s) { if (!s.d.num_infinite_lights) s.d.num_infinite_lights = 1; });
    m.push_back([](Scene &s) { if (!s.d.top_nodes) s.d.num_top_nodes = 1; if (!s.d.wide_nodes) s.d.num_wide_nodes = 1; if (!s.d.media) s.d.num_media = 1; });
    m.push_back([](Scene &s) { static const uint32_t one = 0; s.d.sobol_matrices = &one; s.d.num_sobol_words = uint64_t(TGHIP_SOBOL_DIMS)*TGHIP_SOBOL_BITS - rnd(2); });
    // array pointers to NULL, counts left standing
    m.push_back([](Scene &s) {
        switch (rnd(12)) {
        case 0: s.d.nodes = nullptr; break;      case 1: s.d.recs = nullptr; break;        case 2: s.d.tri_attrs = nullptr; break;
        case 3: s.d.objects = nullptr; break;    case 4: s.d.lights = nullptr; break;      case 5: s.d.bsdfs = nullptr; break;
        case 6: s.d.textures = nullptr; break;   case 7: s.d.texels = nullptr; break;      case 8: s.d.dist = nullptr; break;
        case 9: s.d.light_tris = nullptr; break; case 10: s.d.media = nullptr; break;      default: s.d.wide_nodes = nullptr; s.d.top_nodes = nullptr; break;
        }
    });
#undef FIELD
    return m;
}

} // namespace

int main(int argc, char **argv)
{
    const long rounds = argc > 1 ? std::atol(argv[1]) : 200000;
    const Scene bases[2] = {meshScene(), flatScene()};
    std::vector<Mutation> muts[2] = {mutations(bases[0]), mutations(bases[1])};
    std::string error;
    for (int b = 0; b < 2; ++b) {
        SceneTraits t;
        const int rc = checkScene(&bases[b].d, SceneCheckOptions(), t, error);
        if (rc != TGHIP_OK) { std::fprintf(stderr, "base description %d refused: %s\n", b, error.c_str()); return 1; }
    }
    long accepted = 0, invalid = 0, unsupported = 0;
    for (long i = 0; i < rounds; ++i) {
        const int b = int(rnd(2));
        Scene s(bases[b]);
        s.fix();
        const int count = 1 + int(rnd(2));
        for (int k = 0; k < count; ++k)
            muts[b][rnd(uint32_t(muts[b].size()))](s);
        SceneCheckOptions opt;
        opt.top_tree = rnd(8) != 0;
        opt.wide_node_stride = rnd(8) ? 80u : 128u;
        SceneTraits t;
        const int rc = checkScene(&s.d, opt, t, error);
        if (rc == TGHIP_OK) ++accepted;
        else if (rc == TGHIP_E_INVALID) ++invalid;
        else if (rc == TGHIP_E_UNSUPPORTED) ++unsupported;
        else { std::fprintf(stderr, "mutation %ld: unexpected return code %d\n", i, rc); return 1; }
    }
    std::printf("scene_check_fuzz: %ld mutated descriptions: %ld accepted, %ld invalid, %ld unsupported\n", rounds, accepted, invalid, unsupported);
    return 0;
}
