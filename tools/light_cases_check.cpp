// Stand-alone sanitizer run of the light code's table lookups on the cases of tests/light_cases.py, no device and no Python preload:
//
//     python tests/light_cases.py build/light_cases                 # the six scenes.light_corners scenes and their case files
//     gcc -std=c99 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -c oracle/oracle.c -o build/oracle_asan.o
//     g++ -std=c++11 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/light_cases_check.cpp \
//         $(ls tungsten_amd/csrc/host/*.cpp | grep -v -e main.cpp -e capi.cpp -e Integrator.cpp) build/oracle_asan.o -o tools/bin/light_cases_check -lpthread
//     TUNGSTEN_HIP_SKYDOME_TABLES=tungsten_amd/data/skydome_tables.bin tools/bin/light_cases_check build/light_cases
//
// (the host loader's own classes, Scene::load and TraceableScene, without the C entry points of capi.cpp: those link the Integrator, which needs the device)
//
// The oracle restates the device's table lookups to the letter -- the mesh emitter's CDF search (upper_bound over light_tris), the bitmap
// environment's marginal and conditional tables, the cube's face CDF -- so a crafted input that drove one of those indices out of its table would do
// the same on the GPU, where an out-of-bounds read is not a test failure but a fault on a shared machine.  Each scene is loaded by the host loader;
// the tables the light code indexes are then copied into heap blocks of EXACTLY their size (the loader's own vectors may have spare capacity), so a
// read one element past a table is a sanitizer report.  oracle_light_cases runs over every case of every light; per light the program prints how
// many cases chose, sampled and hit, and a checksum of the result words.  Exit 0 without a report is the result (profiles/light_cases_check.txt).
#include "../tungsten_amd/csrc/host/Scene.hpp"
#include "../tungsten_amd/csrc/host/SceneCheck.hpp"
#include "../tungsten_amd/csrc/host/TraceableScene.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

extern "C" void oracle_light_cases(const TgHipSceneDesc *s, int n, const int32_t *light, const float *p, const float *w,
                                   const float *xi_choose, int nxc, const float *xi_sample, int nxs, uint32_t *out);

namespace {

// a malloc'ed copy of n elements (nullptr for n == 0): the block ends where the table ends
template<typename T> const T *exact(const T *src, size_t n, std::vector<void *> &blocks)
{
    if (!src || n == 0) return nullptr;
    T *dst = static_cast<T *>(std::malloc(n*sizeof(T)));
    if (!dst) { std::fprintf(stderr, "light_cases_check: out of memory\n"); std::exit(1); }
    std::memcpy(dst, src, n*sizeof(T));
    blocks.push_back(dst);
    return dst;
}

int runScene(const std::string &dir, const char *which)
{
    const std::string scenePath = dir + "/light_corners_" + which + ".json", casePath = dir + "/light_cases_" + which + ".bin";
    std::unique_ptr<tungsten_amd::Scene> scene;
    std::unique_ptr<tungsten_amd::TraceableScene> flattened;
    try {
        scene = tungsten_amd::Scene::load(scenePath);
        flattened.reset(new tungsten_amd::TraceableScene(*scene, nullptr, 0));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "light_cases_check: %s: %s\n", scenePath.c_str(), e.what());
        return 1;
    }
    SceneTraits traits;
    std::string error;
    if (checkScene(&flattened->desc(), SceneCheckOptions(), traits, error) != TGHIP_OK) { std::fprintf(stderr, "light_cases_check: %s: %s\n", which, error.c_str()); return 1; }
    TgHipSceneDesc d = flattened->desc();
    std::vector<void *> blocks;
    d.objects = exact(d.objects, d.num_objects, blocks);
    d.lights = exact(d.lights, d.num_lights, blocks);
    d.textures = exact(d.textures, d.num_textures, blocks);
    d.texels = exact(d.texels, size_t(d.num_texel_floats), blocks);
    d.dist = exact(d.dist, size_t(d.num_dist_floats), blocks);
    d.light_tris = exact(d.light_tris, size_t(d.num_light_tri_floats), blocks);

    FILE *f = std::fopen(casePath.c_str(), "rb");
    uint32_t header[4] = {0, 0, 0, 0};
    if (!f || std::fread(header, sizeof(header), 1, f) != 1) { std::fprintf(stderr, "light_cases_check: cannot read %s\n", casePath.c_str()); return 1; }
    const uint32_t lights = header[0], n = header[1], nxc = header[2], nxs = header[3];
    if (lights != d.num_lights || n == 0 || n > (1u << 20) || nxc > 64 || nxs > 64) { std::fprintf(stderr, "light_cases_check: %s does not fit the scene\n", casePath.c_str()); return 1; }
    const size_t stride = 6 + nxc + nxs;
    std::vector<float> rec(size_t(n)*stride), p(size_t(n)*3), w(size_t(n)*3), xc(size_t(n)*nxc), xs(size_t(n)*nxs);
    std::vector<int32_t> slot(n);
    std::vector<uint32_t> out(size_t(n)*20);
    for (uint32_t li = 0; li < lights; ++li) {
        if (std::fread(rec.data(), sizeof(float), rec.size(), f) != rec.size()) { std::fprintf(stderr, "light_cases_check: %s ends early\n", casePath.c_str()); return 1; }
        for (uint32_t i = 0; i < n; ++i) {
            const float *r = &rec[size_t(i)*stride];
            std::memcpy(&p[size_t(i)*3], r, 12);
            std::memcpy(&w[size_t(i)*3], r + 3, 12);
            std::memcpy(&xc[size_t(i)*nxc], r + 6, nxc*sizeof(float));
            std::memcpy(&xs[size_t(i)*nxs], r + 6 + nxc, nxs*sizeof(float));
            slot[i] = int32_t(li);
        }
        oracle_light_cases(&d, int(n), slot.data(), p.data(), w.data(), xc.data(), int(nxc), xs.data(), int(nxs), out.data());
        uint32_t chosen = 0, sampled = 0, hit = 0, hash = 2166136261u;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t *o = &out[size_t(i)*20];
            chosen += int32_t(o[0]) >= 0; sampled += o[2]; hit += o[9];
            for (int k = 0; k < 20; ++k) hash = (hash ^ o[k])*16777619u;
        }
        std::printf("%-6s light %2u (object %3d, type %d): %u cases, chose %u, sampled %u, hit %u, words %08x\n", which, li, d.lights[li],
                    d.objects[d.lights[li]].type, n, chosen, sampled, hit, hash);
    }
    std::fclose(f);
    for (void *b : blocks) std::free(b);
    return 0;
}

}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: light_cases_check <directory written by `python tests/light_cases.py <directory>`>\n"); return 2; }
    const char *scenes[6] = {"lean", "solids", "mesh", "all", "backs", "unknown"};
    for (const char *which : scenes)
        if (int rc = runScene(argv[1], which)) return rc;
    std::printf("light_cases_check: no out-of-bounds lookup, no undefined behaviour\n");
    return 0;
}
