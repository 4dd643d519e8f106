// Stand-alone sanitizer run of the medium code on the cases of tests/medium_cases.py, no device and no Python preload:
//
//     python tests/medium_cases.py build/medium_cases              # the scenes.medium_corners scene and its case file
//     gcc -std=c99 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -c oracle/oracle.c -o build/oracle_asan.o
//     g++ -std=c++11 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/medium_cases_check.cpp \
//         $(ls tungsten_amd/csrc/host/*.cpp | grep -v -e main.cpp -e capi.cpp -e Integrator.cpp) build/oracle_asan.o -o tools/bin/medium_cases_check -lpthread
//     tools/bin/medium_cases_check build/medium_cases
//
// (the host loader's own classes, Scene::load and TraceableScene, without the C entry points of capi.cpp: those link the Integrator, which needs the device)
//
// The oracle restates the device's medium code to the letter -- an `interpolated` medium reads its operands through (&m)[1] and (&m)[2], the entries
// behind it -- so a case that sent one of those reads past the media array would do the same on the GPU, where an out-of-bounds read is not a test
// failure but a fault on a shared machine.  The scene is loaded by the host loader; the media array is then copied into a heap block of EXACTLY its
// size (the loader's own vector may have spare capacity), so a read one entry past it is a sanitizer report.  oracle_medium_cases runs over every case
// of every medium; per medium the program prints how many cases sampled a distance, exited and scattered, and a checksum of the result words.
// Exit 0 without a report is the result (profiles/medium_units/host_sanitizers.txt).
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

extern "C" void oracle_medium_cases(const TgHipSceneDesc *s, int n, const int32_t *medium, const int32_t *state_bounce, const float *p, const float *d,
                                    const float *max_t, const float *wo, const float *xi_dist, int nxd, const float *xi_phase, int nxp, uint32_t *out);

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: medium_cases_check <directory written by `python tests/medium_cases.py <directory>`>\n"); return 2; }
    const std::string dir = argv[1], scenePath = dir + "/medium_corners.json", casePath = dir + "/medium_cases.bin";
    std::unique_ptr<tungsten_amd::Scene> scene;
    std::unique_ptr<tungsten_amd::TraceableScene> flattened;
    try {
        scene = tungsten_amd::Scene::load(scenePath);
        flattened.reset(new tungsten_amd::TraceableScene(*scene, nullptr, 0));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "medium_cases_check: %s: %s\n", scenePath.c_str(), e.what());
        return 1;
    }
    SceneTraits traits;
    std::string error;
    if (checkScene(&flattened->desc(), SceneCheckOptions(), traits, error) != TGHIP_OK) { std::fprintf(stderr, "medium_cases_check: %s\n", error.c_str()); return 1; }
    TgHipSceneDesc d = flattened->desc();
    // a malloc'ed copy of the media: the block ends where the table ends
    TgHipMedium *media = static_cast<TgHipMedium *>(std::malloc(size_t(d.num_media)*sizeof(TgHipMedium)));
    if (!media || d.num_media == 0) { std::fprintf(stderr, "medium_cases_check: the scene has no media\n"); return 1; }
    std::memcpy(media, d.media, size_t(d.num_media)*sizeof(TgHipMedium));
    d.media = media;

    FILE *f = std::fopen(casePath.c_str(), "rb");
    uint32_t header[4] = {0, 0, 0, 0};
    if (!f || std::fread(header, sizeof(header), 1, f) != 1) { std::fprintf(stderr, "medium_cases_check: cannot read %s\n", casePath.c_str()); return 1; }
    const uint32_t count = header[0], n = header[1], nxd = header[2], nxp = header[3];
    if (count == 0 || count > d.num_media || n == 0 || n > (1u << 20) || nxd > 64 || nxp > 64) { std::fprintf(stderr, "medium_cases_check: %s does not fit the scene\n", casePath.c_str()); return 1; }
    const size_t stride = 11 + nxd + nxp;
    std::vector<float> rec(size_t(n)*stride), p(size_t(n)*3), dir3(size_t(n)*3), wo(size_t(n)*3), maxT(n), xd(size_t(n)*nxd), xp(size_t(n)*nxp);
    std::vector<int32_t> medium(n), bounce(n);
    std::vector<uint32_t> out(size_t(n)*26);
    uint32_t operands = 0;
    for (uint32_t mi = 0; mi < count; ++mi) {
        int32_t index = -1;
        if (std::fread(&index, sizeof(index), 1, f) != 1 || std::fread(rec.data(), sizeof(float), rec.size(), f) != rec.size()) {
            std::fprintf(stderr, "medium_cases_check: %s ends early\n", casePath.c_str());
            return 1;
        }
        if (index < 0 || uint32_t(index) >= d.num_media || traits.mediumOperand[size_t(index)]) {
            std::fprintf(stderr, "medium_cases_check: medium %u of the case file names entry %d, which is no medium of the scene\n", mi, index);
            return 1;
        }
        for (uint32_t i = 0; i < n; ++i) {
            const float *r = &rec[size_t(i)*stride];
            std::memcpy(&bounce[i], r, 4);
            std::memcpy(&p[size_t(i)*3], r + 1, 12);
            std::memcpy(&dir3[size_t(i)*3], r + 4, 12);
            maxT[i] = r[7];
            std::memcpy(&wo[size_t(i)*3], r + 8, 12);
            std::memcpy(&xd[size_t(i)*nxd], r + 11, nxd*sizeof(float));
            std::memcpy(&xp[size_t(i)*nxp], r + 11 + nxd, nxp*sizeof(float));
            medium[i] = index;
        }
        oracle_medium_cases(&d, int(n), medium.data(), bounce.data(), p.data(), dir3.data(), maxT.data(), wo.data(), xd.data(), int(nxd), xp.data(), int(nxp), out.data());
        uint32_t ok = 0, exited = 0, hash = 2166136261u;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t *o = &out[size_t(i)*26];
            ok += o[0]; exited += o[0] & o[5];
            for (int k = 0; k < 26; ++k) hash = (hash ^ o[k])*16777619u;
        }
        const bool interpolated = d.media[index].trans_type == TGHIP_TRANS_INTERPOLATED;
        operands += interpolated ? 2u : 0u;
        std::printf("medium %2u (entry %2d, medium type %d, transmittance %d%s): %u cases, sampled %u, exited %u, scattered %u, words %08x\n", mi, index,
                    d.media[index].medium_type, d.media[index].trans_type, interpolated ? ", operands in the two entries behind it" : "", n, ok, exited,
                    ok - exited, hash);
    }
    std::fclose(f);
    if (count + operands != d.num_media) { std::fprintf(stderr, "medium_cases_check: %u media and %u operand entries are not the scene's %u entries\n", count, operands, d.num_media); return 1; }
    std::free(media);
    std::printf("medium_cases_check: no out-of-bounds read of the media table, no undefined behaviour\n");
    return 0;
}
