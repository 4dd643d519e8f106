// TEST INFRASTRUCTURE, not product code: drives the reference's own NL-means filter (denoiser/NlMeans.hpp, included from the reference's tree)
// on raw float planes, so that its results can be recorded as fixtures (tools/make_denoise_golden.py -> tests/golden/nlmeans.npz) and timed
// (tools/denoise_bench.py).  Built into oracle/_ref/ against the reference's libcore.a; never linked by the product.
//
//   ref_nlmeans W H C F R k varianceScale threads in.raw out.raw [runs]
//     C: 1 (nlMeans<float>) or 3 (nlMeans<Vec3f>); in.raw: image, guide, variance -- W*H*C float32 each; out.raw: W*H*C float32;
//     prints the seconds of each of `runs` calls (default 1).
#include "denoiser/NlMeans.hpp"

#include "thread/ThreadUtils.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace Tungsten;

template<typename Texel>
static int run(int w, int h, int F, int R, float k, float scale, const std::vector<float> &in, const char *outPath, int runs)
{
    const size_t n = size_t(w)*h*(sizeof(Texel)/sizeof(float));
    Pixmap<Texel> image(w, h, reinterpret_cast<const Texel *>(in.data()));
    Pixmap<Texel> guide(w, h, reinterpret_cast<const Texel *>(in.data() + n));
    Pixmap<Texel> variance(w, h, reinterpret_cast<const Texel *>(in.data() + 2*n));
    Pixmap<Texel> result;
    for (int i = 0; i < runs; ++i) {
        auto t0 = std::chrono::steady_clock::now();
        result = nlMeans(image, guide, variance, F, R, k, scale, false);
        std::printf("%.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    FILE *f = std::fopen(outPath, "wb");
    if (!f || std::fwrite(&result[0], sizeof(float), n, f) != n) { std::fprintf(stderr, "cannot write %s\n", outPath); return 1; }
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 11) { std::fprintf(stderr, "usage: ref_nlmeans W H C F R k varianceScale threads in.raw out.raw [runs]\n"); return 2; }
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), C = std::atoi(argv[3]), F = std::atoi(argv[4]), R = std::atoi(argv[5]);
    const float k = float(std::atof(argv[6])), scale = float(std::atof(argv[7]));
    const int threads = std::atoi(argv[8]), runs = argc > 11 ? std::atoi(argv[11]) : 1;
    if (w < 1 || h < 1 || (C != 1 && C != 3) || threads < 1) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const size_t n = size_t(w)*h*C;
    std::vector<float> in(3*n);
    FILE *f = std::fopen(argv[9], "rb");
    if (!f || std::fread(in.data(), sizeof(float), 3*n, f) != 3*n) { std::fprintf(stderr, "cannot read %s\n", argv[9]); return 1; }
    std::fclose(f);
    ThreadUtils::startThreads(threads);
    return C == 1 ? run<float>(w, h, F, R, k, scale, in, argv[10], runs) : run<Vec3f>(w, h, F, R, k, scale, in, argv[10], runs);
}
