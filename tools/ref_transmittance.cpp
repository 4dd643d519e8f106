// The reference's own TraceBase::generalizedShadowRay on caller-supplied rays: the yardstick of tghip_query_transmittance.  Built against the
// reference's headers and oracle/_ref/libcore.a by tools/make_transmittance_golden.py into the git-ignored oracle/_ref/ref_transmittance; what it
// answers for the cases of tests/transmittance_cases.py is recorded in tests/golden/transmittance_cases.npz.
//
//     ref_transmittance <scene.json> <cases.txt> <out.txt>
//
// cases.txt, whitespace-separated: per group a line `group <n> <medium> <end_cap> <bounce> <starts_on_surface> <ends_on_surface> <per_ray_media>`
// -- the start medium and the end cap by their JSON names, `-` = none -- and n lines `<o.x> <o.y> <o.z> <tmin> <d.x> <d.y> <d.z> <tmax> [<medium>]`,
// every float as the eight hex digits of its bits, the medium name only with per_ray_media = 1.  out.txt: per ray `<r> <g> <b> <crossed> <end>`:
// generalizedShadowRay's three floats as hex bits, and -- for the census of the cases only, from a second walk of this file's own -- the see-through
// surfaces crossed and what ended the walk (0 a miss, 1 the end cap, 2 a surface without a forward lobe, 3 a transparency of zero, 4 max_bounces,
// 5 a miss although the end cap's own Primitive::intersect finds the segment: the scene's Embree tree culled its box).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include <sstream>
#include "integrators/TraceBase.hpp"
#include "primitives/Primitive.hpp"
#include "math/Quaternion.hpp"
#include "bvh/BinaryBvh.hpp"
// Instance keeps its masters private, and Instance::loadResources does not reach them: open the one class definition up (every header it uses is
// included already)
#define private public
#define class struct
#include "primitives/Instance.hpp"
#undef private
#undef class
#include "integrators/path_tracer/PathTraceIntegrator.hpp"
#include "io/DirectoryChange.hpp"
#include "io/Scene.hpp"
#include "media/Medium.hpp"
#include "primitives/EmbreeUtil.hpp"
#include "primitives/Primitive.hpp"
#include "renderer/TraceableScene.hpp"
#include "sampling/UniformPathSampler.hpp"
#include "thread/ThreadUtils.hpp"

using namespace Tungsten;

namespace {

class ShadowTracer : public TraceBase
{
public:
    ShadowTracer(TraceableScene *scene, const TraceSettings &settings) : TraceBase(scene, settings, 0) {}
    using TraceBase::generalizedShadowRay;

    // how far generalizedShadowRay's loop gets on this ray, for the census: the same steps without the throughput
    void census(Ray ray, const Primitive *endCap, int bounce, int &crossed, int &end) const
    {
        IntersectionTemporary data;
        IntersectionInfo info;
        float remaining = ray.farT();
        crossed = 0;
        for (;;) {
            const bool hit = _scene->intersect(ray, data, info);
            if (!hit) {
                // nothing found -- although the end cap's own intersect() finds the segment: Embree's slab test kept the ray out of its box
                IntersectionTemporary probe;
                Ray copy(ray);
                end = endCap && endCap->intersect(copy, probe) ? 5 : 0;
                return;
            }
            if (info.primitive == endCap) { end = 1; return; }
            if (!info.bsdf->lobes().hasForward()) { end = 2; return; }
            SurfaceScatterEvent event = makeLocalScatterEvent(data, info, ray, nullptr);
            if (info.bsdf->eval(event.makeForwardEvent(), false) == 0.0f) { end = 3; return; }
            crossed++;
            if (++bounce >= _settings.maxBounces) { end = 4; return; }
            ray.setPos(ray.hitpoint());
            remaining -= ray.farT();
            ray.setNearT(info.epsilon);
            ray.setFarT(remaining);
        }
    }
};

float fromHex(const std::string &s)
{
    const uint32_t bits = uint32_t(std::stoul(s, nullptr, 16));
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

uint32_t bitsOf(float f)
{
    uint32_t bits;
    std::memcpy(&bits, &f, 4);
    return bits;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 4) {
        std::fprintf(stderr, "usage: ref_transmittance <scene.json> <cases.txt> <out.txt>\n");
        return 2;
    }
    EmbreeUtil::initDevice();
    ThreadUtils::startThreads(1);
    std::unique_ptr<Scene> scene;
    std::unique_ptr<TraceableScene> ts;
    try {
        Path scenePath(argv[1]);
        Path dir = scenePath.parent();
        scene.reset(Scene::load(scenePath, nullptr, &dir));
        scene->loadResources();
        DirectoryChange context(dir);
        // (Instance::loadResources does not reach its masters, Instance.cpp:265-282)
        for (const std::shared_ptr<Primitive> &p : scene->primitives())
            if (Instance *inst = dynamic_cast<Instance *>(p.get()))
                for (std::shared_ptr<Primitive> &m : inst->_master)
                    m->loadResources();
        ts.reset(scene->makeTraceable(0xBA5EBA11u));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ref_transmittance: %s\n", e.what());
        return 1;
    }
    PathTraceIntegrator *pti = dynamic_cast<PathTraceIntegrator *>(scene->integrator());
    if (!pti) { std::fprintf(stderr, "ref_transmittance: the scene does not use the path_tracer integrator\n"); return 1; }
    ShadowTracer tracer(ts.get(), pti->settings());
    UniformPathSampler sampler(0xBA5EBA11u);

    auto mediumNamed = [&](const std::string &name, const Medium *&out) {
        out = nullptr;
        if (name == "-") return true;
        for (const std::shared_ptr<Medium> &m : scene->media())
            if (m->name() == name) { out = m.get(); return true; }
        std::fprintf(stderr, "ref_transmittance: no medium named '%s'\n", name.c_str());
        return false;
    };

    std::ifstream in(argv[2]);
    std::FILE *out = std::fopen(argv[3], "w");
    if (!in || !out) { std::fprintf(stderr, "ref_transmittance: cannot open the case or the output file\n"); return 1; }
    std::string word;
    while (in >> word) {
        if (word != "group") { std::fprintf(stderr, "ref_transmittance: expected `group`, found '%s'\n", word.c_str()); return 1; }
        unsigned n = 0;
        std::string mediumName, capName;
        int bounce = 0, starts = 0, ends = 0, perRay = 0;
        in >> n >> mediumName >> capName >> bounce >> starts >> ends >> perRay;
        if (!in) { std::fprintf(stderr, "ref_transmittance: malformed group line\n"); return 1; }
        const Medium *groupMedium = nullptr;
        if (!mediumNamed(mediumName, groupMedium)) return 1;
        const Primitive *endCap = nullptr;
        if (capName != "-") {
            for (const std::shared_ptr<Primitive> &p : scene->primitives())
                if (p->name() == capName) endCap = p.get();
            if (!endCap) { std::fprintf(stderr, "ref_transmittance: no primitive named '%s'\n", capName.c_str()); return 1; }
        }
        for (unsigned i = 0; i < n; ++i) {
            float f[8];
            for (int k = 0; k < 8; ++k) { in >> word; f[k] = fromHex(word); }
            const Medium *medium = groupMedium;
            if (perRay) { in >> word; if (!mediumNamed(word, medium)) return 1; }
            if (!in) { std::fprintf(stderr, "ref_transmittance: the case file ends inside a group\n"); return 1; }
            Ray ray(Vec3f(f[0], f[1], f[2]), Vec3f(f[4], f[5], f[6]), f[3], f[7]);
            int crossed = 0, end = 0;
            tracer.census(ray, endCap, bounce, crossed, end);
            const Vec3f t = tracer.generalizedShadowRay(sampler, ray, medium, endCap, starts != 0, ends != 0, bounce);
            std::fprintf(out, "%08x %08x %08x %d %d\n", bitsOf(t.x()), bitsOf(t.y()), bitsOf(t.z()), crossed, end);
        }
    }
    std::fclose(out);
    return 0;
}
