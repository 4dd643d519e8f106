// The reference's own TraceBase::estimateDirect and volumeEstimateDirect at the hit (or origin) of caller-supplied rays: the yardstick of
// tghip_query_direct.  Built against the reference's headers and oracle/_ref/libcore.a by tools/make_direct_golden.py into the git-ignored
// oracle/_ref/ref_direct; what it answers for the cases of tests/direct_cases.py is recorded in tests/golden/direct_cases.npz.
//
//     ref_direct <scene.json> <cases.txt> <out.txt>
//
// cases.txt, whitespace-separated: per group a line `group <n> <spp_begin> <spp_end> <seed> <medium> <bounce> <light> <skip> <volume> <per_ray_media>`
// -- the start medium by its JSON name, `-` = none; light -1 = chooseLight, else an index into the scene's lights -- and n lines
// `<o.x> <o.y> <o.z> <tmin> <d.x> <d.y> <d.z> <tmax> [<medium>]`, every float as the eight hex digits of its bits, the medium name only with
// per_ray_media = 1.  out.txt: per ray and sample `<r> <g> <b> <t> <recorded> <taken> <legs> <light> <hit>`: the estimate's three floats and the
// transmittance's avg() as hex bits; whether a transmittance was reported (it is not the -1 it was initialised to); whether the sample was taken (the
// ray hit something / started in a medium); and -- for the census of the cases only, from a second run of the same sample through the pieces of
// sampleDirect -- the legs it reached (LEG_* below), the chosen light's index in the scene's primitives (-1 = none) and the hit primitive's.
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
#include "bsdfs/TransparencyBsdf.hpp"
#include "integrators/path_tracer/PathTraceIntegrator.hpp"
#include "io/DirectoryChange.hpp"
#include "io/Scene.hpp"
#include "math/MathUtil.hpp"
#include "media/Medium.hpp"
#include "phasefunctions/PhaseFunction.hpp"
#include "primitives/EmbreeUtil.hpp"
#include "primitives/TriangleMesh.hpp"
#include "renderer/TraceableScene.hpp"
#include "samplerecords/LightSample.hpp"
#include "samplerecords/MediumSample.hpp"
#include "sampling/PathSampleGenerator.hpp"
#include "thread/ThreadUtils.hpp"

using namespace Tungsten;

namespace {

enum {
    LEG_LIGHT_TERM = 1, LEG_BSDF_TERM = 2, LEG_DIRAC = 4, LEG_PURE_SPECULAR = 8, LEG_FORWARD = 16, LEG_INCONSISTENT = 32, LEG_FLIPPED = 64,
    LEG_MESH_REJECTED = 128, LEG_MESH_ACCEPTED = 256, LEG_CROSSED_FORWARD = 512, LEG_CROSSED_FRACTIONAL = 1024, LEG_MAX_BOUNCES = 2048,
    LEG_INSTANCE = 4096, LEG_MEDIUM_SELECTED = 8192, LEG_UNKNOWN_WEIGHT = 16384
};

// The counter-based stream of the device (csrc/hip/pt_math.h: rngStart) with `skip` numbers thrown away first
class KeyedSampler : public PathSampleGenerator
{
    UniformSampler _sampler;
    uint32 _seed, _skip;

public:
    KeyedSampler(uint32 seed, uint32 skip) : _sampler(0), _seed(seed), _skip(skip) {}

    virtual void startPath(uint32 pixelId, uint32 sample) override
    {
        uint32 a = MathUtil::hash32(_seed) ^ pixelId;
        uint32 b = MathUtil::hash32(a) + sample;
        uint32 hi = MathUtil::hash32(b), lo = MathUtil::hash32(b ^ 0x9E3779B9u);
        _sampler = UniformSampler((uint64(hi) << 32) | lo, (uint64(pixelId) << 1) | 1u);
        for (uint32 i = 0; i < _skip; ++i) _sampler.nextI();
    }
    virtual void advancePath() override {}
    virtual void saveState(OutputStreamHandle &) override {}
    virtual void loadState(InputStreamHandle &) override {}
    virtual float next1D() override final { return _sampler.next1D(); }
    virtual bool nextBoolean(float pTrue) override final { return next1D() < pTrue; }
    virtual int nextDiscrete(int numChoices) override final { return int(next1D()*numChoices); }
    virtual Vec2f next2D() override final { float a = next1D(); float b = next1D(); return Vec2f(a, b); }
    virtual UniformSampler &uniformGenerator() override final { return _sampler; }
};

class DirectTracer : public TraceBase
{
public:
    DirectTracer(TraceableScene *scene, const TraceSettings &settings) : TraceBase(scene, settings, 0) {}
    using TraceBase::estimateDirect;
    using TraceBase::sampleDirect;
    using TraceBase::volumeEstimateDirect;
    using TraceBase::volumeSampleDirect;
    using TraceBase::makeLocalScatterEvent;
    using TraceBase::chooseLight;
    using TraceBase::isConsistent;
    using TraceBase::lightSample;
    using TraceBase::bsdfSample;
    using TraceBase::volumeLightSample;
    using TraceBase::volumePhaseSample;

    const TraceableScene &scene() const { return *_scene; }
    const TraceSettings &settings() const { return _settings; }

    // the surfaces a shadow ray from `ray` towards the light goes through: generalizedShadowRay's steps without the throughput
    int shadowCensus(Ray ray, const Primitive *endCap, int bounce) const
    {
        int legs = 0;
        IntersectionTemporary data;
        IntersectionInfo info;
        float remaining = ray.farT();
        for (;;) {
            if (!_scene->intersect(ray, data, info) || info.primitive == endCap) return legs;
            if (!info.bsdf->lobes().hasForward()) return legs;
            SurfaceScatterEvent event = makeLocalScatterEvent(data, info, ray, nullptr);
            const Vec3f transparency = info.bsdf->eval(event.makeForwardEvent(), false);
            if (transparency == 0.0f) return legs;
            if (dynamic_cast<const TransparencyBsdf *>(info.bsdf)) { if (transparency != 1.0f) legs |= LEG_CROSSED_FRACTIONAL; }
            else legs |= LEG_CROSSED_FORWARD;
            if (++bounce >= _settings.maxBounces) return legs | LEG_MAX_BOUNCES;
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
        std::fprintf(stderr, "usage: ref_direct <scene.json> <cases.txt> <out.txt>\n");
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
        std::fprintf(stderr, "ref_direct: %s\n", e.what());
        return 1;
    }
    PathTraceIntegrator *pti = dynamic_cast<PathTraceIntegrator *>(scene->integrator());
    if (!pti) { std::fprintf(stderr, "ref_direct: the scene does not use the path_tracer integrator\n"); return 1; }
    DirectTracer tracer(ts.get(), pti->settings());
    const std::vector<std::shared_ptr<Primitive>> &lights = ts->lights();

    auto mediumNamed = [&](const std::string &name, const Medium *&out) {
        out = nullptr;
        if (name == "-") return true;
        for (const std::shared_ptr<Medium> &m : scene->media())
            if (m->name() == name) { out = m.get(); return true; }
        std::fprintf(stderr, "ref_direct: no medium named '%s'\n", name.c_str());
        return false;
    };
    auto primitiveIndex = [&](const Primitive *p) {
        for (size_t i = 0; i < scene->primitives().size(); ++i)
            if (scene->primitives()[i].get() == p) return int(i);
        return -1;
    };

    std::ifstream in(argv[2]);
    std::FILE *out = std::fopen(argv[3], "w");
    if (!in || !out) { std::fprintf(stderr, "ref_direct: cannot open the case or the output file\n"); return 1; }
    std::string word;
    while (in >> word) {
        if (word != "group") { std::fprintf(stderr, "ref_direct: expected `group`, found '%s'\n", word.c_str()); return 1; }
        unsigned n = 0, sppBegin = 0, sppEnd = 0, seed = 0, skip = 0;
        std::string mediumName;
        int bounce = 0, lightSlot = -1, volume = 0, perRay = 0;
        in >> n >> sppBegin >> sppEnd >> seed >> mediumName >> bounce >> lightSlot >> skip >> volume >> perRay;
        if (!in) { std::fprintf(stderr, "ref_direct: malformed group line\n"); return 1; }
        if (lightSlot >= int(lights.size())) { std::fprintf(stderr, "ref_direct: the scene has no light %d\n", lightSlot); return 1; }
        const Medium *groupMedium = nullptr;
        if (!mediumNamed(mediumName, groupMedium)) return 1;
        const Primitive *fixedLight = lightSlot >= 0 ? lights[lightSlot].get() : nullptr;
        KeyedSampler sampler(seed, skip);
        for (unsigned i = 0; i < n; ++i) {
            float f[8];
            for (int k = 0; k < 8; ++k) { in >> word; f[k] = fromHex(word); }
            const Medium *medium = groupMedium;
            if (perRay) { in >> word; if (!mediumNamed(word, medium)) return 1; }
            if (!in) { std::fprintf(stderr, "ref_direct: the case file ends inside a group\n"); return 1; }
            for (unsigned s = sppBegin; s < sppEnd; ++s) {
                Vec3f estimate(0.0f), transmittance(-1.0f);
                int taken = 0, legs = 0, chosen = -1, hitPrimitive = -1;
                if (volume) {
                    if (medium) {
                        taken = 1;
                        const Ray parent(Vec3f(f[0], f[1], f[2]), Vec3f(f[4], f[5], f[6]), f[3], f[7]);
                        MediumSample ms;
                        ms.p = parent.pos();
                        ms.phase = const_cast<PhaseFunction *>(medium->phaseFunction(ms.p));
                        sampler.startPath(i, s);
                        estimate = fixedLight ? tracer.volumeSampleDirect(*fixedLight, sampler, ms, medium, bounce, parent)
                                              : tracer.volumeEstimateDirect(sampler, ms, medium, bounce, parent);
                        // the census: the same sample through the pieces
                        sampler.startPath(i, s);
                        float weight = 1.0f;
                        const Primitive *light = fixedLight ? fixedLight : tracer.chooseLight(sampler, ms.p, weight);
                        if (light) {
                            chosen = primitiveIndex(light);
                            if (light->isDirac()) legs |= LEG_DIRAC;
                            if (light->approximateRadiance(0, ms.p) < 0.0f) legs |= LEG_UNKNOWN_WEIGHT;
                            if (tracer.volumeLightSample(sampler, ms, *light, medium, bounce, parent) != 0.0f) legs |= LEG_LIGHT_TERM;
                            if (!light->isDirac() && tracer.volumePhaseSample(*light, sampler, ms, medium, bounce, parent) != 0.0f) legs |= LEG_BSDF_TERM;
                        }
                    }
                } else {
                    Ray ray(Vec3f(f[0], f[1], f[2]), Vec3f(f[4], f[5], f[6]), f[3], f[7]);
                    IntersectionTemporary data;
                    IntersectionInfo info;
                    if (tracer.scene().intersect(ray, data, info)) {
                        taken = 1;
                        hitPrimitive = primitiveIndex(info.primitive);
                        sampler.startPath(i, s);
                        SurfaceScatterEvent event = tracer.makeLocalScatterEvent(data, info, ray, &sampler);
                        estimate = fixedLight ? tracer.sampleDirect(*fixedLight, event, medium, bounce, ray, &transmittance)
                                              : tracer.estimateDirect(event, medium, bounce, ray, &transmittance);
                        // the census: the same sample through the pieces
                        sampler.startPath(i, s);
                        SurfaceScatterEvent ev = tracer.makeLocalScatterEvent(data, info, ray, &sampler);
                        if (ev.flippedFrame) legs |= LEG_FLIPPED;
                        if (dynamic_cast<const Instance *>(info.primitive)) legs |= LEG_INSTANCE;
                        float weight = 1.0f;
                        const Primitive *light = fixedLight ? fixedLight : tracer.chooseLight(sampler, info.p, weight);
                        if (light) {
                            chosen = primitiveIndex(light);
                            if (light->isDirac()) legs |= LEG_DIRAC;
                            if (light->approximateRadiance(0, info.p) < 0.0f) legs |= LEG_UNKNOWN_WEIGHT;
                            if (info.bsdf->lobes().isPureSpecular()) legs |= LEG_PURE_SPECULAR;
                            else if (info.bsdf->lobes().isForward()) legs |= LEG_FORWARD;
                            else {
                                // what the light sample meets, from a copy of the stream: the direction, its consistency, the medium of its side,
                                // a mesh emitter's distance test, the surfaces its shadow ray goes through
                                KeyedSampler probe(sampler);
                                LightSample ls;
                                if (light->sampleDirect(0, info.p, probe, ls)) {
                                    ev.wo = ev.frame.toLocal(ls.d);
                                    if (!tracer.isConsistent(ev, ls.d)) {
                                        legs |= LEG_INCONSISTENT;
                                    } else {
                                        const Medium *side = info.primitive->selectMedium(medium, ls.d.dot(info.Ng) < 0.0f);
                                        if (side != medium) legs |= LEG_MEDIUM_SELECTED;
                                        ev.requestedLobe = BsdfLobes::AllButSpecular;
                                        if (info.bsdf->eval(ev, false) != 0.0f) {
                                            Ray shadow = ray.scatter(info.p, ls.d, info.epsilon);
                                            shadow.setPrimaryRay(false);
                                            IntersectionTemporary ld;
                                            bool reached = true;
                                            if (light->isDirac()) shadow.setFarT(ls.dist);
                                            else reached = light->intersect(shadow, ld);
                                            if (reached && !light->isDirac() && dynamic_cast<const TriangleMesh *>(light))
                                                legs |= shadow.farT()*(1.0f + 1e-3f) < ls.dist ? LEG_MESH_REJECTED : LEG_MESH_ACCEPTED;
                                            if (reached && (light->isDirac() || !(shadow.farT()*(1.0f + 1e-3f) < ls.dist)))
                                                legs |= tracer.shadowCensus(shadow, light, bounce);
                                        }
                                    }
                                }
                                Vec3f unused(-1.0f);
                                if (tracer.lightSample(*light, ev, medium, bounce, ray, &unused) != 0.0f) legs |= LEG_LIGHT_TERM;
                                if (!light->isDirac() && tracer.bsdfSample(*light, ev, medium, bounce, ray) != 0.0f) legs |= LEG_BSDF_TERM;
                            }
                        }
                    }
                }
                const bool recorded = transmittance != -1.0f;
                std::fprintf(out, "%08x %08x %08x %08x %d %d %d %d %d\n", bitsOf(estimate.x()), bitsOf(estimate.y()), bitsOf(estimate.z()),
                             bitsOf(recorded ? transmittance.avg() : 0.0f), int(recorded), taken, legs, chosen, hitPrimitive);
            }
        }
    }
    std::fclose(out);
    return 0;
}
