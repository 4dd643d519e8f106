// path_tracer_hip: kernels + the extern "C" shim declared in include/tungsten_hip.h.
// gfx950 (MI355X) only.  See pt_kernels.h for the execution model and DESIGN.md for the layout.
#define PT_WAVEFRONT_MAIN
#include "pt_wavefront.h"
#include "pt_instances.h"
#include "shim_context.h"
#include "debug_units.h"
#include "denoise.h"
#include "develop.h"
#include "ray_query.h"
#include "radiance_query.h"
#include "surface_query.h"
#include "transmittance_query.h"
#include "direct_query.h"
#include "vertex_query.h"
#include "../host/RayQuery.hpp"
#include "../host/RadianceQuery.hpp"
#include "../host/SurfaceQuery.hpp"
#include "../host/TransmittanceQuery.hpp"
#include "../host/DirectQuery.hpp"
#include "../host/VertexQuery.hpp"

#include <chrono>

// The kernels other units instantiate (pt_instances.h: which, and where): declared, so that this unit instantiates none of them again
#define PT_KERNEL PT_DECLARE_KERNEL
PT_ALL_UNITS
#undef PT_KERNEL

// CubemapCamera's layout tables (cameras/CubemapCamera.cpp:10-46), indexed by projection mode and face
__device__ const int g_cubeResU[4] = {4, 3, 6, 1}, g_cubeResV[4] = {3, 4, 1, 6};
__device__ const int g_cubeOffsetU[4][6] = {{2, 0, 1, 1, 1, 3}, {1, 1, 1, 1, 0, 2}, {0, 1, 2, 3, 4, 5}, {0, 0, 0, 0, 0, 0}};
__device__ const int g_cubeOffsetV[4][6] = {{1, 1, 0, 2, 1, 1}, {1, 3, 0, 2, 1, 1}, {0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5}};
__device__ const int g_cubeBasisU[4][6] = {{5, 4, 0, 0, 0, 1}, {5, 5, 5, 5, 0, 1}, {5, 4, 0, 0, 0, 1}, {5, 4, 0, 0, 0, 1}};     // indices of +x -x +y -y +z -z
__device__ const int g_cubeBasisV[4][6] = {{3, 3, 4, 5, 3, 3}, {3, 2, 0, 1, 3, 3}, {3, 3, 4, 5, 3, 3}, {3, 3, 4, 5, 3, 3}};
PT_DEV f3 cubeBasis(int i) { const float sgn = (i & 1) ? -1.0f : 1.0f; return mk3((i >> 1) == 0 ? sgn : 0.0f, (i >> 1) == 1 ? sgn : 0.0f, (i >> 1) == 2 ? sgn : 0.0f); }

// cameras/EquirectangularCamera.cpp (TGHIP_CAMERA_EQUIRECTANGULAR): the full sphere around the camera's position.  nextPath writes every fresh camera path
// with the pinhole's ray; for this camera the direction is replaced here, in a launch in front of every closest-hit launch, for the slots of the
// workgroup's Q_EXTP (the freshly generated camera rays) -- from the same two random numbers: the path's stream restarted at (seed, pixel, sample) or
// at Sobol' dimension 0, as nextPath drew them (EquirectangularCamera::sampleDirection draws its filter offset exactly where the pinhole's does,
// :70-83).  Keeps the camera's sine and cosine out of every kernel that holds nextPath -- the metric's closest-hit kernel among them.  Idempotent.
__global__ __launch_bounds__(256) void k_camera_rays(DeviceScene s, PathState st, PassParams pp)
{
    const uint32_t W = st.slots_per_block >> 5;
    const uint32_t first = blockIdx.x*st.slots_per_block;
    CameraRef cam = *asConst(s.camera);
    for (uint32_t local = threadIdx.x; local < st.slots_per_block; local += blockDim.x) {
        const uint32_t word = st.bm[(uint32_t)Q_EXTP*st.bmStride + blockIdx.x*W + (local >> 5)];
        if (!((word >> (local & 31u)) & 1u))
            continue;
        const uint32_t slot = first + local;
        const uint4 misc = slotU4(st, A_MISC, slot), sm = slotU4(st, A_SAMP, slot);
        const uint32_t pixel = misc.z, px = pixel % pp.width, py = pixel/pp.width;
        Rng rng = rngStart(pp.seed, pixel, sm.x);
        if (pp.flags & TGHIP_PASS_SOBOL)
            rngStartSobol(rng, s, pp, px, py, pixel, sm.x, 0u);
        const float xi0 = rngNext1DT<true>(rng), xi1 = rngNext1DT<true>(rng);
        float fu = 0.0f, fv = 0.0f;
        if (cam.filter_type == TGHIP_FILTER_BOX) { fu = xi0 - 0.5f; fv = xi1 - 0.5f; }
        else if (cam.filter_type == TGHIP_FILTER_TABULATED) { fu = filterSample1D(cam, xi0); fv = filterSample1D(cam, xi1); }
        f3 l;
        bool ok = true;
        if (cam.type == TGHIP_CAMERA_CUBEMAP) {
            // CubemapCamera::sampleDirection / uvToFace / uvToDirection / faceToDirection (cameras/CubemapCamera.cpp:153-166, 95-112, 74-80) with the tables of
            // :10-46 and prepareForRender (:217-232); blade_count = the projection mode.  A pixel outside the six faces: the sample fails (black, PathTracer.cpp:27-28)
            const int mode = cam.blade_count;
            const float faceW = 1.0f/(float)g_cubeResU[mode], faceH = 1.0f/(float)g_cubeResV[mode];
            float u = ((float)px + 0.5f)*cam.pixel_size_x, v = ((float)py + 0.5f)*cam.inv_xf[9];
            int face = -1;
            for (int i = 0; i < 6 && face < 0; ++i) {
                const float dx = u - (float)g_cubeOffsetU[mode][i]*faceW, dy = v - (float)g_cubeOffsetV[mode][i]*faceH;
                if (dx >= 0.0f && dy >= 0.0f && dx <= faceW && dy <= faceH) face = i;
            }
            ok = face >= 0;
            if (ok) {
                u += fu*cam.pixel_size_x; v += fv*cam.inv_xf[9];
                const float dx = u - (float)g_cubeOffsetU[mode][face]*faceW, dy = v - (float)g_cubeOffsetV[mode][face]*faceH;
                const float ox = dx/faceW, oy = dy/faceH;
                const f3 b = cubeBasis(face), bu = cubeBasis(g_cubeBasisU[mode][face]), bv = cubeBasis(g_cubeBasisV[mode][face]);
                l = normalized(b + bu*(ox*2.0f - 1.0f) + bv*(oy*2.0f - 1.0f));
            } else {
                l = mk3(0.0f, 0.0f, 1.0f);
            }
        } else {
        // uvToDirection (:26-36); inv_xf holds _rot and 1 / res_y (include/tungsten_hip.h)
        const float u = ((float)px + 0.5f + fu)*cam.pixel_size_x, v = ((float)py + 0.5f + fv)*cam.inv_xf[9];
        const float phi = (u - 0.5f)*PT_TWO_PI, theta = (1.0f - v)*PT_PI;
        const float sinTheta = sinfH(theta);
        l = mk3(cosfH(phi)*sinTheta, -cosfH(theta), sinfH(phi)*sinTheta);
        }
        const f3 d = mk3(cam.inv_xf[0]*l.x + cam.inv_xf[1]*l.y + cam.inv_xf[2]*l.z + 0.0f,      // Mat4f*Vec3f: the (zero) translation column is added
                         cam.inv_xf[3]*l.x + cam.inv_xf[4]*l.y + cam.inv_xf[5]*l.z + 0.0f,
                         cam.inv_xf[6]*l.x + cam.inv_xf[7]*l.y + cam.inv_xf[8]*l.z + 0.0f);
        if (ok) {
            const float4 rd = slotF4(st, A_RAY_D, slot);
            slotF4(st, A_RAY_D, slot) = mk4(d, rd.w);
        } else {                                 // as nextPath leaves a failed camera sample: a ray that can hit nothing, no throughput
            slotF4(st, A_RAY_D, slot) = mk4(d, -1.0f);
            const float4 thr = slotF4(st, A_THR, slot);
            slotF4(st, A_THR, slot) = make_float4(0.0f, 0.0f, 0.0f, thr.w);
        }
    }
}


// =============================================================================================
// Host-side shim
// =============================================================================================

namespace {

std::mutex g_errMutex;
std::string g_createError = "no error";

std::mutex g_streamMutex;
std::map<int, std::vector<StreamSet>> g_freeStreams;   // device ordinal -> sets no context holds (never destroyed: they live as long as the process)
} // namespace

template<typename T, typename P>
static int uploadArray(tghip_ctx *ctx, DeviceBuffers &mem, const T *src, size_t count, P *dst, size_t padBytes = 0)   // P = (restrict-qualified) const T *
{
    size_t bytes = std::max<size_t>(count, 1)*sizeof(T) + padBytes;   // (padBytes: readable, uninitialised room behind the last element)
    void *p = nullptr;
    HIP_TRY(ctx, hipMalloc(&p, bytes));
    mem.allocs.push_back(p);
    if (count)
        HIP_TRY(ctx, hipMemcpyAsync(p, src, count*sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *dst = static_cast<const T *>(p);
    return TGHIP_OK;
}

template<typename T>
static int allocArray(tghip_ctx *ctx, DeviceBuffers &mem, size_t count, T **dst)
{
    void *p = nullptr;
    HIP_TRY(ctx, hipMalloc(&p, std::max<size_t>(count, 1)*sizeof(T)));
    mem.allocs.push_back(p);
    *dst = static_cast<T *>(p);
    return TGHIP_OK;
}

// ---- Kernel identities (csrc/host/LaunchChoice.hpp) to kernels: per family the one place where run-time flags become template arguments.  What
// walkKernelFn names is what this translation unit instantiates; the kernels of the other units are looked up in their list (pt_instances.h).
#define KERNEL(...) reinterpret_cast<const void *>(&__VA_ARGS__)
template<typename F>
static const void *withBool(bool b, F f) { return b ? f(std::true_type()) : f(std::false_type()); }

static const void *walkKernelFn(const KernelId &k)
{
    return withBool(k.count, [&](auto C) { return withBool(k.solids, [&](auto S) -> const void * {
        constexpr bool c = decltype(C)::value, s = decltype(S)::value;
        switch (k.family) {
        case K_CLOSEST:             return k.inst == 1 ? KERNEL(k_trace_closest<c, false, 1>) : k.inst == 2 ? KERNEL(k_trace_closest<c, false, 2>)
                                         : k.flat ? KERNEL(k_trace_closest<c, true>) : KERNEL(k_trace_closest<c, false>);
        case K_CLOSEST_DYN:         return KERNEL(k_trace_closest_dyn<c, s>);
        case K_CLOSEST_INST:        return KERNEL(k_trace_closest_inst<c, s>);
        case K_CLOSEST_INSTW:       return KERNEL(k_trace_closest_instw<c, s>);
        case K_CLOSEST_WIDE:        return k.inst ? KERNEL(k_trace_closest_wide<c, s, true, false>) : k.decoupled ? KERNEL(k_trace_closest_wide<c, s, false, true>)
                                                                                                                  : KERNEL(k_trace_closest_wide<c, s, false, false>);
        case K_FINISH_CLOSEST_WIDE: return KERNEL(k_finish_trace_closest_wide<c, s>);
        case K_SHADOW:
            if (k.mask == BSDF_MASK_ALL) return nullptr;   // (walk_shadow_tex.hip's, listed: never this unit's default-mask walk in their place)
            return withBool(k.forward, [&](auto FW) -> const void * {
                constexpr bool fw = decltype(FW)::value;
                return k.inst == 1 ? KERNEL(k_trace_shadow<c, fw, false, 1>) : k.inst == 2 ? KERNEL(k_trace_shadow<c, fw, false, 2>)
                     : k.flat ? KERNEL(k_trace_shadow<c, fw, true>) : KERNEL(k_trace_shadow<c, fw, false>);
            });
        case K_SHADOW_DYN:          return KERNEL(k_trace_shadow_dyn<c, s>);
        // (rounds 2 and 3 launched the counting variant for instanced scenes: the non-counting one lost occluders inside instances.  The cause is the loop
        // latch the backend generates for the turn without PT_TURN_JOIN, pt_wavefront.h; "inst_shadow_join" = 0 launches that variant for tools/repro_latch_miscompile.py)
        case K_SHADOW_WIDE:         return !k.join ? KERNEL(k_trace_shadow_wide<false, false, true, false>)
                                         : k.inst ? KERNEL(k_trace_shadow_wide<c, s, true>) : KERNEL(k_trace_shadow_wide<c, s, false>);
        case K_TRACE_RAYS:          return k.decoupled ? KERNEL(k_trace_rays<c, false, 0, true>) : k.inst ? KERNEL(k_trace_rays<c, false, 1>)
                                         : k.flat ? KERNEL(k_trace_rays<c, true>) : KERNEL(k_trace_rays<c, false>);
        default:                    return nullptr;
        }
    }); });
}

// the explicitly instantiated kernels: every entry of every unit's list is one lookup
static const void *explicitKernelFn(const KernelId &k)
{
#define PT_KERNEL(match, params, ...) if (match) return KERNEL(__VA_ARGS__);
    PT_ALL_UNITS
#undef PT_KERNEL
    return nullptr;
}
static const void *kernelFn(const KernelId &k)
{
    const void *fn = explicitKernelFn(k);
    return fn ? fn : walkKernelFn(k);
}

// hipLaunchKernel takes the arguments by address and does not know the kernel's parameter list: every argument must HAVE the type of its parameter.  The
// kernels launched through here take structs, pointers, `int` and `uint32_t`; a number of any other type is refused at compile time.
template<typename... A>
static void launchKernel(const ResolvedLaunch &l, int grid, hipStream_t stream, const A &... args)
{
    static_assert(((!std::is_arithmetic<A>::value || (std::is_integral<A>::value && sizeof(A) == 4)) && ...),
                  "launchKernel: pass structs, pointers, int or uint32_t -- the kernel's own parameter types");
    void *argv[] = {(void *)&args...};
    (void)hipLaunchKernel(l.fn, dim3(grid), dim3(l.threads), argv, l.lds, stream);
}

static int launchGrid(const tghip_ctx *ctx) { return ctx->prop.multiProcessorCount*std::max(ctx->lp.choice.blocksPerCu, 1)*std::max(ctx->gridRounds, 1); }

// Workgroups of `fn` resident on a CU at `threads` threads with `lds` bytes of dynamic LDS.  Asked of the runtime once per context: passes of
// alternating kinds (adaptive renders: normal and record passes) plan again without asking again.
static int residentBlocks(tghip_ctx *ctx, const void *fn, int threads, size_t lds)
{
    const auto key = std::make_tuple(fn, threads, lds);
    const auto it = ctx->occupancy.find(key);
    if (it != ctx->occupancy.end()) return it->second;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, lds) != hipSuccess) nb = 0;
    return ctx->occupancy[key] = nb;
}

// Resolves the choice for a pass of `kind` on the uploaded scene into `p`: kernels, workgroup sizes (threads per workgroup, per kernel: chosen so that
// blocksPerCu workgroups of EVERY kernel are resident at once -- no second scheduling round --, i.e. each kernel runs at its own best occupancy on one
// grid) and dynamic LDS bytes.  Runs when an input changes -- an upload, an option, a pass of another kind; an iteration only reads the result.
static int planLaunches(tghip_ctx *ctx, const PassKind &kind, LaunchPlan &p)
{
    p.kind = kind;
    LaunchChoice &c = p.choice;
    chooseLaunches(ctx->sc, ctx->scene.num_recs, ctx->numWideNodes, ctx->opt, kind, c);
    auto threadsFor = [&](const WorkgroupSize &w) {
        if (w.fixed) return w.fixed;
        const void *fn = kernelFn(w.sizedBy);
        for (int t = w.maxThreads; t >= 128; t -= 64)
            if (residentBlocks(ctx, fn, t, ldsBytes(ctx->sc, c, w.lds, t)) >= c.blocksPerCu) return t;
        return 128;
    };
    bool missing = false;
    const WalkLaunch *walks[2] = {&c.closest, &c.shadow};
    ResolvedLaunch *resolved[2] = {&p.closest, &p.shadow};
    for (int i = 0; i < 2; ++i) {
        const int t = threadsFor(walks[i]->size);
        *resolved[i] = ResolvedLaunch{kernelFn(walks[i]->kernel), t, ldsBytes(ctx->sc, c, walks[i]->lds, t)};
        missing = missing || !resolved[i]->fn || !kernelFn(walks[i]->size.sizedBy);
    }
    for (int i = 0; i < 3; ++i) {
        p.thrShade[i] = threadsFor(c.shadeSize[i]);
        missing = missing || !kernelFn(c.shadeSize[i].sizedBy);
    }
    for (int i = 0; i < c.numShade; ++i) {
        p.shade[i] = ResolvedLaunch{kernelFn(c.shade[i].kernel), p.thrShade[c.shade[i].size], 0};
        missing = missing || !p.shade[i].fn;
    }
    // (k_tail runs 256 threads whatever the depth of the tree: it is used only where a workgroup of it fits a CU -- its static LDS plus the walk stacks
    // of a very deep tree may not)
    p.tail = ResolvedLaunch{kernelFn(c.tail), 256, ldsBytes(ctx->sc, c, LDS_WIDE, 256)};
    p.tailFits = c.tailEligible && residentBlocks(ctx, kernelFn(c.tailProbe), 256, p.tail.lds) >= 1;
    missing = missing || !p.tail.fn || !kernelFn(c.tailProbe);
    if (missing) { ctx->error = "launch plan: a chosen kernel is not among the instantiated ones"; return TGHIP_E_UNSUPPORTED; }
    if (std::getenv("TGHIP_VERBOSE") && &p == &ctx->lp)
        std::fprintf(stderr, "[tghip] grid %d x threads closest %d (%s) shadow %d (%s) shade %d/%d/%d (flat %d, forward %d, complex mask 0x%x)\n",
                     launchGrid(ctx), p.closest.threads, kernelName(c.closest.kernel).c_str(), p.shadow.threads, kernelName(c.shadow.kernel).c_str(),
                     p.thrShade[SIZE_SIMPLE], p.thrShade[SIZE_COMPLEX], p.thrShade[SIZE_ALL], int(c.flat), int(ctx->sc.haveForward), ctx->sc.complexMask);
    return TGHIP_OK;
}
// ... for the context itself: the kind of the last pass (an upload or an option between two passes keeps it), "count_traversal" as it stands
static int replan(tghip_ctx *ctx)
{
    PassKind kind = ctx->lp.kind;
    kind.countTraversal = ctx->countTraversal;
    return planLaunches(ctx, kind, ctx->lp);
}

// Adds the per-workgroup statistics on the device to ctx->counters and zeroes them there.
static int foldCounters(tghip_ctx *ctx)
{
    if (!ctx->poolSlots)
        return TGHIP_OK;
    const size_t g = ctx->poolGrid;
    ctx->hostCtl.resize(g);
    ctx->hostStats.resize(g);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(ctx->hostCtl.data(), ctx->pool.ctl, g*sizeof(BlockCtl), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(ctx->hostStats.data(), ctx->pool.stats, g*sizeof(BlockStats), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < g; ++b) {
        BlockCtl &c = ctx->hostCtl[b];
        ctx->counters.samples += c.samples; ctx->counters.closest_rays += c.closest_rays;
        ctx->counters.shadow_rays += c.shadow_rays; ctx->counters.shadow_slots += c.shadow_slots;
        c.samples = c.closest_rays = c.shadow_rays = c.shadow_slots = 0;
        const BlockStats &t = ctx->hostStats[b];
        if (ctx->countTraversal) {
            ctx->counters.nodes_visited += t.nodes_visited; ctx->counters.prims_tested += t.prims_tested;
            ctx->counters.nodes_visited_shadow += t.nodes_visited_shadow; ctx->counters.prims_tested_shadow += t.prims_tested_shadow;
        }
    }
    if (ctx->countTraversal)
        for (int k = 0; k < 2; ++k)
            for (size_t b = 0; b < g; ++b)
                for (int i = 0; i < PT_WALK_STATS; ++i) {
                    if (i == 11) ctx->walkStats[k][i] = std::max(ctx->walkStats[k][i], ctx->hostStats[b].walk[k][i]);
                    else ctx->walkStats[k][i] += ctx->hostStats[b].walk[k][i];
                }
    if (std::getenv("TGHIP_VERBOSE") && ctx->countTraversal) {
        for (int k = 0; k < 2; ++k) {
            unsigned long long t[12] = {0};
            for (size_t b = 0; b < g; ++b) for (int i = 0; i < 12; ++i) { if (i == 11) t[i] = std::max(t[i], ctx->hostStats[b].walk[k][i]); else t[i] += ctx->hostStats[b].walk[k][i]; }
            if (!t[4]) continue;
            const double waves = double(t[4]), us = 0.01;
            std::fprintf(stderr, "[tghip] %s walk, per wave launch: expand %.1f us | loop with queue %.1f us (%.1f turns, %.1f busy lanes) | dry %.1f us (%.1f turns, %.1f busy lanes) | wait+write-back %.1f us | "
                                 "longest loop %.1f us | suspended %llu resumed %llu walks in %llu wave launches\n", k == 0 ? "closest-hit" : "shadow",
                         double(t[0])*us/waves, double(t[1])*us/waves, double(t[5])/waves, t[5] ? double(t[7])/double(t[5]) : 0.0,
                         double(t[2])*us/waves, double(t[6])/waves, t[6] ? double(t[8])/double(t[6]) : 0.0, double(t[3])*us/waves, double(t[11])*us, t[9], t[10], t[4]);
        }
    }
    if (std::getenv("TGHIP_VERBOSE")) {
        unsigned long long turns = 0, dry = 0;
        for (size_t b = 0; b < g; ++b) { turns += ctx->hostStats[b].prof[10]; dry += ctx->hostStats[b].prof[11]; }
        if (turns) std::fprintf(stderr, "[tghip] closest-hit walk: %llu wave turns (%llu after the queue ran dry)\n", turns, dry);
    }
#ifdef PT_PROFILE
    {
        unsigned long long tot[16] = {0};
        for (size_t b = 0; b < g; ++b) for (int k = 0; k < 16; ++k) if (k != 10 && k != 11) tot[k] += ctx->hostStats[b].prof[k];
        unsigned long long sum = 0; for (int k = 0; k < 16; ++k) sum += tot[k];
        if (sum) { std::fprintf(stderr, "[PT_PROFILE] k_shade wave-cycles by section:"); for (int k = 0; k < 16; ++k) if (k != 10 && k != 11) std::fprintf(stderr, " s%d=%.1f%%", k, 100.0*double(tot[k])/double(sum)); std::fprintf(stderr, " total=%llu\n", sum); }
        // per shading class, and how evenly the class's work is spread: per workgroup and per set of workgroups b, b + CUs, ... (one CU's, if
        // the dispatcher deals workgroups to the CUs in order)
        const size_t cus = size_t(ctx->prop.multiProcessorCount);
        for (int c = 0; c <= PT_NUM_CLASSES; ++c) {
            unsigned long long ct[16] = {0}, csum = 0;
            std::vector<double> perBlock(g, 0.0), perCu(std::min(cus, g), 0.0);
            for (size_t b = 0; b < g; ++b) for (int k = 0; k < 16; ++k) { ct[k] += ctx->hostStats[b].profCls[c][k]; perBlock[b] += double(ctx->hostStats[b].profCls[c][k]); }
            for (size_t b = 0; b < g; ++b) perCu[b % perCu.size()] += perBlock[b];
            for (int k = 0; k < 16; ++k) csum += ct[k];
            if (!csum) continue;
            csum -= ct[10];
            std::fprintf(stderr, "[PT_PROFILE] class %d: %llu wave turns, %.2f us per turn:", c, ct[10], ct[10] ? double(csum)*0.01/double(ct[10]) : 0.0);
            for (int k = 0; k < 16; ++k) if (k != 10 && k != 11) {
                unsigned long long ln = 0;
                for (size_t b = 0; b < g; ++b) ln += ctx->hostStats[b].profLanes[c][k];
                std::fprintf(stderr, " s%d=%.2fus(%.0f lanes)", k, ct[10] ? double(ct[k])*0.01/double(ct[10]) : 0.0, ct[k] ? double(ln)/double(ct[k]) : 0.0);
            }
            auto spread = [](std::vector<double> v, const char *what) {
                std::sort(v.begin(), v.end());
                double mean = 0.0; for (double x : v) mean += x; mean /= double(v.size());
                std::fprintf(stderr, " | %s min %.2f p50 %.2f p95 %.2f max %.2f of the mean", what, v.front()/mean, v[v.size()/2]/mean, v[v.size()*95/100]/mean, v.back()/mean);
            };
            spread(perBlock, "per workgroup");
            spread(perCu, "per CU");
            std::fprintf(stderr, " total=%llu\n", csum);
        }
    }
#endif
    // no pass is running here (calls on one handle are serialised), so the records can be written back whole
    HIP_TRY(ctx, hipMemcpy(ctx->pool.ctl, ctx->hostCtl.data(), g*sizeof(BlockCtl), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(ctx->pool.stats, 0, g*sizeof(BlockStats)));
    return TGHIP_OK;
}

// The pool goes: the next pass lays it out again (an option its layout depends on has changed, or ensurePool wants another one)
static void dropPool(tghip_ctx *ctx) { ctx->poolMem.release(); ctx->poolSlots = 0; }

// Pool layout: `grid` persistent workgroups x slotsPerBlock slots (a multiple of 64); queue segments and the
// per-workgroup control records are laid out the same way.
static int ensurePool(tghip_ctx *ctx, uint32_t wantSlots)
{
    const uint32_t grid = uint32_t(launchGrid(ctx));
    uint32_t perBlock = (wantSlots + grid - 1)/grid;
    const LaunchPlan &lp = ctx->lp;
    uint32_t cap = lp.choice.slotCap;
    if (lp.choice.orderRegsCap)
        cap = std::min<uint32_t>(cap, 16u*uint32_t(std::min(lp.closest.threads, lp.shadow.threads))/64u*64u);   // OrderRegs
    perBlock = std::min<uint32_t>(cap, std::max<uint32_t>(64u, (perBlock + 63u)/64u*64u));
    const uint32_t slots = perBlock*grid;
    PathState &p = ctx->pool;
    // the walk arrays behind the A_* ones (suspended walks of the wide kernels, PathState::walk_base): only where they fit the 32-bit offsets
    uint32_t walkArrays = lp.choice.walkArrays;
    if (ctx->poolSlots >= slots && ctx->poolGrid == grid && (ctx->poolWalkWanted == walkArrays || ctx->poolWalkArrays >= walkArrays)) {
        p.num_slots = slots;
        p.slots_per_block = perBlock;
        return TGHIP_OK;
    }
    ctx->poolWalkWanted = walkArrays;
    int rc = foldCounters(ctx);                  // the per-workgroup statistics live in the pool
    if (rc != TGHIP_OK) return rc;
    dropPool(ctx);
#define POOL_ALLOC(field, n) do { std::remove_reference<decltype(*p.field)>::type *tmp_ = nullptr; \
        if ((rc = allocArray(ctx, ctx->poolMem, (n), &tmp_)) != TGHIP_OK) return rc; p.field = tmp_; } while (0)
    // arrays are skewed by an odd number of 256-byte units so that element i of different arrays does not map to
    // the same HBM channel (a power-of-two array stride made the kernels' speed depend on allocation luck)
    const uint64_t strideBytes = uint64_t(slots)*16u + uint64_t(ctx->poolPad);
    // (a group of eight arrays is addressed with a 32-bit offset from its own base, PathState::poolg)
    const uint64_t groupArrays = 1ull << PT_POOL_GROUP_SHIFT;
    if (strideBytes*groupArrays >= (1ull << 32)) { ctx->error = "path pool too large for 32-bit slot offsets within an array group"; return TGHIP_E_INVALID; }
    if (A_COUNT + walkArrays > groupArrays*PT_POOL_GROUPS) walkArrays = 0;
    ctx->poolWalkArrays = walkArrays;
    char *poolBase = nullptr;
    if ((rc = allocArray(ctx, ctx->poolMem, size_t(strideBytes*(A_COUNT + walkArrays)), &poolBase)) != TGHIP_OK) return rc;
    for (uint32_t g = 0; g < PT_POOL_GROUPS; ++g)
        p.poolg[g] = poolBase + size_t(g)*size_t(groupArrays)*size_t(strideBytes);   // (groups past the last array are never addressed)
    p.walk_base = A_COUNT;
    p.stride = uint32_t(strideBytes);
    POOL_ALLOC(bm, size_t(slots/32)*Q_COUNT);
    p.bmStride = slots/32;
    POOL_ALLOC(ctl, grid); POOL_ALLOC(stats, grid); POOL_ALLOC(live, 4);
#undef POOL_ALLOC
    HIP_TRY(ctx, hipMemsetAsync(p.ctl, 0, sizeof(BlockCtl)*grid, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(p.stats, 0, sizeof(BlockStats)*grid, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(p.live, 0, 4*sizeof(uint32_t), ctx->stream));
    p.abort_flag = ctx->abortFlagDev.get();
    p.num_slots = slots;
    p.slots_per_block = perBlock;
    ctx->poolSlots = slots;
    ctx->poolGrid = grid;
    return TGHIP_OK;
}

extern "C" {

int tghip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

tghip_ctx *tghip_create(int device_ordinal)
{
    int n = tghip_device_count();
    if (device_ordinal < 0 || device_ordinal >= n) {
        std::lock_guard<std::mutex> lock(g_errMutex);
        g_createError = n == 0 ? "no HIP device available" : "device ordinal out of range";
        return nullptr;
    }
    tghip_ctx *ctx = new tghip_ctx();
    ctx->device = device_ordinal;
    std::memset(&ctx->counters, 0, sizeof(ctx->counters));
    std::memset(&ctx->pool, 0, sizeof(ctx->pool));
    std::memset(&ctx->scene, 0, sizeof(ctx->scene));
    hipError_t e = hipSetDevice(device_ordinal);
    if (e == hipSuccess) e = hipGetDeviceProperties(&ctx->prop, device_ordinal);
    {
        // (creation order matters: HIP deals its streams round-robin to a few hardware queues and streams on one hardware queue run their
        // kernels one after the other; the main stream and the part streams come first)
        StreamSet set;
        bool reused = false;
        {
            std::lock_guard<std::mutex> lock(g_streamMutex);
            std::vector<StreamSet> &pool = g_freeStreams[device_ordinal];
            if (!pool.empty()) { set = pool.back(); pool.pop_back(); reused = true; }
        }
        if (!reused) {
            // TGHIP_STREAM_PRIORITIES="p0,p1,..." (an experiment's hook, profiles/r6_ab_stream_priorities.txt): HIP stream priorities of the main stream and the part
            // streams, in creation order (lower = served first; the device's range is clamped by HIP); unset: plain streams
            int prio[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            bool withPrio = false;
            if (const char *env = std::getenv("TGHIP_STREAM_PRIORITIES")) {
                withPrio = true;
                int k = 0;
                for (const char *c = env; *c && k < 8; ) {
                    prio[k++] = int(std::strtol(c, const_cast<char **>(&c), 10));
                    while (*c == ',' || *c == ' ') ++c;
                }
            }
            auto create = [&](hipStream_t *st, int p) { return withPrio ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, p) : hipStreamCreateWithFlags(st, hipStreamNonBlocking); };
            if (e == hipSuccess) e = create(&set.main, prio[0]);
            for (int k = 0; k < 7; ++k)
                if (e == hipSuccess) e = create(&set.part[k], prio[k + 1]);
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&set.abort, hipStreamNonBlocking);
        }
        ctx->stream = set.main;
        for (int k = 0; k < 7; ++k) ctx->partStream[k] = set.part[k];
        ctx->abortStream = set.abort;
    }
    for (int k = 0; k < 7; ++k)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->evPart[k], hipEventDisableTiming);
    for (int k = 0; k < 8; ++k) {
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->evFork[k], hipEventDisableTiming);
        for (int a = 0; a < 2; ++a)
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->evJoin[k][a], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->evMain, hipEventDisableTiming);
    ctx->launchStream = ctx->stream;
    if (e == hipSuccess) e = hipEventCreate(&ctx->evA);
    if (e == hipSuccess) e = hipEventCreate(&ctx->evB);
    if (e == hipSuccess) e = hipEventCreate(&ctx->evSurfMid);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&ctx->hostLive), 2*sizeof(uint32_t), hipHostMallocDefault);
    if (e == hipSuccess) e = ctx->abortFlagDev.once(16);
    if (e == hipSuccess) e = hipMemset(ctx->abortFlagDev.get(), 0, 64);
    if (e != hipSuccess) {
        {
            std::lock_guard<std::mutex> lock(g_errMutex);
            g_createError = std::string("tghip_create: ") + hipGetErrorString(e);
        }
        tghip_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void tghip_destroy(tghip_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    // every stream idle before the first buffer goes -- with the context, at the end: its arrays free themselves (device_array.h) -- (the part /
    // class streams join the main one at the end of a pass, an aborted or failed pass may have left them behind)
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (int k = 0; k < 7; ++k) if (ctx->partStream[k]) (void)hipStreamSynchronize(ctx->partStream[k]);
    for (int k = 0; k < 8; ++k)
        for (int a = 0; a < 2; ++a) if (ctx->classStream[k][a]) (void)hipStreamSynchronize(ctx->classStream[k][a]);
    if (ctx->abortStream) (void)hipStreamSynchronize(ctx->abortStream);
    if (ctx->rankComm) tghipDestroyRankComm(ctx->rankComm);
    if (ctx->evA) (void)hipEventDestroy(ctx->evA);
    if (ctx->evB) (void)hipEventDestroy(ctx->evB);
    if (ctx->evSurfMid) (void)hipEventDestroy(ctx->evSurfMid);
    for (hipEvent_t e : ctx->evPool) (void)hipEventDestroy(e);
    for (int k = 0; k < 7; ++k) if (ctx->evPart[k]) (void)hipEventDestroy(ctx->evPart[k]);
    if (ctx->evMain) (void)hipEventDestroy(ctx->evMain);
    for (int k = 0; k < 8; ++k) {
        if (ctx->evFork[k]) (void)hipEventDestroy(ctx->evFork[k]);
        for (int a = 0; a < 2; ++a) {
            if (ctx->evJoin[k][a]) (void)hipEventDestroy(ctx->evJoin[k][a]);
            if (ctx->classStream[k][a]) (void)hipStreamDestroy(ctx->classStream[k][a]);
        }
    }
    {
        // the streams go back to the device's free list (idle: synchronised above)
        StreamSet set;
        set.main = ctx->stream; set.abort = ctx->abortStream;
        bool complete = set.main != nullptr && set.abort != nullptr;
        for (int k = 0; k < 7; ++k) { set.part[k] = ctx->partStream[k]; complete = complete && set.part[k] != nullptr; }
        if (complete) {
            std::lock_guard<std::mutex> lock(g_streamMutex);
            g_freeStreams[ctx->device].push_back(set);
        } else {                                 // (a context whose creation failed half way)
            if (set.main) (void)hipStreamDestroy(set.main);
            if (set.abort) (void)hipStreamDestroy(set.abort);
            for (int k = 0; k < 7; ++k) if (set.part[k]) (void)hipStreamDestroy(set.part[k]);
        }
    }
    delete ctx;                                  // (and with it every device array it holds: the device is current, the streams are idle)
}

const char *tghip_last_error(tghip_ctx *ctx)
{
    if (!ctx) {
        std::lock_guard<std::mutex> lock(g_errMutex);
        static thread_local std::string copy;
        copy = g_createError;
        return copy.c_str();
    }
    return ctx->error.c_str();
}

int tghip_set_option(tghip_ctx *ctx, const char *key, long long value)
{
    if (!ctx || !key) return TGHIP_E_INVALID;
    std::string k(key);
    // the options the choice of a pass's kernels reads: stored, and the plan of the uploaded scene made again
    if (k == "count_traversal" || setLaunchOption(ctx->opt, k, value)) {
        if (k == "count_traversal") ctx->countTraversal = value != 0;
        if (k == "slots_per_block") dropPool(ctx);
        for (int kk = 0; kk < 8 && k == "class_streams" && value != 0; ++kk)     // (created when the option is first switched on: an experiment's streams)
            for (int a = 0; a < 2; ++a)
                if (!ctx->classStream[kk][a]) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->classStream[kk][a], hipStreamNonBlocking));
        return ctx->haveScene ? replan(ctx) : TGHIP_OK;
    }
    if (k == "max_slots") { ctx->maxSlots = std::max<long long>(value, 256); ctx->maxSlotsSet = true; }
    else if (k == "max_items") ctx->maxItems = std::max<long long>(value, 256);
    else if (k == "chunk_samples") ctx->chunkSamples = int(std::min<long long>(std::max<long long>(value, 0), 1 << 20));
    else if (k == "check_interval") ctx->checkInterval = int(std::min<long long>(std::max<long long>(value, 0), 64));
    else if (k == "time_kernels") ctx->timeKernels = value != 0;
    else if (k == "inst_phase_min") ctx->instPhaseMin = int(std::min<long long>(std::max<long long>(value, 1), 64));
    else if (k == "inst_refill_at") ctx->instRefillAt = int(std::min<long long>(std::max<long long>(value, 0), 63));
    else if (k == "grid_rounds") { ctx->gridRounds = int(std::min<long long>(std::max<long long>(value, 1), 8)); dropPool(ctx); }
    else if (k == "leaf_batch_bvh2") ctx->leafBatchBvh2 = int(std::min<long long>(std::max<long long>(value, 0), 64));
    else if (k == "suspend_lanes") ctx->suspendLanes = int(std::min<long long>(std::max<long long>(value, 0), 64));
    else if (k == "suspend_turns") ctx->suspendTurns = int(std::min<long long>(std::max<long long>(value, 1), 1 << 20));   // (>= 1: every launch advances every walk)
    else if (k == "suspend_min_queue") ctx->suspendMinQueue = int(std::min<long long>(std::max<long long>(value, 0), 1 << 20));
    else if (k == "fail_reduce") ctx->failReduce = value != 0;   // fault injection: tghip_reduce_framebuffers with this context as a rank fails (the hosts' fallbacks are tested with it)
    else if (k == "hoist_quad") { ctx->hoistOpt = value != 0; if (!ctx->hoistOpt) ctx->scene.hoisted_rec = -1; else ctx->scene.hoisted_rec = ctx->sc.hoisted.record; }
    else if (k == "top_tree") ctx->topTreeOpt = value != 0;
    else if (k == "env_lds") ctx->scene.env_tex = value != 0 ? ctx->sc.env_tex : -1;
    else if (k == "tail_threshold") ctx->tailThreshold = value;
    else if (k == "lds_nodes") {}   // (accepted, no effect: the top of the wide tree in LDS was measured without gain and is gone, profiles/r5_ab_walk_fetch.txt)
    else if (k == "leaf_batch") ctx->leafBatch = int(std::min<long long>(std::max<long long>(value, 1), 64));
    else if (k == "develop_host") ctx->developHost = value != 0;   // tghip_develop answers TGHIP_E_UNSUPPORTED: the host integrator then develops a download itself
    else if (k == "nlmeans_batch") ctx->nlmBatch = uint32_t(std::min<long long>(std::max<long long>(value, 0), NLMEANS_MAX_BATCH));   // offsets box-filtered at once by tghip_nlmeans (0: the measured choice, denoise.hip)
    else if (k == "query_blocks") ctx->queryBlocks = int(std::min<long long>(std::max<long long>(value, 0), 1 << 16));       // workgroups of tghip_query_rays (0: the measured default)
    else if (k == "query_refill_at") ctx->queryRefillAt = int(std::min<long long>(std::max<long long>(value, 0), 64));   // idle lanes of a wave at which it claims rays (0: the measured default)
    else if (k == "surface_time_stage") ctx->surfTimeDense = value == 1;   // tghip_query_surface_kernel_time: 0 = both launches, 1 = the dense one alone (instrumentation)
    else if (k == "pool_pad") { ctx->poolPad = std::max<long long>(value, 0)/16*16; dropPool(ctx); }
    else if (k == "wide_node_stride") {
        if (value != 128 && value != 80) { ctx->error = "wide_node_stride is 80 or 128"; return TGHIP_E_INVALID; }
        ctx->wideStride = int(value);
    }
    else { ctx->error = "unknown option '" + k + "'"; return TGHIP_E_INVALID; }
    return TGHIP_OK;
}

int tghip_upload_scene(tghip_ctx *ctx, const TgHipSceneDesc *sd)
{
    if (!ctx || !sd) return TGHIP_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // everything that can refuse the description, and everything derived from it, before the context is touched (csrc/host/SceneCheck.cpp)
    SceneCheckOptions opt;
    opt.top_tree = ctx->topTreeOpt;
    opt.wide_node_stride = uint32_t(ctx->wideStride);
    SceneTraits traits;
    int rc = checkScene(sd, opt, traits, ctx->error);
    if (rc != TGHIP_OK) return rc;

    if (ctx->stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->sceneMem.release();
    ctx->haveScene = false;
    ctx->sc = std::move(traits);   // (its tables are copied from below: they live until the next upload, which waits for the stream first)
    const SceneTraits &sc = ctx->sc;
    DeviceScene &s = ctx->scene;
    std::memset(&s, 0, sizeof(s));
    const TgHipBvhNode *dn; const TgHipPrimRec *dr; const TgHipTriAttr *da;
    if ((rc = uploadArray(ctx, ctx->sceneMem, sd->nodes, sd->num_nodes, &dn)) != TGHIP_OK) return rc;
    ctx->numWideNodes = 0;
    if (sc.wideDepth > 0) {
        // the wide nodes and the primitive records share ONE allocation, so that a lane of the wide kernels addresses
        // "a node or a record" with one base pointer and one 32-bit offset
        const size_t stride = size_t(ctx->wideStride);
        const size_t nodeBytes = (size_t(sd->num_wide_nodes)*stride + 127u) & ~size_t(127);
        const size_t recBytes = std::max<size_t>(sd->num_recs, 1)*sizeof(TgHipPrimRec);
        char *p = nullptr;
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&p), nodeBytes + recBytes));
        ctx->sceneMem.allocs.push_back(p);
        HIP_TRY(ctx, hipMemcpy2DAsync(p, stride, sd->wide_nodes, sizeof(TgHipWideNode), sizeof(TgHipWideNode), sd->num_wide_nodes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(p + nodeBytes, sd->recs, size_t(sd->num_recs)*sizeof(TgHipPrimRec), hipMemcpyHostToDevice, ctx->stream));
        if (sc.hoisted.record >= 0) {
            // the hoisted quad's bit in the `reserved` word of the wide node that holds it (SceneTraits::hoisted) -- on the device copy only; the
            // sequential walks (tghip_trace_rays, "decouple" = 0) do not read it.
            // (on ctx->stream, behind the 2-D copy of the nodes queued above: that stream is non-blocking, so a copy on the null stream would
            // not wait for it and could be overwritten by it -- the quad would then be tested before AND inside every walk; `word` is on
            // the stack, so the copy is waited for here)
            const uint32_t word = 1u << sc.hoisted.bit;
            HIP_TRY(ctx, hipMemcpyAsync(p + size_t(sc.hoisted.node)*stride + offsetof(TgHipWideNode, reserved), &word, sizeof(word), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        s.wide = reinterpret_cast<const float4 *>(p);
        s.recs_offset = uint32_t(nodeBytes);
        s.wide_stride = uint32_t(stride);
        dr = reinterpret_cast<const TgHipPrimRec *>(p + nodeBytes);
        ctx->numWideNodes = sd->num_wide_nodes;
    } else if ((rc = uploadArray(ctx, ctx->sceneMem, sd->recs, sd->num_recs, &dr)) != TGHIP_OK) {
        return rc;
    }
    s.hoisted_rec = ctx->hoistOpt ? sc.hoisted.record : -1;
    if ((rc = uploadArray(ctx, ctx->sceneMem, sd->tri_attrs, sd->num_recs, &da)) != TGHIP_OK) return rc;
    s.nodes = reinterpret_cast<const float4 *>(dn);
    s.recs = reinterpret_cast<const float4 *>(dr);
    s.tri_attrs = reinterpret_cast<const float4 *>(da);
    if ((rc = uploadArray(ctx, ctx->sceneMem, sd->objects, sd->num_objects, &s.objects)) != TGHIP_OK) return rc;
    if ((rc = uploadArray(ctx, ctx->sceneMem, sd->lights, sd->num_lights, &s.lights)) != TGHIP_OK) return rc;
    if ((rc = uploadArray(ctx, ctx->sceneMem, sd->infinite_lights, sd->num_infinite_lights, &s.infinite_lights)) != TGHIP_OK) return rc;
    if ((rc = uploadArray(ctx, ctx->sceneMem, sd->bsdfs, sd->num_bsdfs, &s.bsdfs)) != TGHIP_OK) return rc;
    if ((rc = uploadArray(ctx, ctx->sceneMem, sd->textures, sd->num_textures, &s.textures)) != TGHIP_OK) return rc;
    // (16 bytes of room behind the texels: bitmapTexel reads three floats of a one-channel texture's texel too, pt_scene.h)
    if ((rc = uploadArray(ctx, ctx->sceneMem, sd->texels, sd->num_texel_floats, &s.texels, 16)) != TGHIP_OK) return rc;
    if ((rc = uploadArray(ctx, ctx->sceneMem, sd->dist, sd->num_dist_floats, &s.dist)) != TGHIP_OK) return rc;
    if ((rc = uploadArray(ctx, ctx->sceneMem, sd->light_tris, sd->num_light_tri_floats, &s.light_tris)) != TGHIP_OK) return rc;
    // the tables derived from the description (SceneTraits)
    if ((rc = uploadArray(ctx, ctx->sceneMem, sc.guide.data(), sc.guide.size(), &s.guide)) != TGHIP_OK) return rc;
    if ((rc = uploadArray(ctx, ctx->sceneMem, sc.texGuide.data(), sc.texGuide.size(), &s.tex_guide)) != TGHIP_OK) return rc;
    if ((rc = uploadArray(ctx, ctx->sceneMem, reinterpret_cast<const float2 *>(sc.rows.data()), sc.rows.size()/2, &s.rows)) != TGHIP_OK) return rc;
    if ((rc = uploadArray(ctx, ctx->sceneMem, sc.texRows.data(), sc.texRows.size(), &s.tex_rows)) != TGHIP_OK) return rc;
    s.env_tex = sc.env_tex; s.env_h = sc.env_h;
    s.env_marginal = sc.env_tex >= 0 ? s.dist + sd->textures[sc.env_tex].dist_offset : nullptr;   // mpdf[h] mcdf[h + 1] (device pointer arithmetic only)
    if ((rc = uploadArray(ctx, ctx->sceneMem, sc.envGuide.data(), sc.envGuide.size(), &s.env_guide)) != TGHIP_OK) return rc;
    ctx->opt.ldsTables = true;            // ("lds_tables" = 0 holds until the next upload)
    if ((rc = uploadArray(ctx, ctx->sceneMem, sc.recClass.data(), sc.recClass.size(), &s.rec_class)) != TGHIP_OK) return rc;
    s.num_nodes = sd->num_nodes; s.num_recs = sd->num_recs; s.num_objects = sd->num_objects;
    s.num_lights = sd->num_lights; s.num_infinite_lights = sd->num_infinite_lights;
    s.num_bsdfs = sd->num_bsdfs; s.num_textures = sd->num_textures;
    s.num_instances = sd->num_instances;
    if (sd->num_instances) {
        if ((rc = uploadArray(ctx, ctx->sceneMem, sd->inst_prims, size_t(sd->num_inst_prims), &s.inst_prims)) != TGHIP_OK) return rc;
        const float4 *boxes = nullptr;
        if ((rc = uploadArray(ctx, ctx->sceneMem, reinterpret_cast<const float4 *>(sd->inst_leaf_boxes), size_t(sd->num_inst_prims)*2, &boxes)) != TGHIP_OK) return rc;
        s.inst_leaf_boxes = boxes;
        const float4 *tight = nullptr;
        if ((rc = uploadArray(ctx, ctx->sceneMem, reinterpret_cast<const float4 *>(sd->inst_tight_boxes), size_t(sd->num_top_recs)*2, &tight)) != TGHIP_OK) return rc;
        s.inst_tight_boxes = tight;
    }
    if (sc.topTree) {
        static_assert(sizeof(TgHipTopNode) == 28*sizeof(float), "TgHipTopNode layout");
        if ((rc = uploadArray(ctx, ctx->sceneMem, reinterpret_cast<const float *>(sd->top_nodes), size_t(sd->num_top_nodes)*28, &s.top_nodes)) != TGHIP_OK) return rc;
        if ((rc = uploadArray(ctx, ctx->sceneMem, reinterpret_cast<const float4 *>(sc.flatBoxes.data()), sc.flatBoxes.size()/4, &s.flat_boxes)) != TGHIP_OK) return rc;
    }
    s.num_media = sd->num_media;
    if (sd->num_media && (rc = uploadArray(ctx, ctx->sceneMem, sd->media, size_t(sd->num_media), &s.media)) != TGHIP_OK) return rc;
    if ((rc = uploadArray(ctx, ctx->sceneMem, &sd->camera, 1, &s.camera)) != TGHIP_OK) return rc;
    if (sd->sobol_matrices && (rc = uploadArray(ctx, ctx->sceneMem, sd->sobol_matrices, size_t(sd->num_sobol_words), &s.sobol)) != TGHIP_OK) return rc;
    s.settings = sd->settings;

    // framebuffer
    if (ctx->width != uint32_t(sd->camera.res_x) || ctx->height != uint32_t(sd->camera.res_y) || !ctx->fbSum) {
        ctx->fbSum.release(); ctx->fbCount.release(); ctx->dAux.release();
        ctx->width = uint32_t(sd->camera.res_x); ctx->height = uint32_t(sd->camera.res_y);
        size_t npix = size_t(ctx->width)*ctx->height;
        if ((rc = ctx->fbSum.grow(ctx, npix*3)) != TGHIP_OK) return rc;
        if ((rc = ctx->fbCount.grow(ctx, npix)) != TGHIP_OK) return rc;
        // tile seeds, SampleRecords and the per-record pass arrays
        ctx->extMem.release();
        const size_t tiles = size_t((ctx->width + 15)/16)*((ctx->height + 15)/16);
        const size_t recs = size_t((ctx->width + 3)/4)*((ctx->height + 3)/4);
        if ((rc = allocArray(ctx, ctx->extMem, tiles, &ctx->dTileSeeds)) != TGHIP_OK) return rc;
        if ((rc = allocArray(ctx, ctx->extMem, recs, &ctx->dRecIndex)) != TGHIP_OK) return rc;
        if ((rc = allocArray(ctx, ctx->extMem, recs, &ctx->dRecCount)) != TGHIP_OK) return rc;
        if ((rc = allocArray(ctx, ctx->extMem, recs, &ctx->dRecLum)) != TGHIP_OK) return rc;
        if ((rc = allocArray(ctx, ctx->extMem, recs, &ctx->dRecords)) != TGHIP_OK) return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->haveScene = true;
    if ((rc = replan(ctx)) != TGHIP_OK) return rc;
    return tghip_clear_framebuffer(ctx);
}

int tghip_clear_framebuffer(tghip_ctx *ctx)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t npix = size_t(ctx->width)*ctx->height;
    float *sum = ctx->frameSum();
    uint32_t *cnt = ctx->frameCount();
    HIP_TRY(ctx, hipMemsetAsync(sum, 0, npix*3*sizeof(float), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(cnt, 0, npix*sizeof(uint32_t), ctx->stream));
    const size_t recs = size_t((ctx->width + 3)/4)*((ctx->height + 3)/4);
    HIP_TRY(ctx, hipMemsetAsync(ctx->dRecords, 0, recs*sizeof(TgHipSampleRecord), ctx->stream));
    if (ctx->dAux) HIP_TRY(ctx, hipMemsetAsync(ctx->dAux.get(), 0, npix*sizeof(TgHipAuxPixel), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TGHIP_OK;
}

int tghip_bind_framebuffer(tghip_ctx *ctx, float *dev_rgb_sum, uint32_t *dev_count)
{
    if (!ctx) return TGHIP_E_INVALID;
    if ((dev_rgb_sum == nullptr) != (dev_count == nullptr)) { ctx->error = "bind both buffers or neither"; return TGHIP_E_INVALID; }
    ctx->extSum = dev_rgb_sum;
    ctx->extCount = dev_count;
    return TGHIP_OK;
}


// Runs the wavefront loop for one batch of work items until every slot is drained.
static int runBatch(tghip_ctx *ctx, const PassParams &pp, const PassTarget &target)
{
    if (ctx->abortRequested.load(std::memory_order_acquire))
        return TGHIP_E_ABORTED;                  // aborted before this batch started: nothing to drain
    PathState st = ctx->pool;
    st.partial = ctx->partial.get();
    st.abort_flag = ctx->abortFlagDev.get();
    st.leaf_batch = uint32_t(ctx->leafBatch);
    const LaunchPlan &lp = ctx->lp;              // (tghip_wait planned the pass's kind)
    const LaunchChoice &choice = lp.choice;
    st.inst_tree_depth = uint32_t(choice.instTreeDepth);
    st.inst_phase_min = uint32_t(ctx->instPhaseMin);
    st.inst_refill_at = uint32_t(ctx->instRefillAt);
    st.nee_factors = choice.neeFactors ? 1u : 0u;   // the closest-hit shadow walk, k_trace_shadow<., FORWARD>
    st.suspend_lanes = ctx->poolWalkArrays ? uint32_t(ctx->suspendLanes) : 0u;
    st.suspend_turns = uint32_t(std::max(ctx->suspendTurns, 1));
    st.suspend_min_queue = uint32_t(ctx->suspendMinQueue);
    st.leaf_batch_bvh2 = uint32_t(ctx->leafBatchBvh2 > 0 ? ctx->leafBatchBvh2 : ctx->sc.haveInstances ? 16 : ctx->leafBatch);
    const DeviceScene &s = ctx->scene;
    const int grid = int(ctx->poolGrid);
    const bool fused = choice.fusedFlat;
    const bool runToCompletion = choice.oneLaunch;   // one launch renders the whole batch

    // optional per-launch timing: one event pair per kernel launch of a check interval, read back at the
    // interval's host sync (events live on ctx->stream, the stream the kernels are launched on)
    const bool timing = ctx->timeKernels;
    // (short batches: 8 -- every check drains all streams, ~0.2 ms in which nothing runs, and most of a short pass is its drain: 27 near-empty
    // iterations of ~150 us each for the 16-spp passes of the as-shipped materialtest, profiles/README.md; the price is <= 7 empty iterations
    // of ~55 us after the last path has ended)
    const int checkInterval = ctx->checkInterval > 0 ? ctx->checkInterval : (uint64_t(pp.total_items) >= 4ull*st.num_slots ? 16 : 8);
    const size_t evNeeded = size_t(checkInterval)*3*2*8;          // (every part's launches are timed: up to eight parts)
    if (timing) {
        while (ctx->evPool.size() < evNeeded) {
            hipEvent_t e = nullptr;
            HIP_TRY(ctx, hipEventCreate(&e));
            ctx->evPool.push_back(e);
        }
    }
    size_t evUsed = 0;
    // (on the stream the launch goes to: ctx->launchStream is the part's own stream inside the split loop)
    auto ticMain = [&]() { if (timing) (void)hipEventRecord(ctx->evPool[evUsed++], ctx->launchStream); };
    auto tic = ticMain;

    // "streams" = N > 1: the workgroups (and with them the slots, queues and work items) are split into N parts that run the same
    // wavefront loop on N streams: kernels of different parts share the CUs (csrc/host/LaunchChoice.cpp), and the drain tail of one part's kernel
    // overlaps the other parts' kernels
    int parts = choice.parts;
    if (grid < 2*parts || grid % parts != 0 || pp.total_items < uint32_t(2*parts)*PT_ITEM_GROUP)
        parts = 1;
    const bool split = parts > 1;
    PathState stPart[8] = {st, st, st, st, st, st, st, st};
    PassParams ppPart[8] = {pp, pp, pp, pp, pp, pp, pp, pp};
    hipStream_t streamOf[8] = {ctx->stream, ctx->partStream[0], ctx->partStream[1], ctx->partStream[2], ctx->partStream[3], ctx->partStream[4], ctx->partStream[5], ctx->partStream[6]};
    if (split) {
        const uint32_t groups = (pp.total_items + PT_ITEM_GROUP - 1)/PT_ITEM_GROUP;
        uint32_t itemBegin = 0;
        for (int k = 0; k < parts; ++k) {
            const uint32_t off = uint32_t(grid/parts)*uint32_t(k);
            for (uint32_t g = 0; g < PT_POOL_GROUPS; ++g)
                stPart[k].poolg[g] = st.poolg[g] + size_t(off)*st.slots_per_block*16u;
            stPart[k].bm = st.bm + size_t(off)*(st.slots_per_block >> 5);
            stPart[k].ctl = st.ctl + off;
            stPart[k].stats = st.stats + off;
            stPart[k].num_slots = st.num_slots/uint32_t(parts);
            const uint32_t itemEnd = k + 1 == parts ? pp.total_items : std::min(pp.total_items, uint32_t((uint64_t(groups)*(k + 1) + parts - 1)/parts)*PT_ITEM_GROUP);
            ppPart[k].item_begin = pp.item_begin + itemBegin;
            ppPart[k].total_items = itemEnd - itemBegin;
            itemBegin = itemEnd;
        }
    }
    HIP_TRY(ctx, hipMemsetAsync(st.partial, 0, size_t(pp.total_items)*sizeof(float4), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(st.live, 0, 4*sizeof(uint32_t), ctx->stream));
    if (split) {
        HIP_TRY(ctx, hipEventRecord(ctx->evMain, ctx->stream));            // (the memsets above come first for the other streams as well)
        for (int k = 0; k < parts; ++k) {
            if (k) HIP_TRY(ctx, hipStreamWaitEvent(streamOf[k], ctx->evMain, 0));
            hipLaunchKernelGGL(k_start, dim3(grid/parts), dim3(256), 0, streamOf[k], s, stPart[k], ppPart[k]);
        }
    } else {
        hipLaunchKernelGGL(k_start, dim3(grid), dim3(256), 0, ctx->stream, s, st, pp);
    }
    // k_tail: per-launch timing does not see it (the few thousand rays it traces are in the counters, its one launch is in none of the three kernel classes)
    const bool tailEligible = choice.tailEligible && st.slots_per_block <= PT_MAX_SLOTS_PER_BLOCK;
    const bool tailFits = tailEligible && lp.tailFits;
    const uint64_t tailThreshold = uint64_t(std::max<long long>(ctx->tailThreshold, 0));
    const bool foldFinish = choice.foldFinish;   // k_finish rides in front of the next iteration's closest-hit launch
    const int shadeLaunches = choice.shadeLaunches;
    uint32_t iterTag = 1;                        // k_start publishes tag 1 when it queued anything
    bool first = true;
    int roundIters = checkInterval;              // launches of the wavefront loop between two host checks
        // the launches of one wavefront iteration over the workgroups [0, grid) of `st` (the whole pool, or one part of it)
        // The shading launches of an iteration, in the choice's order.  The classes (the escaped paths, Q_MISS; 0; the classes 1 .. 3 that occur) consume queues
        // of their own and OR what they append into the workgroup's bitmaps (k_shade: CONCURRENT), so their launches MAY run side by side on three
        // streams: the "class_streams" option gives launches a lane beside the part's stream.  Measured slower than one after the other (materialtest
        // 735-800 against 825-830 Msamples/s, mesh1m 409 against 508, for 2 to 24 hardware queues): with four parts in flight the chip is not short of
        // independent launches.
        auto launchShading = [&](const PathState &st, const PassParams &pp, int grid, int part) {
            const hipStream_t mainStream = ctx->launchStream;
            bool forked = false, lanes[3] = {false, false, false};
            for (int i = 0; i < choice.numShade; ++i) {
                const int lane = choice.shade[i].lane;
                hipStream_t stream = mainStream;
                if (lane) {
                    stream = ctx->classStream[part][lane - 1];
                    if (!forked) (void)hipEventRecord(ctx->evFork[part], mainStream);
                    (void)hipStreamWaitEvent(stream, ctx->evFork[part], 0);
                    forked = lanes[lane] = true;
                }
                launchKernel(lp.shade[i], grid, stream, s, st, pp, choice.shade[i].cls);
                if (lane) (void)hipEventRecord(ctx->evJoin[part][lane - 1], stream);
            }
            for (int lane = 1; lane < 3; ++lane)
                if (lanes[lane]) (void)hipStreamWaitEvent(mainStream, ctx->evJoin[part][lane - 1], 0);
        };
        // the launches of one wavefront iteration over the workgroups [0, grid) of `st` (the whole pool, or one part of it)
        auto launchIteration = [&](const PathState &st, const PassParams &pp, int grid, uint32_t iterTag, bool timed, int part) {
            auto tic = [&]() { if (timed) ticMain(); };
            if (choice.queryPaths)                  // (the fresh paths of the previous iteration's finish / of k_start get the caller's rays before they are traced)
                radianceQueryLaunchPaths(ctx->launchStream, grid, st, target.rays, target.numRays);
            else if (choice.cameraRays)             // (the fresh camera rays of the previous iteration's finish / of k_start, before they are traced)
                hipLaunchKernelGGL(k_camera_rays, dim3(grid), dim3(256), 0, ctx->launchStream, s, st, pp);
            tic();
            if (choice.closest.kernel.family == K_FINISH_CLOSEST_WIDE)   // (k_finish's work of the previous iteration in front of the walk, pt_wavefront.h)
                launchKernel(lp.closest, grid, ctx->launchStream, s, st, pp);
            else
                launchKernel(lp.closest, grid, ctx->launchStream, s, st);
            tic();
            // (the end of a query's first segment, before the hits are shaded.  Launched whether or not a ray of the batch has a finite tmax: the rays
            // may be device memory, which the host could only know that of after a reduction over them -- about 10 us per launch, profiles/radiance_query/bench.txt)
            if (choice.queryPaths)
                radianceQueryLaunchClip(ctx->launchStream, grid, st, target.rays, target.numRays);
            tic();
            launchShading(st, pp, grid, part);
            tic(); tic();
            launchKernel(lp.shadow, grid, ctx->launchStream, s, st, pp, iterTag);
            tic();
            if (!foldFinish)                     // (always: the shading launches leave their finished paths to k_finish as well; folded: the next iteration's
                                                 // closest-hit launch, or finishParts before a host check)
                hipLaunchKernelGGL(k_finish, dim3(grid), dim3(256), 0, ctx->launchStream, s, st, pp, iterTag);
        };
        // folded k_finish: the last iteration's finish as a launch of its own -- before the host reads the liveness word, before k_tail
        auto finishParts = [&](uint32_t tag) {
            for (int k = 0; k < parts; ++k)
                hipLaunchKernelGGL(k_finish, dim3(grid/parts), dim3(256), 0, split ? streamOf[k] : ctx->stream, s, split ? stPart[k] : st, split ? ppPart[k] : pp, tag);
        };
    for (;;) {
        evUsed = 0;
        {
            // an abort request that arrived since the last check (or before the pass's first launch): make sure the device
            // word is set -- in stream order, so the launches below see it and drain their slots
            for (int k = 1; k < parts; ++k) {   // the main stream waits for the other parts before it reads the flag
                HIP_TRY(ctx, hipEventRecord(ctx->evPart[k - 1], streamOf[k]));
                HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->evPart[k - 1], 0));
            }
            if (ctx->abortRequested.load(std::memory_order_acquire))
                HIP_TRY(ctx, hipMemsetAsync(ctx->abortFlagDev.get(), 0xFF, sizeof(uint32_t), ctx->stream));
            if (tailEligible) hipLaunchKernelGGL(k_live_slots, dim3(1), dim3(256), 0, ctx->stream, st, uint32_t(grid));
            HIP_TRY(ctx, hipMemcpyAsync(ctx->hostLive, st.live, 2*sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (timing && !first) {
                double *acc[3] = {&ctx->counters.ms_trace_closest, &ctx->counters.ms_shade, &ctx->counters.ms_trace_shadow};
                // (split loop: EVERY part's launches are bracketed, each on its own stream -- three pairs per part and iteration, in launch
                // order.  Rounds 2-4 timed part 0 only and counted the others "as long on average": they are not -- the parts whose
                // streams the hardware queues serve later run ~45 % longer launches (rocprofv3's kernel trace, profiles/README.md) --, so the
                // per-kernel averages were part 0's, a fifth below the mean)
                size_t pairs = size_t(roundIters)*3*size_t(parts);
                for (size_t k = 0; k < pairs; ++k) {
                    float ms = 0.0f;
                    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->evPool[2*k], ctx->evPool[2*k + 1]));
                    *acc[k % 3] += double(ms);
                }
                const int perIter = parts;
                ctx->counters.launches_trace_closest += roundIters*perIter;
                ctx->counters.launches_trace_shadow += roundIters*perIter;
                ctx->counters.launches_shade += roundIters*perIter*shadeLaunches;   // (one event pair brackets them: ms_shade is their sum)
            }
            if (ctx->hostLive[0] != iterTag)
                break;                           // the last iteration left every extension queue empty
            if (tailFits && uint64_t(ctx->hostLive[1]) <= tailThreshold) {
                // few paths left: each part of the pool finishes in one launch of k_tail (its workgroups iterate on their own)
                uint32_t classes = 1u;
                for (int c = 1; c < PT_NUM_CLASSES; ++c)
                    if (ctx->sc.classPresent[c]) classes |= 1u << c;
                for (int k = 0; k < parts; ++k) {
                    const hipStream_t stream = split ? streamOf[k] : ctx->stream;
                    if (k) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->evMain, 0));   // (after the main stream's check above)
                    else if (split) HIP_TRY(ctx, hipEventRecord(ctx->evMain, ctx->stream));
                    launchKernel(lp.tail, grid/parts, stream, s, split ? stPart[k] : st, split ? ppPart[k] : pp, classes);
                }
                for (int k = 1; k < parts; ++k) {
                    HIP_TRY(ctx, hipEventRecord(ctx->evPart[k - 1], streamOf[k]));
                    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->evPart[k - 1], 0));
                }
                ctx->counters.tail_launches++;
                if (std::getenv("TGHIP_VERBOSE")) {
                    const auto t0 = std::chrono::steady_clock::now();
                    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                    std::fprintf(stderr, "[tghip]   tail kernel after %llu iterations with %u paths alive: %.2f ms\n", (unsigned long long)(iterTag - 1), ctx->hostLive[1],
                                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
                }
                break;
            }
        }
        first = false;
        roundIters = runToCompletion ? 1 : checkInterval;
        for (int it = 0; it < roundIters; ++it) {
            ++iterTag;
            if (fused) {
                // flat-list scene: intersection and shadow tests happen inside the shading launches
                PassParams ppi = pp;
                ppi.iter_tag = iterTag;
                tic(); tic(); tic();
                launchShading(st, ppi, grid, 0);
                tic(); tic(); tic();
                ctx->counters.iterations++;
                continue;
            }
            if (split) {
                // (rejected, round 5: part k's iteration i on stream (k + i) mod parts, so that every part spends the same time on every hardware
                // queue: profiles/r5_sweep_rotate_streams.jsonl)
                for (int k = 0; k < parts; ++k) {
                    ctx->launchStream = streamOf[k];
                    launchIteration(stPart[k], ppPart[k], grid/parts, iterTag, true, k);
                }
                ctx->launchStream = ctx->stream;
            } else {
                launchIteration(st, pp, grid, iterTag, true, 0);
            }
            ctx->counters.iterations++;
        }
        if (foldFinish && !fused)
            finishParts(iterTag);
    }
    float *sum = target.sum;
    uint32_t *cnt = target.count;
    if (pp.rec_sorted) hipLaunchKernelGGL(k_resolve_records, dim3((pp.num_sorted*16u + 255)/256), dim3(256), 0, ctx->stream, st, pp, sum, cnt);
    else               hipLaunchKernelGGL(k_resolve, dim3((pp.pix_slots + 255)/256), dim3(256), 0, ctx->stream, st, pp, sum, cnt);
    HIP_TRY(ctx, hipGetLastError());
    return ctx->abortRequested.load(std::memory_order_acquire) ? TGHIP_E_ABORTED : TGHIP_OK;
}

// PassParams::rec_hint of a record pass: hint[g] = the chunk item 64 g lies in -- the last c < chunks with start[c] <= 64 g (the chunk starts never
// decrease; nextPath walks on from there while its item is >= start[c + 1], which ends at the sentinel behind the last chunk at the latest)
__global__ void k_record_hints(const uint32_t *start, uint32_t chunks, uint32_t *hint, uint32_t n)
{
    const uint32_t g = blockIdx.x*blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint64_t item = uint64_t(g)*64u;
    uint32_t lo = 0, hi = chunks;                 // invariant: start[lo] <= item, and start[hi] > item or hi == chunks
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (uint64_t(start[mid]) <= item) lo = mid; else hi = mid;
    }
    hint[g] = lo;
}

// The pass itself is driven synchronously from tghip_wait (the integrator calls it from its worker
// thread, which gives the reference's "startRender returns immediately" contract).
int tghip_render_pass(tghip_ctx *ctx, const TgHipPassDesc *pass)
{
    if (!ctx || !pass) return TGHIP_E_INVALID;
    if (!ctx->haveScene) { ctx->error = "render before upload"; return TGHIP_E_NOSCENE; }
    const int rc = checkPass(*pass, ctx->width, ctx->height, ctx->scene.sobol != nullptr, ctx->error);   // (csrc/host/PassPlan.cpp)
    if (rc != TGHIP_OK) return rc;
    ctx->abortRequested.store(false, std::memory_order_release);   // a request is cleared where a pass begins: here, and in tghip_query_radiance for its pass
    ctx->passPending = true;
    ctx->passResult = TGHIP_OK;
    ctx->pendingPass = *pass;
    return TGHIP_OK;
}

} // extern "C"

// The planned pass `plan` of `pass` over a w x h image, into `target`: the launch plan of its kind, the device arrays the plan names, the pool, the
// wavefront loop batch by batch.  What tghip_wait runs for a render pass (w x h the scene's image, the target the context's framebuffer) and
// tghip_query_radiance for a query (the virtual image of the rays, a framebuffer of its own).  Synchronous.
static int runPass(tghip_ctx *ctx, const TgHipPassDesc &pass, uint32_t w, uint32_t h, PassPlan &plan, const PassTarget &target)
{
    const bool verbose = std::getenv("TGHIP_VERBOSE") != nullptr;
    const auto tWait0 = std::chrono::steady_clock::now();
    auto msSince = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    int rc = TGHIP_OK;
    // the kernels of a pass of this kind -- a short batch runs on ONE stream with 4 workgroups per CU (PassPlan.cpp: shortBatch) --: planned again only
    // when the kind differs from the last pass's
    PassKind kind = passKindOf(ctx->sc, pass.flags, plan.shortBatch, ctx->countTraversal);
    kind.rayPaths = target.rayPaths;
    if (!(kind == ctx->lp.kind) && (rc = planLaunches(ctx, kind, ctx->lp)) != TGHIP_OK)
        return rc;

    // the device arrays the plan names
    auto upload = [&](DeviceArray<uint32_t> &dev, const std::vector<uint32_t> &src) -> int {
        const int grc = dev.grow(ctx, src.size());
        if (grc != TGHIP_OK) return grc;
        if (!src.empty())
            HIP_TRY(ctx, hipMemcpyAsync(dev.get(), src.data(), src.size()*sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        return TGHIP_OK;
    };
    PassParams base{};
    base.shard_index = pass.shard_index; base.shard_count = plan.shardCount;
    base.shard_skew = plan.shardSkew;
    base.tiles_x = plan.tilesX; base.num_tiles = plan.numTiles;
    base.width = w; base.height = h;
    // (a query's paths start behind the camera: no lens point is drawn for them)
    base.flags = pass.flags | (ctx->sc.thinlens && !target.rayPaths ? PT_PASS_THINLENS : 0u) | (ctx->sc.haveMedia ? PT_PASS_MEDIA : 0u);
    base.variance_w = plan.varianceW;
    if (plan.shardCount > 1) {
        if (plan.ownedStale) {                   // the shard's tile list changed: rare
            if ((rc = upload(ctx->dOwnedTiles, plan.ownedList)) != TGHIP_OK) return rc;
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            plan.ownedStale = false;
        }
        base.owned_tiles = ctx->dOwnedTiles.get();
    }
    if ((pass.flags & TGHIP_PASS_SOBOL) && target.tileSeeds) {
        base.tile_seeds = target.tileSeeds;
    } else if (pass.flags & TGHIP_PASS_SOBOL) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dTileSeeds, pass.tile_seeds, size_t(plan.numTiles)*sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        base.tile_seeds = ctx->dTileSeeds;
    }
    if (plan.recordPass) {
        const size_t recBytes = size_t(plan.numRecords)*sizeof(uint32_t);
        if ((rc = ctx->lum.grow(ctx, size_t(plan.lumFloats))) != TGHIP_OK) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dRecIndex, plan.recIndex.data(), recBytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dRecCount, plan.recCount.data(), recBytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dRecLum, plan.recLum.data(), recBytes, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = upload(ctx->dSorted, plan.sorted)) != TGHIP_OK) return rc;
        if ((rc = upload(ctx->dChunkStart, plan.chunkStart)) != TGHIP_OK) return rc;
        // the hint table -- for every 64 items the chunk their first one lies in -- is filled by a launch from the chunk starts
        if ((rc = ctx->dHint.grow(ctx, plan.hintEntries)) != TGHIP_OK) return rc;
        hipLaunchKernelGGL(k_record_hints, dim3(uint32_t((plan.hintEntries + 255)/256)), dim3(256), 0, ctx->stream, ctx->dChunkStart.get(), plan.chunksAll, ctx->dHint.get(), uint32_t(plan.hintEntries));
        HIP_TRY(ctx, hipGetLastError());
        base.rec_index = ctx->dRecIndex; base.rec_count = ctx->dRecCount; base.rec_lum = ctx->dRecLum;
        base.lum = ctx->lum.get();
        base.rec_sorted = ctx->dSorted.get(); base.rec_chunk_start = ctx->dChunkStart.get(); base.rec_hint = ctx->dHint.get();
        base.num_sorted = uint32_t(plan.sorted.size());
        base.num_chunks = plan.chunksAll;
    }
    if (plan.auxPass && !ctx->dAux) {
        const size_t npix = size_t(w)*h;
        if ((rc = ctx->dAux.grow(ctx, npix)) != TGHIP_OK) return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->dAux.get(), 0, npix*sizeof(TgHipAuxPixel), ctx->stream));
    }
    base.aux = ctx->dAux.get();
    if (pass.flags & TGHIP_PASS_SAMPLES) {
        const size_t need = size_t(w)*h*plan.spp*3u;
        if ((rc = ctx->dSamples.grow(ctx, need)) != TGHIP_OK) return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->dSamples.get(), 0, need*sizeof(float), ctx->stream));
        ctx->samplesFloats = need;
        base.samples = ctx->dSamples.get(); base.samples_begin = plan.sppBegin; base.samples_spp = plan.spp;
    }

    uint64_t wantSlots = std::min<uint64_t>(uint64_t(ctx->maxSlots), plan.batchItems);
    // the run-to-completion kernel (runBatch) gives every thread its own slots for the whole launch: one slot per
    // thread keeps the whole path state (112 B x 0.5 M slots) inside the Infinity Cache -- measured +5 % over four
    if (ctx->lp.choice.oneLaunch && !ctx->maxSlotsSet)
        wantSlots = std::min<uint64_t>(wantSlots, uint64_t(launchGrid(ctx))*uint64_t(ctx->lp.thrShade[SIZE_SIMPLE]));
    if ((rc = ensurePool(ctx, uint32_t(wantSlots))) != TGHIP_OK) return rc;
    if ((rc = ctx->partial.grow(ctx, size_t(plan.batchItems))) != TGHIP_OK) return rc;
    // the device word still holds the previous pass's abort, if any; a request for THIS pass is re-mirrored by runBatch
    HIP_TRY(ctx, hipMemsetAsync(ctx->abortFlagDev.get(), 0, sizeof(uint32_t), ctx->stream));

    const double msSetup = msSince(tWait0);
    const unsigned long long itersBefore = ctx->counters.iterations;
    const auto tLoop0 = std::chrono::steady_clock::now();
    HIP_TRY(ctx, hipEventRecord(ctx->evA, ctx->stream));
    for (size_t bi = 0; bi < plan.batches.size() && rc == TGHIP_OK; ++bi) {
        const PassBatch &b = plan.batches[bi];
        PassParams pp = base;
        pp.spp_begin = b.sppBegin; pp.spp_end = b.sppEnd; pp.seed = pass.seed;
        pp.chunk = plan.chunk;
        pp.group = target.rayPaths ? 1u : plan.group;   // (a query's one-sample items are added to the ray's sum one by one: tghip_query_radiance)
        pp.chunks = b.chunks;
        pp.pix_slots = b.pixSlots;
        pp.item_base = b.itemBase;
        pp.total_items = b.totalItems;
        pp.first_tile = b.firstTile;
        rc = runBatch(ctx, pp, target);
    }
    if (plan.recordPass && rc == TGHIP_OK) {
        hipLaunchKernelGGL(k_records, dim3((plan.numRecords + 63)/64), dim3(64), 0, ctx->stream, base, ctx->dRecords, plan.numRecords);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->evB, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->evA, ctx->evB));
    ctx->counters.ms_total += ms;
    if (verbose)
        std::fprintf(stderr, "[tghip] pass spp [%u, %u) flags %u: %llu items of %u samples in batches of %llu, %u slots, short %d; setup %.2f ms, loop %.2f ms (%llu iterations, device %.2f ms)\n",
                     pass.spp_begin, pass.spp_end, pass.flags, (unsigned long long)plan.totalItems, plan.chunk,
                     (unsigned long long)plan.batchItems, ctx->pool.num_slots, int(plan.shortBatch), msSetup, msSince(tLoop0), (unsigned long long)(ctx->counters.iterations - itersBefore), double(ms));
    return rc;
}

// The launches of `launch` between the context's two timing events, `after` -- the copies back into host memory -- behind them and, once the stream
// has run dry, the launches' milliseconds in `ms`.
template<typename Launch, typename After>
static int timedLaunches(tghip_ctx *ctx, double &ms, Launch launch, After after)
{
    HIP_TRY(ctx, hipEventRecord(ctx->evA, ctx->stream));
    int rc = launch();
    if (rc != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->evB, ctx->stream));
    if ((rc = after()) != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float elapsed = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&elapsed, ctx->evA, ctx->evB));
    ms = elapsed;
    return TGHIP_OK;
}
// ... and what the tghip_*_kernel_time functions answer: the milliseconds the last such call stored
static int kernelTime(const tghip_ctx *ctx, double tghip_ctx::*stored, double *ms)
{
    if (!ctx || !ms) return TGHIP_E_INVALID;
    *ms = ctx->*stored;
    return TGHIP_OK;
}

// Idle lanes of a wave at which the wide walk of tghip_query_rays claims new rays, and its workgroups per CU (swept: profiles/ray_query_ab.txt)
#define RAY_QUERY_REFILL_AT 48
#define RAY_QUERY_BLOCKS_PER_CU 2

// How tghip_query_rays, _surface, _transmittance and _direct walk on the uploaded scene: the walk tghip_trace_rays answers with, its stack in LDS,
// the refill threshold, whether hits are reached through instances, and the workgroups of a launch over `live` rays -- "query_blocks", or as many as
// stay resident, no more than there are waves for (a workgroup without a ray only reads the counter).
struct QueryWalk {
    RayQueryWalk walk;
    size_t lds;
    uint32_t refillAt, fixedBlocks, residentBlocks;
    bool inst;
    uint32_t blocks(size_t live) const { return fixedBlocks ? fixedBlocks : uint32_t(std::min<size_t>(residentBlocks, ((live + 63)/64 + 3)/4)); }
};
static QueryWalk queryWalk(const tghip_ctx *ctx)
{
    const LaunchChoice &choice = ctx->lp.choice;
    const bool wide = choice.rayWalk == LaunchChoice::RAYS_WIDE;
    QueryWalk q;
    q.inst = choice.rayWalk == LaunchChoice::RAYS_INST;
    q.walk = wide ? RAY_QUERY_WIDE : q.inst ? RAY_QUERY_INST : choice.rayWalk == LaunchChoice::RAYS_FLAT ? RAY_QUERY_FLAT : RAY_QUERY_BVH2;
    q.lds = wide ? size_t(std::max(ctx->sc.wideDepth, 1))*RAY_QUERY_THREADS*sizeof(uint2)
                 : std::max<size_t>(ldsBytes(ctx->sc, choice, LDS_TRACE, RAY_QUERY_THREADS), sizeof(int));
    q.refillAt = uint32_t(ctx->queryRefillAt > 0 ? ctx->queryRefillAt : RAY_QUERY_REFILL_AT);
    q.fixedBlocks = uint32_t(std::max(ctx->queryBlocks, 0));
    q.residentBlocks = uint32_t(ctx->prop.multiProcessorCount)*RAY_QUERY_BLOCKS_PER_CU;
    return q;
}

// A query needs a scene ...
static int queryScene(tghip_ctx *ctx, const char *fn)
{
    if (!ctx->haveScene) ctx->error = std::string(fn) + " before tghip_upload_scene";
    return ctx->haveScene ? TGHIP_OK : TGHIP_E_NOSCENE;
}
// ... and, behind its own argument check, begins like this: the scene; for a batch that is not empty -- the caller answers an empty one -- the pass
// under way run out (one that was aborted is no error of the query's), the device, the counter words.
static int queryBegin(tghip_ctx *ctx, const char *fn, size_t n)
{
    int rc = queryScene(ctx, fn);
    if (rc != TGHIP_OK || n == 0) return rc;
    rc = tghip_wait(ctx);
    if (rc != TGHIP_OK && rc != TGHIP_E_ABORTED) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, ctx->queryCounter.once(16));
    return TGHIP_OK;
}

// The start medium of a description: TGHIP_MEDIUM_OF_CAMERA is the camera's
template<typename Params>
static void queryStartMedium(const tghip_ctx *ctx, int32_t medium, Params &p)
{
    p.cameraMedium = ctx->sc.cameraMedium;
    p.medium = medium == TGHIP_MEDIUM_OF_CAMERA ? p.cameraMedium : medium;
}

extern "C" {

int tghip_wait(tghip_ctx *ctx)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!ctx->passPending)
        return ctx->passResult;
    ctx->passPending = false;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const TgHipPassDesc pass = ctx->pendingPass;
    // which tiles, records, work items and batches the pass is made of: host arithmetic on its own (csrc/host/PassPlan.cpp)
    const PassPlanOptions planOpt = {uint64_t(std::max<long long>(ctx->maxItems, 256)), uint64_t(ctx->maxSlots), uint32_t(std::max(ctx->chunkSamples, 0))};
    const int rc = planPass(pass, ctx->width, ctx->height, planOpt, ctx->plan, ctx->error);
    if (rc != TGHIP_OK || ctx->plan.empty)
        return ctx->passResult = rc;
    PassTarget target;
    target.sum = ctx->frameSum();
    target.count = ctx->frameCount();
    return ctx->passResult = runPass(ctx, pass, ctx->width, ctx->height, ctx->plan, target);
}

int tghip_abort(tghip_ctx *ctx)
{
    if (!ctx) return TGHIP_E_INVALID;
    // The request itself is host state: tghip_wait looks at it before every batch and at every liveness check, so it holds
    // even when no kernel of the pass has been launched yet.  The device word (polled whenever a slot asks for new work) is
    // written from a stream of its own so that the copy does not queue behind the running pass.
    ctx->abortRequested.store(true, std::memory_order_release);
    std::lock_guard<std::mutex> lock(ctx->abortMutex);
    static const uint32_t one = 1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipMemcpyAsync(ctx->abortFlagDev.get(), &one, sizeof(one), hipMemcpyHostToDevice, ctx->abortStream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->abortStream);
    if (e != hipSuccess) return TGHIP_E_HIP;    // (ctx->error belongs to the thread driving the pass)
    return TGHIP_OK;
}

int tghip_download_framebuffer(tghip_ctx *ctx, float *rgb_sum, uint32_t *count, size_t npixels)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (npixels != size_t(ctx->width)*ctx->height) { ctx->error = "pixel count mismatch"; return TGHIP_E_INVALID; }
    int rc = tghip_wait(ctx);
    if (rc != TGHIP_OK && rc != TGHIP_E_ABORTED) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const float *sum = ctx->frameSum();
    const uint32_t *cnt = ctx->frameCount();
    if (rgb_sum) HIP_TRY(ctx, hipMemcpyAsync(rgb_sum, sum, npixels*3*sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (count) HIP_TRY(ctx, hipMemcpyAsync(count, cnt, npixels*sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TGHIP_OK;
}

int tghip_upload_framebuffer(tghip_ctx *ctx, const float *rgb_sum, const uint32_t *count, size_t npixels)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (!rgb_sum || !count || npixels != size_t(ctx->width)*ctx->height) { ctx->error = "pixel count mismatch"; return TGHIP_E_INVALID; }
    int rc = tghip_wait(ctx);
    if (rc != TGHIP_OK && rc != TGHIP_E_ABORTED) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    float *sum = ctx->frameSum();
    uint32_t *cnt = ctx->frameCount();
    HIP_TRY(ctx, hipMemcpyAsync(sum, rgb_sum, npixels*3*sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(cnt, count, npixels*sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TGHIP_OK;
}

int tghip_download_records(tghip_ctx *ctx, TgHipSampleRecord *out, size_t n)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (!out || n != size_t((ctx->width + 3)/4)*((ctx->height + 3)/4)) { ctx->error = "record count mismatch"; return TGHIP_E_INVALID; }
    int rc = tghip_wait(ctx);
    if (rc != TGHIP_OK && rc != TGHIP_E_ABORTED) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->dRecords, n*sizeof(TgHipSampleRecord), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TGHIP_OK;
}

int tghip_upload_records(tghip_ctx *ctx, const TgHipSampleRecord *in, size_t n)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (!in || n != size_t((ctx->width + 3)/4)*((ctx->height + 3)/4)) { ctx->error = "record count mismatch"; return TGHIP_E_INVALID; }
    int rc = tghip_wait(ctx);
    if (rc != TGHIP_OK && rc != TGHIP_E_ABORTED) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dRecords, in, n*sizeof(TgHipSampleRecord), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TGHIP_OK;
}

int tghip_download_aux(tghip_ctx *ctx, TgHipAuxPixel *out, size_t npixels)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (!out || npixels != size_t(ctx->width)*ctx->height) { ctx->error = "pixel count mismatch"; return TGHIP_E_INVALID; }
    int rc = tghip_wait(ctx);
    if (rc != TGHIP_OK && rc != TGHIP_E_ABORTED) return rc;
    if (!ctx->dAux) { std::memset(out, 0, npixels*sizeof(TgHipAuxPixel)); return TGHIP_OK; }   // no TGHIP_PASS_AUX pass yet
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->dAux.get(), npixels*sizeof(TgHipAuxPixel), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TGHIP_OK;
}

int tghip_upload_aux(tghip_ctx *ctx, const TgHipAuxPixel *in, size_t npixels)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (!in || npixels != size_t(ctx->width)*ctx->height) { ctx->error = "pixel count mismatch"; return TGHIP_E_INVALID; }
    int rc = tghip_wait(ctx);
    if (rc != TGHIP_OK && rc != TGHIP_E_ABORTED) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->dAux && (rc = ctx->dAux.grow(ctx, npixels)) != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dAux.get(), in, npixels*sizeof(TgHipAuxPixel), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TGHIP_OK;
}

int tghip_download_samples(tghip_ctx *ctx, float *rgb, size_t nfloats)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    int rc = tghip_wait(ctx);
    if (rc != TGHIP_OK && rc != TGHIP_E_ABORTED) return rc;
    if (!rgb || !ctx->dSamples || nfloats != ctx->samplesFloats) { ctx->error = "no TGHIP_PASS_SAMPLES pass of that size has been rendered"; return TGHIP_E_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(rgb, ctx->dSamples.get(), nfloats*sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TGHIP_OK;
}

int tghip_develop(tghip_ctx *ctx, const TgHipDevelopDesc *desc, float *hdr_out, uint8_t *ldr_out, size_t npixels)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_develop: no description"; return TGHIP_E_INVALID; }
    if (!ctx->haveScene) { ctx->error = "tghip_develop before tghip_upload_scene"; return TGHIP_E_NOSCENE; }
    const bool frame = desc->source == TGHIP_DEVELOP_FRAME;
    if (!frame && desc->source >= TGHIP_AUX_OUTPUTS) { ctx->error = "tghip_develop: unknown source"; return TGHIP_E_INVALID; }
    if (desc->part > TGHIP_DEVELOP_VARIANCE) { ctx->error = "tghip_develop: unknown part"; return TGHIP_E_INVALID; }
    if (frame && desc->tonemap > TGHIP_TONEMAP_PBRT) { ctx->error = "tghip_develop: unknown tone-mapping operator"; return TGHIP_E_INVALID; }
    if (frame && desc->part != TGHIP_DEVELOP_MEAN) { ctx->error = "tghip_develop: the framebuffer has no A / B halves and no variance"; return TGHIP_E_INVALID; }
    if (npixels != size_t(ctx->width)*ctx->height) { ctx->error = "pixel count mismatch"; return TGHIP_E_INVALID; }
    if (ctx->developHost) { ctx->error = "tghip_develop: the develop_host option is set (the caller develops on the host)"; return TGHIP_E_UNSUPPORTED; }
    int rc = tghip_wait(ctx);
    if (rc != TGHIP_OK && rc != TGHIP_E_ABORTED) return rc;
    if (!frame && !ctx->dAux) { ctx->error = "tghip_develop: no auxiliary output buffers yet (no TGHIP_PASS_AUX pass, no tghip_upload_aux)"; return TGHIP_E_INVALID; }
    const float *sum = ctx->frameSum();
    const uint32_t *cnt = ctx->frameCount();
    if (frame && ((reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(cnt)) & 15u)) { ctx->error = "tghip_develop: the bound framebuffer is not 16-byte aligned"; return TGHIP_E_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t hdrFloats = npixels*(frame || (desc->source != TGHIP_AUX_DEPTH && desc->source != TGHIP_AUX_VISIBILITY) ? 3 : 1);
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    if (device && ((reinterpret_cast<uintptr_t>(hdr_out) & 15u) || (reinterpret_cast<uintptr_t>(ldr_out) & 3u))) { ctx->error = "tghip_develop: device outputs must be aligned (hdr_out to 16 bytes, ldr_out to 4)"; return TGHIP_E_INVALID; }
    float *hdr = nullptr;
    uint8_t *ldr = nullptr;
    if ((rc = stageOutput(ctx, device, hdr_out, hdrFloats*sizeof(float), ctx->developHdr, hdr)) != TGHIP_OK) return rc;
    if ((rc = stageOutput(ctx, device, ldr_out, npixels*3, ctx->developLdr, ldr)) != TGHIP_OK) return rc;
    HIP_TRY(ctx, ctx->developMax.once(16));
    return timedLaunches(ctx, ctx->developMs, [&]() -> int {
        if (frame) HIP_TRY(ctx, developLaunchFrame(ctx->stream, sum, cnt, npixels, desc->tonemap, hdr, ldr));
        else HIP_TRY(ctx, developLaunchAux(ctx->stream, ctx->dAux.get(), npixels, desc->source, desc->part, hdr, ldr, ctx->developMax.get()));
        return TGHIP_OK;
    }, [&]() -> int {
        const int crc = copyBack(ctx, hdr_out, hdr, hdrFloats*sizeof(float));
        return crc != TGHIP_OK ? crc : copyBack(ctx, ldr_out, ldr, npixels*3);
    });
}

int tghip_develop_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::developMs, ms); }

int tghip_nlmeans(tghip_ctx *ctx, const TgHipNlMeansDesc *desc, const float *image, const float *guide, const float *variance, float *out)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_nlmeans: no description"; return TGHIP_E_INVALID; }
    const bool pointers = desc->source == TGHIP_NLMEANS_POINTERS;
    if (!pointers && desc->source >= TGHIP_AUX_OUTPUTS) { ctx->error = "tghip_nlmeans: unknown source"; return TGHIP_E_INVALID; }
    uint32_t channels = desc->channels;
    if (!pointers) channels = (desc->source == TGHIP_AUX_DEPTH || desc->source == TGHIP_AUX_VISIBILITY) ? 1 : 3;
    if (channels < 1 || channels > 4) { ctx->error = "tghip_nlmeans: channels must be 1..4"; return TGHIP_E_INVALID; }
    if (desc->F > NLMEANS_MAX_F) { ctx->error = "tghip_nlmeans: F must be 0..8"; return TGHIP_E_INVALID; }
    if (desc->R > NLMEANS_MAX_R) { ctx->error = "tghip_nlmeans: R must be 0..16"; return TGHIP_E_INVALID; }
    if (!(desc->k > 0.0f)) { ctx->error = "tghip_nlmeans: k must be positive"; return TGHIP_E_INVALID; }
    if (desc->width == 0 || desc->height == 0) { ctx->error = "tghip_nlmeans: the image has no pixels"; return TGHIP_E_INVALID; }
    if (desc->width > (1u << 20) || desc->height > (1u << 20)) { ctx->error = "tghip_nlmeans: the image is too large"; return TGHIP_E_INVALID; }
    if (!out) { ctx->error = "tghip_nlmeans: no output array"; return TGHIP_E_INVALID; }
    if (pointers && (!image || !guide || !variance)) { ctx->error = "tghip_nlmeans: image, guide and variance are needed without an aux source"; return TGHIP_E_INVALID; }
    if (!pointers && (image || guide || variance)) { ctx->error = "tghip_nlmeans: an aux source takes no image, guide or variance pointers"; return TGHIP_E_INVALID; }
    if (!pointers && (desc->image_part > TGHIP_DEVELOP_B || desc->guide_part > TGHIP_DEVELOP_B)) { ctx->error = "tghip_nlmeans: image_part and guide_part are the mean or a half"; return TGHIP_E_INVALID; }
    int rc = tghip_wait(ctx);
    if (rc != TGHIP_OK && rc != TGHIP_E_ABORTED) return rc;
    if (!pointers && (!ctx->haveScene || !ctx->dAux)) { ctx->error = "tghip_nlmeans: no auxiliary output buffers yet (no TGHIP_PASS_AUX pass, no tghip_upload_aux)"; return TGHIP_E_INVALID; }
    if (!pointers && (desc->width != uint32_t(ctx->width) || desc->height != uint32_t(ctx->height))) { ctx->error = "tghip_nlmeans: an aux source has the frame's size"; return TGHIP_E_INVALID; }
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    const uintptr_t align = channels == 4 ? 15u : 3u;
    if (device) {
        const uintptr_t all = reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(guide) | reinterpret_cast<uintptr_t>(variance) | reinterpret_cast<uintptr_t>(out);
        if (all & align) { ctx->error = "tghip_nlmeans: device arrays must be aligned (to 16 bytes with four channels, to 4 otherwise)"; return TGHIP_E_INVALID; }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t npixels = size_t(desc->width)*desc->height, nfloats = npixels*channels, nbytes = nfloats*sizeof(float);
    // scratch planes 0..2: image, guide, variance (uploaded, or developed from the aux buffers); 3: the result of a call with host memory
    const float *in[3] = {image, guide, variance};
    float *result = nullptr;
    for (int b = 0; b < 3; ++b) {
        if (pointers) rc = stageInput(ctx, device, in[b], nbytes, ctx->nlmBuf[b], in[b]);
        else { rc = ctx->nlmBuf[b].grow(ctx, nfloats); in[b] = ctx->nlmBuf[b].get(); }   // (developed below)
        if (rc != TGHIP_OK) return rc;
    }
    if ((rc = stageOutput(ctx, device, out, nbytes, ctx->nlmBuf[3], result)) != TGHIP_OK) return rc;
    return timedLaunches(ctx, ctx->nlmMs, [&]() -> int {
        if (!pointers) {
            HIP_TRY(ctx, ctx->developMax.once(16));
            const uint32_t parts[3] = {desc->image_part, desc->guide_part, TGHIP_DEVELOP_VARIANCE};
            for (int b = 0; b < 3; ++b)
                HIP_TRY(ctx, developLaunchAux(ctx->stream, ctx->dAux.get(), npixels, desc->source, parts[b], ctx->nlmBuf[b].get(), nullptr, ctx->developMax.get()));
        }
        HIP_TRY(ctx, nlMeansLaunch(ctx->stream, in[0], in[1], in[2], result, desc->width, desc->height, channels, desc->F, desc->R, desc->k,
                                   desc->variance_scale, ctx->nlmBatch));
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, out, result, nbytes); });
}

int tghip_nlmeans_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::nlmMs, ms); }

// the libm restatements exactly as the shading kernels call them (pt_math.h)
__global__ void k_debug_libm(int fn, const float *x, float *y, uint32_t n)
{
    const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool two = fn == TGHIP_LIBM_ATAN2F || fn == TGHIP_LIBM_POWF;
    const float v = two ? x[2u*i] : x[i], v2 = two ? x[2u*i + 1u] : 0.0f;
    float s, c, r;
    switch (fn) {
    case TGHIP_LIBM_ATAN2F: r = atan2fH(v, v2); break;
    case TGHIP_LIBM_POWF: r = powfH(v, v2); break;
    case TGHIP_LIBM_CBRTF: r = cbrtfH(v); break;
    case TGHIP_LIBM_EMBREE_RCP: r = embreeRcp(v); break;
    case TGHIP_LIBM_RCPPS: r = rcppsIntel(v); break;
    case TGHIP_LIBM_TANF: r = tanfH(v); break;
    case TGHIP_LIBM_SINF: r = sinfH(v); break;
    case TGHIP_LIBM_COSF: r = cosfH(v); break;
    case TGHIP_LIBM_LOGF: r = logfH(v); break;
    case TGHIP_LIBM_EXPF: r = expfH(v); break;
    case TGHIP_LIBM_SINCOS_SIN: sincosfH(v, s, c); r = s; break;
    case TGHIP_LIBM_SINCOS_COS: sincosfH(v, s, c); r = c; break;
    case TGHIP_LIBM_SINHF: r = sinhfH(v); break;
    default: r = acosfExact(v); break;
    }
    y[i] = r;
}

// ... and the double-precision ones of the atmospheric medium (pt_libm.h: expD / logD / erfD; pt_scene.h: sqrtD)
__global__ void k_debug_libmd(int fn, const double *x, double *y, uint32_t n)
{
    const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    y[i] = fn == TGHIP_LIBM_EXPD ? ptlibm::expD(v) : fn == TGHIP_LIBM_LOGD ? ptlibm::logD(v) : fn == TGHIP_LIBM_ERFD ? ptlibm::erfD(v) : sqrtD(v);
}

int tghip_debug_libm(tghip_ctx *ctx, int fn, const float *x, float *y, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (n == 0) return TGHIP_OK;
    if (!x || !y || n > 0x3FFFFFFFu || fn < TGHIP_LIBM_SINF || fn > TGHIP_LIBM_SINHF) { ctx->error = "invalid libm self-test arguments"; return TGHIP_E_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceArray<float> dx, dy;
    const bool dbl = fn >= TGHIP_LIBM_EXPD && fn <= TGHIP_LIBM_SQRTD;   // n doubles in, n doubles out
    const size_t nx = (fn == TGHIP_LIBM_ATAN2F || fn == TGHIP_LIBM_POWF || dbl) ? 2*n : n, ny = dbl ? 2*n : n;
    HIP_TRY(ctx, dx.once(nx));
    hipError_t e = dy.once(ny);
    if (e == hipSuccess) e = hipMemcpyAsync(dx.get(), x, nx*sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        if (dbl) hipLaunchKernelGGL(k_debug_libmd, dim3(uint32_t((n + 255)/256)), dim3(256), 0, ctx->stream, fn, reinterpret_cast<const double *>(dx.get()), reinterpret_cast<double *>(dy.get()), uint32_t(n));
        else     hipLaunchKernelGGL(k_debug_libm, dim3(uint32_t((n + 255)/256)), dim3(256), 0, ctx->stream, fn, static_cast<const float *>(dx.get()), dy.get(), uint32_t(n));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(y, dy.get(), ny*sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->error = hipGetErrorString(e); return TGHIP_E_HIP; }
    return TGHIP_OK;
}

// the BSDF wrappers exactly as the shading kernels call them, per shading family (debug_units.hip)
int tghip_debug_bsdf(tghip_ctx *ctx, const TgHipBsdfCase *cases, TgHipBsdfResult *results, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (n == 0) return TGHIP_OK;
    if (!cases || !results || n > 0x3FFFFFFFu) { ctx->error = "invalid bsdf self-test arguments"; return TGHIP_E_INVALID; }
    if (!ctx->haveScene) { ctx->error = "bsdf self-test without an uploaded scene"; return TGHIP_E_INVALID; }
    uint32_t variants = 0;
    for (size_t i = 0; i < n; ++i) {
        if (cases[i].bsdf < 0 || uint32_t(cases[i].bsdf) >= ctx->scene.num_bsdfs) { ctx->error = "bsdf self-test: bsdf index outside the scene's table"; return TGHIP_E_INVALID; }
        if (cases[i].variant >= TGHIP_BSDF_VARIANT_COUNT) { ctx->error = "bsdf self-test: unknown variant"; return TGHIP_E_INVALID; }
        variants |= 1u << cases[i].variant;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    DeviceArray<TgHipBsdfCase> dc;
    DeviceArray<TgHipBsdfResult> dr;
    HIP_TRY(ctx, dc.once(n));
    hipError_t e = dr.once(n);
    if (e == hipSuccess) e = hipMemcpyAsync(dc.get(), cases, n*sizeof(TgHipBsdfCase), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(dr.get(), 0, n*sizeof(TgHipBsdfResult), ctx->stream);
    if (e == hipSuccess) e = debugBsdfLaunch(ctx->stream, ctx->scene, dc.get(), dr.get(), uint32_t(n), variants);
    if (e == hipSuccess) e = hipMemcpyAsync(results, dr.get(), n*sizeof(TgHipBsdfResult), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->error = hipGetErrorString(e); return TGHIP_E_HIP; }
    return TGHIP_OK;
}

int tghip_debug_bsdf_info(tghip_ctx *ctx, int variant, uint32_t *type_mask, uint32_t *forward, uint32_t *covered, uint32_t *variant_mask)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!ctx->haveScene) { ctx->error = "bsdf self-test without an uploaded scene"; return TGHIP_E_INVALID; }
    if (variant < 0 || variant >= TGHIP_BSDF_VARIANT_COUNT) { ctx->error = "bsdf self-test: unknown variant"; return TGHIP_E_INVALID; }
    if (variant_mask) *variant_mask = familyMask(uint32_t(variant));
    for (size_t i = 0; i < ctx->sc.bsdfTypes.size(); ++i) {
        if (type_mask) type_mask[i] = ctx->sc.bsdfTypes[i];
        if (forward) forward[i] = ctx->sc.bsdfForward[i];
        if (covered) covered[i] = familyCovers(uint32_t(variant), ctx->sc.bsdfTypes[i], ctx->sc.bsdfForward[i] != 0) ? 1u : 0u;
    }
    return TGHIP_OK;
}

// the light functions exactly as the shading kernels' next-event estimation calls them, per shading family (debug_units.hip)
int tghip_debug_light(tghip_ctx *ctx, const TgHipLightCase *cases, TgHipLightResult *results, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (n == 0) return TGHIP_OK;
    if (!cases || !results || n > 0x3FFFFFFFu) { ctx->error = "invalid light self-test arguments"; return TGHIP_E_INVALID; }
    if (!ctx->haveScene) { ctx->error = "light self-test without an uploaded scene"; return TGHIP_E_INVALID; }
    uint32_t variants = 0;
    for (size_t i = 0; i < n; ++i) {
        if (cases[i].light < 0 || uint32_t(cases[i].light) >= ctx->scene.num_lights) { ctx->error = "light self-test: light slot outside the scene's table"; return TGHIP_E_INVALID; }
        if (cases[i].variant >= TGHIP_BSDF_VARIANT_COUNT) { ctx->error = "light self-test: unknown variant"; return TGHIP_E_INVALID; }
        variants |= 1u << cases[i].variant;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    DeviceArray<TgHipLightCase> dc;
    DeviceArray<TgHipLightResult> dr;
    HIP_TRY(ctx, dc.once(n));
    hipError_t e = dr.once(n);
    if (e == hipSuccess) e = hipMemcpyAsync(dc.get(), cases, n*sizeof(TgHipLightCase), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(dr.get(), 0, n*sizeof(TgHipLightResult), ctx->stream);
    if (e == hipSuccess) e = debugLightLaunch(ctx->stream, ctx->scene, dc.get(), dr.get(), uint32_t(n), variants);
    if (e == hipSuccess) e = hipMemcpyAsync(results, dr.get(), n*sizeof(TgHipLightResult), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->error = hipGetErrorString(e); return TGHIP_E_HIP; }
    return TGHIP_OK;
}

int tghip_debug_light_info(tghip_ctx *ctx, int variant, uint32_t *needs, uint32_t *covered, uint32_t *variant_mask)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!ctx->haveScene) { ctx->error = "light self-test without an uploaded scene"; return TGHIP_E_INVALID; }
    if (variant < 0 || variant >= TGHIP_BSDF_VARIANT_COUNT) { ctx->error = "light self-test: unknown variant"; return TGHIP_E_INVALID; }
    const uint32_t mask = familyMask(uint32_t(variant));
    if (variant_mask) *variant_mask = mask;
    for (size_t i = 0; i < ctx->sc.lightNeeds.size(); ++i) {
        if (needs) needs[i] = ctx->sc.lightNeeds[i];
        if (covered) covered[i] = (ctx->sc.lightNeeds[i] & ~mask) == 0u ? 1u : 0u;
    }
    return TGHIP_OK;
}

// the medium functions exactly as k_shade and the shadow walks call them, for the two families that carry them (debug_units.hip); the refusals
// are csrc/host/SceneCheck.cpp's checkMediumCases, made before anything is launched
int tghip_debug_medium(tghip_ctx *ctx, const TgHipMediumCase *cases, TgHipMediumResult *results, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (n == 0) return TGHIP_OK;
    if (!ctx->haveScene) { ctx->error = "medium self-test without an uploaded scene"; return TGHIP_E_INVALID; }
    uint32_t variants = 0;
    const int rc = checkMediumCases(ctx->sc, cases, results, n, variants, ctx->error);
    if (rc != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    DeviceArray<TgHipMediumCase> dc;
    DeviceArray<TgHipMediumResult> dr;
    HIP_TRY(ctx, dc.once(n));
    hipError_t e = dr.once(n);
    if (e == hipSuccess) e = hipMemcpyAsync(dc.get(), cases, n*sizeof(TgHipMediumCase), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(dr.get(), 0, n*sizeof(TgHipMediumResult), ctx->stream);
    if (e == hipSuccess) e = debugMediumLaunch(ctx->stream, ctx->scene, dc.get(), dr.get(), uint32_t(n), variants);
    if (e == hipSuccess) e = hipMemcpyAsync(results, dr.get(), n*sizeof(TgHipMediumResult), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->error = hipGetErrorString(e); return TGHIP_E_HIP; }
    return TGHIP_OK;
}

int tghip_debug_launch_plan(tghip_ctx *ctx, const TgHipPassDesc *pass, TgHipLaunchPlan *out)
{
    if (!ctx || !pass || !out) return TGHIP_E_INVALID;
    if (!ctx->haveScene) { ctx->error = "launch plan without an uploaded scene"; return TGHIP_E_NOSCENE; }
    int rc = checkPass(*pass, ctx->width, ctx->height, ctx->scene.sobol != nullptr, ctx->error);
    if (rc != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassPlan passPlan;
    const PassPlanOptions planOpt = {uint64_t(std::max<long long>(ctx->maxItems, 256)), uint64_t(ctx->maxSlots), uint32_t(std::max(ctx->chunkSamples, 0))};
    if ((rc = planPass(*pass, ctx->width, ctx->height, planOpt, passPlan, ctx->error)) != TGHIP_OK) return rc;
    LaunchPlan lp;
    if ((rc = planLaunches(ctx, passKindOf(ctx->sc, pass->flags, passPlan.shortBatch, ctx->countTraversal), lp)) != TGHIP_OK) return rc;
    std::memset(out, 0, sizeof *out);
    exportLaunchChoice(lp.choice, &out->choice);
    out->threads_closest = lp.closest.threads; out->threads_shadow = lp.shadow.threads; out->threads_tail = lp.tail.threads;
    for (int i = 0; i < 3; ++i) out->threads_shade[i] = lp.thrShade[i];
    if (!lp.choice.fusedFlat) { out->lds_closest = uint32_t(lp.closest.lds); out->lds_shadow = uint32_t(lp.shadow.lds); }   // (fused flat lists launch no walk)
    out->lds_tail = uint32_t(lp.tail.lds);
    out->grid = uint32_t(ctx->prop.multiProcessorCount*std::max(lp.choice.blocksPerCu, 1)*std::max(ctx->gridRounds, 1));
    out->parts = (int(out->grid) < 2*lp.choice.parts || int(out->grid) % lp.choice.parts != 0) ? 1 : lp.choice.parts;
    out->tail_fits = lp.tailFits;
    return TGHIP_OK;
}

int tghip_trace_rays(tghip_ctx *ctx, const TgHipRay *rays, TgHipHit *hits, size_t n, int repeats, double *ms_per_launch)
{
    if (!ctx || !ctx->haveScene) return TGHIP_E_NOSCENE;
    if (n == 0) return TGHIP_OK;
    if (!rays || !hits || n > 0x7FFFFFFFu) { ctx->error = "invalid ray batch"; return TGHIP_E_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceArray<float4> rayMem, hitMem;          // (a ray is two float4, a hit one)
    HIP_TRY(ctx, rayMem.once(n*sizeof(TgHipRay)/sizeof(float4)));
    hipError_t e = hitMem.once(n*sizeof(TgHipHit)/sizeof(float4));
    if (e != hipSuccess) { ctx->error = hipGetErrorString(e); return TGHIP_E_HIP; }
    float4 *dRays = rayMem.get(), *dHits = hitMem.get();
    int rc = ensurePool(ctx, ctx->poolSlots ? ctx->pool.num_slots : 256);   // the traversal statistics live in the pool
    if (rc != TGHIP_OK) return rc;
    (void)hipMemcpyAsync(dRays, rays, n*sizeof(TgHipRay), hipMemcpyHostToDevice, ctx->stream);
    const int grid = int(std::min<size_t>(size_t(launchGrid(ctx)), (n + 255)/256));
    // the walk of the choice (csrc/host/LaunchChoice.cpp); the wide one keeps no queue in LDS, only its group stack
    const LaunchChoice &choice = ctx->lp.choice;
    KernelId kernel = choice.traceRays;
    const size_t lds = choice.rayWalk == LaunchChoice::RAYS_WIDE ? size_t(std::max(ctx->sc.wideDepth, 1))*256u*sizeof(uint2) : ldsBytes(ctx->sc, choice, LDS_TRACE, 256);
    const uint32_t count = uint32_t(n);
    repeats = std::max(repeats, 1);
    (void)hipEventRecord(ctx->evA, ctx->stream);
    for (int r = 0; r < repeats; ++r) {
        kernel.count = ctx->countTraversal && r == 0;
        launchKernel(ResolvedLaunch{walkKernelFn(kernel), 256, lds}, grid, ctx->stream, ctx->scene, dRays, dHits, count, ctx->pool.stats);
    }
    (void)hipEventRecord(ctx->evB, ctx->stream);
    (void)hipMemcpyAsync(hits, dHits, n*sizeof(TgHipHit), hipMemcpyDeviceToHost, ctx->stream);
    e = hipStreamSynchronize(ctx->stream);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ctx->evA, ctx->evB);
    if (e != hipSuccess) { ctx->error = hipGetErrorString(e); return TGHIP_E_HIP; }
    if (ms_per_launch) *ms_per_launch = double(ms)/repeats;
    return TGHIP_OK;
}

int tghip_query_rays(tghip_ctx *ctx, const TgHipRayQueryDesc *desc, const TgHipRay *rays, void *out, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    int rc = checkRayQuery(desc, rays, out, n, ctx->error);
    if (rc != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_rays", n)) != TGHIP_OK || n == 0) return rc;
    const bool occluded = desc->mode == TGHIP_QUERY_OCCLUDED, device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    const size_t outBytes = occluded ? n : n*sizeof(TgHipHit);
    const float4 *dRays = nullptr;
    float4 *dOut = nullptr;
    if ((rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->queryRays, dRays)) != TGHIP_OK) return rc;
    if ((rc = stageOutput(ctx, device, out, outBytes, ctx->queryOut, dOut)) != TGHIP_OK) return rc;
    const QueryWalk q = queryWalk(ctx);
    HIP_TRY(ctx, hipMemsetAsync(ctx->queryCounter.get(), 0, sizeof(uint32_t), ctx->stream));
    return timedLaunches(ctx, ctx->queryMs, [&]() -> int {
        HIP_TRY(ctx, rayQueryLaunch(ctx->stream, ctx->scene, q.walk, occluded, dRays, dOut, uint32_t(n), ctx->queryCounter.get(), q.blocks(n), q.refillAt, q.lds));
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, out, dOut, outBytes); });
}

int tghip_query_rays_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::queryMs, ms); }

int tghip_query_radiance(tghip_ctx *ctx, const TgHipRadianceQueryDesc *desc, const TgHipRay *rays, float *rgb_sum, uint32_t *count, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_query_radiance: no description"; return TGHIP_E_INVALID; }
    int rc = queryScene(ctx, "tghip_query_radiance");
    if (rc != TGHIP_OK) return rc;
    if ((rc = checkRadianceQuery(desc, rays, rgb_sum, count, n, ctx->scene.sobol != nullptr, ctx->error)) != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_radiance", n)) != TGHIP_OK || n == 0) return rc;
    // the pass over the virtual image (csrc/host/RadianceQuery.cpp).  Its work items hold ONE sample each, whatever "chunk_samples" says, and k_resolve
    // adds them to the ray's sum one by one (runPass: group 1): the order of the additions is part of the answer, not a matter of options.
    const RadianceQueryImage im = radianceQueryImage(n);
    const TgHipPassDesc pass = radianceQueryPass(*desc);
    const PassPlanOptions planOpt = {uint64_t(std::max<long long>(ctx->maxItems, 256)), uint64_t(ctx->maxSlots), 1u};
    PassPlan &plan = ctx->radPlan;
    if ((rc = planRadianceQuery(*desc, n, planOpt, plan, ctx->error)) != TGHIP_OK) return rc;
    // the scratch: the image's framebuffer (zero: k_resolve adds), its tile seeds, the rays when they are host memory
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    const size_t npix = size_t(im.width)*im.height;
    if ((rc = ctx->radSum.grow(ctx, npix*3)) != TGHIP_OK) return rc;
    if ((rc = ctx->radCount.grow(ctx, npix)) != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->radSum.get(), 0, npix*3*sizeof(float), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->radCount.get(), 0, npix*sizeof(uint32_t), ctx->stream));
    PassTarget target;
    target.sum = ctx->radSum.get(); target.count = ctx->radCount.get();
    target.rayPaths = true;
    target.numRays = uint32_t(n);
    if (pass.flags & TGHIP_PASS_SOBOL) {
        bool fresh = false;
        if ((rc = ctx->radTileSeeds.grow(ctx, size_t(plan.numTiles), &fresh)) != TGHIP_OK) return rc;
        if (fresh) ctx->radTileSeedsSet = 0;
        if (ctx->radTileSeedsSet < plan.numTiles || ctx->radTileSeed != desc->sobol_seed) {
            HIP_TRY(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->radTileSeeds.get()), int(desc->sobol_seed), size_t(plan.numTiles), ctx->stream));
            ctx->radTileSeedsSet = plan.numTiles; ctx->radTileSeed = desc->sobol_seed;
        }
        target.tileSeeds = ctx->radTileSeeds.get();
    }
    if ((rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->radRays, target.rays)) != TGHIP_OK) return rc;
    // what the pass borrows of the context and gets back: the launch plan of the last render pass's kind (so that the next one plans nothing anew).
    // An abort request left over from an earlier pass -- tghip_wait above has honoured it -- is cleared and NOT put back, as tghip_render_pass clears
    // it where a pass begins; an abort DURING the query ends the query like a pass (TGHIP_E_ABORTED) and stays set until the next pass or query.
    const LaunchPlan lpBefore = ctx->lp;
    const double msTotalBefore = ctx->counters.ms_total;
    ctx->abortRequested.store(false, std::memory_order_release);
    rc = runPass(ctx, pass, im.width, im.height, plan, target);
    ctx->lp = lpBefore;
    ctx->radMs = ctx->counters.ms_total - msTotalBefore;
    if (rc != TGHIP_OK) return rc;
    // the answers: a launch into the caller's device memory, whose time counts with the pass's, or copies of the image's first n pixels -- the n rays
    double msCopy = 0.0;
    rc = timedLaunches(ctx, msCopy, [&]() -> int {
        if (device) HIP_TRY(ctx, radianceQueryLaunchResults(ctx->stream, ctx->radSum.get(), ctx->radCount.get(), rgb_sum, count, uint32_t(n)));
        if (device) return TGHIP_OK;
        const int crc = copyBack(ctx, rgb_sum, ctx->radSum.get(), n*3*sizeof(float));
        return crc != TGHIP_OK ? crc : copyBack(ctx, count, ctx->radCount.get(), n*sizeof(uint32_t));
    }, []() { return TGHIP_OK; });
    if (rc == TGHIP_OK && device) ctx->radMs += msCopy;
    return rc;
}

int tghip_query_radiance_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::radMs, ms); }

int tghip_query_surface(tghip_ctx *ctx, const TgHipSurfaceQueryDesc *desc, const TgHipRay *rays, TgHipSurface *out, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    int rc = checkSurfaceQuery(desc, rays, out, n, ctx->error);
    if (rc != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_surface", n)) != TGHIP_OK || n == 0) return rc;
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    const size_t outBytes = n*sizeof(TgHipSurface);
    const float4 *dRays = nullptr;
    float4 *dOut = nullptr;
    if ((rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->queryRays, dRays)) != TGHIP_OK) return rc;
    if ((rc = stageOutput(ctx, device, out, outBytes, ctx->queryOut, dOut)) != TGHIP_OK) return rc;
    // what the walk leaves for the dense launch
    const QueryWalk q = queryWalk(ctx);
    if ((rc = ctx->surfHits.grow(ctx, n)) != TGHIP_OK) return rc;
    if (q.inst && (rc = ctx->surfInst.grow(ctx, n)) != TGHIP_OK) return rc;
    int *dInst = q.inst ? ctx->surfInst.get() : nullptr;
    HIP_TRY(ctx, hipMemsetAsync(ctx->queryCounter.get(), 0, sizeof(uint32_t), ctx->stream));
    rc = timedLaunches(ctx, ctx->surfMs, [&]() -> int {
        HIP_TRY(ctx, surfaceQueryLaunchWalk(ctx->stream, ctx->scene, q.walk, dRays, ctx->surfHits.get(), dInst, uint32_t(n), ctx->queryCounter.get(), q.blocks(n), q.refillAt, q.lds));
        HIP_TRY(ctx, hipEventRecord(ctx->evSurfMid, ctx->stream));
        HIP_TRY(ctx, surfaceQueryLaunchDescribe(ctx->stream, ctx->scene, dRays, ctx->surfHits.get(), dInst, dOut, uint32_t(n)));
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, out, dOut, outBytes); });
    if (rc != TGHIP_OK) return rc;
    float dense = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&dense, ctx->evSurfMid, ctx->evB));
    ctx->surfDenseMs = dense;
    return TGHIP_OK;
}

int tghip_query_surface_kernel_time(tghip_ctx *ctx, double *ms)
{
    return kernelTime(ctx, ctx && ctx->surfTimeDense ? &tghip_ctx::surfDenseMs : &tghip_ctx::surfMs, ms);
}

int tghip_query_transmittance(tghip_ctx *ctx, const TgHipTransmittanceQueryDesc *desc, const TgHipRay *rays, const int32_t *media, TgHipTransmittance *out, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_query_transmittance: no description"; return TGHIP_E_INVALID; }
    int rc = queryScene(ctx, "tghip_query_transmittance");
    if (rc != TGHIP_OK) return rc;
    const TgHostTransmittanceScene facts = {uint32_t(ctx->sc.mediumOperand.size()), ctx->sc.mediumOperand.data(), uint32_t(ctx->sc.objectType.size()), ctx->sc.objectType.data()};
    if ((rc = checkTransmittanceQuery(desc, rays, media, out, n, &facts, ctx->error)) != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_transmittance", n)) != TGHIP_OK || n == 0) return rc;
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0;
    const size_t outBytes = n*sizeof(TgHipTransmittance);
    const float4 *dRays = nullptr;
    const int *dMedia = nullptr;
    float4 *dOut = nullptr;
    if ((rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->queryRays, dRays)) != TGHIP_OK) return rc;
    if (media && (rc = stageInput(ctx, device, media, n*sizeof(int32_t), ctx->queryMedia, dMedia)) != TGHIP_OK) return rc;
    if ((rc = stageOutput(ctx, device, out, outBytes, ctx->queryOut, dOut)) != TGHIP_OK) return rc;
    const QueryWalk q = queryWalk(ctx);
    // the state between the rounds.  A scene without a forward-lobe BSDF ends every ray in round 0: nothing but the hits is ever stored.
    const bool oneRound = !ctx->sc.haveForwardBsdf;
    if ((rc = ctx->trHits.grow(ctx, n)) != TGHIP_OK) return rc;
    if (q.inst && (rc = ctx->trInst.grow(ctx, n)) != TGHIP_OK) return rc;
    if (!oneRound) {
        if ((rc = ctx->trO.grow(ctx, n)) != TGHIP_OK || (rc = ctx->trD.grow(ctx, n)) != TGHIP_OK || (rc = ctx->trT.grow(ctx, n)) != TGHIP_OK ||
            (rc = ctx->trB.grow(ctx, n)) != TGHIP_OK || (rc = ctx->trList[0].grow(ctx, n)) != TGHIP_OK || (rc = ctx->trList[1].grow(ctx, n)) != TGHIP_OK)
            return rc;
    }
    const TransmittanceState st = {ctx->trO.get(), ctx->trD.get(), ctx->trT.get(), ctx->trB.get(), ctx->trHits.get(), q.inst ? ctx->trInst.get() : nullptr};
    TransmittanceParams p;
    queryStartMedium(ctx, desc->medium, p);
    p.endCap = desc->end_cap;
    p.bounce = desc->bounce;
    p.startsOnSurface = (desc->flags & TGHIP_TRANSMITTANCE_STARTS_ON_SURFACE) ? 1u : 0u;
    p.endsOnSurface = (desc->flags & TGHIP_TRANSMITTANCE_ENDS_ON_SURFACE) ? 1u : 0u;
    // A ray that goes on has crossed a surface: bounce < max_bounces bounds the rounds whatever the rays do
    const long long maxRounds = oneRound ? 1 : std::max<long long>(1, (long long)ctx->scene.settings.max_bounces - (long long)desc->bounce);
    uint32_t *counters = ctx->queryCounter.get();
    ctx->trRounds = 0;
    return timedLaunches(ctx, ctx->trMs, [&]() -> int {
        uint32_t live = uint32_t(n);
        for (long long round = 0; round < maxRounds && live > 0; ++round) {
            const uint32_t *list = round == 0 ? nullptr : ctx->trList[(round - 1) & 1].get();
            uint32_t *next = ctx->trList[round & 1].get();
            HIP_TRY(ctx, hipMemsetAsync(counters, 0, 2*sizeof(uint32_t), ctx->stream));
            HIP_TRY(ctx, transmittanceQueryLaunchWalk(ctx->stream, ctx->scene, q.walk, dRays, st, list, live, counters, q.blocks(live), q.refillAt, q.lds));
            HIP_TRY(ctx, transmittanceQueryLaunchSegment(ctx->stream, ctx->scene, p, dRays, dMedia, st, list, live, dOut, next, counters + 1));
            ctx->trRounds++;
            if (oneRound) break;
            // the one word a round hands back: how many rays the next one has
            HIP_TRY(ctx, hipMemcpyAsync(&live, counters + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, out, dOut, outBytes); });
}

int tghip_query_transmittance_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::trMs, ms); }

int tghip_query_transmittance_rounds(tghip_ctx *ctx, uint32_t *rounds)
{
    if (!ctx || !rounds) return TGHIP_E_INVALID;
    *rounds = ctx->trRounds;
    return TGHIP_OK;
}

// (ray, sample) items of tghip_query_direct that are under way at once: what its scratch grows to at most (about 300 bytes an item); a larger call
// runs in parts, whole rays where a ray's samples fit and runs of one ray's samples where they do not.  A part changes no bit of an answer: a ray's
// samples are added in sample order, a later part going on from the sums the earlier ones stored.
#define DIRECT_QUERY_CHUNK (1u << 20)
// rounds of shadow walks per part, whatever the scene's max_bounces
#define DIRECT_QUERY_MAX_ROUNDS 257

// The scratch of `items` direct estimates under way at once (tghip_query_direct's items, tghip_query_vertex's live paths): st for the dense stages,
// walkState for the shadow walks -- tghip_query_transmittance's, reading segments through a list: of its state they touch o, d, hits and inst
static int directScratch(tghip_ctx *ctx, const QueryWalk &q, size_t items, DirectState &st, TransmittanceState &walkState)
{
    int rc;
    if ((rc = ctx->dqStatus.grow(ctx, items)) != TGHIP_OK || (rc = ctx->dqWeight.grow(ctx, items)) != TGHIP_OK || (rc = ctx->dqOrigin.grow(ctx, items)) != TGHIP_OK ||
        (rc = ctx->dqO.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqD.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqHits.grow(ctx, 2*items)) != TGHIP_OK ||
        (rc = ctx->dqT.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqB.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqC.grow(ctx, 2*items)) != TGHIP_OK ||
        (rc = ctx->dqE.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqRes.grow(ctx, 2*items)) != TGHIP_OK ||
        (rc = ctx->dqList[0].grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->dqList[1].grow(ctx, 2*items)) != TGHIP_OK)
        return rc;
    if (q.inst && (rc = ctx->dqInst.grow(ctx, 2*items)) != TGHIP_OK) return rc;
    st = {ctx->dqStatus.get(), ctx->dqWeight.get(), ctx->dqOrigin.get(), ctx->dqO.get(), ctx->dqD.get(), ctx->dqHits.get(),
          q.inst ? ctx->dqInst.get() : nullptr, ctx->dqT.get(), ctx->dqB.get(), ctx->dqC.get(), ctx->dqE.get(), ctx->dqRes.get()};
    walkState = {st.o, st.d, nullptr, nullptr, st.hits, st.inst};
    return TGHIP_OK;
}

// The shadow rounds of the `live` segments a setup or front stage left in dqList[1]: per round the walk, k_direct_round and the one word it hands back,
// how many segments the next one has.  A segment that goes on has crossed a surface (bounce++) and bounce >= max_bounces ends it: bounded.  fn: the caller.
static int directShadowRounds(tghip_ctx *ctx, const char *fn, const QueryWalk &q, const DirectState &st, const TransmittanceState &walkState, uint32_t live)
{
    uint32_t *counters = ctx->queryCounter.get();
    for (int round = 0; live > 0; ++round) {
        if (round >= DIRECT_QUERY_MAX_ROUNDS) { ctx->error = std::string(fn) + ": shadow rays still under way after 257 rounds"; return TGHIP_E_UNSUPPORTED; }
        const uint32_t *list = ctx->dqList[(round + 1) & 1].get();
        uint32_t *next = ctx->dqList[round & 1].get();
        HIP_TRY(ctx, hipMemsetAsync(counters, 0, 2*sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, transmittanceQueryLaunchWalk(ctx->stream, ctx->scene, q.walk, nullptr, walkState, list, live, counters, q.blocks(live), q.refillAt, q.lds));
        HIP_TRY(ctx, directQueryLaunchRound(ctx->stream, ctx->scene, st, list, live, next, counters + 1));
        HIP_TRY(ctx, hipMemcpyAsync(&live, counters + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return TGHIP_OK;
}

int tghip_query_direct(tghip_ctx *ctx, const TgHipDirectQueryDesc *desc, const TgHipRay *rays, const int32_t *media, TgHipDirect *out, size_t n)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_query_direct: no description"; return TGHIP_E_INVALID; }
    int rc = queryScene(ctx, "tghip_query_direct");
    if (rc != TGHIP_OK) return rc;
    const TgHostDirectScene facts = {uint32_t(ctx->sc.mediumOperand.size()), ctx->sc.mediumOperand.data(), ctx->scene.num_lights, ctx->sc.cameraMedium};
    if ((rc = checkDirectQuery(desc, rays, media, out, n, &facts, ctx->error)) != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_direct", n)) != TGHIP_OK || n == 0) return rc;
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0, volume = (desc->flags & TGHIP_DIRECT_VOLUME) != 0;
    const size_t outBytes = n*sizeof(TgHipDirect);
    const float4 *dRays = nullptr;
    const int *dMedia = nullptr;
    float4 *dOut = nullptr;
    if ((rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->queryRays, dRays)) != TGHIP_OK) return rc;
    if (media && (rc = stageInput(ctx, device, media, n*sizeof(int32_t), ctx->queryMedia, dMedia)) != TGHIP_OK) return rc;
    if ((rc = stageOutput(ctx, device, out, outBytes, ctx->queryOut, dOut)) != TGHIP_OK) return rc;
    const QueryWalk q = queryWalk(ctx);
    // the parts: raysPer rays by samplesPer samples, at most DIRECT_QUERY_CHUNK items
    const uint64_t spp = uint64_t(desc->spp_end) - desc->spp_begin;
    const uint64_t samplesPer = std::min<uint64_t>(spp, DIRECT_QUERY_CHUNK);
    const uint64_t raysPer = std::min<uint64_t>(n, std::max<uint64_t>(1, DIRECT_QUERY_CHUNK/samplesPer));
    DirectState st;
    TransmittanceState walkState;
    if ((rc = directScratch(ctx, q, size_t(raysPer*samplesPer), st, walkState)) != TGHIP_OK) return rc;
    if (!volume && (rc = ctx->dqRayHits.grow(ctx, size_t(raysPer))) != TGHIP_OK) return rc;
    if (!volume && q.inst && (rc = ctx->dqRayInst.grow(ctx, size_t(raysPer))) != TGHIP_OK) return rc;
    const float4 *rayHits = volume ? nullptr : ctx->dqRayHits.get();
    int *rayInst = !volume && q.inst ? ctx->dqRayInst.get() : nullptr;
    DirectParams p;
    p.seed = desc->seed; p.skip = desc->skip; p.bounce = desc->bounce; p.light = desc->light;
    queryStartMedium(ctx, desc->medium, p);
    uint32_t *counters = ctx->queryCounter.get();
    return timedLaunches(ctx, ctx->dqMs, [&]() -> int {
        for (uint64_t r0 = 0; r0 < n; r0 += raysPer) {
            for (uint64_t s0 = desc->spp_begin; s0 < desc->spp_end; s0 += samplesPer) {
                p.ray0 = uint32_t(r0); p.rays = uint32_t(std::min<uint64_t>(raysPer, n - r0));
                p.sample0 = uint32_t(s0); p.samples = uint32_t(std::min<uint64_t>(samplesPer, desc->spp_end - s0));
                p.first = s0 == desc->spp_begin ? 1u : 0u;
                HIP_TRY(ctx, hipMemsetAsync(counters, 0, 2*sizeof(uint32_t), ctx->stream));
                if (!volume && p.first)      // the point: tghip_query_surface's walk as it is (the hits stay for the ray's later parts)
                    HIP_TRY(ctx, surfaceQueryLaunchWalk(ctx->stream, ctx->scene, q.walk, dRays + r0*2u, ctx->dqRayHits.get(), rayInst, p.rays, counters, q.blocks(p.rays), q.refillAt, q.lds));
                HIP_TRY(ctx, directQueryLaunchSetup(ctx->stream, ctx->scene, p, volume, dRays, dMedia, rayHits, rayInst, st, ctx->dqList[1].get(), counters + 1));
                uint32_t live = 0;
                HIP_TRY(ctx, hipMemcpyAsync(&live, counters + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                if ((rc = directShadowRounds(ctx, "tghip_query_direct", q, st, walkState, live)) != TGHIP_OK) return rc;
                HIP_TRY(ctx, directQueryLaunchFinish(ctx->stream, p, volume, dMedia, ctx->scene.num_media, rayHits, st, dOut));
            }
        }
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, out, dOut, outBytes); });
}

int tghip_query_direct_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::dqMs, ms); }

// Paths of tghip_query_vertex that are under way at once: what its scratch grows to at most; a larger call runs in parts, each through all its turns.
// A part changes no bit of an answer: a path's turn reads nothing but its own state and the scene.  The shadow segments use tghip_query_direct's
// scratch, one item per live path.
#define VERTEX_QUERY_CHUNK (1u << 20)

int tghip_query_vertex(tghip_ctx *ctx, const TgHipVertexQueryDesc *desc, const TgHipRay *rays, const int32_t *media, TgHipPath *paths, size_t n, uint32_t *alive)
{
    if (!ctx) return TGHIP_E_INVALID;
    if (!desc) { ctx->error = "tghip_query_vertex: no description"; return TGHIP_E_INVALID; }
    int rc = queryScene(ctx, "tghip_query_vertex");
    if (rc != TGHIP_OK) return rc;
    const TgHostVertexScene facts = {uint32_t(ctx->sc.mediumOperand.size()), ctx->sc.mediumOperand.data()};
    if ((rc = checkVertexQuery(desc, rays, media, paths, alive, n, &facts, ctx->error)) != TGHIP_OK) return rc;
    if ((rc = queryBegin(ctx, "tghip_query_vertex", n)) != TGHIP_OK) return rc;
    const bool device = (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0, start = (desc->flags & TGHIP_VERTEX_START) != 0;
    // *alive, where it is asked for: device memory, or a host word (see the header)
    auto putAlive = [&](uint32_t count) -> int {
        if (alive && device) HIP_TRY(ctx, hipMemcpy(alive, &count, sizeof count, hipMemcpyDefault));
        else if (alive) *alive = count;
        return TGHIP_OK;
    };
    if (n == 0) return putAlive(0);
    const size_t pathBytes = n*sizeof(TgHipPath);
    const float4 *dRays = nullptr;
    const int *dMedia = nullptr;
    float4 *dPaths = nullptr;
    if (start && (rc = stageInput(ctx, device, rays, n*sizeof(TgHipRay), ctx->queryRays, dRays)) != TGHIP_OK) return rc;
    if (start && media && (rc = stageInput(ctx, device, media, n*sizeof(int32_t), ctx->queryMedia, dMedia)) != TGHIP_OK) return rc;
    if (start || device) {
        if ((rc = stageOutput(ctx, device, paths, pathBytes, ctx->vqPaths, dPaths)) != TGHIP_OK) return rc;
    } else {
        const float4 *staged = nullptr;
        if ((rc = stageInput(ctx, false, paths, pathBytes, ctx->vqPaths, staged)) != TGHIP_OK) return rc;
        dPaths = ctx->vqPaths.get();
    }
    const QueryWalk q = queryWalk(ctx);
    const size_t items = std::min<size_t>(n, VERTEX_QUERY_CHUNK);
    DirectState st;
    TransmittanceState walkState;
    if ((rc = directScratch(ctx, q, items, st, walkState)) != TGHIP_OK ||
        (rc = ctx->vqWalkRays.grow(ctx, 2*items)) != TGHIP_OK || (rc = ctx->vqHits.grow(ctx, items)) != TGHIP_OK || (rc = ctx->vqW.grow(ctx, items)) != TGHIP_OK ||
        (rc = ctx->vqP.grow(ctx, items)) != TGHIP_OK || (rc = ctx->vqList[0].grow(ctx, items)) != TGHIP_OK || (rc = ctx->vqList[1].grow(ctx, items)) != TGHIP_OK)
        return rc;
    if (q.inst && (rc = ctx->vqInst.grow(ctx, items)) != TGHIP_OK) return rc;
    const VertexState vs = {ctx->vqW.get(), ctx->vqP.get()};
    int *pathInst = q.inst ? ctx->vqInst.get() : nullptr;
    VertexParams p;
    p.seed = desc->seed; p.sample = desc->sample; p.firstIndex = desc->first_index; p.firstNumber = desc->first_number;
    p.start = start ? 1u : 0u;
    queryStartMedium(ctx, desc->medium, p);
    uint32_t *counters = ctx->queryCounter.get();
    uint32_t aliveTotal = 0;
    rc = timedLaunches(ctx, ctx->vqMs, [&]() -> int {
        for (size_t p0 = 0; p0 < n; p0 += VERTEX_QUERY_CHUNK) {
            p.path0 = uint32_t(p0); p.paths = uint32_t(std::min<size_t>(VERTEX_QUERY_CHUNK, n - p0));
            HIP_TRY(ctx, hipMemsetAsync(counters, 0, 3*sizeof(uint32_t), ctx->stream));
            HIP_TRY(ctx, vertexQueryLaunchBegin(ctx->stream, p, ctx->scene.num_media, dRays, dMedia, dPaths, ctx->vqList[0].get(), ctx->vqWalkRays.get(), counters + 2));
            uint32_t live = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&live, counters + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            for (uint32_t turn = 0; turn < desc->turns && live > 0; ++turn) {
                const uint32_t *list = ctx->vqList[turn & 1].get();
                uint32_t *next = ctx->vqList[(turn + 1) & 1].get();
                HIP_TRY(ctx, hipMemsetAsync(counters, 0, 3*sizeof(uint32_t), ctx->stream));
                // the closest hit: tghip_query_surface's walk as it is, over the live paths' rays
                HIP_TRY(ctx, surfaceQueryLaunchWalk(ctx->stream, ctx->scene, q.walk, ctx->vqWalkRays.get(), ctx->vqHits.get(), pathInst, live, counters, q.blocks(live), q.refillAt, q.lds));
                HIP_TRY(ctx, vertexQueryLaunchFront(ctx->stream, ctx->scene, dPaths, list, live, ctx->vqHits.get(), pathInst, st, vs, ctx->dqList[1].get(), counters + 1));
                uint32_t segments = 0;
                HIP_TRY(ctx, hipMemcpyAsync(&segments, counters + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                if ((rc = directShadowRounds(ctx, "tghip_query_vertex", q, st, walkState, segments)) != TGHIP_OK) return rc;   // tghip_query_direct's, as they are
                HIP_TRY(ctx, vertexQueryLaunchBack(ctx->stream, dPaths, list, live, st, vs, next, ctx->vqWalkRays.get(), counters + 2));
                // the one word a turn hands back: how many paths the next one has
                HIP_TRY(ctx, hipMemcpyAsync(&live, counters + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            }
            aliveTotal += live;
        }
        return TGHIP_OK;
    }, [&]() { return copyBack(ctx, paths, dPaths, pathBytes); });
    return rc != TGHIP_OK ? rc : putAlive(aliveTotal);
}

int tghip_query_vertex_kernel_time(tghip_ctx *ctx, double *ms) { return kernelTime(ctx, &tghip_ctx::vqMs, ms); }

int tghip_get_counters(tghip_ctx *ctx, TgHipCounters *out)
{
    if (!ctx || !out) return TGHIP_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = foldCounters(ctx);
    if (rc != TGHIP_OK) return rc;
    *out = ctx->counters;
    return TGHIP_OK;
}

int tghip_reset_counters(tghip_ctx *ctx)
{
    if (!ctx) return TGHIP_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = foldCounters(ctx);
    if (rc != TGHIP_OK) return rc;
    std::memset(&ctx->counters, 0, sizeof(ctx->counters));
    std::memset(ctx->walkStats, 0, sizeof(ctx->walkStats));
    return TGHIP_OK;
}

int tghip_get_walk_stats(tghip_ctx *ctx, int walk, uint64_t *out, int n)
{
    if (!ctx || !out || walk < 0 || walk > 1 || n < 0) return TGHIP_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = foldCounters(ctx);
    if (rc != TGHIP_OK) return rc;
    const int m = std::min(n, int(PT_WALK_STATS));
    for (int i = 0; i < m; ++i) out[i] = ctx->walkStats[walk][i];
    return m;
}

} // extern "C"
