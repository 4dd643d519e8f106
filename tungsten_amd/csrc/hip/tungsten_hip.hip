// path_tracer_hip: the kernels' unit -- the tracer's non-template kernels, the walks walkKernelFn names -- and the core of the extern "C" shim of
// include/tungsten_hip.h: context, options, upload, launch plan, render pass, tghip_trace_rays, counters.  The entry points that launch none of these kernels
// are host-only units (shim_queries.hip, shim_images.hip, shim_debug.hip, reduce.hip; shared: shim_context.h).  gfx950 (MI355X) only; pt_kernels.h: the execution model, DESIGN.md: the layout.
#define PT_WAVEFRONT_MAIN
#include "pt_wavefront.h"
#include "pt_instances.h"
#include "shim_context.h"
#include "denoise.h"          // NLMEANS_MAX_BATCH ("nlmeans_batch")
#include "radiance_query.h"   // the ray source and the clip of a query's pass (runBatch)

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
            int prio[TGHIP_MAX_PARTS] = {};
            bool withPrio = false;
            if (const char *env = std::getenv("TGHIP_STREAM_PRIORITIES")) {
                withPrio = true;
                int k = 0;
                for (const char *c = env; *c && k < TGHIP_MAX_PARTS; ) {
                    prio[k++] = int(std::strtol(c, const_cast<char **>(&c), 10));
                    while (*c == ',' || *c == ' ') ++c;
                }
            }
            auto create = [&](hipStream_t *st, int p) { return withPrio ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, p) : hipStreamCreateWithFlags(st, hipStreamNonBlocking); };
            if (e == hipSuccess) e = create(&set.main, prio[0]);
            for (int k = 0; k < TGHIP_MAX_PARTS - 1; ++k)
                if (e == hipSuccess) e = create(&set.part[k], prio[k + 1]);
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&set.abort, hipStreamNonBlocking);
        }
        ctx->stream = set.main;
        for (int k = 0; k < TGHIP_MAX_PARTS - 1; ++k) ctx->partStream[k] = set.part[k];
        ctx->abortStream = set.abort;
    }
    for (int k = 0; k < TGHIP_MAX_PARTS - 1; ++k)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->evPart[k], hipEventDisableTiming);
    for (int k = 0; k < TGHIP_MAX_PARTS; ++k) {
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->evFork[k], hipEventDisableTiming);
        for (int a = 0; a < 2; ++a)
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->evJoin[k][a], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->evMain, hipEventDisableTiming);
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
    for (int k = 0; k < TGHIP_MAX_PARTS - 1; ++k) if (ctx->partStream[k]) (void)hipStreamSynchronize(ctx->partStream[k]);
    for (int k = 0; k < TGHIP_MAX_PARTS; ++k)
        for (int a = 0; a < 2; ++a) if (ctx->classStream[k][a]) (void)hipStreamSynchronize(ctx->classStream[k][a]);
    if (ctx->abortStream) (void)hipStreamSynchronize(ctx->abortStream);
    if (ctx->rankComm) tghipDestroyRankComm(ctx->rankComm);
    if (ctx->evA) (void)hipEventDestroy(ctx->evA);
    if (ctx->evB) (void)hipEventDestroy(ctx->evB);
    if (ctx->evSurfMid) (void)hipEventDestroy(ctx->evSurfMid);
    for (hipEvent_t e : ctx->evPool) (void)hipEventDestroy(e);
    for (int k = 0; k < TGHIP_MAX_PARTS - 1; ++k) if (ctx->evPart[k]) (void)hipEventDestroy(ctx->evPart[k]);
    if (ctx->evMain) (void)hipEventDestroy(ctx->evMain);
    for (int k = 0; k < TGHIP_MAX_PARTS; ++k) {
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
        for (int k = 0; k < TGHIP_MAX_PARTS - 1; ++k) { set.part[k] = ctx->partStream[k]; complete = complete && set.part[k] != nullptr; }
        if (complete) {
            std::lock_guard<std::mutex> lock(g_streamMutex);
            g_freeStreams[ctx->device].push_back(set);
        } else {                                 // (a context whose creation failed half way)
            if (set.main) (void)hipStreamDestroy(set.main);
            if (set.abort) (void)hipStreamDestroy(set.abort);
            for (int k = 0; k < TGHIP_MAX_PARTS - 1; ++k) if (set.part[k]) (void)hipStreamDestroy(set.part[k]);
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
        for (int kk = 0; kk < TGHIP_MAX_PARTS && k == "class_streams" && value != 0; ++kk)     // (created when the option is first switched on: an experiment's streams)
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

// ---- One batch of the wavefront loop (runBatch): its path state, its parts, start, host check, k_tail, a round of iterations, resolve ----
namespace {
// A part of a batch: a run of the pool's workgroups with their slots, queues and work items, and the stream its launches go to
struct BatchPart { PathState st; PassParams pp; hipStream_t stream; int grid; int index; };
// what a timing bracket measures: TgHipCounters has milliseconds and launches of each
enum TimedClass { TIMED_CLOSEST, TIMED_SHADE, TIMED_SHADOW, TIMED_CLASSES };
// The batch's path state: the pool, with what the context's options and the pass's launch choice say about the walks
PathState batchState(const tghip_ctx *ctx)
{
    const LaunchChoice &choice = ctx->lp.choice;
    PathState st = ctx->pool;
    st.partial = ctx->partial.get();
    st.abort_flag = ctx->abortFlagDev.get();
    st.leaf_batch = uint32_t(ctx->leafBatch);
    st.inst_tree_depth = uint32_t(choice.instTreeDepth);
    st.inst_phase_min = uint32_t(ctx->instPhaseMin);
    st.inst_refill_at = uint32_t(ctx->instRefillAt);
    st.nee_factors = choice.neeFactors ? 1u : 0u;   // the closest-hit shadow walk, k_trace_shadow<., FORWARD>
    st.suspend_lanes = ctx->poolWalkArrays ? uint32_t(ctx->suspendLanes) : 0u;
    st.suspend_turns = uint32_t(std::max(ctx->suspendTurns, 1));
    st.suspend_min_queue = uint32_t(ctx->suspendMinQueue);
    st.leaf_batch_bvh2 = uint32_t(ctx->leafBatchBvh2 > 0 ? ctx->leafBatchBvh2 : ctx->sc.haveInstances ? 16 : ctx->leafBatch);
    return st;
}

// "streams" = N > 1: the workgroups (and with them the slots, queues and work items) are split into N parts that run the same
// wavefront loop on N streams: kernels of different parts share the CUs (csrc/host/LaunchChoice.cpp), and the drain tail of one part's kernel
// overlaps the other parts' kernels.  A grid or a batch too small for the parts wanted is ONE part: the whole pool on the context's stream.
std::vector<BatchPart> splitBatch(const tghip_ctx *ctx, const PathState &st, const PassParams &pp)
{
    const int grid = int(ctx->poolGrid);
    int parts = ctx->lp.choice.parts;
    if (grid < 2*parts || grid % parts != 0 || pp.total_items < uint32_t(2*parts)*PT_ITEM_GROUP)
        parts = 1;
    const uint32_t groups = (pp.total_items + PT_ITEM_GROUP - 1)/PT_ITEM_GROUP;
    uint32_t itemBegin = 0;
    std::vector<BatchPart> part;
    part.reserve(size_t(parts));
    for (int k = 0; k < parts; ++k) {
        BatchPart p{st, pp, ctx->streamOfPart(k), grid/parts, k};
        const uint32_t off = uint32_t(p.grid)*uint32_t(k);
        for (uint32_t g = 0; g < PT_POOL_GROUPS; ++g)
            p.st.poolg[g] = st.poolg[g] + size_t(off)*st.slots_per_block*16u;
        p.st.bm = st.bm + size_t(off)*(st.slots_per_block >> 5);
        p.st.ctl = st.ctl + off;
        p.st.stats = st.stats + off;
        p.st.num_slots = st.num_slots/uint32_t(parts);
        const uint32_t itemEnd = k + 1 == parts ? pp.total_items : std::min(pp.total_items, uint32_t((uint64_t(groups)*(k + 1) + parts - 1)/parts)*PT_ITEM_GROUP);
        p.pp.item_begin = pp.item_begin + itemBegin;
        p.pp.total_items = itemEnd - itemBegin;
        itemBegin = itemEnd;
        part.push_back(p);
    }
    return part;
}

struct Batch {
    enum Outcome { DONE, TAIL, GO_ON };          // what a host check finds: every queue empty, few enough paths for k_tail, neither
    tghip_ctx *const ctx;
    const PassParams &pp;                        // the whole batch's (the parts hold their shares)
    const PassTarget &target;
    const LaunchPlan &lp;                        // (tghipRunPass planned the pass's kind)
    const LaunchChoice &choice;
    const DeviceScene &s;
    const PathState st;                          // the whole pool
    const int checkInterval;                     // iterations between two host checks
    std::vector<BatchPart> part;                 // at most TGHIP_MAX_PARTS
    const int parts;
    uint32_t iterTag = 1;                        // k_start publishes tag 1 when it queued anything
    size_t brackets[TIMED_CLASSES] = {0, 0, 0};  // timing brackets of each class since the last host check
    // (short batches: 8 -- every check drains all streams, ~0.2 ms in which nothing runs, and most of a short pass is its drain: 27 near-empty
    // iterations of ~150 us each for the 16-spp passes of the as-shipped materialtest, profiles/README.md; the price is <= 7 empty iterations
    // of ~55 us after the last path has ended)
    Batch(tghip_ctx *c, const PassParams &p, const PassTarget &t)
        : ctx(c), pp(p), target(t), lp(c->lp), choice(c->lp.choice), s(c->scene), st(batchState(c)),
          checkInterval(c->checkInterval > 0 ? c->checkInterval : (uint64_t(p.total_items) >= 4ull*st.num_slots ? 16 : 8)),
          part(splitBatch(c, st, p)), parts(int(part.size())) {}
    // Fork: what the main stream holds so far comes first for the other parts' streams.  Join: the main stream waits for them.  (One part: no call.)
    int forkParts() {
        if (parts > 1) HIP_TRY(ctx, hipEventRecord(ctx->evMain, ctx->stream));
        for (int k = 1; k < parts; ++k)
            HIP_TRY(ctx, hipStreamWaitEvent(part[k].stream, ctx->evMain, 0));
        return TGHIP_OK;
    }
    int joinParts() {
        for (int k = 1; k < parts; ++k) {
            HIP_TRY(ctx, hipEventRecord(ctx->evPart[k - 1], part[k].stream));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->evPart[k - 1], 0));
        }
        return TGHIP_OK;
    }
    // Per-launch timing ("time_kernels"): `launches` between two events of the pool on the part's stream, read back class by class at the next host
    // check.  A round brackets each class once per part and iteration: a class's brackets are a run of the pool's pairs, sized for the most parts.
    size_t bracketEvent(int cls, size_t n) const { return 2*((size_t(cls)*checkInterval)*TGHIP_MAX_PARTS + n); }
    template<typename Launches>
    void timed(TimedClass cls, const BatchPart &p, Launches launches) {
        const size_t e = bracketEvent(cls, brackets[cls]);
        if (ctx->timeKernels) (void)hipEventRecord(ctx->evPool[e], p.stream);
        launches();
        if (ctx->timeKernels) { (void)hipEventRecord(ctx->evPool[e + 1], p.stream); brackets[cls]++; }
    }
    // The event pool grown to a round's brackets, the two memsets, the fork (the memsets come first for the other streams as well), k_start
    int start() {
        while (ctx->timeKernels && ctx->evPool.size() < bracketEvent(TIMED_CLASSES, 0)) {
            hipEvent_t e = nullptr;
            HIP_TRY(ctx, hipEventCreate(&e));
            ctx->evPool.push_back(e);
        }
        HIP_TRY(ctx, hipMemsetAsync(st.partial, 0, size_t(pp.total_items)*sizeof(float4), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(st.live, 0, 4*sizeof(uint32_t), ctx->stream));
        const int rc = forkParts();
        for (int k = 0; k < parts && rc == TGHIP_OK; ++k)
            hipLaunchKernelGGL(k_start, dim3(part[k].grid), dim3(256), 0, part[k].stream, s, part[k].st, part[k].pp);
        return rc;
    }
    // The host check: the parts joined, the liveness word (and, where k_tail may follow, the live paths) read back on a dry main stream, the
    // round's brackets added to the counters
    int check(Outcome &outcome) {
        // k_tail: per-launch timing does not see it (the few thousand rays it traces are in the counters, its one launch is in none of the three kernel classes)
        const bool tailEligible = choice.tailEligible && st.slots_per_block <= PT_MAX_SLOTS_PER_BLOCK;
        const int rc = joinParts();              // the main stream waits for the other parts before it reads the flag
        if (rc != TGHIP_OK) return rc;
        // an abort request that arrived since the last check (or before the pass's first launch): make sure the device
        // word is set -- in stream order, so the launches below see it and drain their slots
        if (ctx->abortRequested.load(std::memory_order_acquire))
            HIP_TRY(ctx, hipMemsetAsync(ctx->abortFlagDev.get(), 0xFF, sizeof(uint32_t), ctx->stream));
        if (tailEligible) hipLaunchKernelGGL(k_live_slots, dim3(1), dim3(256), 0, ctx->stream, st, ctx->poolGrid);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->hostLive, st.live, 2*sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        // (split loop: EVERY part's launches are bracketed, each on its own stream -- three pairs per part and iteration, in launch
        // order.  Rounds 2-4 timed part 0 only and counted the others "as long on average": they are not -- the parts whose
        // streams the hardware queues serve later run ~45 % longer launches (rocprofv3's kernel trace, profiles/README.md) --, so the
        // per-kernel averages were part 0's, a fifth below the mean)
        TgHipCounters &c = ctx->counters;
        double *ms[TIMED_CLASSES] = {&c.ms_trace_closest, &c.ms_shade, &c.ms_trace_shadow};
        for (int cls = 0; cls < TIMED_CLASSES; ++cls)
            for (size_t k = 0; k < brackets[cls]; ++k) {
                float elapsed = 0.0f;
                HIP_TRY(ctx, hipEventElapsedTime(&elapsed, ctx->evPool[bracketEvent(cls, k)], ctx->evPool[bracketEvent(cls, k) + 1]));
                *ms[cls] += double(elapsed);
            }
        c.launches_trace_closest += brackets[TIMED_CLOSEST];
        c.launches_trace_shadow += brackets[TIMED_SHADOW];
        c.launches_shade += brackets[TIMED_SHADE]*size_t(choice.shadeLaunches);   // (one bracket around them: ms_shade is their sum)
        brackets[TIMED_CLOSEST] = brackets[TIMED_SHADE] = brackets[TIMED_SHADOW] = 0;
        if (ctx->hostLive[0] != iterTag) outcome = DONE;   // the last iteration left every extension queue empty
        else if (tailEligible && lp.tailFits && uint64_t(ctx->hostLive[1]) <= uint64_t(std::max<long long>(ctx->tailThreshold, 0))) outcome = TAIL;
        else outcome = GO_ON;
        return TGHIP_OK;
    }
    // Few paths left: each part of the pool finishes in one launch of k_tail (its workgroups iterate on their own), forked behind the main stream's check
    int tail() {
        uint32_t classes = 1u;
        for (int c = 1; c < PT_NUM_CLASSES; ++c)
            if (ctx->sc.classPresent[c]) classes |= 1u << c;
        int rc = forkParts();
        for (int k = 0; k < parts && rc == TGHIP_OK; ++k)
            launchKernel(lp.tail, part[k].grid, part[k].stream, s, part[k].st, part[k].pp, classes);
        if (rc != TGHIP_OK || (rc = joinParts()) != TGHIP_OK) return rc;
        ctx->counters.tail_launches++;
        if (std::getenv("TGHIP_VERBOSE")) {
            const auto t0 = std::chrono::steady_clock::now();
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            std::fprintf(stderr, "[tghip]   tail kernel after %llu iterations with %u paths alive: %.2f ms\n", (unsigned long long)(iterTag - 1), ctx->hostLive[1],
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        return TGHIP_OK;
    }
    // The shading launches of an iteration, in the choice's order.  The classes (the escaped paths, Q_MISS; 0; the classes 1 .. 3 that occur) consume queues
    // of their own and OR what they append into the workgroup's bitmaps (k_shade: CONCURRENT), so their launches MAY run side by side on three
    // streams: the "class_streams" option gives launches a lane beside the part's stream.  Measured slower than one after the other (materialtest
    // 735-800 against 825-830 Msamples/s, mesh1m 409 against 508, for 2 to 24 hardware queues): with four parts in flight the chip is not short of
    // independent launches.
    void launchShading(const BatchPart &p) {
        bool forked = false, lanes[3] = {false, false, false};
        for (int i = 0; i < choice.numShade; ++i) {
            const int lane = choice.shade[i].lane;
            hipStream_t stream = p.stream;
            if (lane) {
                stream = ctx->classStream[p.index][lane - 1];
                if (!forked) (void)hipEventRecord(ctx->evFork[p.index], p.stream);
                (void)hipStreamWaitEvent(stream, ctx->evFork[p.index], 0);
                forked = lanes[lane] = true;
            }
            launchKernel(lp.shade[i], p.grid, stream, s, p.st, p.pp, choice.shade[i].cls);
            if (lane) (void)hipEventRecord(ctx->evJoin[p.index][lane - 1], stream);
        }
        for (int lane = 1; lane < 3; ++lane)
            if (lanes[lane]) (void)hipStreamWaitEvent(p.stream, ctx->evJoin[p.index][lane - 1], 0);
    }
    void launchFinish(const BatchPart &p) { hipLaunchKernelGGL(k_finish, dim3(p.grid), dim3(256), 0, p.stream, s, p.st, p.pp, iterTag); }
    // the launches of one wavefront iteration over a part
    void launchIteration(const BatchPart &p) {
        if (choice.queryPaths)                   // (the fresh paths of the previous iteration's finish / of k_start get the caller's rays before they are traced)
            radianceQueryLaunchPaths(p.stream, p.grid, p.st, target.rays, target.numRays);
        else if (choice.cameraRays)              // (the fresh camera rays of the previous iteration's finish / of k_start, before they are traced)
            hipLaunchKernelGGL(k_camera_rays, dim3(p.grid), dim3(256), 0, p.stream, s, p.st, p.pp);
        timed(TIMED_CLOSEST, p, [&] {
            if (choice.closest.kernel.family == K_FINISH_CLOSEST_WIDE)   // (k_finish's work of the previous iteration in front of the walk, pt_wavefront.h)
                launchKernel(lp.closest, p.grid, p.stream, s, p.st, p.pp);
            else
                launchKernel(lp.closest, p.grid, p.stream, s, p.st);
        });
        // (the end of a query's first segment, before the hits are shaded.  Launched whether or not a ray of the batch has a finite tmax: the rays
        // may be device memory, which the host could only know that of after a reduction over them -- about 10 us per launch, profiles/radiance_query/bench.txt)
        if (choice.queryPaths)
            radianceQueryLaunchClip(p.stream, p.grid, p.st, target.rays, target.numRays);
        timed(TIMED_SHADE, p, [&] { launchShading(p); });
        timed(TIMED_SHADOW, p, [&] { launchKernel(lp.shadow, p.grid, p.stream, s, p.st, p.pp, iterTag); });
        if (!choice.foldFinish)                  // (always: the shading launches leave their finished paths to k_finish as well; folded: the next iteration's
            launchFinish(p);                     // closest-hit launch, or the end of the round)
    }
    // One round: the iterations between two host checks -- one where a single launch renders the whole batch
    void iterate() {
        const int roundIters = choice.oneLaunch ? 1 : checkInterval;
        for (int it = 0; it < roundIters; ++it, ctx->counters.iterations++) {
            ++iterTag;
            if (choice.fusedFlat) {
                // flat-list scene: intersection and shadow tests happen inside the shading launches, over the whole pool -- flat scenes are never
                // split (chooseLaunches, LaunchChoice.cpp) -- and the two walks' brackets stay empty
                part[0].pp.iter_tag = iterTag;
                timed(TIMED_CLOSEST, part[0], [] {});
                timed(TIMED_SHADE, part[0], [&] { launchShading(part[0]); });
                timed(TIMED_SHADOW, part[0], [] {});
            } else {
                // (rejected, round 5: part k's iteration i on stream (k + i) mod parts, so that every part spends the same time on every hardware
                // queue: profiles/r5_sweep_rotate_streams.jsonl)
                for (int k = 0; k < parts; ++k)
                    launchIteration(part[k]);
            }
        }
        // folded k_finish: the last iteration's finish as a launch of its own -- before the host reads the liveness word, before k_tail
        for (int k = 0; k < parts && choice.foldFinish && !choice.fusedFlat; ++k)
            launchFinish(part[k]);
    }
    int resolve() {
        if (pp.rec_sorted) hipLaunchKernelGGL(k_resolve_records, dim3((pp.num_sorted*16u + 255)/256), dim3(256), 0, ctx->stream, st, pp, target.sum, target.count);
        else               hipLaunchKernelGGL(k_resolve, dim3((pp.pix_slots + 255)/256), dim3(256), 0, ctx->stream, st, pp, target.sum, target.count);
        HIP_TRY(ctx, hipGetLastError());
        return ctx->abortRequested.load(std::memory_order_acquire) ? TGHIP_E_ABORTED : TGHIP_OK;
    }
};
} // namespace

// Runs the wavefront loop for one batch of work items until every slot is drained.
static int runBatch(tghip_ctx *ctx, const PassParams &pp, const PassTarget &target)
{
    if (ctx->abortRequested.load(std::memory_order_acquire))
        return TGHIP_E_ABORTED;                  // aborted before this batch started: nothing to drain
    Batch batch(ctx, pp, target);
    Batch::Outcome found = Batch::GO_ON;
    int rc = batch.start();
    while (rc == TGHIP_OK) {
        if ((rc = batch.check(found)) != TGHIP_OK || found == Batch::DONE) break;
        if (found == Batch::TAIL) { rc = batch.tail(); break; }
        batch.iterate();
    }
    return rc == TGHIP_OK ? batch.resolve() : rc;
}

// The device arrays the plan of a pass names -- the shard's tiles, the tile seeds, a record pass's six arrays and its hint table, the auxiliary
// pixels, the per-sample radiance --, grown, filled on the context's stream and named in `base`, the pass's parameters every batch starts from
static int placePassArrays(tghip_ctx *ctx, const TgHipPassDesc &pass, uint32_t w, uint32_t h, PassPlan &plan, const PassTarget &target, PassParams &base)
{
    int rc = TGHIP_OK;
    auto upload = [&](DeviceArray<uint32_t> &dev, const std::vector<uint32_t> &src) -> int {
        const int grc = dev.grow(ctx, src.size());
        if (grc != TGHIP_OK) return grc;
        if (!src.empty())
            HIP_TRY(ctx, hipMemcpyAsync(dev.get(), src.data(), src.size()*sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        return TGHIP_OK;
    };
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
    return TGHIP_OK;
}

// The planned pass `plan` of `pass` over a w x h image, into `target`: the launch plan of its kind, the device arrays the plan names, the pool, the
// wavefront loop batch by batch.  What tghip_wait runs for a render pass (w x h the scene's image, the target the context's framebuffer) and
// tghip_query_radiance (shim_queries.hip) for a query (the virtual image of the rays, a framebuffer of its own).  Synchronous.
int tghipRunPass(tghip_ctx *ctx, const TgHipPassDesc &pass, uint32_t w, uint32_t h, PassPlan &plan, const PassTarget &target)
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
    PassParams base{};
    if ((rc = placePassArrays(ctx, pass, w, h, plan, target, base)) != TGHIP_OK)
        return rc;

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
    const int rc = planPass(pass, ctx->width, ctx->height, passPlanOptions(ctx, ctx->chunkSamples), ctx->plan, ctx->error);
    if (rc != TGHIP_OK || ctx->plan.empty)
        return ctx->passResult = rc;
    PassTarget target;
    target.sum = ctx->frameSum();
    target.count = ctx->frameCount();
    return ctx->passResult = tghipRunPass(ctx, pass, ctx->width, ctx->height, ctx->plan, target);
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

// the libm restatements exactly as the shading kernels call them (pt_math.h).  (In this unit, alone of the debug-case family: without these two kernels
// the unit's other kernels -- the walks, k_camera_rays -- come out with other code hashes, profiles/shim_split/kernel_resources_diff.txt)
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

int tghip_debug_launch_plan(tghip_ctx *ctx, const TgHipPassDesc *pass, TgHipLaunchPlan *out)
{
    if (!ctx || !pass || !out) return TGHIP_E_INVALID;
    if (!ctx->haveScene) { ctx->error = "launch plan without an uploaded scene"; return TGHIP_E_NOSCENE; }
    int rc = checkPass(*pass, ctx->width, ctx->height, ctx->scene.sobol != nullptr, ctx->error);
    if (rc != TGHIP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassPlan passPlan;
    if ((rc = planPass(*pass, ctx->width, ctx->height, passPlanOptions(ctx, ctx->chunkSamples), passPlan, ctx->error)) != TGHIP_OK) return rc;
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
