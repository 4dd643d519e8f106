// The explicitly instantiated kernels of pt_wavefront.h -- k_shade, k_shade_fused, k_tail, k_trace_shadow_fast, k_trace_shadow_fast_inst and the
// BSDF_MASK_ALL closest-hit shadow walk --, each named ONCE, grouped by the translation unit that instantiates it (the units are built with flags of
// their own: Makefile).  All three uses are generated from these lists:
//     the unit itself, its list   PT_KERNEL = PT_INSTANTIATE_KERNEL   the explicit instantiation
//     the shim, every list        PT_KERNEL = PT_DECLARE_KERNEL       the declaration that keeps the shim's unit from instantiating it again
//     the shim's explicitKernelFn PT_KERNEL = a lookup                if (<the KernelId names this variant>) return &k<...>;
// so a variant is instantiated, declared and dispatched, or none of the three.
//
// An entry expands into PT_KERNEL(match, parameters, kernel<arguments>) -- `match` is the condition on a KernelId `k` (csrc/host/LaunchChoice.hpp) under
// which the variant is the one meant -- and a second time for its FEAT_QMC twin; the three variants without a twin are the lists' PT_SHADE_ONLY entries.
// (The order within a list is the order of the instantiations in the unit's code object.)
#pragma once

#define PT_SHADE_PARAMS (DeviceScene, PathState, PassParams, int)
#define PT_WALK_PARAMS  (DeviceScene, PathState, PassParams, uint32_t)

// k_shade<M, W, FUSE> and its twin
#define PT_SHADE(M, W, F) PT_SHADE_ONLY(M, W, F, false) PT_SHADE_ONLY(((M) | FEAT_QMC), W, F, false)
// ... and the variants without a twin (FEAT_QMC is in their masks): BSDF_MASK_ALL, MASK_MEDIA, the GLOBAL_TABLES one
#define PT_SHADE_ONLY(M, W, F, G) \
    PT_KERNEL(k.family == K_SHADE && k.mask == (M) && k.fuse == (F) && k.globalTables == (G), PT_SHADE_PARAMS, k_shade<M, W, F, G>)
// k_shade_fused<M, MASK_SIMPLE, W>: one further class + class 0 and the escaped paths in one launch
#define PT_SHADE_FUSED(M, W) \
    PT_KERNEL(k.family == K_SHADE_FUSED && k.mask == (M), PT_SHADE_PARAMS, k_shade_fused<M, MASK_SIMPLE, W>) \
    PT_KERNEL(k.family == K_SHADE_FUSED && k.mask == ((M) | FEAT_QMC), PT_SHADE_PARAMS, k_shade_fused<((M) | FEAT_QMC), (MASK_SIMPLE | FEAT_QMC), W>)
// k_tail<M, SOLIDS> and its twin; ... for both values of SOLIDS
#define PT_TAIL_ONLY(M, S) PT_KERNEL(k.family == K_TAIL && k.mask == (M) && k.solids == (S), PT_WALK_PARAMS, k_tail<M, S>)
#define PT_TAIL(M, S)      PT_TAIL_ONLY(M, S) PT_TAIL_ONLY(((M) | FEAT_QMC), S)
#define PT_TAIL_SOLIDS(M)  PT_TAIL_ONLY(M, false) PT_TAIL_ONLY(M, true) PT_TAIL_ONLY(((M) | FEAT_QMC), false) PT_TAIL_ONLY(((M) | FEAT_QMC), true)
// k_trace_shadow_fast<COUNT, SOLIDS> / k_trace_shadow_fast_inst<COUNT, SOLIDS>
#define PT_SHADOW_FAST(C, S) \
    PT_KERNEL(k.family == K_SHADOW_FAST && k.count == (C) && k.solids == (S), PT_WALK_PARAMS, k_trace_shadow_fast<C, S>)
#define PT_SHADOW_FAST_INST(C, S) \
    PT_KERNEL(k.family == K_SHADOW_FAST_INST && k.count == (C) && k.solids == (S), PT_WALK_PARAMS, k_trace_shadow_fast_inst<C, S>)
// k_trace_shadow<COUNT, true, FLAT, INST, BSDF_MASK_ALL>: closest-hit shadow walks only (of an instanced scene INST = 1 / 2, whatever `flat` says)
#define PT_SHADOW_TEX(C, FLAT, INST) \
    PT_KERNEL(k.family == K_SHADOW && k.mask == BSDF_MASK_ALL && k.count == (C) && ((INST) ? k.inst == (INST) : (k.inst != 1 && k.inst != 2 && k.flat == (FLAT))), \
              PT_WALK_PARAMS, k_trace_shadow<C, true, FLAT, INST, BSDF_MASK_ALL>)

// ---- the lists, one per translation unit ----
#define PT_UNIT_shade_simple \
    PT_SHADE(MASK_LEAN, LEAN_WAVES, 0) PT_SHADE(MASK_LEAN, LEAN_WAVES, 3) PT_SHADE(MASK_LEAN, LEAN_WAVES, 7) \
    PT_SHADE(MASK_SIMPLE, SIMPLE_WAVES, 0) PT_SHADE(MASK_SIMPLE_INST, SIMPLE_WAVES, 0) PT_SHADE(MASK_SIMPLE, SIMPLE_WAVES, 3) PT_SHADE(MASK_SIMPLE, SIMPLE_WAVES, 7)
#define PT_UNIT_shade_class \
    PT_SHADE(MASK_COAT, COAT_WAVES, 0) PT_SHADE(MASK_COAT, COAT_WAVES, 2) PT_SHADE(MASK_GLASS, 2, 0) PT_SHADE(MASK_GLASS, 2, 2)
#define PT_UNIT_shade_plastic   PT_SHADE(MASK_PLASTIC, 2, 0) PT_SHADE(MASK_PLASTIC, 2, 2)
// (the per-family class variants of scenes with instance records)
#define PT_UNIT_shade_inst      PT_SHADE(MASK_COAT_INST, 2, 0) PT_SHADE(MASK_GLASS_INST, 2, 0)
#define PT_UNIT_shade_inst2     PT_SHADE(MASK_PLASTIC_INST, 2, 0)
// (BSDF_MASK_ALL: the one variant with FEAT_MEDIA / FEAT_AUX / FEAT_CYLINDER)
#define PT_UNIT_shade_full      PT_SHADE(MASK_FULL, 2, 0) PT_SHADE(MASK_FULL, 2, 2) PT_SHADE_ONLY(BSDF_MASK_ALL, 2, 0, false)
#define PT_UNIT_shade_media     PT_SHADE_ONLY(MASK_MEDIA, 2, 0, false)
#define PT_UNIT_shade_global    PT_SHADE_ONLY(BSDF_MASK_ALL, 2, 0, true)
#define PT_UNIT_shade_fused     PT_SHADE_FUSED(MASK_COAT, COAT_WAVES) PT_SHADE_FUSED(MASK_GLASS, 2) PT_SHADE_FUSED(MASK_PLASTIC, 2)
// (MASK_COAT: the tail of scenes whose materials are Lambert / null and the conductor family only (the metric's scene): a third of the instructions
// of the all-types variant, at one wave per SIMD where instruction latency is what a tail iteration takes)
#define PT_UNIT_tail            PT_TAIL_SOLIDS(MASK_TAIL) PT_TAIL(MASK_COAT, false)
#define PT_UNIT_walk_shadow \
    PT_SHADOW_FAST(false, false) PT_SHADOW_FAST(false, true) PT_SHADOW_FAST(true, false) PT_SHADOW_FAST(true, true) \
    PT_SHADOW_FAST_INST(false, false) PT_SHADOW_FAST_INST(false, true) PT_SHADOW_FAST_INST(true, false) PT_SHADOW_FAST_INST(true, true)
#define PT_UNIT_walk_shadow_tex \
    PT_SHADOW_TEX(false, false, 0) PT_SHADOW_TEX(true, false, 0) PT_SHADOW_TEX(false, true, 0) PT_SHADOW_TEX(true, true, 0) \
    PT_SHADOW_TEX(false, false, 1) PT_SHADOW_TEX(true, false, 1) PT_SHADOW_TEX(false, false, 2) PT_SHADOW_TEX(true, false, 2)

#define PT_ALL_UNITS \
    PT_UNIT_shade_simple PT_UNIT_shade_class PT_UNIT_shade_plastic PT_UNIT_shade_inst PT_UNIT_shade_inst2 PT_UNIT_shade_full PT_UNIT_shade_media \
    PT_UNIT_shade_global PT_UNIT_shade_fused PT_UNIT_tail PT_UNIT_walk_shadow PT_UNIT_walk_shadow_tex

// ---- the uses: PT_KERNEL is looked up when a list is expanded ----
#define PT_INSTANTIATE_KERNEL(match, params, ...) template __global__ void __VA_ARGS__ params;
#define PT_DECLARE_KERNEL(match, params, ...)     extern template __global__ void __VA_ARGS__ params;
