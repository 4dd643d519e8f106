# Builds the in-tree native artefacts:
#   tungsten_amd/lib/libtungsten_hip.so   product: C++11 host side + HIP kernels + extern "C" shim (gfx950)
#   tungsten_amd/lib/tungsten_hip         product: CLI (same role as the reference's `tungsten` binary)
#   oracle/liboracle.so                   TEST INFRASTRUCTURE: CPU restatement (never linked by the product)
#   oracle/libm_host.so                   TEST INFRASTRUCTURE: csrc/hip/pt_libm.h compiled for the host (checked against the host libm)
#   oracle/_ref/*                         TEST INFRASTRUCTURE: the reference itself (only where /root/reference exists)
HIPCC    ?= hipcc
CC       ?= gcc
ARCH     ?= gfx950
LIBDIR   := tungsten_amd/lib
# PROFILE=1: the development build with k_shade's section timers (-DPT_PROFILE) as libtungsten_hip_prof.so next to the product
# library (TUNGSTEN_AMD_LIB=... python tools/sweep.py ...); objects of its own
# VARIANT=name VARFLAGS="-D..." : an experiment's build of the device code next to the product library, libtungsten_hip_<name>.so with objects
# of its own (A/B runs within one GPU session: TUNGSTEN_AMD_LIB=tungsten_amd/lib/libtungsten_hip_<name>.so python bench.py ...)
OBJDIR   := $(if $(PROFILE),build/obj_prof,$(if $(VARIANT),build/obj_$(VARIANT),build/obj))
LIBNAME  := $(if $(PROFILE),libtungsten_hip_prof.so,$(if $(VARIANT),libtungsten_hip_$(VARIANT).so,libtungsten_hip.so))
HOSTSRC  := $(wildcard tungsten_amd/csrc/host/*.cpp)
HOSTLIB  := $(filter-out tungsten_amd/csrc/host/main.cpp,$(HOSTSRC))
HOSTOBJ  := $(patsubst tungsten_amd/csrc/host/%.cpp,$(OBJDIR)/host_%.o,$(HOSTLIB))
# the kernels' unit and the core of the shim (tungsten_hip.hip: context, options, upload, launch plan, render pass, tghip_debug_libm with its two kernels; the
# context and what the shim's units share: shim_context.h, device_array.h) + the shim's host-only units, which hold no kernel and take no kernel's address --
# shim_queries.hip (tghip_query_*), shim_images.hip (the transfers, tghip_develop, tghip_nlmeans), shim_debug.hip (tghip_debug_bsdf / _light / _medium), reduce.hip
# (the RCCL reduces): a change to one of them compiles in seconds and moves no kernel + debug_units.hip, the kernels behind shim_debug.hip + one translation unit per family of
# explicit instantiations (pt_instances.h lists each unit's; they compile in parallel under make -j) + develop.hip, the kernels of tghip_develop,
# + denoise.hip, the NL-means kernel of tghip_nlmeans (its host comparator csrc/host/Denoise.cpp comes in through HOSTSRC)
# + ray_query.hip, the kernels of tghip_query_rays (its argument check csrc/host/RayQuery.cpp comes in through HOSTSRC; the claim, the ray load and the
#   8-wide loop it shares with the units below, their ballot-append, start medium and far distance: query_walk.h, query_walk_wide.h; the clauses the five checks share: csrc/host/QueryCheck.hpp)
# + radiance_query.hip, the ray source and the result copy of tghip_query_radiance (its check and virtual image, csrc/host/RadianceQuery.cpp, likewise)
# + surface_query.hip, the instanced walk and the dense launch of tghip_query_surface -- its other walks are ray_query.hip's kernels -- (its argument check,
#   csrc/host/SurfaceQuery.cpp, likewise)
# + transmittance_query.hip, the walk and the dense launch of a round of tghip_query_transmittance (its argument check, csrc/host/TransmittanceQuery.cpp, likewise)
# + direct_query.hip, the three dense launches of tghip_query_direct around those two units' walks (its argument check, csrc/host/DirectQuery.cpp, likewise)
# + direct_estimate.h, the direct estimate at one point -- surface and volume body, once -- for direct_query.hip's setup and vertex_query.hip's front stage
# + vertex_query.hip, the three dense launches of tghip_query_vertex around the surface query's walk and the direct query's shadow rounds (its argument
#   check, csrc/host/VertexQuery.cpp, likewise; its stand-alone sanitizer run: tools/vertex_query_check.cpp, the command in its header)
HIPSRC   := $(wildcard tungsten_amd/csrc/hip/*.hip)
HIPOBJ   := $(patsubst tungsten_amd/csrc/hip/%.hip,$(OBJDIR)/%.o,$(HIPSRC))
# (the shim reads what csrc/host/SceneCheck.cpp decided about a scene, SceneTraits, what csrc/host/PassPlan.cpp decided about a pass, PassPlan, what
# csrc/host/LaunchChoice.cpp decided about the pass's kernels, LaunchChoice; shim_queries.hip calls the queries' checks, csrc/host/*Query.cpp)
HIPHDR   := $(wildcard tungsten_amd/csrc/hip/*.h) include/tungsten_hip.h tungsten_amd/csrc/host/SceneCheck.hpp tungsten_amd/csrc/host/PassPlan.hpp tungsten_amd/csrc/host/RayQuery.hpp tungsten_amd/csrc/host/RadianceQuery.hpp tungsten_amd/csrc/host/SurfaceQuery.hpp tungsten_amd/csrc/host/TransmittanceQuery.hpp tungsten_amd/csrc/host/DirectQuery.hpp tungsten_amd/csrc/host/VertexQuery.hpp tungsten_amd/csrc/host/LaunchChoice.hpp
# -ffp-contract=off: no FMA contraction, so device arithmetic rounds like the CPU reference/oracle
# (DESIGN.md "Numerics"); TG_FAST=1 allows contraction.
FPFLAGS  := $(if $(TG_FAST),-ffp-contract=fast,-ffp-contract=off)
# (-ffp-contract=off: the host restates float32 arithmetic of the reference whose bits matter -- the instance tree and Embree's top-level tree,
# bounds, CDF tables --, so no flag a packager adds, -march=native say, may fuse a multiply with an add)
HOSTFLAGS:= -std=c++11 -O2 -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter
# -fno-slp-vectorize (round 5): the SLP vectoriser packs the kernels' float arithmetic into v_pk_mul / v_pk_add -- 3.7 cycles per pair on gfx950
# against 2 x 2.0 for the scalar pair, plus the v_mov that put operands side by side -- and the packing costs registers: the shadow walk 119 -> 98
# VGPRs (five waves per SIMD instead of four), k_shade's conductor-family variant 43 -> 0 spilled registers.  Same IEEE operations either way.
# Metric's workload +3.5 %, mesh1m +2 %, instances10k +1.8 %, Cornell box +0.9 % (profiles/r5_ab_no_slp.txt).  SLP=1 gives the vectoriser back.
HIPFLAGS := --offload-arch=$(ARCH) $(if $(HIPOPT),$(HIPOPT),-O3) -std=c++17 -fPIC $(FPFLAGS) $(if $(SLP),,-fno-slp-vectorize) -Wno-unused-result $(if $(PROFILE),-DPT_PROFILE,) $(VARFLAGS)

all: $(LIBDIR)/$(LIBNAME) $(if $(PROFILE)$(VARIANT),,$(LIBDIR)/tungsten_hip oracle/liboracle.so oracle/libm_host.so)

# (pt_variants.h: the kernel variants' type / feature masks, which SceneCheck.cpp sorts materials by)
$(OBJDIR)/host_%.o: tungsten_amd/csrc/host/%.cpp $(wildcard tungsten_amd/csrc/host/*.hpp) include/tungsten_hip.h include/tungsten_host.h tungsten_amd/csrc/hip/pt_variants.h
	@mkdir -p $(OBJDIR)
	g++ $(HOSTFLAGS) -c $< -o $@

# shade_simple.hip -- the Cornell box's one-launch kernel (k_shade<MASK_LEAN, ., FUSE_TRACE | FUSE_SHADOW | FUSE_LOOP>) and the class-0 shading variants -- is scheduled with
# the AMDGPU back end's max-ilp strategy: Cornell box 2 551 -> 2 600 Msamples/s (+1.9 %, two alternations, images identical), the metric's workload and mesh1m level
# (profiles/r6_ab_compiler_options.txt; on the traversal and the other shading translation units the strategy changes nothing, round 5 and the same file).  SCHED= gives the default back.
SCHED ?= max-ilp
$(OBJDIR)/shade_simple.o: HIPFLAGS += $(if $(SCHED),-mllvm -amdgpu-sched-strategy=$(SCHED),)
# tail.hip -- k_tail, one latency-bound launch per part at the end of every pass (a sixth of a 16-spp pass of the as-shipped materialtest) -- is built -Os: 264 -> 234 VGPRs,
# as shipped 743 -> 750 Msamples/s in three alternations (profiles/r6_ab_compiler_options.txt, session 55); the throughput kernels keep -O3.  TAILOPT=-O3 gives it back.
TAILOPT ?= -Os
$(OBJDIR)/tail.o: HIPFLAGS := $(if $(HIPOPT),$(HIPFLAGS),$(subst -O3,$(TAILOPT),$(HIPFLAGS)))
# tungsten_hip.hip and walk_shadow.hip -- the closest-hit and shadow walks and the small kernels around them -- are built -Os as well: the metric's workload 1 167 -> 1 175 Msamples/s
# (+0.7 %, better in seven of seven alternations), mesh1m +0.5 %, instances10k level (profiles/r6_ab_compiler_options.txt, sessions 57 / 58; -O2 had read level to +0.6 % in session 49).
# The shading units keep -O3 (-Os: level or slower).  WALKOPT=-O3 gives it back.
# walk_shadow.hip alone reads another 0.3 % at -O1 (its launches 603 -> 596 us; the metric better in five of five alternations, session 62; mesh1m level): SHADOWOPT.
WALKOPT ?= -Os
SHADOWOPT ?= -O1
$(OBJDIR)/tungsten_hip.o: HIPFLAGS := $(if $(HIPOPT),$(HIPFLAGS),$(subst -O3,$(WALKOPT),$(HIPFLAGS)))
# (walk_shadow_tex.hip: the shim's closest-hit shadow walk once more, for scenes with `disk` / `blade` textures -- built like the shim's)
$(OBJDIR)/walk_shadow_tex.o: HIPFLAGS := $(if $(HIPOPT),$(HIPFLAGS),$(subst -O3,$(WALKOPT),$(HIPFLAGS)))
$(OBJDIR)/walk_shadow.o: HIPFLAGS := $(if $(HIPOPT),$(HIPFLAGS),$(subst -O3,$(SHADOWOPT),$(HIPFLAGS)))

$(OBJDIR)/%.o: tungsten_amd/csrc/hip/%.hip $(HIPHDR)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/$(LIBNAME): $(HOSTOBJ) $(HIPOBJ)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@ -lpthread -ldl

$(LIBDIR)/tungsten_hip: tungsten_amd/csrc/host/main.cpp $(LIBDIR)/libtungsten_hip.so
	g++ $(HOSTFLAGS) $< -o $@ -L$(LIBDIR) -ltungsten_hip -Wl,-rpath,'$$ORIGIN' -lpthread

oracle/liboracle.so: oracle/oracle.c include/tungsten_hip.h
	$(CC) -std=c99 -O2 -ffp-contract=off -fopenmp -fPIC -shared $< -o $@ -lm

oracle/libm_host.so: oracle/libm_host.cpp tungsten_amd/csrc/hip/pt_libm.h
	$(CXX) -std=c++17 -O2 -ffp-contract=off -mfma -fopenmp -fPIC -shared $< -o $@ -lm

# the reference itself, only where its sources are mounted
ref:
	@if [ -d /root/reference/src ]; then $(MAKE) -f oracle/Makefile.ref -j$$(nproc) all; else echo "no /root/reference: keeping prebuilt oracle/_ref"; fi

clean:
	rm -rf build $(LIBDIR) oracle/liboracle.so oracle/libm_host.so

.PHONY: all ref clean
