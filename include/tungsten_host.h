/*
 * tungsten_host.h -- C view of the C++11 host side (scene loading, flattening, the
 * Integrator render loop) so that tests/bench (Python ctypes) and foreign hosts can drive it.
 * Mirrors what the reference's CLI does around the plugin surface
 * (src/tungsten/Shared.hpp:191-337: Scene::load -> loadResources -> makeTraceable(seed) ->
 * while (!integrator.done()) { startRender; waitForCompletion; } -> saveOutputs).
 * All functions return 0 on success, negative on error with a message in `err`.
 */
#ifndef TUNGSTEN_HOST_H_
#define TUNGSTEN_HOST_H_

#include "tungsten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tgh_scene tgh_scene;        /* Scene + TraceableScene (flattened, BVH built), no device */
typedef struct tgh_renderer tgh_renderer;  /* the above + PathTraceHipIntegrator bound to HIP device(s) */

typedef struct TgHostSceneInfo {
    uint32_t width, height, spp, spp_step;
    uint32_t num_nodes, num_recs, num_objects, num_lights, num_bsdfs, num_textures;
    int32_t  bvh_depth;
    double   bvh_sah_cost, build_seconds;
    int32_t  adaptive_sampling, stratified_sampler;
    uint32_t current_spp;      /* tgh_renderer_info only: Integrator::currentSpp() */
} TgHostSceneInfo;

/* Scene::load + loadResources + flatten (Scene.cpp:378-391,281-306; TraceableScene.hpp:57-137) */
tgh_scene *tgh_scene_load(const char *json_path, char *err, size_t errlen);
const TgHipSceneDesc *tgh_scene_desc(tgh_scene *s);
int  tgh_scene_info(tgh_scene *s, TgHostSceneInfo *out);
/* The items of the reference's top-level Embree geometry (renderer/TraceableScene.hpp:101-118): the scene's finite primitives in scene order, each
 * with the box its bounds() returns after prepareForRender -- restated per primitive class in csrc/host/Scene.cpp, held to the reference's own by
 * tests/test_top_tree.py -- as 6 floats (lower, upper), and the index of its object.  Returns the number of items; the arrays live as long as `s`. */
uint32_t tgh_scene_items(tgh_scene *s, const float **boxes, const int32_t **objects);
void tgh_scene_free(tgh_scene *s);

/* makeTraceable(seed) with the path_tracer_hip integrator (needs a HIP device) */
tgh_renderer *tgh_renderer_open(const char *json_path, uint32_t seed, int spp_override, int devices,
                                char *err, size_t errlen);
tghip_ctx *tgh_renderer_context(tgh_renderer *r, int device);
int  tgh_renderer_info(tgh_renderer *r, TgHostSceneInfo *out);
/* one pass: startRender + waitForCompletion; *done_out = integrator.done() */
int  tgh_renderer_step(tgh_renderer *r, int *done_out, char *err, size_t errlen);
/* while (!done) step; returns wall seconds of the loop in *seconds (Shared.hpp:281-315) */
int  tgh_renderer_render(tgh_renderer *r, double *seconds, char *err, size_t errlen);
int  tgh_renderer_image(tgh_renderer *r, float *rgb_mean, float *rgb_sum, uint32_t *count, size_t npixels,
                        char *err, size_t errlen);
int  tgh_renderer_save_outputs(tgh_renderer *r, char *err, size_t errlen);
/* Integrator::saveRenderResumeData / resumeRender (integrators/Integrator.cpp:108-162) on renderer.resume_render_file:
 * current spp, sampler flags, a hash of the flattened scene, the framebuffer and the integrator state (SampleRecords,
 * the scheduler's sampler).  *resumed_out = 1 when a matching state was found and restored (call before the first step). */
int  tgh_renderer_save_resume_data(tgh_renderer *r, char *err, size_t errlen);
int  tgh_renderer_resume(tgh_renderer *r, int *resumed_out, char *err, size_t errlen);
void tgh_renderer_close(tgh_renderer *r);

/* ---- pass scheduling (PathTraceIntegrator.cpp:27-134) -------------------------------------------------
 * SampleRecord as the integrator holds it (path_tracer/SampleRecord.hpp:13-16).  sample_count, mean and
 * running_variance are accumulated on the device (TGHIP_PASS_RECORDS); the rest is host state. */
typedef struct TgHostSampleRecord {
    uint32_t sample_count, next_sample_count, sample_index;
    float    adaptive_weight, mean, running_variance;
} TgHostSampleRecord;

/* records of the renderer after the last pass: n = ceil(W/4)*ceil(H/4) */
int  tgh_renderer_records(tgh_renderer *r, TgHostSampleRecord *out, size_t n, char *err, size_t errlen);

/* the renderer's auxiliary output buffers (renderer.output_buffers; cameras/OutputBuffer.hpp), one TgHipAuxPixel per pixel,
 * merged over its devices; all zero when the scene requests none */
int  tgh_renderer_output_buffers(tgh_renderer *r, TgHipAuxPixel *out, size_t npixels, char *err, size_t errlen);

/* One image of the renderer's output files (include/tungsten_hip.h: tghip_develop, TgHipDevelopDesc) into HOST arrays: developed on the device by a
 * renderer on one device; by the host functions below over a download by a renderer sharded over several devices, or when the context's
 * "develop_host" option is set -- the same bytes either way.  hdr_out: 3 floats per pixel for the frame, the output's channel count otherwise;
 * ldr_out: 3 bytes per pixel; either may be NULL. */
int  tgh_renderer_develop(tgh_renderer *r, const TgHipDevelopDesc *desc, float *hdr_out, uint8_t *ldr_out, size_t npixels, char *err, size_t errlen);
/* the scene camera's "tonemap" as TGHIP_TONEMAP_* (-1: a name cameras/Tonemap.hpp does not know) */
int  tgh_renderer_tonemap(tgh_renderer *r);
/* The host's own development of a downloaded framebuffer / downloaded auxiliary buffers: the loops of Integrator::writeBuffers (integrators/
 * Integrator.cpp:56-80) and OutputBuffer::save / saveLdr (cameras/OutputBuffer.hpp:56-86, 146-189) over plain arrays, no device.  What tghip_develop
 * is held to, bit for bit.  tonemap: TGHIP_TONEMAP_*; output: TGHIP_AUX_*; part: TGHIP_DEVELOP_*.  -1 on an unknown operator / output / part. */
int  tgh_develop_host_frame(const float *rgb_sum, const uint32_t *count, size_t npixels, uint32_t tonemap, float *hdr_out, uint8_t *ldr_out);
int  tgh_develop_host_aux(const TgHipAuxPixel *aux, size_t npixels, uint32_t output, uint32_t part, float *hdr_out, uint8_t *ldr_out);
/* The host's own NL-means filter (include/tungsten_hip.h: tghip_nlmeans, TgHipNlMeansDesc; denoiser/NlMeans.hpp:95-157 restated in
 * csrc/host/Denoise.cpp) over host arrays of height x width pixels of `channels` interleaved floats, no device: what tghip_nlmeans is held to, bit
 * for bit, and itself held to results recorded from the reference (tests/golden/nlmeans.npz).  Threaded over the tiles; the bits do not depend on
 * that.  The description's source must be TGHIP_NLMEANS_POINTERS; its flags are ignored.  -1 on a description tghip_nlmeans would refuse. */
int  tgh_nlmeans_host(const TgHipNlMeansDesc *desc, const float *image, const float *guide, const float *variance, float *out);

/* The scheduler on its own (no device): tile seeds + generateWork over caller-supplied record statistics. */
typedef struct tgh_scheduler tgh_scheduler;
tgh_scheduler *tgh_scheduler_create(uint32_t width, uint32_t height, uint32_t seed);
size_t tgh_scheduler_num_tiles(tgh_scheduler *s);
size_t tgh_scheduler_num_records(tgh_scheduler *s);
const uint32_t *tgh_scheduler_tile_seeds(tgh_scheduler *s);
TgHostSampleRecord *tgh_scheduler_records(tgh_scheduler *s);   /* mutable view */
/* returns 1 when the pass has work, 0 when not (PathTraceIntegrator.cpp:108-134) */
int  tgh_scheduler_generate_work(tgh_scheduler *s, uint32_t current_spp, uint32_t next_spp, int adaptive);
/* the state of the scheduler's own sampler -- the one distributeAdaptiveSamples draws from (PathTraceIntegrator.cpp:93-134) --: what a
 * render-resume state holds next to the records (Integrator::saveState / loadState of a host that drives the scheduler through this API) */
uint64_t tgh_scheduler_sampler_state(tgh_scheduler *s);
void tgh_scheduler_set_sampler_state(tgh_scheduler *s, uint64_t state);
void tgh_scheduler_free(tgh_scheduler *s);
/* the Sobol' generator matrices the host hands to the device (NULL + message when the data file is missing) */
const uint32_t *tgh_sobol_matrices(size_t *num_words, char *err, size_t errlen);

/* ---- the acceleration-structure half of the flattening, on its own ------------------------------------
 * For hosts that fill a TgHipSceneDesc from their OWN scene classes -- the reference-side binding of INTEGRATION.md
 * section 3 (oracle/ref_binding/HipSceneFlattener.cpp walks Tungsten's TraceableScene) -- and want exactly the trees this
 * library's own loader builds: the binned-SAH BVH2 over the records' boxes (tghip nodes) collapsed into the 8-wide BVH
 * (wide_nodes; none for flat-list scenes of <= TGHIP_FLAT_MAX_RECS records).  Replaces the rtcCommit of the reference's
 * TraceableScene / TriangleMesh (renderer/TraceableScene.hpp:112-134, primitives/TriangleMesh.cpp:565).
 * `recs` and `tri_attrs` (num_recs entries each, single-level scenes: no instance records) are PERMUTED IN PLACE into the
 * order both trees refer to; bounds = 6 floats per record (lo.xyz, hi.xyz) in the caller's original order. */
typedef struct tgh_accel tgh_accel;
tgh_accel *tgh_accel_build(TgHipPrimRec *recs, TgHipTriAttr *tri_attrs, const float *bounds, uint32_t num_recs, char *err, size_t errlen);
const TgHipBvhNode  *tgh_accel_nodes(tgh_accel *a, uint32_t *num_nodes);
const TgHipWideNode *tgh_accel_wide_nodes(tgh_accel *a, uint32_t *num_wide_nodes);   /* NULL / 0: walk the BVH2 */
void tgh_accel_free(tgh_accel *a);

/* The same for a scene with `instances` primitives (Instance.cpp): the trees of include/tungsten_hip.h's instance-set layout -- the scene's
 * BVH2 with the reference's own tree over the instances behind it (restated node for node: the walk's visiting order is the reference's),
 * the wide BVH over the non-instance and the instance records, every master's two subtrees -- from plain arrays.
 *   recs / tri_attrs / bounds (num_recs, may be 0): the scene's non-instance records;
 *   sets: one per `instances` primitive -- its TGHIP_REC_INSTANCE records (a = position, p0 | b = rotation quaternion w | x y z, c[0] = index
 *         into `masters` as uint32 bits, meta = kind | the primitive's object index), and per instance the reference's box (the master box's
 *         eight rotated corners, Instance.cpp:409-421) and the tight box of its geometry (tgh_instance_tight_bounds);
 *   masters: each master mesh's triangle records in master space (meta = kind | the master's object index), attributes and boxes.
 * The result's record array (tgh_accel_recs / tgh_accel_tri_attrs) is the scene's whole array in the trees' order. */
typedef struct {
    uint32_t object, num_instances;
    const TgHipPrimRec *recs;
    const float *ref_bounds;        /* 6 floats per instance: lo.xyz, hi.xyz */
    const float *tight_bounds;      /* 6 floats per instance */
} TghInstanceSet;
typedef struct {
    const TgHipPrimRec *recs;
    const TgHipTriAttr *tri_attrs;
    const float *bounds;            /* 6 floats per record */
    uint32_t num_recs;
} TghMaster;
tgh_accel *tgh_accel_build_instanced(const TgHipPrimRec *recs, const TgHipTriAttr *tri_attrs, const float *bounds, uint32_t num_recs,
                                     const TghInstanceSet *sets, uint32_t num_sets, const TghMaster *masters, uint32_t num_masters,
                                     char *err, size_t errlen);
const TgHipPrimRec *tgh_accel_recs(tgh_accel *a, uint32_t *num_recs);                 /* instanced builds only (else NULL / 0) */
const TgHipTriAttr *tgh_accel_tri_attrs(tgh_accel *a);
const uint32_t *tgh_accel_inst_prims(tgh_accel *a, uint32_t *num_inst_prims);          /* TgHipSceneDesc::inst_prims */
const float *tgh_accel_inst_leaf_boxes(tgh_accel *a);                                  /* 8 floats per inst_prims slot */
const float *tgh_accel_inst_tight_boxes(tgh_accel *a);                                 /* 8 floats per top-level record */
void tgh_accel_counts(tgh_accel *a, uint32_t *num_top_recs, uint32_t *num_instances);
/* master_verts: 3 floats every stride_floats, in master space; rot = w x y z; ref_bounds / out = lo.xyz, hi.xyz */
void tgh_instance_tight_bounds(const float *master_verts, uint32_t stride_floats, uint32_t num_verts, const float pos[3], const float rot[4],
                               const float ref_bounds[6], float out[6]);

/* The reference's top-level Embree tree (include/tungsten_hip.h: TgHipTopNode) over n items given by their boxes (6 floats each: lower xyz,
 * upper xyz), as Embree 2.11's BVH4 builder for user geometry builds it (kernels/bvh/bvh_builder_sah.cpp:811-815 -> builders/bvh_builder_sah.h:
 * 176-282; restated in csrc/host/EmbreeTopTree.cpp).  Writes at most `capacity` nodes and returns the number the tree has (n - 1 at most;
 * 0 for n < 2 and for boxes Embree would drop as invalid), or -1 when `capacity` is too small. */
int tgh_top_tree_build(const float *boxes, uint32_t n, TgHipTopNode *nodes, uint32_t capacity);
/* TgHipSceneDesc::top_nodes for a flattened scene: the tree over the objects that have a record (in object order: the reference's _finites),
 * leaves naming records, when the scene is a flat list of quads / cubes / spheres / disks / cylinders; 0 nodes otherwise.  Same return convention. */
int tgh_top_tree_for_scene(const TgHipObject *objects, uint32_t num_objects, const TgHipPrimRec *recs, uint32_t num_recs,
                           TgHipTopNode *nodes, uint32_t capacity);
/* The box the reference's bounds callback reports for a record's primitive (TraceableScene.hpp:116-118): Quad::bounds / Cube::bounds /
 * Sphere::bounds / Disk::bounds / Cylinder::bounds (primitives/Quad.cpp:281-289, Cube.cpp:333-344, Sphere.cpp:273-276, Disk.cpp:298-306,
 * Cylinder.cpp:272-279) restated from the flattened object.  1 and the box, 0 for
 * a record kind (TGHIP_REC_*) whose bounds are not restated. */
int tgh_leaf_bounds(const TgHipObject *object, uint32_t kind, float lo[3], float hi[3]);

/* What tghip_upload_scene decides about a description before it touches the device (csrc/host/SceneCheck.cpp), on its own, no device: TGHIP_OK, or the
 * upload's refusal -- its code (TGHIP_E_INVALID / TGHIP_E_UNSUPPORTED) and in `err` its message -- under the default options.  `out` (may be NULL)
 * receives the facts the launch code branches on: flags (0 / 1), the stack depths of the BVH2 and the wide BVH walks and their parts inside a master,
 * the shading classes present among the records and the BSDF types inside each, the quad hoisted out of the wide walks and the environment map
 * whose marginal tables ride in LDS (-1: none). */
typedef struct TgHostSceneTraits {
    int32_t  have_media, have_instances, have_mesh_light, have_forward, have_solids, all_features_shading, have_proc_tex;
    int32_t  lean_scene, media_simple, thinlens, camera_fix, have_complex, top_tree, tables_fit;
    int32_t  bvh_depth, bvh_master_depth, wide_depth, wide_master_depth;
    int32_t  class_present[4];
    uint32_t class_mask[4], complex_mask;
    int32_t  hoisted_rec, env_tex;
    int32_t  have_fibre;      /* the bsdf table holds a fibre BCSDF (TGHIP_BSDF_LAMBERTIAN_FIBER / _ROUGH_WIRE): steers where have_proc_tex steers */
} TgHostSceneTraits;
int tgh_scene_check(const TgHipSceneDesc *scene, TgHostSceneTraits *out /* may be NULL */, char *err, size_t errlen);
/* What tghip_debug_light_info answers (tungsten_hip.h), on its own, no device: per slot of scene->lights the feature bits the light's code needs
 * (csrc/host/SceneCheck.cpp: lightNeeds) and whether the mask of shading family `variant` (TGHIP_BSDF_VARIANT_*, without the Sobol' sampler's bit) holds
 * them; variant_mask: that mask.  Any output pointer may be NULL.  TGHIP_E_INVALID for no scene, an unknown variant or a description tgh_scene_check refuses. */
int tgh_light_needs(const TgHipSceneDesc *scene, int variant, uint32_t *needs, uint32_t *covered, uint32_t *variant_mask);
/* What tghip_debug_medium decides about a call before it launches anything (tungsten_hip.h), on its own, no device: TGHIP_OK, or TGHIP_E_INVALID with
 * the refusal in err (csrc/host/SceneCheck.cpp: checkMediumCases).  Also TGHIP_E_INVALID for no scene or a description tgh_scene_check refuses. */
int tgh_medium_cases_check(const TgHipSceneDesc *scene, const TgHipMediumCase *cases, const TgHipMediumResult *results, size_t n, char *err, size_t errlen);

/* Which kernels a pass runs on a scene (csrc/host/LaunchChoice.cpp), on its own, no device: the choice tghip_wait makes for a pass with the flags `pass_flags`
 * (TGHIP_PASS_*), short or not (TgHostPassPlan::short_batch), under the options keys[i] = values[i] (tghip_set_option's keys; "count_traversal" among them)
 * over the defaults.  Kernels are named in one canonical spelling -- every template argument, no blanks, masks as the decimal numbers of
 * csrc/hip/pt_variants.h: k_trace_closest_wide<false,false,false,true> --; a launch that does not happen has an empty name.  lds_formula: 0 none, 1 the BVH2
 * walks' stack over the queue, 2 the dynamic-fetch walks' queue + stack, 3 the wide walks' queue + group stack, 4 k_trace_closest_instw's.  A workgroup size is
 * `fixed_threads`, or (0) the largest multiple of 64 from max_threads down at which blocks_per_cu workgroups of `sized_by` are resident.  TGHIP_E_INVALID for
 * no scene or no `out`, an option the choice does not read, or a description tgh_scene_check refuses.
 * TGH_CHOICE_RAY_PATHS in pass_flags: the choice for the pass of a tghip_query_radiance call, whose paths start on the caller's rays -- a flag of this
 * question only, never of a TgHipPassDesc.  It behaves as the equirectangular and cubemap cameras do (camera_fix): no fused_flat / one_launch, no
 * fold_finish, no tail, camera_rays with the name k_query_paths. */
#define TGH_CHOICE_RAY_PATHS 0x40000000u
int tgh_launch_choice(const TgHipSceneDesc *scene, const char *const *keys, const long long *values, uint32_t num_options,
                      uint32_t pass_flags, int short_batch, TgHipLaunchChoice *out /* tungsten_hip.h */, char *err, size_t errlen);

/* What tghip_render_pass and tghip_wait decide about a pass before they touch the device (csrc/host/PassPlan.cpp), on its own, no device: the plan of
 * `pass` for a width x height image under the options "max_items", "max_slots" and "chunk_samples" -- or NULL, in *rc (may be NULL) the refusal's code
 * (TGHIP_E_INVALID from the checks of tghip_render_pass, TGHIP_E_UNSUPPORTED for a pass past 2^32 samples or items) and in `err` its message.
 * scene_has_sobol: whether the scene the pass is meant for carries sobol_matrices.  The arrays belong to the plan and live until tgh_pass_plan_free. */
typedef struct TgHostPassPlan {
    uint32_t empty;                                   /* 1: nothing to render (no owned tile, or no sample); the fields from `chunk` on are then 0 */
    uint32_t tiles_x, tiles_y, num_tiles;
    uint32_t shard_count, shard_skew, owned_tiles;
    uint32_t record_pass, variance_w, num_records;    /* TGHIP_PASS_RECORDS; records per row; records */
    uint32_t spp, spp_begin;                          /* the sample range the batches cut (record passes: [0, largest count of an owned record)) */
    uint32_t aux_pass;
    uint32_t chunk, group, chunks_all;                /* samples per work item; chunks k_resolve adds up together; chunks of the whole range */
    uint32_t short_batch;                             /* 2*batch_items <= max_slots */
    uint32_t reserved;
    uint64_t lum_floats;                              /* record passes: 16 x count floats per owned record */
    uint64_t record_items, hint_entries;              /* record passes: items of the gap-free enumeration; entries of the device's hint table */
    uint64_t total_items, batch_items;                /* of the whole pass; of its largest batch */
} TgHostPassPlan;
/* what differs between the batches of one pass (PassParams of the same names) */
typedef struct TgHostPassBatch { uint32_t spp_begin, spp_end, chunks, pix_slots, total_items, first_tile, item_base; } TgHostPassBatch;
typedef struct tgh_pass_plan tgh_pass_plan;
tgh_pass_plan *tgh_pass_plan_create(const TgHipPassDesc *pass, uint32_t width, uint32_t height, int scene_has_sobol,
                                    uint64_t max_items, uint64_t max_slots, uint32_t chunk_samples, int *rc, char *err, size_t errlen);
void tgh_pass_plan_info(tgh_pass_plan *p, TgHostPassPlan *out);
const TgHostPassBatch *tgh_pass_plan_batches(tgh_pass_plan *p, uint32_t *num_batches);
const uint32_t *tgh_pass_plan_owned_tiles(tgh_pass_plan *p, uint32_t *n);    /* the shard's tiles, row-major; NULL / 0 for an unsharded pass (it owns every tile) */
/* record passes (else NULL / 0): per record its first sample index, its samples per pixel, the offset of its luminance block (num_records entries each) */
const uint32_t *tgh_pass_plan_rec_index(tgh_pass_plan *p);
const uint32_t *tgh_pass_plan_rec_count(tgh_pass_plan *p);
const uint32_t *tgh_pass_plan_rec_lum(tgh_pass_plan *p);
/* ... the owned records with a count above 0 by descending count, ties in record order; the first item of every chunk of that order, the item total and
 * the sentinel 0xFFFFFFFF behind them (chunks_all + 2 entries).  An empty plan has neither. */
const uint32_t *tgh_pass_plan_sorted(tgh_pass_plan *p, uint32_t *n);
const uint32_t *tgh_pass_plan_chunk_starts(tgh_pass_plan *p, uint32_t *n);
void tgh_pass_plan_free(tgh_pass_plan *p);

/* What tghip_query_rays decides about a call before it touches the device (csrc/host/RayQuery.cpp), on its own, no device and no scene: TGHIP_OK, or
 * TGHIP_E_INVALID and in `err` the refusal's message.  Only the pointers' values are looked at, nothing is read through them. */
int tgh_query_rays_check(const TgHipRayQueryDesc *desc, const void *rays, const void *out, size_t n, char *err, size_t errlen);

/* What tghip_query_radiance decides about a call before it touches the device (csrc/host/RadianceQuery.cpp), on its own, no device and no scene:
 * TGHIP_OK, or the call's refusal -- TGHIP_E_INVALID, or TGHIP_E_UNSUPPORTED for n (spp_end - spp_begin) >= 2^32 samples -- and in `err` its message.
 * scene_has_sobol: whether the scene the call is meant for carries sobol_matrices.  Only the pointers' values are looked at, nothing is read through them. */
int tgh_query_radiance_check(const TgHipRadianceQueryDesc *desc, const void *rays, const void *rgb_sum, const void *count, size_t n, int scene_has_sobol,
                             char *err, size_t errlen);

/* What tghip_query_surface decides about a call before it touches the device (csrc/host/SurfaceQuery.cpp), on its own, no device and no scene: TGHIP_OK,
 * or TGHIP_E_INVALID and in `err` the refusal's message.  Only the pointers' values are looked at, nothing is read through them. */
int tgh_query_surface_check(const TgHipSurfaceQueryDesc *desc, const void *rays, const void *out, size_t n, char *err, size_t errlen);

/* What tghip_query_transmittance decides about a call before it touches the device (csrc/host/TransmittanceQuery.cpp), on its own, no device: TGHIP_OK,
 * or TGHIP_E_INVALID and in `err` the refusal's message.  `scene`: what the refusals that depend on the uploaded scene read -- per entry of media[]
 * whether it is an operand of an `interpolated` medium (NULL: none is), per object its TGHIP_OBJ_* type; NULL checks a call against a scene without
 * media and without objects.  Only the pointers' values of rays, media and out are looked at, nothing is read through them. */
typedef struct TgHostTransmittanceScene {
    uint32_t num_media;   const uint8_t *medium_operand;   /* num_media bytes, or NULL */
    uint32_t num_objects; const int32_t *object_type;      /* num_objects words */
} TgHostTransmittanceScene;
int tgh_query_transmittance_check(const TgHipTransmittanceQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n,
                                  const TgHostTransmittanceScene *scene, char *err, size_t errlen);

/* What tghip_query_direct decides about a call before it touches the device (csrc/host/DirectQuery.cpp), on its own, no device: TGHIP_OK, or the
 * call's refusal -- TGHIP_E_INVALID, or TGHIP_E_UNSUPPORTED for n (spp_end - spp_begin) >= 2^32 items -- and in `err` its message.  `scene`: what the
 * refusals that depend on the uploaded scene read -- per entry of media[] whether it is an operand of an `interpolated` medium (NULL: none is), the
 * number of sampled lights, the medium the camera is in (-1: none); NULL checks a call against a scene without media and lights.  Only the pointers'
 * values of rays, media and out are looked at, nothing is read through them. */
typedef struct TgHostDirectScene {
    uint32_t num_media;   const uint8_t *medium_operand;   /* num_media bytes, or NULL */
    uint32_t num_lights;
    int32_t  camera_medium;
} TgHostDirectScene;
int tgh_query_direct_check(const TgHipDirectQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n,
                           const TgHostDirectScene *scene, char *err, size_t errlen);

/* What tghip_query_vertex decides about a call before it touches the device (csrc/host/VertexQuery.cpp), on its own, no device: TGHIP_OK, or
 * TGHIP_E_INVALID and in `err` the refusal's message.  `scene`: what the refusals that depend on the uploaded scene read -- per entry of media[] whether
 * it is an operand of an `interpolated` medium (NULL: none is); NULL checks a call against a scene without media.  Only the pointers' values of rays,
 * media, paths and alive are looked at, nothing is read through them. */
typedef struct TgHostVertexScene {
    uint32_t num_media;   const uint8_t *medium_operand;   /* num_media bytes, or NULL */
} TgHostVertexScene;
int tgh_query_vertex_check(const TgHipVertexQueryDesc *desc, const void *rays, const void *media, const void *paths, const void *alive, size_t n,
                           const TgHostVertexScene *scene, char *err, size_t errlen);

/* file-format helpers used by the tests */
int tgh_save_pfm(const char *path, const float *rgb, int w, int h);
int tgh_load_hdr(const char *path, float *rgb /* may be NULL to query size */, int *w, int *h);

#ifdef __cplusplus
}
#endif
#endif
