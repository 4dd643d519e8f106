"""ctypes mirror of include/tungsten_hip.h and include/tungsten_host.h.

This module only *describes* the C-ABI (struct layouts, prototypes) and loads the in-tree shared
library built by ``__graft_entry__.build()`` / ``make``.  There is no Python or CPU fallback for
any compute entry point: if the library is missing, importing :mod:`tungsten_amd` fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtungsten_hip.so")

f32, i32, u32, i64, u64 = C.c_float, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64


class TgHipBvhNode(C.Structure):
    _fields_ = [("lo0", f32*3), ("hi0", f32*3), ("lo1", f32*3), ("hi1", f32*3),
                ("child0", i32), ("child1", i32), ("pad", u32*2)]


class TgHipWideNode(C.Structure):
    _fields_ = [("origin", f32*3), ("exp", C.c_uint8*3), ("imask", C.c_uint8), ("child_base", u32), ("rec_base", u32),
                ("leaf_valid", u32), ("reserved", u32), ("qlo", (C.c_uint8*8)*3), ("qhi", (C.c_uint8*8)*3)]


class TgHipPrimRec(C.Structure):
    _fields_ = [("a", f32*3), ("meta", u32), ("b", f32*3), ("p0", f32), ("c", f32*3), ("p1", f32)]


class TgHipTriAttr(C.Structure):
    _fields_ = [("n0", f32*3), ("n1", f32*3), ("n2", f32*3), ("uv0", f32*2), ("uv1", f32*2), ("uv2", f32*2),
                ("bsdf", i32)]


class TgHipObject(C.Structure):
    _fields_ = [("type", i32), ("bsdf", i32), ("emission", i32), ("light", i32), ("flags", u32),
                ("area", f32), ("inv_area", f32), ("first_light_tri", i32),
                ("base", f32*3), ("edge0", f32*3), ("edge1", f32*3), ("normal", f32*3), ("inv_uv_sq", f32*2),
                ("pos", f32*3), ("scale", f32*3), ("rot", f32*9), ("face_cdf", f32*3), ("num_light_tris", i32), ("int_medium", i32), ("ext_medium", i32)]


class TgHipBsdf(C.Structure):
    _fields_ = [("type", i32), ("lobes", u32), ("albedo", i32), ("distribution", i32), ("roughness", i32),
                ("sub0", i32), ("sub1", i32), ("tex1", i32),
                ("ior", f32), ("thickness", f32), ("avg_transmittance", f32), ("diffuse_fresnel", f32),
                ("enable_refraction", i32), ("eta", f32*3), ("k", f32*3), ("sigma_a", f32*3),
                ("scaled_sigma_a", f32*3), ("bump1", i32), ("pad", f32)]


class TgHipTexture(C.Structure):
    _fields_ = [("type", i32), ("flags", u32), ("w", i32), ("h", i32), ("value", f32*3), ("scale", f32),
                ("on_color", f32*3), ("res_u", i32), ("off_color", f32*3), ("res_v", i32),
                ("avg", f32*3), ("pad", f32), ("texel_offset", i64), ("dist_offset", i64)]


# TgHipTexture.type (an `ies` texture is baked by the host and arrives as TGHIP_TEX_BITMAP)
(TGHIP_TEX_CONSTANT, TGHIP_TEX_CHECKER, TGHIP_TEX_BITMAP, TGHIP_TEX_DISK, TGHIP_TEX_BLADE) = range(5)
(TGHIP_TEXF_LINEAR, TGHIP_TEXF_CLAMP, TGHIP_TEXF_RGB, TGHIP_TEXF_VALID) = (1, 2, 4, 8)    # TgHipTexture.flags


class TgHipMedium(C.Structure):
    _fields_ = [("sigma_a", f32*3), ("sigma_s", f32*3), ("sigma_t", f32*3), ("absorption_only", i32), ("max_bounce", i32),
                ("phase_type", i32), ("phase_g", f32), ("trans_type", i32), ("trans_p", f32*3),
                ("medium_type", i32), ("falloff_scale", f32), ("unit_point", f32*3), ("falloff_dir", f32*3), ("pad", f32*3)]


class TgHipCamera(C.Structure):
    _fields_ = [("pos", f32*3), ("plane_dist", f32), ("xf", f32*9), ("ratio", f32), ("pixel_size_x", f32),
                ("res_x", i32), ("res_y", i32), ("filter_type", i32), ("filter_width", f32),
                ("filter_bin_size", f32), ("filter_cdf", f32*32),
                ("type", i32), ("focus_dist", f32), ("aperture_size", f32), ("cat_eye", f32), ("inv_xf", f32*12), ("medium", i32),
                ("aperture_type", i32), ("blade_count", i32), ("blade_angle", f32), ("blade_step", f32), ("blade_edge", f32*2),
                ("aperture_w", i32), ("aperture_h", i32), ("aperture_dist", u32)]


# TgHipCamera.aperture_type (3 is no aperture; a checker: aperture_w / aperture_h = res_u / res_v, blade_edge = the two colours' maxima)
(TGHIP_APERTURE_DISK, TGHIP_APERTURE_BLADE, TGHIP_APERTURE_BITMAP) = range(3)
(TGHIP_APERTURE_CONSTANT, TGHIP_APERTURE_CHECKER) = (4, 5)


class TgHipSettings(C.Structure):
    _fields_ = [("min_bounces", i32), ("max_bounces", i32), ("enable_light_sampling", i32),
                ("enable_two_sided_shading", i32), ("enable_consistency_checks", i32), ("enable_volume_light_sampling", i32), ("pad", i32*2)]


class TgHipTopNode(C.Structure):
    _fields_ = [("lower", (f32*3)*4), ("upper", (f32*3)*4), ("child", i32*4)]


TGHIP_TOP_EMPTY = 0x7FFFFFFF


class TgHipSceneDesc(C.Structure):
    _fields_ = [("abi_version", u32), ("num_nodes", u32), ("num_recs", u32), ("num_objects", u32),
                ("num_lights", u32), ("num_infinite_lights", u32), ("num_bsdfs", u32), ("num_textures", u32),
                ("nodes", C.POINTER(TgHipBvhNode)), ("recs", C.POINTER(TgHipPrimRec)),
                ("tri_attrs", C.POINTER(TgHipTriAttr)), ("objects", C.POINTER(TgHipObject)),
                ("lights", C.POINTER(i32)), ("infinite_lights", C.POINTER(i32)),
                ("bsdfs", C.POINTER(TgHipBsdf)), ("textures", C.POINTER(TgHipTexture)),
                ("texels", C.POINTER(f32)), ("num_texel_floats", u64),
                ("dist", C.POINTER(f32)), ("num_dist_floats", u64),
                ("light_tris", C.POINTER(f32)), ("num_light_tri_floats", u64),
                ("sobol_matrices", C.POINTER(u32)), ("num_sobol_words", u64),
                ("num_instances", u32), ("num_top_recs", u32),
                ("inst_prims", C.POINTER(u32)), ("num_inst_prims", u32),
                ("inst_leaf_boxes", C.POINTER(f32)), ("inst_tight_boxes", C.POINTER(f32)),
                ("media", C.POINTER(TgHipMedium)), ("num_media", u32),
                ("wide_nodes", C.POINTER(TgHipWideNode)), ("num_wide_nodes", u32),
                ("top_nodes", C.POINTER(TgHipTopNode)), ("num_top_nodes", u32),
                ("camera", TgHipCamera), ("settings", TgHipSettings),
                ("bounds_lo", f32*3), ("bounds_hi", f32*3)]


(TGHIP_OK, TGHIP_E_INVALID, TGHIP_E_NODEVICE, TGHIP_E_HIP, TGHIP_E_NOSCENE, TGHIP_E_ABORTED, TGHIP_E_UNSUPPORTED) = (0, -1, -2, -3, -4, -5, -6)
TGHIP_PASS_SOBOL, TGHIP_PASS_RECORDS, TGHIP_PASS_AUX, TGHIP_PASS_SAMPLES = 1, 2, 4, 8
(TGHIP_LIBM_SINF, TGHIP_LIBM_COSF, TGHIP_LIBM_LOGF, TGHIP_LIBM_EXPF, TGHIP_LIBM_SINCOS_SIN, TGHIP_LIBM_SINCOS_COS,
 TGHIP_LIBM_ACOSF, TGHIP_LIBM_ATAN2F, TGHIP_LIBM_POWF, TGHIP_LIBM_CBRTF, TGHIP_LIBM_EMBREE_RCP, TGHIP_LIBM_RCPPS, TGHIP_LIBM_TANF,
 TGHIP_LIBM_EXPD, TGHIP_LIBM_LOGD, TGHIP_LIBM_ERFD, TGHIP_LIBM_SQRTD, TGHIP_LIBM_SINHF) = range(18)


class TgHipAuxPixel(C.Structure):
    _fields_ = [("a", f32*11), ("b", f32*11), ("variance", f32*11), ("count", u32*5)]


(TGHIP_TONEMAP_LINEAR, TGHIP_TONEMAP_GAMMA, TGHIP_TONEMAP_REINHARD, TGHIP_TONEMAP_FILMIC, TGHIP_TONEMAP_PBRT) = range(5)
TGHIP_DEVELOP_MEAN, TGHIP_DEVELOP_A, TGHIP_DEVELOP_B, TGHIP_DEVELOP_VARIANCE = range(4)
TGHIP_DEVELOP_FRAME = 0xFFFFFFFF
TGHIP_DEVELOP_DEVICE_POINTERS = 1
(TGHIP_AUX_COLOR, TGHIP_AUX_DEPTH, TGHIP_AUX_NORMAL, TGHIP_AUX_ALBEDO, TGHIP_AUX_VISIBILITY) = range(5)
TGHIP_AUX_CHANNEL_COUNT = (3, 1, 3, 3, 1)


class TgHipDevelopDesc(C.Structure):
    _fields_ = [("source", u32), ("part", u32), ("tonemap", u32), ("flags", u32)]


TGHIP_NLMEANS_POINTERS = 0xFFFFFFFF


class TgHipNlMeansDesc(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("channels", u32), ("F", u32), ("R", u32), ("k", f32), ("variance_scale", f32),
                ("source", u32), ("image_part", u32), ("guide_part", u32), ("flags", u32)]


(TGHIP_BSDF_VARIANT_LEAN, TGHIP_BSDF_VARIANT_SIMPLE, TGHIP_BSDF_VARIANT_COAT, TGHIP_BSDF_VARIANT_GLASS, TGHIP_BSDF_VARIANT_PLASTIC,
 TGHIP_BSDF_VARIANT_MEDIA, TGHIP_BSDF_VARIANT_TAIL, TGHIP_BSDF_VARIANT_FULL, TGHIP_BSDF_VARIANT_ALL, TGHIP_BSDF_VARIANT_COUNT) = range(10)
TGHIP_BSDF_VARIANT_NAMES = ("lean", "simple", "coat", "glass", "plastic", "media", "tail", "full", "all")


class TgHipBsdfCase(C.Structure):
    _fields_ = [("bsdf", i32), ("requested", u32), ("wi", f32*3), ("wo", f32*3), ("uv", f32*2), ("seed", u32), ("stream", u32),
                ("variant", u32), ("reserved", u32)]


class TgHipBsdfResult(C.Structure):
    _fields_ = [("f", f32*3), ("pdf", f32), ("sample_ok", u32), ("sample_wo", f32*3), ("sample_weight", f32*3), ("sample_pdf", f32),
                ("sampled", u32), ("next", f32), ("reserved", u32*2)]


class TgHipLightCase(C.Structure):
    _fields_ = [("light", i32), ("variant", u32), ("p", f32*3), ("w", f32*3), ("seed", u32), ("stream", u32)]


class TgHipLightResult(C.Structure):
    _fields_ = [("chosen", i32), ("choose_weight", f32), ("sample_ok", u32), ("d", f32*3), ("dist", f32), ("pdf", f32), ("approx", f32),
                ("hit", u32), ("t", f32), ("u", f32), ("v", f32), ("back_side", u32), ("emission", f32*3), ("direct_pdf", f32),
                ("choose_next", f32), ("sample_next", f32), ("reserved", u32*4)]


class TgHipMediumCase(C.Structure):
    _fields_ = [("medium", i32), ("variant", u32), ("seed", u32), ("stream", u32), ("state_bounce", u32), ("p", f32*3), ("d", f32*3), ("max_t", f32),
                ("wo", f32*3), ("reserved", u32)]


class TgHipMediumResult(C.Structure):
    _fields_ = [("ok", u32), ("t", f32), ("weight", f32*3), ("exited", u32), ("bounce_after", u32), ("tr", (f32*3)*4), ("phase_f", f32), ("w", f32*3),
                ("phase_pdf", f32), ("dist_next", f32), ("phase_next", f32), ("reserved", u32*2)]


class TgHipPassDesc(C.Structure):
    _fields_ = [("spp_begin", u32), ("spp_end", u32), ("seed", u32), ("shard_index", u32), ("shard_count", u32),
                ("flags", u32),
                ("tile_seeds", C.POINTER(u32)), ("record_index", C.POINTER(u32)), ("record_count", C.POINTER(u32))]


class TgHipSampleRecord(C.Structure):
    _fields_ = [("sample_count", u32), ("mean", f32), ("running_variance", f32)]


class TgHostSampleRecord(C.Structure):
    _fields_ = [("sample_count", u32), ("next_sample_count", u32), ("sample_index", u32),
                ("adaptive_weight", f32), ("mean", f32), ("running_variance", f32)]


class TgHipCounters(C.Structure):
    _fields_ = [("samples", u64), ("closest_rays", u64), ("shadow_rays", u64), ("nodes_visited", u64),
                ("prims_tested", u64), ("iterations", u64),
                ("ms_trace_closest", C.c_double), ("ms_trace_shadow", C.c_double), ("ms_shade", C.c_double),
                ("ms_other", C.c_double), ("ms_total", C.c_double),
                ("launches_trace_closest", u64), ("launches_trace_shadow", u64), ("launches_shade", u64),
                ("nodes_visited_shadow", u64), ("prims_tested_shadow", u64), ("shadow_slots", u64), ("tail_launches", u64)]


class TgHipRay(C.Structure):
    _fields_ = [("o", f32*3), ("tmin", f32), ("d", f32*3), ("tmax", f32)]


class TgHipHit(C.Structure):
    _fields_ = [("t", f32), ("u", f32), ("v", f32), ("rec", i32)]


TGHIP_QUERY_CLOSEST, TGHIP_QUERY_OCCLUDED = 0, 1


class TgHipRayQueryDesc(C.Structure):
    _fields_ = [("mode", u32), ("flags", u32), ("reserved", u32*2)]


TGHIP_RADIANCE_SOBOL = 2
TGH_CHOICE_RAY_PATHS = 0x40000000      # tgh_launch_choice's pass_flags: the choice for a tghip_query_radiance call


class TgHipRadianceQueryDesc(C.Structure):
    _fields_ = [("flags", u32), ("seed", u32), ("spp_begin", u32), ("spp_end", u32), ("sobol_seed", u32), ("reserved", u32*3)]


TGHIP_SURFACE_HIT, TGHIP_SURFACE_BACK_SIDE, TGHIP_SURFACE_EMISSIVE, TGHIP_SURFACE_INFINITE = 1, 2, 4, 8


class TgHipSurface(C.Structure):
    _fields_ = [("p", f32*3), ("t", f32), ("ng", f32*3), ("rec", i32), ("ns", f32*3), ("instance", i32), ("uv", f32*2), ("object", i32), ("bsdf", i32),
                ("albedo", f32*3), ("flags", u32), ("emission", f32*3), ("reserved", u32)]


class TgHipSurfaceQueryDesc(C.Structure):
    _fields_ = [("flags", u32), ("reserved", u32*3)]


# TgHipObject::type
(TGHIP_OBJ_MESH, TGHIP_OBJ_QUAD, TGHIP_OBJ_CUBE, TGHIP_OBJ_SPHERE, TGHIP_OBJ_INFINITE_SPHERE, TGHIP_OBJ_INSTANCES, TGHIP_OBJ_DISK,
 TGHIP_OBJ_INFINITE_SPHERE_CAP, TGHIP_OBJ_POINT, TGHIP_OBJ_CYLINDER) = range(10)
TGHIP_TRANSMITTANCE_STARTS_ON_SURFACE, TGHIP_TRANSMITTANCE_ENDS_ON_SURFACE = 2, 4
TGHIP_MEDIUM_NONE, TGHIP_MEDIUM_OF_CAMERA = -1, -2


class TgHipTransmittanceQueryDesc(C.Structure):
    _fields_ = [("flags", u32), ("medium", i32), ("end_cap", i32), ("bounce", u32), ("reserved", u32*4)]


class TgHipTransmittance(C.Structure):
    _fields_ = [("rgb", f32*3), ("crossed", u32)]


class TgHostTransmittanceScene(C.Structure):
    _fields_ = [("num_media", u32), ("medium_operand", C.POINTER(C.c_uint8)), ("num_objects", u32), ("object_type", C.POINTER(i32))]


TGHIP_DIRECT_VOLUME = 2


class TgHipDirectQueryDesc(C.Structure):
    _fields_ = [("flags", u32), ("seed", u32), ("spp_begin", u32), ("spp_end", u32), ("medium", i32), ("bounce", u32), ("light", i32), ("skip", u32)]


class TgHipDirect(C.Structure):
    _fields_ = [("rgb", f32*3), ("visibility", f32), ("count", u32), ("visibility_count", u32), ("rec", i32), ("reserved", u32)]


class TgHostDirectScene(C.Structure):
    _fields_ = [("num_media", u32), ("medium_operand", C.POINTER(C.c_uint8)), ("num_lights", u32), ("camera_medium", i32)]


TGHIP_VERTEX_START = 2
# TgHipPath::status
(TGHIP_PATH_ALIVE, TGHIP_PATH_END_ESCAPED, TGHIP_PATH_END_MAX_BOUNCES, TGHIP_PATH_END_ABSORBED, TGHIP_PATH_END_ZERO_THROUGHPUT, TGHIP_PATH_END_ROULETTE,
 TGHIP_PATH_END_NAN) = range(7)
TGHIP_PATH_WAS_SPECULAR = 1


class TgHipVertexQueryDesc(C.Structure):
    _fields_ = [("flags", u32), ("seed", u32), ("sample", u32), ("first_index", u32), ("first_number", u32), ("medium", i32), ("turns", u32), ("reserved", u32)]


class TgHipPath(C.Structure):
    _fields_ = [("o", f32*3), ("tmin", f32), ("d", f32*3), ("tmax", f32), ("throughput", f32*3), ("emission", f32*3), ("status", u32), ("medium", i32),
                ("medium_state_bounce", u32), ("bounce", u32), ("flags", u32), ("rec", i32), ("t", f32), ("rng_state", u32*2), ("key", u32),
                ("drawn", u32), ("reserved", u32*3)]


class TgHostVertexScene(C.Structure):
    _fields_ = [("num_media", u32), ("medium_operand", C.POINTER(C.c_uint8))]


class TgHostSceneInfo(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("spp", u32), ("spp_step", u32),
                ("num_nodes", u32), ("num_recs", u32), ("num_objects", u32), ("num_lights", u32),
                ("num_bsdfs", u32), ("num_textures", u32), ("bvh_depth", i32),
                ("bvh_sah_cost", C.c_double), ("build_seconds", C.c_double),
                ("adaptive_sampling", i32), ("stratified_sampler", i32), ("current_spp", u32)]


class TgHostSceneTraits(C.Structure):
    _fields_ = [(n, i32) for n in ("have_media", "have_instances", "have_mesh_light", "have_forward", "have_solids", "all_features_shading", "have_proc_tex",
                                   "lean_scene", "media_simple", "thinlens", "camera_fix", "have_complex", "top_tree", "tables_fit",
                                   "bvh_depth", "bvh_master_depth", "wide_depth", "wide_master_depth")] + \
               [("class_present", i32*4), ("class_mask", u32*4), ("complex_mask", u32), ("hoisted_rec", i32), ("env_tex", i32), ("have_fibre", i32)]


class TgHostPassPlan(C.Structure):
    _fields_ = [(n, u32) for n in ("empty", "tiles_x", "tiles_y", "num_tiles", "shard_count", "shard_skew", "owned_tiles",
                                   "record_pass", "variance_w", "num_records", "spp", "spp_begin", "aux_pass",
                                   "chunk", "group", "chunks_all", "short_batch", "reserved")] + \
               [(n, u64) for n in ("lum_floats", "record_items", "hint_entries", "total_items", "batch_items")]


class TgHostPassBatch(C.Structure):
    _fields_ = [(n, u32) for n in ("spp_begin", "spp_end", "chunks", "pix_slots", "total_items", "first_tile", "item_base")]


TGHIP_KERNEL_NAME_LEN = 80
_NAME = C.c_char*TGHIP_KERNEL_NAME_LEN


class TgHipWalkLaunch(C.Structure):
    _fields_ = [("name", _NAME), ("sized_by", _NAME)] + [(n, i32) for n in ("lds_formula", "sized_lds_formula", "max_threads", "fixed_threads")]


class TgHipShadeLaunch(C.Structure):
    _fields_ = [("name", _NAME), ("cls", i32), ("variant", i32), ("mask", u32), ("fuse", i32), ("global_tables", i32), ("size", i32), ("lane", i32)]


class TgHipShadeSize(C.Structure):
    _fields_ = [("sized_by", _NAME), ("max_threads", i32), ("fixed_threads", i32)]


class TgHipLaunchChoice(C.Structure):
    """Which kernels a pass runs on a scene (csrc/host/LaunchChoice.cpp; include/tungsten_host.h: tgh_launch_choice documents the fields)."""
    _fields_ = [(n, i32) for n in ("flat", "fused_flat", "one_launch", "paired", "paired_inst", "blocks_per_cu", "parts",
                                   "slot_cap", "order_regs_cap", "walk_arrays", "fold_finish", "nee_factors", "camera_rays", "tables_fit")] + \
               [("closest", TgHipWalkLaunch), ("shadow", TgHipWalkLaunch), ("num_shade", i32), ("fused_pair", i32), ("shade_launches", i32),
                ("shade", TgHipShadeLaunch*6), ("shade_size", TgHipShadeSize*3), ("tail_eligible", i32), ("reserved", i32),
                ("tail", _NAME), ("tail_probe", _NAME), ("camera_rays_name", _NAME), ("ray_walk", i32), ("reserved2", i32), ("trace_rays", _NAME)]

    def kernel_names(self):
        """The kernels an iteration of the pass launches, k_tail where the pass may end in it, and k_camera_rays: the names a kernel trace of a render shows
        (next to the fixed kernels around the loop: k_start, k_finish, k_resolve ...)."""
        names = [l.name for l in self.shade[:self.num_shade]] + [self.tail, self.camera_rays_name]
        if not self.fused_flat:
            names += [self.closest.name, self.shadow.name]
        return {n.decode() for n in names if n}


class TgHipLaunchPlan(C.Structure):
    _fields_ = [("choice", TgHipLaunchChoice), ("threads_closest", i32), ("threads_shadow", i32), ("threads_shade", i32*3), ("threads_tail", i32),
                ("lds_closest", u32), ("lds_shadow", u32), ("lds_tail", u32), ("grid", u32), ("parts", i32), ("tail_fits", i32)]


def launch_choice(lib, desc, options=(), pass_flags=0, short_batch=False):
    """tgh_launch_choice for the scene description `desc` under options = {key: value} (or pairs): the TgHipLaunchChoice, or ValueError with the refusal."""
    pairs = list(dict(options).items())
    keys = (C.c_char_p*max(len(pairs), 1))(*[k.encode() for k, _ in pairs])
    values = (C.c_longlong*max(len(pairs), 1))(*[int(v) for _, v in pairs])
    out, err = TgHipLaunchChoice(), C.create_string_buffer(512)
    if lib.tgh_launch_choice(desc, keys, values, len(pairs), int(pass_flags), int(bool(short_batch)), C.byref(out), err, len(err)) != 0:
        raise ValueError(err.value.decode(errors="replace"))
    return out


# every symbol the two headers declare: name -> (restype, argtypes)
VP = C.c_void_p
TGHIP_COMM_ID_BYTES = 128

PROTOTYPES = {
    # include/tungsten_hip.h
    "tghip_create": (VP, [C.c_int]),
    "tghip_destroy": (None, [VP]),
    "tghip_last_error": (C.c_char_p, [VP]),
    "tghip_device_count": (C.c_int, []),
    "tghip_upload_scene": (C.c_int, [VP, C.POINTER(TgHipSceneDesc)]),
    "tghip_render_pass": (C.c_int, [VP, C.POINTER(TgHipPassDesc)]),
    "tghip_wait": (C.c_int, [VP]),
    "tghip_abort": (C.c_int, [VP]),
    "tghip_clear_framebuffer": (C.c_int, [VP]),
    "tghip_bind_framebuffer": (C.c_int, [VP, VP, VP]),
    "tghip_download_framebuffer": (C.c_int, [VP, VP, VP, C.c_size_t]),
    "tghip_upload_framebuffer": (C.c_int, [VP, VP, VP, C.c_size_t]),
    "tghip_download_records": (C.c_int, [VP, VP, C.c_size_t]),
    "tghip_upload_records": (C.c_int, [VP, VP, C.c_size_t]),
    "tghip_download_aux": (C.c_int, [VP, VP, C.c_size_t]),
    "tghip_upload_aux": (C.c_int, [VP, VP, C.c_size_t]),
    "tghip_download_samples": (C.c_int, [VP, VP, C.c_size_t]),
    "tghip_develop": (C.c_int, [VP, C.POINTER(TgHipDevelopDesc), VP, VP, C.c_size_t]),
    "tghip_develop_kernel_time": (C.c_int, [VP, C.POINTER(C.c_double)]),
    "tghip_nlmeans": (C.c_int, [VP, C.POINTER(TgHipNlMeansDesc), VP, VP, VP, VP]),
    "tghip_nlmeans_kernel_time": (C.c_int, [VP, C.POINTER(C.c_double)]),
    "tghip_reduce_framebuffers": (C.c_int, [C.POINTER(VP), C.c_int, C.c_int, VP, VP, C.c_size_t]),
    "tghip_trace_rays": (C.c_int, [VP, VP, VP, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "tghip_query_rays": (C.c_int, [VP, C.POINTER(TgHipRayQueryDesc), VP, VP, C.c_size_t]),
    "tghip_query_rays_kernel_time": (C.c_int, [VP, C.POINTER(C.c_double)]),
    "tghip_query_radiance": (C.c_int, [VP, C.POINTER(TgHipRadianceQueryDesc), VP, VP, VP, C.c_size_t]),
    "tghip_query_radiance_kernel_time": (C.c_int, [VP, C.POINTER(C.c_double)]),
    "tghip_query_surface": (C.c_int, [VP, C.POINTER(TgHipSurfaceQueryDesc), VP, VP, C.c_size_t]),
    "tghip_query_surface_kernel_time": (C.c_int, [VP, C.POINTER(C.c_double)]),
    "tghip_query_transmittance": (C.c_int, [VP, C.POINTER(TgHipTransmittanceQueryDesc), VP, VP, VP, C.c_size_t]),
    "tghip_query_transmittance_kernel_time": (C.c_int, [VP, C.POINTER(C.c_double)]),
    "tghip_query_transmittance_rounds": (C.c_int, [VP, C.POINTER(C.c_uint32)]),
    "tghip_query_direct": (C.c_int, [VP, C.POINTER(TgHipDirectQueryDesc), VP, VP, VP, C.c_size_t]),
    "tghip_query_direct_kernel_time": (C.c_int, [VP, C.POINTER(C.c_double)]),
    "tghip_query_vertex": (C.c_int, [VP, C.POINTER(TgHipVertexQueryDesc), VP, VP, VP, C.c_size_t, VP]),
    "tghip_query_vertex_kernel_time": (C.c_int, [VP, C.POINTER(C.c_double)]),
    "tghip_debug_libm": (C.c_int, [VP, C.c_int, VP, VP, C.c_size_t]),
    "tghip_debug_bsdf": (C.c_int, [VP, VP, VP, C.c_size_t]),
    "tghip_debug_bsdf_info": (C.c_int, [VP, C.c_int, VP, VP, VP, VP]),
    "tghip_debug_light": (C.c_int, [VP, VP, VP, C.c_size_t]),
    "tghip_debug_light_info": (C.c_int, [VP, C.c_int, VP, VP, VP]),
    "tghip_debug_medium": (C.c_int, [VP, VP, VP, C.c_size_t]),
    "tghip_debug_launch_plan": (C.c_int, [VP, C.POINTER(TgHipPassDesc), C.POINTER(TgHipLaunchPlan)]),
    "tghip_set_option": (C.c_int, [VP, C.c_char_p, C.c_longlong]),
    "tghip_get_counters": (C.c_int, [VP, C.POINTER(TgHipCounters)]),
    "tghip_reset_counters": (C.c_int, [VP]),
    "tghip_comm_unique_id": (C.c_int, [VP, C.c_size_t]),
    "tghip_comm_init_rank": (C.c_int, [VP, VP, C.c_size_t, C.c_int, C.c_int]),
    "tghip_reduce_framebuffer_rank": (C.c_int, [VP, C.c_int, VP, VP, C.c_size_t]),
    "tghip_get_walk_stats": (C.c_int, [VP, C.c_int, C.POINTER(C.c_uint64), C.c_int]),
    # include/tungsten_host.h
    "tgh_scene_load": (VP, [C.c_char_p, C.c_char_p, C.c_size_t]),
    "tgh_scene_desc": (C.POINTER(TgHipSceneDesc), [VP]),
    "tgh_scene_info": (C.c_int, [VP, C.POINTER(TgHostSceneInfo)]),
    "tgh_scene_free": (None, [VP]),
    "tgh_renderer_open": (VP, [C.c_char_p, u32, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "tgh_renderer_context": (VP, [VP, C.c_int]),
    "tgh_renderer_info": (C.c_int, [VP, C.POINTER(TgHostSceneInfo)]),
    "tgh_renderer_step": (C.c_int, [VP, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "tgh_renderer_render": (C.c_int, [VP, C.POINTER(C.c_double), C.c_char_p, C.c_size_t]),
    "tgh_renderer_image": (C.c_int, [VP, VP, VP, VP, C.c_size_t, C.c_char_p, C.c_size_t]),
    "tgh_renderer_save_outputs": (C.c_int, [VP, C.c_char_p, C.c_size_t]),
    "tgh_renderer_close": (None, [VP]),
    "tgh_renderer_save_resume_data": (C.c_int, [VP, C.c_char_p, C.c_size_t]),
    "tgh_renderer_resume": (C.c_int, [VP, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "tgh_renderer_records": (C.c_int, [VP, VP, C.c_size_t, C.c_char_p, C.c_size_t]),
    "tgh_renderer_output_buffers": (C.c_int, [VP, VP, C.c_size_t, C.c_char_p, C.c_size_t]),
    "tgh_renderer_develop": (C.c_int, [VP, C.POINTER(TgHipDevelopDesc), VP, VP, C.c_size_t, C.c_char_p, C.c_size_t]),
    "tgh_renderer_tonemap": (C.c_int, [VP]),
    "tgh_develop_host_frame": (C.c_int, [VP, VP, C.c_size_t, u32, VP, VP]),
    "tgh_develop_host_aux": (C.c_int, [VP, C.c_size_t, u32, u32, VP, VP]),
    "tgh_nlmeans_host": (C.c_int, [C.POINTER(TgHipNlMeansDesc), VP, VP, VP, VP]),
    "tgh_scheduler_create": (VP, [u32, u32, u32]),
    "tgh_scheduler_num_tiles": (C.c_size_t, [VP]),
    "tgh_scheduler_num_records": (C.c_size_t, [VP]),
    "tgh_scheduler_tile_seeds": (C.POINTER(u32), [VP]),
    "tgh_scheduler_records": (C.POINTER(TgHostSampleRecord), [VP]),
    "tgh_scheduler_generate_work": (C.c_int, [VP, u32, u32, C.c_int]),
    "tgh_scheduler_sampler_state": (u64, [VP]),
    "tgh_scheduler_set_sampler_state": (None, [VP, u64]),
    "tgh_scheduler_free": (None, [VP]),
    "tgh_sobol_matrices": (C.POINTER(u32), [C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]),
    "tgh_accel_build": (VP, [VP, VP, VP, C.c_uint32, C.c_char_p, C.c_size_t]),
    "tgh_accel_nodes": (VP, [VP, C.POINTER(C.c_uint32)]),
    "tgh_accel_wide_nodes": (VP, [VP, C.POINTER(C.c_uint32)]),
    "tgh_accel_free": (None, [VP]),
    "tgh_accel_build_instanced": (VP, [VP, VP, VP, C.c_uint32, VP, C.c_uint32, VP, C.c_uint32, C.c_char_p, C.c_size_t]),
    "tgh_accel_recs": (VP, [VP, C.POINTER(C.c_uint32)]),
    "tgh_accel_tri_attrs": (VP, [VP]),
    "tgh_accel_inst_prims": (VP, [VP, C.POINTER(C.c_uint32)]),
    "tgh_accel_inst_leaf_boxes": (VP, [VP]),
    "tgh_accel_inst_tight_boxes": (VP, [VP]),
    "tgh_accel_counts": (None, [VP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "tgh_instance_tight_bounds": (None, [VP, C.c_uint32, C.c_uint32, VP, VP, VP, VP]),
    "tgh_scene_items": (C.c_uint32, [VP, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_int32))]),
    "tgh_top_tree_build": (C.c_int, [VP, C.c_uint32, VP, C.c_uint32]),
    "tgh_top_tree_for_scene": (C.c_int, [VP, C.c_uint32, VP, C.c_uint32, VP, C.c_uint32]),
    "tgh_leaf_bounds": (C.c_int, [VP, C.c_uint32, VP, VP]),
    "tgh_scene_check": (C.c_int, [C.POINTER(TgHipSceneDesc), C.POINTER(TgHostSceneTraits), C.c_char_p, C.c_size_t]),
    "tgh_light_needs": (C.c_int, [C.POINTER(TgHipSceneDesc), C.c_int, VP, VP, VP]),
    "tgh_medium_cases_check": (C.c_int, [C.POINTER(TgHipSceneDesc), VP, VP, C.c_size_t, C.c_char_p, C.c_size_t]),
    "tgh_launch_choice": (C.c_int, [C.POINTER(TgHipSceneDesc), C.POINTER(C.c_char_p), C.POINTER(C.c_longlong), u32, u32, C.c_int,
                                    C.POINTER(TgHipLaunchChoice), C.c_char_p, C.c_size_t]),
    "tgh_pass_plan_create": (VP, [C.POINTER(TgHipPassDesc), u32, u32, C.c_int, u64, u64, u32, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "tgh_pass_plan_info": (None, [VP, C.POINTER(TgHostPassPlan)]),
    "tgh_pass_plan_batches": (C.POINTER(TgHostPassBatch), [VP, C.POINTER(u32)]),
    "tgh_pass_plan_owned_tiles": (C.POINTER(u32), [VP, C.POINTER(u32)]),
    "tgh_pass_plan_rec_index": (C.POINTER(u32), [VP]),
    "tgh_pass_plan_rec_count": (C.POINTER(u32), [VP]),
    "tgh_pass_plan_rec_lum": (C.POINTER(u32), [VP]),
    "tgh_pass_plan_sorted": (C.POINTER(u32), [VP, C.POINTER(u32)]),
    "tgh_pass_plan_chunk_starts": (C.POINTER(u32), [VP, C.POINTER(u32)]),
    "tgh_pass_plan_free": (None, [VP]),
    "tgh_query_rays_check": (C.c_int, [C.POINTER(TgHipRayQueryDesc), VP, VP, C.c_size_t, C.c_char_p, C.c_size_t]),
    "tgh_query_radiance_check": (C.c_int, [C.POINTER(TgHipRadianceQueryDesc), VP, VP, VP, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]),
    "tgh_query_surface_check": (C.c_int, [C.POINTER(TgHipSurfaceQueryDesc), VP, VP, C.c_size_t, C.c_char_p, C.c_size_t]),
    "tgh_query_transmittance_check": (C.c_int, [C.POINTER(TgHipTransmittanceQueryDesc), VP, VP, VP, C.c_size_t, C.POINTER(TgHostTransmittanceScene),
                                                C.c_char_p, C.c_size_t]),
    "tgh_query_direct_check": (C.c_int, [C.POINTER(TgHipDirectQueryDesc), VP, VP, VP, C.c_size_t, C.POINTER(TgHostDirectScene), C.c_char_p, C.c_size_t]),
    "tgh_query_vertex_check": (C.c_int, [C.POINTER(TgHipVertexQueryDesc), VP, VP, VP, VP, C.c_size_t, C.POINTER(TgHostVertexScene), C.c_char_p, C.c_size_t]),
    "tgh_save_pfm": (C.c_int, [C.c_char_p, VP, C.c_int, C.c_int]),
    "tgh_load_hdr": (C.c_int, [C.c_char_p, VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
}


def bind(lib):
    """Attach restype/argtypes for every declared symbol; raises AttributeError on a missing export."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


def load_library(path=None):
    path = path or os.environ.get("TUNGSTEN_AMD_LIB", LIB_PATH)
    if not os.path.exists(path):
        raise ImportError(
            "tungsten_amd: native library %s not found. Build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make`). There is no Python/CPU fallback for the path tracer." % path)
    return bind(C.CDLL(path))
