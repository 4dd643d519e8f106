"""The host-side check of a scene description (tungsten_amd/csrc/host/SceneCheck.cpp, through tgh_scene_check): what tghip_upload_scene decides
before it touches the device -- every refusal, and the facts the launch code branches on.  No device.

The expected traits are stated from how each scene is made.  The expected refusals -- return code and a piece of the message -- are those of
tghip_upload_scene before the check moved out of it; one field of a valid description is changed at a time, on a copy.  (The record kind is the
top three bits of TgHipPrimRec::meta and all eight values are kinds, so "a kind above TGHIP_REC_INSTANCE_SET" cannot be written down; the case here
is a kind the scene cannot hold.)"""
import ctypes as C

import pytest

import scenes
import texture_cases
import tungsten_amd as tg
from tungsten_amd import capi

SIZE = dict(resolution=(32, 18), spp=1)
INVALID, UNSUPPORTED = capi.TGHIP_E_INVALID, capi.TGHIP_E_UNSUPPORTED


def _needs(name):
    if name == "water_caustic" and not scenes.have_water_caustic():
        pytest.skip("water-caustic assets (assets/) not present")
    if ("materialtest" in name or name == "mesh1m") and not scenes.have_materialtest():   # mesh1m is lit by materialtest's HDRI
        pytest.skip("materialtest assets (assets/) not present")


def check(desc):
    """(return code, traits, message) of tgh_scene_check."""
    traits = capi.TgHostSceneTraits()
    err = C.create_string_buffer(512)
    rc = tg.lib.tgh_scene_check(desc, C.byref(traits), err, len(err))
    return rc, traits, err.value.decode()


def _blob(tmp, **kw):
    """A 168-triangle mesh over one floor quad under an environment light: more than TGHIP_FLAT_MAX_RECS records, so it carries a wide BVH."""
    return scenes.mesh1m(tmp, n_lat=8, n_lon=12, **kw)


BASES = {
    "cornell": lambda t: scenes.cornell(t, **SIZE),
    "blob": lambda t: _blob(t, **SIZE),
    "fog": lambda t: scenes.cornell(t, edit=scenes._fog, **SIZE),
    "mesh_light": lambda t: scenes.cornell_mesh_light(t, **SIZE),
    "thinlens": lambda t: scenes.cornell(t, edit=scenes._thinlens(0.0), **SIZE),
    "thinlens_bitmap": lambda t: scenes.cornell_thinlens_bitmap(t, **SIZE),
    "equirectangular": lambda t: scenes.cornell(t, edit=scenes._equirectangular, **SIZE),
    "sobol": lambda t: scenes.cornell(t, renderer={"stratified_sampler": True}, **SIZE),
    "instances": lambda t: scenes.cornell_instances(t, **SIZE),
    "png": lambda t: scenes.cornell_png(t, **SIZE),
    "bump": lambda t: scenes.cornell_bump(t, **SIZE),
    "cylinders": lambda t: scenes.cornell(t, edit=scenes._cylinders, **SIZE),
    "blade": lambda t: texture_cases.build(t, edit=texture_cases._albedo, **SIZE),
    "materialtest": lambda t: scenes.materialtest(t, **SIZE),
}
_flattened = {}


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """name -> the flattened description of BASES[name], made once and left unchanged."""
    def get(name):
        if name not in _flattened:
            _flattened[name] = tg.FlattenedScene(BASES[name](tmp_path_factory.mktemp(name)))
        return _flattened[name].desc.contents
    yield get
    for flat in _flattened.values():
        flat.close()
    _flattened.clear()


@pytest.mark.parametrize("name", sorted(scenes.GOLDEN_CASES))
def test_every_golden_description_passes(name, tmp_path):
    """Nothing the loader makes is refused -- the two bounds checks on a bitmap's texels and distribution tables included."""
    _needs(name)
    mk, kw = scenes.GOLDEN_CASES[name]
    flat = tg.FlattenedScene(mk(tmp_path, **dict(kw, **SIZE)))
    rc, _, msg = check(flat.desc)
    flat.close()
    assert rc == 0, msg


def test_traits_of_the_cornell_box(base):
    d = base("cornell")
    rc, t, msg = check(d)
    assert rc == 0, msg
    # quads and cubes under one quad light, constant textures, lambert throughout: lean, a flat list (no wide BVH), class 0 only, and its top tree
    assert t.lean_scene == 1 and d.num_recs <= 16 and t.wide_depth == 0 and t.have_instances == 0
    assert list(t.class_present) == [1, 0, 0, 0] and t.have_complex == 0 and t.complex_mask == 0
    assert d.num_top_nodes > 0 and t.top_tree == 1
    assert (t.have_media, t.have_forward, t.have_mesh_light, t.all_features_shading, t.thinlens, t.camera_fix) == (0, 0, 0, 0, 0, 0)
    assert t.have_solids == 1 and t.hoisted_rec == -1 and t.env_tex == -1 and t.tables_fit == 1


def test_traits_of_materialtest(base):
    _needs("materialtest")
    rc, t, msg = check(base("materialtest"))
    assert rc == 0, msg
    # triangle meshes with a rough conductor next to lambert, lit by a sampled HDRI: not lean, classes 0 and 1, a wide BVH, the map's tables in LDS
    assert t.lean_scene == 0 and t.class_present[0] == 1 and t.class_present[1] == 1 and t.have_complex == 1
    assert t.wide_depth > 0 and t.bvh_depth > 0 and t.env_tex >= 0 and t.tables_fit == 1


def test_traits_of_the_other_scene_kinds(base):
    rc, t, msg = check(base("instances"))
    assert rc == 0 and t.have_instances == 1 and t.bvh_master_depth > 0 and t.wide_master_depth > 0 and t.hoisted_rec == -1, msg
    rc, t, msg = check(base("fog"))               # one homogeneous medium around lambert surfaces
    assert rc == 0 and t.have_media == 1 and t.media_simple == 1 and t.have_forward == 1 and t.lean_scene == 1, msg
    rc, t, msg = check(base("mesh_light"))
    assert rc == 0 and t.have_mesh_light == 1 and t.lean_scene == 0, msg
    rc, t, msg = check(base("thinlens"))
    assert rc == 0 and t.thinlens == 1 and t.camera_fix == 0, msg
    rc, t, msg = check(base("equirectangular"))
    assert rc == 0 and t.camera_fix == 1 and t.thinlens == 0, msg
    for name in ("bump", "cylinders"):
        rc, t, msg = check(base(name))
        assert rc == 0 and t.all_features_shading == 1 and t.have_proc_tex == 0, (name, msg)
    rc, t, msg = check(base("blade"))             # disk and blade albedos: the all-features family throughout
    assert rc == 0 and t.all_features_shading == 1 and t.have_proc_tex == 1, msg
    d = base("blob")                              # one quad under triangles: the quad is hoisted out of the wide walks
    rc, t, msg = check(d)
    assert rc == 0 and t.wide_depth > 0 and t.hoisted_rec >= 0 and d.recs[t.hoisted_rec].meta >> 29 == 1, msg


# ---- one mutation at a time ----

def _own(bad, keep, field, count, extra=0):
    """Gives `bad` its own copy of the array behind pointer `field` (`extra` more elements, copies of the last) and returns it."""
    ptr = getattr(bad, field)
    arr = (ptr._type_*(count + extra))()
    C.memmove(arr, ptr, count*C.sizeof(ptr._type_))
    for i in range(count, count + extra):
        arr[i] = arr[count - 1]
    keep.append(arr)
    setattr(bad, field, C.cast(arr, type(ptr)))
    return arr


def _set(field, value):
    def m(bad, keep):
        obj, names = bad, field.split(".")
        for n in names[:-1]:
            obj = getattr(obj, n)
        setattr(obj, names[-1], value(bad) if callable(value) else value)
    return m


def _elem(array, count, index, field, value):
    """array[index].field = value on a copy of the array (index: a number, or a function of the description that finds one)."""
    def m(bad, keep):
        arr = _own(bad, keep, array, getattr(bad, count))
        i = index(bad) if callable(index) else index
        v = value(bad) if callable(value) else value
        if field is None:
            arr[i] = v
        else:
            obj, names = arr[i], field.split(".")
            for n in names[:-1]:
                obj = getattr(obj, n)
            if isinstance(getattr(obj, names[-1]), C.Array):
                getattr(obj, names[-1])[0] = v
            else:
                setattr(obj, names[-1], v)
    return m


def _seventeen_lights(bad, keep):
    _own(bad, keep, "lights", bad.num_lights, extra=17 - bad.num_lights)
    bad.num_lights = 17


def _four_coats(bad, keep):
    arr = _own(bad, keep, "bsdfs", bad.num_bsdfs)
    assert bad.num_bsdfs >= 5
    for i in range(4):
        arr[i].type, arr[i].sub0 = 3, i + 1        # TGHIP_BSDF_SMOOTH_COAT over the next


def _black_aperture(bad, keep):
    arr = _own(bad, keep, "dist", bad.num_dist_floats)
    first = bad.camera.aperture_dist + bad.camera.aperture_h
    for i in range(first, first + bad.camera.aperture_h + 1):
        arr[i] = 0.0


def _record_in_two_leaves(bad, keep):
    arr = _own(bad, keep, "top_nodes", bad.num_top_nodes)
    leaves = [(n, i) for n in range(bad.num_top_nodes) for i in range(4) if arr[n].child[i] < 0]
    assert len(leaves) >= 2
    (n0, i0), (n1, i1) = leaves[0], leaves[1]
    arr[n1].child[i1] = arr[n0].child[i0]


def _linear_exponential_medium(bad, keep):
    arr = _own(bad, keep, "media", bad.num_media)
    arr[0].medium_type, arr[0].trans_type = 1, 1     # TGHIP_MEDIUM_EXPONENTIAL with TGHIP_TRANS_LINEAR


def _first(array, count, pred):
    return lambda d: next(i for i in range(getattr(d, count)) if pred(getattr(d, array)[i]))


def _null(field):
    def m(bad, keep):
        setattr(bad, field, C.cast(None, type(getattr(bad, field))))
    return m


_light_object = lambda d: d.lights[0]
_a_bitmap = _first("textures", "num_textures", lambda t: t.type == capi.TGHIP_TEX_BITMAP)
_a_blade = _first("textures", "num_textures", lambda t: t.type == capi.TGHIP_TEX_BLADE)
_an_inner_wide_node = _first("wide_nodes", "num_wide_nodes", lambda w: w.imask != 0)

# id -> (base scene, mutation, return code, piece of the message)
MUTATIONS = {
    "abi_version": ("cornell", _set("abi_version", lambda d: d.abi_version + 1), INVALID, "ABI version mismatch"),
    "no_nodes": ("cornell", _set("num_nodes", 0), INVALID, "no BVH"),
    "res_x_zero": ("cornell", _set("camera.res_x", 0), INVALID, "invalid camera resolution"),
    "seventeen_lights": ("cornell", _seventeen_lights, UNSUPPORTED, "more than 16 sampled lights"),
    # a path's bounce lives in 8 bits of the slot flags (csrc/hip/pt_kernels.h: FLAG_BOUNCE); 255 is the last the device can count to
    "max_bounces_256": ("cornell", _set("settings.max_bounces", 256), UNSUPPORTED, "max_bounces above 255"),
    "light_out_of_range": ("cornell", _elem("lights", "num_lights", 0, None, lambda d: d.num_objects), INVALID, "lights[] entry out of range"),
    "record_kind_the_scene_cannot_hold": ("cornell", _elem("recs", "num_recs", 0, "meta", lambda d: d.recs[0].meta | (7 << 29)), INVALID, "malformed or too deep BVH"),
    "record_object": ("cornell", _elem("recs", "num_recs", 0, "meta", lambda d: (d.recs[0].meta & (7 << 29)) | d.num_objects), INVALID, "refers to an object out of range"),
    "object_bsdf": ("cornell", _elem("objects", "num_objects", 0, "bsdf", lambda d: d.num_bsdfs), INVALID, "object bsdf out of range"),
    "object_emission": ("cornell", _elem("objects", "num_objects", 0, "emission", lambda d: d.num_textures), INVALID, "object emission texture out of range"),
    "object_light": ("cornell", _elem("objects", "num_objects", 0, "light", lambda d: d.num_lights), INVALID, "object light index out of range"),
    "object_medium": ("fog", _elem("objects", "num_objects", 0, "int_medium", lambda d: d.num_media), INVALID, "primitive medium out of range"),
    "bsdf_albedo": ("cornell", _elem("bsdfs", "num_bsdfs", 0, "albedo", lambda d: d.num_textures), INVALID, "bsdf texture out of range"),
    "bsdf_sub0": ("cornell", _elem("bsdfs", "num_bsdfs", 0, "sub0", lambda d: d.num_bsdfs), INVALID, "nested bsdf out of range"),
    "bsdf_bump": ("cornell", _elem("bsdfs", "num_bsdfs", 0, "bump1", lambda d: d.num_textures + 1), INVALID, "bump map index out of range"),
    "camera_medium": ("fog", _set("camera.medium", lambda d: d.num_media), INVALID, "camera medium out of range"),
    "texture_type": ("cornell", _elem("textures", "num_textures", 0, "type", capi.TGHIP_TEX_BLADE + 1), UNSUPPORTED, "unknown texture type"),
    "blade_without_blades": ("blade", _elem("textures", "num_textures", _a_blade, "res_u", 0), INVALID, "blade texture without blades"),
    "node_child": ("cornell", _elem("nodes", "num_nodes", 0, "child0", lambda d: d.num_nodes), INVALID, "malformed or too deep BVH"),
    "four_coats": ("cornell", _four_coats, UNSUPPORTED, "nesting deeper than 3"),
    "mesh_emitter_without_triangles": ("mesh_light", _elem("objects", "num_objects", _light_object, "num_light_tris", 0), INVALID, "without a valid light_tris block"),
    "emitter_type": ("cornell", _elem("objects", "num_objects", _light_object, "type", 10), UNSUPPORTED, "unknown emitter type"),
    "phase_function": ("fog", _elem("media", "num_media", 0, "phase_type", 3), UNSUPPORTED, "unknown phase function"),
    "medium_type": ("fog", _elem("media", "num_media", 0, "medium_type", 3), UNSUPPORTED, "unknown medium type"),
    "transmittance": ("fog", _elem("media", "num_media", 0, "trans_type", 9), UNSUPPORTED, "unknown transmittance"),
    "exponential_medium_linear_transmittance": ("fog", _linear_exponential_medium, UNSUPPORTED, "non-exponential transmittance is not supported"),
    "atmosphere_without_falloff": ("fog", _elem("media", "num_media", 0, "medium_type", 2), INVALID, "positive falloff scale and radius"),
    "interpolated_last": ("fog", _elem("media", "num_media", lambda d: d.num_media - 1, "trans_type", 8), INVALID, "interpolated transmittance needs its two"),
    "camera_type": ("cornell", _set("camera.type", 4), UNSUPPORTED, "unknown camera type"),
    "cubemap_mode": ("equirectangular", lambda bad, keep: (setattr(bad.camera, "type", 3), setattr(bad.camera, "blade_count", 4)), INVALID, "unknown cubemap projection mode"),
    "aperture_type": ("thinlens", _set("camera.aperture_type", 3), UNSUPPORTED, "unknown aperture type"),
    "aperture_past_dist": ("thinlens_bitmap", _set("camera.aperture_dist", lambda d: d.num_dist_floats - 1), INVALID, "aperture's distribution lies outside dist[]"),
    "aperture_all_black": ("thinlens_bitmap", _black_aperture, INVALID, "is not a CDF"),
    "wide_child_base": ("blob", _elem("wide_nodes", "num_wide_nodes", _an_inner_wide_node, "child_base", _an_inner_wide_node), INVALID, "malformed wide BVH"),
    "wide_exponent": ("blob", _elem("wide_nodes", "num_wide_nodes", 0, "exp", 0), INVALID, "malformed wide BVH"),
    "top_record_twice": ("cornell", _record_in_two_leaves, INVALID, "top_nodes: not the tree of a flat list"),
    "sobol_words": ("sobol", _set("num_sobol_words", lambda d: d.num_sobol_words - 1), INVALID, "sobol_matrices must hold"),
    "instances_no_top_recs": ("instances", _set("num_top_recs", 0), INVALID, "malformed scene description"),
    "instances_top_recs_past_recs": ("instances", _set("num_top_recs", lambda d: d.num_recs + 1), INVALID, "malformed scene description"),
    "instances_no_tight_boxes": ("instances", _null("inst_tight_boxes"), INVALID, "malformed scene description"),
    # the two checks the move added: the upload reads dist[] through dist_offset itself, the kernels texels[] through texel_offset
    "bitmap_dist_offset": ("png", _elem("textures", "num_textures", _a_bitmap, "dist_offset", lambda d: d.num_dist_floats), INVALID, "malformed scene description: a bitmap's distribution"),
    "bitmap_texel_offset": ("png", _elem("textures", "num_textures", _a_bitmap, "texel_offset", lambda d: d.num_texel_floats), INVALID, "malformed scene description: a bitmap's texels"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_one_mutation_gives_the_uploads_refusal(name, base):
    scene, mutate, code, text = MUTATIONS[name]
    d = base(scene)
    rc, _, msg = check(C.byref(d))
    assert rc == 0, msg
    bad, keep = tg.TgHipSceneDesc.from_buffer_copy(d), []
    mutate(bad, keep)
    rc, _, msg = check(C.byref(bad))
    assert (rc, text in msg) == (code, True), (rc, msg)


def test_the_last_bounce_count_the_flags_hold_passes(base):
    """settings.max_bounces of 255 is accepted (256 is the mutation "max_bounces_256" above): FLAG_BOUNCE is 8 bits."""
    ok = tg.TgHipSceneDesc.from_buffer_copy(base("cornell"))
    ok.settings.max_bounces = 255
    rc, _, msg = check(C.byref(ok))
    assert rc == 0, msg


def test_null_arguments(base):
    err = C.create_string_buffer(64)
    assert tg.lib.tgh_scene_check(None, None, err, len(err)) == INVALID
    assert tg.lib.tgh_scene_check(None, None, None, 0) == INVALID
    assert tg.lib.tgh_scene_check(C.byref(base("cornell")), None, None, 0) == 0       # traits and message are optional
