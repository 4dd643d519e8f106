"""The sampled-texture cases on the host (no GPU): every case of tests/sampled_texture_cases.py loads and passes the upload's check, the new
apertures arrive in the documented TgHipCamera fields, a pivoted cap flattens to the bytes of the same scene with the pivot's transform written
out, tgh_scene_check accepts the new aperture values and refuses malformed ones, and the class rule sends a scene with a sampled checker
environment -- and no other -- to the all-features family."""
import ctypes as C
import json

import numpy as np
import pytest

import sampled_texture_cases as stc
import scenes
import texture_cases
import tungsten_amd as tg
from tungsten_amd import capi

F = np.float32
INVALID, UNSUPPORTED = capi.TGHIP_E_INVALID, capi.TGHIP_E_UNSUPPORTED


def check(desc):
    """(return code, traits, message) of tgh_scene_check."""
    traits = capi.TgHostSceneTraits()
    err = C.create_string_buffer(512)
    rc = tg.lib.tgh_scene_check(desc, C.byref(traits), err, len(err))
    return rc, traits, err.value.decode()


def _flatten(table, name, tmp_path):
    mk, kw = table[name]
    return tg.FlattenedScene(mk(tmp_path, name=name + ".json", **kw))


def desc_bytes(d):
    """Every array of a flattened description and the structs inside it, as bytes."""
    def arr(ptr, count, size):
        return C.string_at(ptr, count*size) if count and ptr else b""
    return {
        "counts": (d.abi_version, d.num_nodes, d.num_recs, d.num_objects, d.num_lights, d.num_infinite_lights, d.num_bsdfs, d.num_textures,
                   d.num_texel_floats, d.num_dist_floats, d.num_light_tri_floats, d.num_instances, d.num_top_recs, d.num_inst_prims, d.num_media,
                   d.num_wide_nodes, d.num_top_nodes),
        "nodes": arr(d.nodes, d.num_nodes, C.sizeof(capi.TgHipBvhNode)),
        "wide_nodes": arr(d.wide_nodes, d.num_wide_nodes, C.sizeof(capi.TgHipWideNode)),
        "top_nodes": arr(d.top_nodes, d.num_top_nodes, C.sizeof(capi.TgHipTopNode)),
        "recs": arr(d.recs, d.num_recs, C.sizeof(capi.TgHipPrimRec)),
        "tri_attrs": arr(d.tri_attrs, d.num_recs, C.sizeof(capi.TgHipTriAttr)),
        "objects": arr(d.objects, d.num_objects, C.sizeof(capi.TgHipObject)),
        "lights": arr(d.lights, d.num_lights, 4),
        "infinite_lights": arr(d.infinite_lights, d.num_infinite_lights, 4),
        "bsdfs": arr(d.bsdfs, d.num_bsdfs, C.sizeof(capi.TgHipBsdf)),
        "textures": arr(d.textures, d.num_textures, C.sizeof(capi.TgHipTexture)),
        "texels": arr(d.texels, d.num_texel_floats, 4),
        "dist": arr(d.dist, d.num_dist_floats, 4),
        "light_tris": arr(d.light_tris, d.num_light_tri_floats, 4),
        "media": arr(d.media, d.num_media, C.sizeof(capi.TgHipMedium)),
        "camera": bytes(d.camera),
        "settings": bytes(d.settings),
        "bounds": bytes(d.bounds_lo) + bytes(d.bounds_hi),
    }


@pytest.mark.parametrize("name", sorted(stc.CASES))
def test_case_loads_and_passes_the_check(name, tmp_path):
    flat = _flatten(stc.CASES, name, tmp_path)
    rc, t, msg = check(flat.desc)
    d = flat.desc.contents
    assert rc == 0, msg
    assert (flat.width, flat.height) == (48, 27)
    assert t.thinlens == (1 if name in stc.LENS_CASES else 0)
    assert d.num_infinite_lights == (0 if name in stc.LENS_CASES else 2 if name.startswith("stex_sun") else 1)
    flat.close()


def _maximum(colour):
    return F(max(colour)) if isinstance(colour, (list, tuple)) else F(colour)


@pytest.mark.parametrize("name", sorted(stc.LENS_CASES))
def test_the_camera_carries_the_aperture(name, tmp_path):
    flat = _flatten(stc.CASES, name, tmp_path)
    d = flat.desc.contents
    cam, ap = d.camera, stc.LENS_CASES[name]
    assert cam.type == 1                                      # TGHIP_CAMERA_THINLENS
    if ap["type"] == "constant":
        assert cam.aperture_type == capi.TGHIP_APERTURE_CONSTANT == 4
    elif ap["type"] == "checker":
        # aperture_w / aperture_h = res_u / res_v, blade_edge = (_onColor.max(), _offColor.max()): the scalar request leaves a checker's colours alone
        assert cam.aperture_type == capi.TGHIP_APERTURE_CHECKER == 5
        assert (cam.aperture_w, cam.aperture_h) == (ap["res_u"], ap["res_v"])
        assert F(cam.blade_edge[0]) == _maximum(ap["on_color"]) and F(cam.blade_edge[1]) == _maximum(ap["off_color"])
    else:
        # the bake is a scalar bitmap: the aperture is its Distribution2D over 2R x R texels, built with MAP_UNIFORM
        r = ap["resolution"]
        assert cam.aperture_type == capi.TGHIP_APERTURE_BITMAP == 2 and (cam.aperture_w, cam.aperture_h) == (2*r, r)
        n = 2*r*r
        assert cam.aperture_dist + r + (r + 1) + n + (2*r + 1)*r <= d.num_dist_floats
        dist = np.ctypeslib.as_array(d.dist, (d.num_dist_floats,))[cam.aperture_dist:]
        mpdf, mcdf = dist[:r], dist[r:2*r + 1]
        assert mcdf[0] == 0 and mcdf[-1] == 1 and (np.diff(mcdf) >= 0).all() and abs(float(mpdf.sum()) - 1) < 1e-4
        assert mpdf.max() > 2*mpdf.min()                      # a profile, not the uniform fall-back of a file that could not be read
    flat.close()


def _lens_scene(tmp_path, aperture, name):
    return texture_cases.build(tmp_path, name=name, edit=stc._lens(aperture), **texture_cases.SIZE)


def test_apertures_that_sample_like_a_constant(tmp_path):
    """A number, an RGB triple and a checker of two blacks (CheckerTexture::sample's early-out) hand the lens sample back: the square aperture."""
    for i, ap in enumerate((0.5, [0.2, 0.4, 0.6], {"type": "checker", "on_color": 0.0, "off_color": [0, 0, 0], "res_u": 4, "res_v": 4})):
        flat = tg.FlattenedScene(_lens_scene(tmp_path, ap, "square%d.json" % i))
        assert flat.desc.contents.camera.aperture_type == capi.TGHIP_APERTURE_CONSTANT
        assert check(flat.desc)[0] == 0
        flat.close()


def test_an_unknown_aperture_texture_is_still_refused(tmp_path):
    with pytest.raises(tg.TungstenError) as e:
        tg.FlattenedScene(_lens_scene(tmp_path, {"type": "marble"}, "marble.json"))
    assert "Texture type 'marble' is outside the path_tracer_hip hot-path scope" in str(e.value)


@pytest.mark.parametrize("name", sorted(stc.PIVOT_TWINS))
def test_a_pivoted_cap_flattens_like_its_written_out_twin(name, tmp_path, capfd):
    flat = _flatten(stc.CASES, name, tmp_path)
    noted = capfd.readouterr().err
    (tmp_path/"twin").mkdir()
    twin = _flatten(stc.PIVOT_TWINS, name, tmp_path/"twin")
    a, b = desc_bytes(flat.desc.contents), desc_bytes(twin.desc.contents)
    for key in a:
        assert a[key] == b[key], "%s: `%s` differs from the written-out twin's" % (name, key)
    d = flat.desc.contents
    caps = [d.objects[i] for i in range(d.num_objects) if d.objects[i].type == 7]      # TGHIP_OBJ_INFINITE_SPHERE_CAP
    assert len(caps) == 1 and abs(sum(x*x for x in caps[0].normal) - 1) < 1e-6
    if name == "stex_sun_pivot_missing":
        assert "unable to find pivot object 'no_such_sky' for infinity sphere cap" in noted
    else:
        assert "pivot" not in noted
        # ... and the pivot decided the direction: not where the cap's own transform points
        with open(str(tmp_path/(name + ".json"))) as f:
            scene = json.load(f)
        own = dict(next(p for p in scene["primitives"] if p["name"] == "sun"))
        del own["skydome"]
        scene["primitives"] = [own if p["name"] == "sun" else p for p in scene["primitives"]]
        with open(str(tmp_path/"own.json"), "w") as f:
            json.dump(scene, f)
        unpivoted = tg.FlattenedScene(str(tmp_path/"own.json"))
        du = unpivoted.desc.contents
        cap = [du.objects[i] for i in range(du.num_objects) if du.objects[i].type == 7][0]
        assert max(abs(x - y) for x, y in zip(cap.normal, caps[0].normal)) > 0.05
        unpivoted.close()
    flat.close()
    twin.close()


# ---- the upload's check of the new aperture values: one field of a valid description changed at a time, on a copy ----

def _camera(**fields):
    def m(bad):
        for k, v in fields.items():
            if k.startswith("blade_edge"):
                bad.camera.blade_edge[int(k[-1])] = v
            else:
                setattr(bad.camera, k, v)
    return m


MUTATIONS = {
    "type_3": (_camera(aperture_type=3), UNSUPPORTED, "unknown aperture type"),
    "one_past_the_last": (_camera(aperture_type=6), UNSUPPORTED, "unknown aperture type"),
    "negative_type": (_camera(aperture_type=-1), UNSUPPORTED, "unknown aperture type"),
    "res_u_zero": (_camera(aperture_w=0), INVALID, "positive resolutions"),
    "res_v_zero": (_camera(aperture_h=0), INVALID, "positive resolutions"),
    "res_v_negative": (_camera(aperture_h=-3), INVALID, "positive resolutions"),
    "both_weights_zero": (_camera(blade_edge0=0.0, blade_edge1=0.0), INVALID, "not both zero"),
    "weight_nan": (_camera(blade_edge0=float("nan")), INVALID, "must be finite"),
    "weight_inf": (_camera(blade_edge1=float("inf")), INVALID, "must be finite"),
    "weight_negative": (_camera(blade_edge0=-0.5), INVALID, "not negative"),
    "sum_overflows": (_camera(blade_edge0=3e38, blade_edge1=3e38), INVALID, "must be finite"),
}


@pytest.fixture(scope="module")
def checker_lens(tmp_path_factory):
    flat = _flatten(stc.CASES, "stex_lens_checker", tmp_path_factory.mktemp("checker_lens"))
    yield flat.desc.contents
    flat.close()


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_check_refuses_a_malformed_aperture(name, checker_lens):
    mutate, code, piece = MUTATIONS[name]
    assert check(C.byref(checker_lens))[0] == 0
    bad = tg.TgHipSceneDesc.from_buffer_copy(checker_lens)
    mutate(bad)
    rc, _, msg = check(C.byref(bad))
    assert rc == code and piece in msg, (rc, msg)


def test_check_accepts_the_new_aperture_values(checker_lens):
    ok = tg.TgHipSceneDesc.from_buffer_copy(checker_lens)
    _camera(blade_edge0=0.0)(ok)                              # onProb == 0
    assert check(C.byref(ok))[0] == 0
    _camera(blade_edge0=2.5, blade_edge1=0.0)(ok)             # onProb == 1
    assert check(C.byref(ok))[0] == 0
    _camera(aperture_type=capi.TGHIP_APERTURE_CONSTANT, aperture_w=0, aperture_h=0, blade_edge0=0.0)(ok)    # a constant reads none of them
    assert check(C.byref(ok))[0] == 0


# ---- the class rule ----

def _checker_albedo(scene):
    scenes._replace_bsdf(scene, "floor", {"type": "lambert", "albedo": stc.CHECKER})


def _traits(t):
    return dict(all_features_shading=t.all_features_shading, have_proc_tex=t.have_proc_tex, lean_scene=t.lean_scene, have_complex=t.have_complex,
                class_present=list(t.class_present), have_forward=t.have_forward, have_media=t.have_media, media_simple=t.media_simple)


# what tgh_scene_check said of the two scenes on the commit before checker environments were sampled through the texture, recorded there
TRAITS_BEFORE = {
    "stex_env_checker_unsampled": dict(all_features_shading=0, have_proc_tex=0, lean_scene=0, have_complex=0, class_present=[1, 0, 0, 0],
                                       have_forward=0, have_media=0, media_simple=0),
    "checker_albedo": dict(all_features_shading=0, have_proc_tex=0, lean_scene=1, have_complex=0, class_present=[1, 0, 0, 0],
                           have_forward=0, have_media=0, media_simple=0),
}


@pytest.mark.parametrize("name", stc.SAMPLED_CHECKER_CASES)
def test_a_sampled_checker_environment_takes_the_all_features_family(name, tmp_path):
    flat = _flatten(stc.CASES, name, tmp_path)
    rc, t, msg = check(flat.desc)
    assert rc == 0, msg
    assert t.have_proc_tex == 1 and t.all_features_shading == 1   # (all_features_shading also keeps the fog case off the lean media family's kernel)
    flat.close()


def test_checkers_that_are_only_looked_up_stay_where_they_were(tmp_path):
    flat = _flatten(stc.CASES, "stex_env_checker_unsampled", tmp_path)
    rc, t, msg = check(flat.desc)
    assert rc == 0, msg
    assert _traits(t) == TRAITS_BEFORE["stex_env_checker_unsampled"]
    flat.close()
    flat = tg.FlattenedScene(texture_cases.build(tmp_path, name="checker_albedo.json", edit=_checker_albedo, **texture_cases.SIZE))
    rc, t, msg = check(flat.desc)
    assert rc == 0, msg
    assert _traits(t) == TRAITS_BEFORE["checker_albedo"]
    flat.close()


def test_aperture_values_and_struct_size_are_the_documented_ones():
    assert (capi.TGHIP_APERTURE_DISK, capi.TGHIP_APERTURE_BLADE, capi.TGHIP_APERTURE_BITMAP) == (0, 1, 2)
    assert (capi.TGHIP_APERTURE_CONSTANT, capi.TGHIP_APERTURE_CHECKER) == (4, 5)
    assert C.sizeof(capi.TgHipCamera) == 312                 # as before: the checker's parameters ride in existing fields
