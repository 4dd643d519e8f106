"""The fibre BCSDFs on the host (no GPU): `lambertian_fiber` and `rough_wire` load and flatten to the documented TgHipBsdf fields (type, the lobes
word the reference's BsdfLobes gives after prepareForRender, eta / k, _v float for float in `thickness`), the wrappers hand the anisotropic bit up,
tgh_scene_check sends every scene that holds one to the all-features family and no other, an unknown material is a load error, `hair` is still
refused, and the committed goldens say something."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bsdf_cases as bc
import fibre_cases as fc
import scenes
import tungsten_amd as tg
from tungsten_amd import capi
from test_oracle_golden import flat_bsdf_index

F = np.float32
LAMBERTIAN_FIBER, ROUGH_WIRE = 19, 20                   # TGHIP_BSDF_LAMBERTIAN_FIBER / _ROUGH_WIRE (include/tungsten_hip.h)
GR, GT, DR, DT, SR, ST, ANISO, FWD = 1, 2, 4, 8, 16, 32, 64, 128   # bsdfs/BsdfLobes.hpp:13-33
FAMILY_MARKER = 0xF << 20                               # FEAT_BUMP | FEAT_CYLINDER | FEAT_AUX | FEAT_MEDIA (csrc/hip/pt_variants.h)
MASK_FULL = 0xFFFFFFFF & ~((1 << 30) | FAMILY_MARKER)
MASK_MEDIA = (1 | 2 | (1 << 13)) | (0x1F << 24) | (1 << 23) | (1 << 30) | (1 << 12) | (1 << 4) | (1 << 6)
# the constructor's Cu (RoughWireBcsdf.cpp:17-25), as the floats the literals round to
CU_ETA, CU_K = (0.200438, 0.924033, 1.10221), (3.91295, 2.45285, 2.14219)


def check(desc):
    traits = capi.TgHostSceneTraits()
    err = C.create_string_buffer(512)
    rc = tg.lib.tgh_scene_check(desc, C.byref(traits), err, len(err))
    return rc, traits, err.value.decode()


def wire_v(roughness):
    """sqr(_roughness*PI_HALF) in float32 (RoughWireBcsdf.cpp:171-174; PI_HALF = PI*0.5f, math/Angle.hpp:8-9)."""
    beta = F(roughness)*(F(3.1415926536)*F(0.5))
    return F(beta*beta)


@pytest.fixture(scope="module")
def fixture_scene(tmp_path_factory):
    path = fc.bsdf_scene(tmp_path_factory.mktemp("fibre_bsdfs"))
    with open(path) as f:
        sj = json.load(f)
    flat = tg.FlattenedScene(path)
    yield sj, flat
    flat.close()


def _bsdf(fixture_scene, name, nested=0):
    sj, flat = fixture_scene
    return flat.desc.contents.bsdfs[flat_bsdf_index(sj, bc.scene_index(sj, name)) + nested]


def test_abi_names_the_two_types():
    with open(os.path.join(scenes.ROOT, "include", "tungsten_hip.h")) as f:
        header = f.read()
    assert "TGHIP_BSDF_LAMBERTIAN_FIBER = 19" in header and "TGHIP_BSDF_ROUGH_WIRE = 20" in header and "TGHIP_LIBM_SINHF = 17" in header
    assert "TGHIP_ABI_VERSION 10" in " ".join(header.split())
    assert capi.TGHIP_LIBM_SINHF == 17
    assert C.sizeof(capi.TgHipBsdf) == 108                  # as before: the parameters ride in existing fields


def test_lambertian_fiber_flattens(fixture_scene):
    b = _bsdf(fixture_scene, "lambertian_fiber")
    assert b.type == LAMBERTIAN_FIBER and b.lobes == (DR | DT | ANISO)
    assert b.sub0 == -1 and b.sub1 == -1 and b.bump1 == 0
    assert _bsdf(fixture_scene, "fibre_bumped").bump1 > 0


@pytest.mark.parametrize("key", sorted(fc.WIRE))
def test_rough_wire_flattens(key, fixture_scene):
    b, j = _bsdf(fixture_scene, "wire_" + key), fc.WIRE[key]
    assert b.type == ROUGH_WIRE and b.lobes == (GR | GT | ANISO)
    assert b.roughness == -1                                 # a plain float in the reference, not a texture
    assert F(b.thickness).view(np.uint32) == wire_v(j["roughness"]).view(np.uint32)      # _v, float for float
    if "eta" in j:
        want_eta, want_k = j["eta"], j["k"]
    elif "material" in j:
        # the complex-IOR table the conductors use: the same scene's lookup through `conductor`
        want_eta, want_k = _conductor(j["material"])
    else:
        want_eta, want_k = CU_ETA, CU_K
    assert [F(x) for x in b.eta] == [F(x) for x in want_eta] and [F(x) for x in b.k] == [F(x) for x in want_k]


_conductors = {}


def _conductor(material):
    if material not in _conductors:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            def edit(scene):
                scene["bsdfs"][0] = {"name": scene["bsdfs"][0]["name"], "type": "conductor", "albedo": 1, "material": material}
            flat = tg.FlattenedScene(scenes.cornell(tmp, resolution=(16, 9), spp=1, edit=edit, name="conductor.json"))
            b = flat.desc.contents.bsdfs[0]
            assert b.type == 7
            _conductors[material] = (list(b.eta), list(b.k))
            flat.close()
    return _conductors[material]


def test_a_material_lookup_equals_the_conductors():
    for material in ("Au", "Al", "Cu"):
        eta, k = _conductor(material)
        assert all(np.isfinite(eta)) and all(x > 0 for x in k)


def test_eta_without_k_keeps_eta_and_the_default_k(tmp_path):
    """RoughWireBcsdf.cpp:101: `getField("eta", _eta) && getField("k", _k)` -- eta is stored even where k is missing, k is not read without eta."""
    def edit(scene):
        scene["bsdfs"][0] = {"name": scene["bsdfs"][0]["name"], "type": "rough_wire", "eta": [1.5, 1.25, 1.0]}
        scene["bsdfs"][1] = {"name": scene["bsdfs"][1]["name"], "type": "rough_wire", "k": [9.0, 8.0, 7.0]}
    flat = tg.FlattenedScene(scenes.cornell(tmp_path, resolution=(16, 9), spp=1, edit=edit, name="eta_only.json"))
    b0, b1 = flat.desc.contents.bsdfs[0], flat.desc.contents.bsdfs[1]
    assert list(b0.eta) == [1.5, 1.25, 1.0] and [F(x) for x in b0.k] == [F(x) for x in CU_K]
    assert [F(x) for x in b1.eta] == [F(x) for x in CU_ETA] and [F(x) for x in b1.k] == [F(x) for x in CU_K]
    assert F(b0.thickness).view(np.uint32) == wire_v(0.1).view(np.uint32)               # the default roughness
    flat.close()


def test_wrappers_carry_the_anisotropic_bit(fixture_scene):
    """MixedBsdf.cpp:132-135, TransparencyBsdf.cpp:66-69, SmoothCoatBsdf.cpp:218-223 (RoughCoatBsdf.cpp:300-305 likewise): the wrapper's lobes are
    its own united with its children's, the anisotropic bit included."""
    mix, cut, coat = (_bsdf(fixture_scene, n) for n in ("mix", "cut", "coat"))
    assert mix.type == 10 and mix.lobes == (DR | DT | ANISO)                 # lambertian_fiber | lambert
    assert cut.type == 11 and cut.lobes == (FWD | GR | GT | ANISO)
    assert coat.type == 3 and coat.lobes == (SR | DR | DT | ANISO)
    sj, flat = fixture_scene
    d = flat.desc.contents
    assert d.bsdfs[cut.sub0].type == ROUGH_WIRE and d.bsdfs[coat.sub0].type == LAMBERTIAN_FIBER and d.bsdfs[mix.sub0].type == LAMBERTIAN_FIBER


def test_rough_coat_carries_the_bit_too(tmp_path):
    def edit(scene):
        scene["bsdfs"][0] = {"name": scene["bsdfs"][0]["name"], "type": "rough_coat", "roughness": 0.1, "substrate": dict(fc.LAMBERT_FIBRE)}
    flat = tg.FlattenedScene(scenes.cornell(tmp_path, resolution=(16, 9), spp=1, edit=edit, name="rough_coat.json"))
    assert flat.desc.contents.bsdfs[0].lobes == (GR | DR | DT | ANISO)
    rc, t, msg = check(flat.desc)
    assert rc == 0 and t.have_fibre == 1 and t.all_features_shading == 1, msg
    flat.close()


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_case_passes_the_check_and_takes_the_all_features_family(name, tmp_path):
    mk, kw = fc.CASES[name]
    flat = tg.FlattenedScene(mk(tmp_path, name=name + ".json", **kw))
    rc, t, msg = check(flat.desc)
    assert rc == 0, msg
    assert (flat.width, flat.height) == (48, 27)
    assert t.have_fibre == 1 and t.all_features_shading == 1 and t.have_proc_tex == 0 and t.lean_scene in (0, 1) and t.media_simple == 0
    d = flat.desc.contents
    types = [d.bsdfs[i].type for i in range(d.num_bsdfs)]
    assert LAMBERTIAN_FIBER in types or ROUGH_WIRE in types
    # the type words never carry a bit "for" types 19 and 20 (those are FEAT_PHONG and FEAT_BUMP): class masks hold the family marker instead
    fibre_classes = [c for c in range(4) if t.class_present[c] and (t.class_mask[c] & FAMILY_MARKER) == FAMILY_MARKER]
    assert fibre_classes == [3], (list(t.class_present), [hex(m) for m in t.class_mask])
    for c in range(3):
        assert (t.class_mask[c] & FAMILY_MARKER) == 0
    # ... which no other family's mask holds whole (csrc/hip/pt_variants.h: every family but the media one is a subset of MASK_FULL; the media
    # family's rule refuses the marker by name, SceneCheck.cpp: familyCovers): not covered by any family but the all-features one
    assert (t.class_mask[3] & ~MASK_FULL) != 0 and (t.class_mask[3] & FAMILY_MARKER & ~MASK_MEDIA) != 0
    if name == "fibre_instances":
        assert t.have_instances == 1
    if name == "fibre_sobol_fog":
        assert t.have_media == 1 and d.sobol_matrices
    if name == "fibre_nested":
        assert t.have_forward == 1                           # the transparency: shadow rays are closest-hit walks
    flat.close()


def test_a_scene_without_fibres_keeps_its_traits(tmp_path):
    flat = tg.FlattenedScene(scenes.cornell(tmp_path, resolution=(48, 27), spp=8))
    rc, t, msg = check(flat.desc)
    assert rc == 0 and t.have_fibre == 0 and t.all_features_shading == 0 and t.lean_scene == 1, msg
    flat.close()
    mk, kw = scenes.GOLDEN_CASES["cornell_bump"]
    flat = tg.FlattenedScene(mk(tmp_path, name="bump.json", **kw))
    rc, t, msg = check(flat.desc)
    assert rc == 0 and t.have_fibre == 0 and t.all_features_shading == 1, msg
    assert all((t.class_mask[c] & FAMILY_MARKER) == 0 for c in range(4))
    flat.close()


def test_an_unknown_material_is_a_load_error(tmp_path):
    def edit(scene):
        scene["bsdfs"][0] = {"name": scene["bsdfs"][0]["name"], "type": "rough_wire", "material": "Unobtainium"}
    with pytest.raises(tg.TungstenError) as e:
        tg.FlattenedScene(scenes.cornell(tmp_path, resolution=(16, 9), spp=1, edit=edit, name="unobtainium.json"))
    assert "Unable to find material with name 'Unobtainium'" in str(e.value)


def test_hair_is_still_refused(tmp_path):
    def edit(scene):
        scene["bsdfs"][0] = {"name": scene["bsdfs"][0]["name"], "type": "hair"}
    with pytest.raises(tg.TungstenError) as e:
        tg.FlattenedScene(scenes.cornell(tmp_path, resolution=(16, 9), spp=1, edit=edit, name="hair.json"))
    assert "hair" in str(e.value) and "outside the path_tracer_hip hot-path scope" in str(e.value)


# ---- the goldens say something ----
def _samples(name):
    return np.load(os.path.join(scenes.GOLDEN, name + "_samples.npz"))


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_golden_is_finite_not_black_and_not_lambert(name):
    g = _samples(name)
    s = g["samples"]
    assert s.shape == (27, 48, 8, 3) and s.dtype == np.float32 and int(g["seed"]) == tg.DEFAULT_SEED
    assert np.isfinite(s).all() and s.max() > 0
    assert int(g["lambert_twin_differing"]) > 0          # samples that differ from the same scene with lambert (tools/make_fibre_golden.py)


def test_roughness_goldens_differ_pairwise():
    wires = [_samples(n)["samples"].view(np.uint32) for n in fc.ROUGHNESS_CASES]
    for i in range(len(wires)):
        for j in range(i):
            differing = int((wires[i] != wires[j]).any(axis=-1).sum())
            assert differing > 100, (fc.ROUGHNESS_CASES[i], fc.ROUGHNESS_CASES[j], differing)


def test_bsdf_golden_holds_the_fixtures_cases():
    g = np.load(fc.BSDF_GOLDEN)
    names, position, cases, stream, per = fc.bsdf_fixture_cases()
    assert list(g["names"]) == names and int(g["cases_per_bsdf"]) == per and per >= 300
    for k in ("wi", "wo", "uv", "requested"):
        assert (g[k].view(np.uint32) == cases[k].view(np.uint32)).all(), k
    assert (g["stream"] == stream).all() and int(g["seed"]) == bc.SEED
    ref = g["ref"]
    assert ref.shape == (len(names)*per, 14) and ref.dtype == np.uint32
    # the corners are in: wo.z == 0, wo along +-y, wi.y == +-1, and every requested set that switches a branch
    wo, wi = cases["wo"][:per], cases["wi"][:per]
    assert (wo[:, 2] == 0).any() and ((wo[:, 1] == 1) & (wo[:, 0] == 0)).any() and (wo[:, 1] == -1).any() and (wi[:, 1] == 1).any() and (wi[:, 1] == -1).any()
    assert set([1, 2, 3, 4, 8, 12, 64, 128, 0, bc.ALL_LOBES, bc.ALL_BUT_SPECULAR]) <= set(int(r) for r in cases["requested"][:per])
    for pos, name in enumerate(names):
        block = ref[pos*per:(pos + 1)*per]
        f = block[:, :4].view(np.float32)
        assert (f[np.isfinite(f)] != 0).any() and block[:, 4].any(), name
        ok = block[:, 4] == 1
        assert np.isfinite(block[ok][:, 5:8].view(np.float32)).all(), name       # a sampled direction is a direction
    # rough_wire is black at wo.z == 0 (its guard, RoughWireBcsdf.cpp:123) and a refused lobe set fails the sample
    p = names.index("wire_r035")
    block, req, wo = ref[p*per:(p + 1)*per], cases["requested"][p*per:(p + 1)*per], cases["wo"][p*per:(p + 1)*per]
    assert (block[wo[:, 2] == 0][:, :3] == 0).all()
    assert (block[(req & 3) == 0][:, 4] == 0).all() and (block[(req & 3) != 0][:, 4] == 1).all()
    p = names.index("lambertian_fiber")
    block, req = ref[p*per:(p + 1)*per], cases["requested"][p*per:(p + 1)*per]
    assert (block[(req & 12) == 0][:, 4] == 0).all() and (block[(req & 12) != 0][:, 4] == 1).all()
    assert (block[(req & 12) != 0][:, 12] == 12).all()      # sampledLobe = DiffuseLobe, both bits
