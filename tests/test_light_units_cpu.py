"""Single light calls, CPU side: the oracle's chooseLight / light_sampleDirect / light_approximateRadiance / light_intersect / light_evalDirect /
light_directPdf (through oracle_light_cases) against the answers of the reference's own TraceBase::chooseLight and Primitive::sampleDirect /
approximateRadiance / intersect + intersectionInfo / evalDirect / directPdf, recorded in tests/golden/light_corners.npz (tools/make_light_golden.py)
for the first FIXTURE_CASES cases of every sampled light of the six scenes.light_corners scenes -- shading points in the emitter's plane, on and
inside a sphere, at a point light's own position, 1e4 and 1e6 units away; directions through a quad's corners and edges, along and across the
emitter's plane, at the poles, the seam and the texel boundaries of the environment maps, on a cap's rim (tests/light_cases.py).

Every word is compared as a bit pattern: the chosen light, sample_ok, approximateRadiance and hit always; the weight where a light was chosen; d,
dist and pdf where the sample succeeded; t, u, v, back_side, the emission and directPdf where the ray hit (directPdf always for the point light);
and the counts of random numbers chooseLight and sampleDirect consumed.  A NaN matches a NaN.  The numbers the calls draw come from each case's own
counter-based streams; crafted sampling numbers (xi of exactly 0, or 1 - ulp) are out of scope here, because the device, which is held to the same
cases (tests/test_gpu_light_units.py), replays nothing.

A residual would be pinned case by case in tests/golden/light_corners_residual.json; there is none: 0 of 6 720 cases differ (and 0 of the 172 032 of
the device test's full lists: `python tools/make_light_golden.py --cases 4096` measures that).  Before the oracle added the translation column of the reference's Mat4f-times-Vec3f (+0, which turns
a -0 component into +0) to the infinite sphere's direction map, the cases of the unrotated `sky` whose w runs straight along the map's pole differed
in u (0 for the reference's 0.5); the fixture also records the seam both ways: w = (-1, 0, -0) reads u = 1 on `sky` and u = 0 on the skydome, which
maps directions without a matrix."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import light_cases as lc
import oracle_lib
import scenes
import tungsten_amd as tg
from tungsten_amd import capi

SCENES = scenes.LIGHT_CORNER_SCENES
LIGHTS = [(which, slot, name) for which in SCENES for slot, (name, _, _) in enumerate(scenes.light_corner_list(which))]
IDS = ["%s/%s" % (which, name) for which, _, name in LIGHTS]
PINNED = json.load(open(lc.RESIDUAL)) if os.path.exists(lc.RESIDUAL) else {}


@pytest.fixture(scope="module")
def gold():
    return np.load(lc.GOLDEN)


@pytest.fixture(scope="module")
def corner_scenes(tmp_path_factory):
    out = {}
    for which in SCENES:
        path = scenes.light_corners(tmp_path_factory.mktemp("light_corners_" + which), which)
        out[which] = (path, tg.FlattenedScene(path))
    yield out
    for _, flat in out.values():
        flat.close()


def _traits(desc):
    t = capi.TgHostSceneTraits()
    err = C.create_string_buffer(512)
    rc = tg.lib.tgh_scene_check(desc, C.byref(t), err, len(err))
    assert rc == 0, err.value.decode()
    return t


def _needs(desc, variant):
    n = int(desc.contents.num_lights)
    needs, covered, mask = np.zeros(n, np.uint32), np.zeros(n, np.uint32), C.c_uint32(0)
    assert tg.lib.tgh_light_needs(desc, variant, needs.ctypes.data, covered.ctypes.data, C.addressof(mask)) == 0
    return needs, covered.astype(bool), int(mask.value)


def test_scenes_hold_the_listed_emitters_in_order(corner_scenes):
    for which in SCENES:
        d = corner_scenes[which][1].desc.contents
        want = scenes.light_corner_list(which)
        assert d.num_lights == len(want) <= lc.MAX_LIGHTS
        for slot, (name, kind, _) in enumerate(want):
            o = d.objects[d.lights[slot]]
            assert o.type == lc.KIND_OF[kind] and bool(o.flags & lc.OBJF_SKYDOME) == (kind == "skydome"), (which, name)
    assert corner_scenes["all"][1].desc.contents.num_lights == 16
    kinds = {kind for _, kind, _ in scenes.light_corner_list("all")}
    assert kinds == set(lc.KIND_OF)                                    # every emitter kind the device samples
    t = {which: _traits(corner_scenes[which][1].desc) for which in SCENES}
    assert t["lean"].lean_scene == 1 and t["solids"].lean_scene == 0 and t["solids"].all_features_shading == 0 and t["solids"].have_mesh_light == 0
    assert t["backs"].lean_scene == 0 and t["backs"].all_features_shading == 0 and t["unknown"].have_mesh_light == 1 and t["unknown"].all_features_shading == 0
    assert t["mesh"].have_mesh_light == 1 and t["mesh"].all_features_shading == 0 and t["all"].all_features_shading == 1 and t["all"].have_proc_tex == 1


@pytest.mark.parametrize("which", SCENES)
def test_fixture_inputs_are_what_the_generator_produces(which, gold, corner_scenes):
    names = [name for name, _, _ in scenes.light_corner_list(which)]
    n = int(gold["cases_per_light"])
    assert list(gold[which + "_names"]) == names
    assert n == lc.FIXTURE_CASES and int(gold["seed"]) == lc.SEED and int(gold["nxc"]) == lc.NXC and int(gold["nxs"]) == lc.NXS
    assert gold[which + "_ref"].shape == (len(names)*n, 20)
    desc = corner_scenes[which][1].desc
    for slot, name in enumerate(names):
        g = lc.light_geometry(desc, slot)
        c = lc.make_cases(g, name, n)
        for key in ("p", "w"):
            assert (gold["%s_%s" % (which, key)][slot*n:(slot + 1)*n].view(np.uint32) == c[key].view(np.uint32)).all(), (name, key)
        long = lc.make_cases(g, name, 2*n)                              # a prefix of the device test's longer list
        assert all((long[key][:n].view(np.uint32) == c[key].view(np.uint32)).all() for key in ("p", "w"))
        assert np.isfinite(c["p"]).all() and np.isfinite(c["w"]).all()


def test_fixture_cases_hold_every_crafted_point_and_direction(corner_scenes):
    desc = corner_scenes["all"][1].desc
    for slot, (name, kind, _) in enumerate(scenes.light_corner_list("all")):
        g = lc.light_geometry(desc, slot)
        c = lc.make_cases(g, name, lc.FIXTURE_CASES)
        P = lc.crafted_p(g)
        assert {k for k, _ in P} <= set(c["p_kind"]), name
        have = {tuple(p.view(np.uint32)) for p in c["p"]}
        assert all(tuple(p.view(np.uint32)) in have for _, p in P), name
        assert {k for k, _ in lc.crafted_w(g, P[-1][1])} <= set(c["w_kind"]), name
        assert "" not in c["p_kind"][:len(P)] and len(P) <= lc.FIXTURE_CASES//4
    # what the issue names, by kind
    def kinds(name, fn):
        slot = [n for n, _, _ in scenes.light_corner_list("all")].index(name)
        g = lc.light_geometry(desc, slot)
        return {k for k, _ in (lc.crafted_p(g) if fn == "p" else lc.crafted_w(g, lc.crafted_p(g)[-1][1]))}
    assert {"plane", "plane+ulp", "plane-ulp", "behind", "above_1e-4", "normal_10000", "normal_1e+06", "tangent_10000", "tangent_1e+06"} <= kinds("light", "p")
    assert "cone_boundary" in kinds("spot", "p") and {"centre", "surface", "surface+ulp", "surface-ulp"} <= kinds("bulb", "p")
    assert {"centre", "centre+ulp"} <= kinds("lamp", "p") and {"inside", "face", "edge", "corner"} <= kinds("brick", "p")
    assert {"axis", "wall"} <= kinds("neon", "p")
    assert {"towards", "away", "grazing+1e-7", "grazing-1e-7", "grazing_0"} <= kinds("light", "w")
    # through each of the quad's four corners (rim0 .. 3) and four edge midpoints (rim4 .. 7) exactly, and each one ulp outside
    for name in ("light", "speck"):
        assert {"rim%d" % i for i in range(8)} | {"rim%d+ulp" % i for i in range(8)} <= kinds(name, "w"), name
        slot = [n for n, _, _ in scenes.light_corner_list("all")].index(name)
        c = lc.make_cases(lc.light_geometry(desc, slot), name, lc.FIXTURE_CASES)
        assert {"rim%d" % i for i in range(8)} | {"rim%d+ulp" % i for i in range(8)} <= set(c["w_kind"]), name
    assert {"pole+", "pole-", "seam", "seam+ulp", "seam-ulp", "seam+0", "seam-0", "texel0"} <= kinds("env", "w") and {"cap_rim", "cap_rim+ulp", "cap_rim-ulp"} <= kinds("sun", "w")


@pytest.mark.parametrize("which,slot,name", LIGHTS, ids=IDS)
def test_oracle_is_the_reference_in_every_word(which, slot, name, gold, corner_scenes):
    desc = corner_scenes[which][1].desc
    n = lc.FIXTURE_CASES
    c = {k: gold["%s_%s" % (which, k)][slot*n:(slot + 1)*n] for k in ("p", "w")}
    ref = lc.chosen_as_objects(gold[which + "_ref"][slot*n:(slot + 1)*n], desc)
    xc, xs = lc.streams(SCENES.index(which), slot, n, extra=0)
    got = lc.oracle_words(desc, slot, c, xc, xs)
    dirac = desc.contents.objects[desc.contents.lights[slot]].type == lc.POINT
    bad = [int(i) for i in np.nonzero(lc.differing(got, ref, dirac=dirac))[0]]
    print("%s/%s: %d of %d cases differ; chosen %d, sampled %d, hit %d" % (which, name, len(bad), n, int((ref[:, 0].view(np.int32) >= 0).sum()),
                                                                          int((ref[:, 2] == 1).sum()), int((ref[:, 9] == 1).sum())))
    assert bad == PINNED.get("%s/%s" % (which, name), []), "%s/%s: cases %s differ from the reference, e.g. %s" % (
        which, name, bad[:8], [(lc.WORDS[w], hex(got[bad[0], w]), hex(ref[bad[0], w])) for w in np.nonzero(got[bad[0]] != ref[bad[0]])[0]] if bad else None)


def test_residual_is_within_its_cap():
    assert sum(len(v) for v in PINNED.values()) <= 0.001*len(LIGHTS)*lc.FIXTURE_CASES
    assert set(PINNED) <= set(IDS)


def test_fixture_exercises_every_block(gold):
    """No block of a light drops out of the comparison: every light is chosen from, most are sampled and hit in some cases and refused in others."""
    n = lc.FIXTURE_CASES
    for which, slot, name in LIGHTS:
        ref = gold[which + "_ref"][slot*n:(slot + 1)*n]
        kind = scenes.light_corner_list(which)[slot][1]
        ok, hit = int((ref[:, 2] == 1).sum()), int((ref[:, 9] == 1).sum())
        chosen = ref[:, 0].view(np.int32) >= 0
        assert ok >= 8, (which, name)
        if which == "backs":      # every weight 0 above the two face-down quads: chooseLight's total == 0 leg answers "no light"; below them it chooses
            assert 8 <= int(chosen.sum()) <= n - 8, (which, name)
        else:
            assert chosen.all(), (which, name)
        if which == "unknown":    # every weight "unknown": both lights get pdf 1, the weight is their number
            assert (ref[:, 8].view(np.float32) < 0).all() and (ref[:, 1].view(np.float32) == 2.0).all(), (which, name)
        assert (hit == 0) if kind in ("point", "mesh") else hit >= 8, (which, name)
        if kind in ("quad", "disk", "cube", "sphere", "cylinder", "mesh"):
            assert ok < n, (which, name)                                # some shading points lie behind or inside the emitter
        if kind not in ("infinite_sphere", "skydome", "point", "mesh"):
            assert hit < n, (which, name)
    # chooseLight's three legs: one light; known weights only; a light that answers "unknown" (the mesh and the cylinders always, the speck from afar)
    approx = gold["all_ref"][:, 8].view(np.float32)
    assert (approx < 0).any() and (gold["solids_ref"][:, 8].view(np.float32) < 0).any()
    assert np.isnan(gold["solids_ref"][:, 3:8].view(np.float32)).any()   # 0/0 at the point light's own position is recorded, not avoided


def test_batched_entry_is_the_per_call_entry(corner_scenes):
    """oracle_light_cases runs the statics oracle_light_sample runs (lights that draw exactly two numbers)."""
    desc = corner_scenes["all"][1].desc
    names = [n for n, _, _ in scenes.light_corner_list("all")]
    for name in ("light", "bulb", "spot", "env", "sun", "env_blade"):
        slot = names.index(name)
        n = 12
        c = lc.make_cases(lc.light_geometry(desc, slot), name, n)
        xc, xs = lc.streams(3, slot, n, extra=0)
        got = lc.oracle_words(desc, slot, c, xc, xs)
        for k in range(n):
            ok, d, dist, pdf = oracle_lib.light_sample(desc, slot, c["p"][k], float(xs[k, 0]), float(xs[k, 1]))
            assert bool(got[k, 2]) == ok, (name, k)
            if ok:
                want = np.concatenate([np.asarray(d, np.float32), np.float32([dist, pdf])]).view(np.uint32)
                assert (got[k, 3:8] == want).all() and got[k, 19] == 2, (name, k)


def _rule_scenes():
    return [("golden", n) for n in sorted(scenes.GOLDEN_CASES)] + [("light_corners", w) for w in SCENES]


@pytest.mark.parametrize("group,name", _rule_scenes(), ids=["%s-%s" % s for s in _rule_scenes()])
def test_every_family_a_scene_may_get_holds_the_needs_of_all_its_lights(group, name, tmp_path):
    """The rule check: whichever shading family the launch code may pick for a scene (light_cases.families_for, from tgh_scene_check's traits), its mask
    holds the feature bits of every light in the scene (SceneCheck.cpp: lightNeeds) -- or a kernel would fold one of the scene's lights away."""
    if group == "golden":
        if name == "water_caustic" and not scenes.have_water_caustic():
            pytest.skip("water-caustic assets (assets/) not present")
        if "materialtest" in name and not scenes.have_materialtest():
            pytest.skip("materialtest assets (assets/) not present")
        mk, kw = scenes.GOLDEN_CASES[name]
        path = mk(tmp_path, **dict(kw, resolution=(32, 18), spp=1))
    else:
        path = scenes.light_corners(tmp_path, name)
    flat = tg.FlattenedScene(path)
    t = _traits(flat.desc)
    fams = lc.families_for(t)
    for v in sorted(fams):
        needs, covered, mask = _needs(flat.desc, v)
        assert covered.all(), "%s: family %s (mask %#x) lacks %s" % (name, capi.TGHIP_BSDF_VARIANT_NAMES[v], mask, [hex(x & ~mask) for x in needs])
    flat.close()
    if group == "light_corners":
        assert fams == {"lean": {lc.ALL, lc.LEAN, lc.COAT, lc.GLASS, lc.PLASTIC, lc.TAIL, lc.FULL},
                        "solids": {lc.ALL, lc.SIMPLE, lc.COAT, lc.GLASS, lc.PLASTIC, lc.TAIL, lc.FULL},
                        "mesh": {lc.ALL, lc.FULL}, "all": {lc.ALL}, "unknown": {lc.ALL, lc.FULL},
                        "backs": {lc.ALL, lc.SIMPLE, lc.COAT, lc.GLASS, lc.PLASTIC, lc.TAIL, lc.FULL}}[name]


def test_needs_follow_the_emitter(corner_scenes):
    """lightNeeds on the `all` scene, bit by bit (csrc/hip/pt_variants.h)."""
    BITMAP, INFINITE, MULTI, SOLIDS, MESHLIGHT, CYLINDER = 1 << 24, 1 << 25, 1 << 26, 1 << 28, 1 << 29, 1 << 21
    FAMILY_ALL = (1 << 23) | (1 << 22) | (1 << 21) | (1 << 20)
    needs, covered, mask = _needs(corner_scenes["all"][1].desc, lc.ALL)
    want = {"light": 0, "speck": 0, "brick": SOLIDS, "bulb": SOLIDS, "spot": SOLIDS, "lamp": SOLIDS | INFINITE, "sky": INFINITE, "env": INFINITE | BITMAP,
            "sun": INFINITE, "dome": INFINITE | BITMAP, "shard": MESHLIGHT, "neon": CYLINDER, "tube": CYLINDER, "env_checker": INFINITE | FAMILY_ALL,
            "env_disk": INFINITE | FAMILY_ALL, "env_blade": INFINITE | FAMILY_ALL}
    for slot, (name, _, _) in enumerate(scenes.light_corner_list("all")):
        assert needs[slot] == want[name] | MULTI, name
    assert covered.all() and mask & (1 << 30) == 0
    assert (_needs(corner_scenes["lean"][1].desc, lc.LEAN)[0] == 0).all()          # one light: no FEAT_MULTILIGHT
    assert tg.lib.tgh_light_needs(corner_scenes["all"][1].desc, capi.TGHIP_BSDF_VARIANT_COUNT, None, None, None) == capi.TGHIP_E_INVALID
    assert tg.lib.tgh_light_needs(corner_scenes["all"][1].desc, -1, None, None, None) == capi.TGHIP_E_INVALID


@pytest.mark.skipif(not os.path.exists(os.path.join(scenes.ROOT, "oracle", "_ref", "ref_harness")), reason="reference harness (oracle/_ref) not built")
@pytest.mark.parametrize("which", SCENES)
def test_reference_harness_reproduces_the_light_fixture(which, gold, corner_scenes, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(scenes.ROOT, "tools"))
    import make_light_golden
    path, flat = corner_scenes[which]
    names, slots, cases, xc, xs = make_light_golden.scene_cases(flat.desc, which, lc.FIXTURE_CASES)
    ref = make_light_golden.reference_words(path, slots, cases, xc, xs, str(tmp_path))
    same = (ref == gold[which + "_ref"]) | (np.isnan(ref.view(np.float32)) & np.isnan(gold[which + "_ref"].view(np.float32)))
    assert same.all()
