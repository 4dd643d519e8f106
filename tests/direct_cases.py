"""Case table of tghip_query_direct: the scenes, the seeded rays and the per-call parameters whose answers the reference's own
TraceBase::estimateDirect / volumeEstimateDirect gives (tools/ref_direct.cpp, recorded by tools/make_direct_golden.py into
tests/golden/direct_cases.npz), and the census of the legs those cases reach.  tests/test_direct_query_cpu.py takes the census from the committed
golden; tests/test_gpu_direct_query.py holds the device to every case, bit for bit.

A group is one call: a scene, its rays, the sample indices, the seed, a start medium by its JSON name (or one per ray), the bounce, a light by its
JSON name (or chooseLight), the numbers skipped and the mode.  Scenes are 16 x 9 variants of the Cornell box from tests/scenes.py."""
import json
import os

import numpy as np

import scenes
from scenes import (_area_lights, _atmosphere, _checker_light, _expfog, _fog, _fog_and_smoke, _point_lights, _rayleigh_fog, _sun_and_sky, _two_lights)
from transmittance_cases import _box, _caps, _panes, _segments, _veil, _with, names_of

GOLDEN = os.path.join(scenes.GOLDEN, "direct_cases.npz")
SEED = 0xD12EC7
SMALL = dict(resolution=(16, 9), spp=1)
(LEG_LIGHT_TERM, LEG_BSDF_TERM, LEG_DIRAC, LEG_PURE_SPECULAR, LEG_FORWARD, LEG_INCONSISTENT, LEG_FLIPPED, LEG_MESH_REJECTED, LEG_MESH_ACCEPTED,
 LEG_CROSSED_FORWARD, LEG_CROSSED_FRACTIONAL, LEG_MAX_BOUNCES, LEG_INSTANCE, LEG_MEDIUM_SELECTED, LEG_UNKNOWN_WEIGHT) = (1 << k for k in range(15))


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------

CORNER_MATERIALS = {"floor": "plain_rough_conductor", "backWall": "plain_rough_coat", "leftWall": "plain_transparency", "rightWall": "plain_rough_plastic",
                    "shortBox": "plain_smooth_coat", "tallBox": "plain_rough_dielectric", "ceiling": "plain_oren_nayar"}
ROUGH, COATED, TRANSPARENCY = ("plain_rough_conductor", "plain_rough_plastic", "plain_rough_dielectric"), ("plain_rough_coat", "plain_smooth_coat"), ("plain_transparency",)


def _corner_materials(scene):
    for p in scene["primitives"]:
        if p["name"] in CORNER_MATERIALS:
            p["bsdf"] = CORNER_MATERIALS[p["name"]]


def _haze_block(scene):
    """The fogged box with the short block an ordinary surface that says which medium is around and inside it: a shadow ray that leaves it travels
    in the haze, not in the fog the ray arrived in"""
    _fog(scene)
    scene["media"].append({"name": "haze", "type": "homogeneous", "sigma_a": [0.3, 0.2, 0.1], "sigma_s": [0.4, 0.5, 0.6]})
    block = next(p for p in scene["primitives"] if p["name"] == "shortBox")
    block["int_medium"] = block["ext_medium"] = "haze"


def _hg_fog(scene):
    _fog(scene)
    scene["media"][-1]["phase_function"] = {"type": "henyey_greenstein", "g": 0.6}


SCENES = {
    "dq_box": lambda t, n: scenes.cornell(t, name=n, **SMALL),
    "dq_two_lights": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_two_lights),
    "dq_area_lights": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_area_lights),
    "dq_point_lights": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_point_lights),
    "dq_mesh_light": lambda t, n: scenes.cornell_mesh_light(t, name=n, **SMALL),
    "dq_caps": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_caps),
    "dq_sun_and_sky": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_sun_and_sky),
    "dq_light_corners": lambda t, n: scenes.light_corners(t, "all", name=n, **SMALL),
    "dq_bsdf_corners": lambda t, n: scenes.bsdf_corners(t, name=n, **SMALL, edit=_corner_materials),
    "dq_panes": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_panes),
    "dq_panes_mb3": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_with(_panes, max_bounces=3)),
    "dq_instances": lambda t, n: scenes.cornell_instances(t, name=n, **SMALL, edit=_with(_veil, enable_consistency_checks=True)),
    "dq_haze": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_haze_block),
    "dq_fog_smoke": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_fog_and_smoke),
    "dq_fog": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_fog),
    "dq_fog_hg": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_hg_fog),
    "dq_fog_rayleigh": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_rayleigh_fog),
    "dq_expfog": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_expfog),
    "dq_atmosphere": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_atmosphere),
    "dq_checker_light": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_checker_light),
}


def build_scene(name, tmpdir):
    return SCENES[name](str(tmpdir), name + ".json")


def light_slots(path):
    """name -> slot in TgHipSceneDesc::lights and TraceableScene::lights(): the scene's sampled emitters in file order"""
    with open(path) as f:
        scene = json.load(f)
    lights = [p["name"] for p in scene["primitives"]
              if ("emission" in p or "power" in p or p["type"] == "skydome") and (p["type"] not in ("infinite_sphere", "infinite_sphere_cap", "skydome") or p.get("sample", True))]
    return {name: i for i, name in enumerate(lights)}


def primitives_of(path):
    with open(path) as f:
        return json.load(f)["primitives"]


# ---- rays ---------------------------------------------------------------------------------------------------------------------------------------

def into_box(rs, n):
    """From in front of the open box at points inside it, never ending: walls, floor, ceiling, blocks, whatever stands in the box"""
    a = _box(rs, n, (-0.8, 0.3, 1.2), (0.8, 1.7, 2.5))
    b = _box(rs, n, (-0.95, 0.02, -0.95), (0.95, 1.95, 0.9))
    return _segments(a, b, True)


def at_region(rs, n, lo, hi):
    a = _box(rs, n, (-0.8, 0.3, 1.2), (0.8, 1.7, 2.5))
    return _segments(a, _box(rs, n, lo, hi), True)


def from_outside(rs, n):
    """At the walls from outside the box: their back sides, with a few misses past the box"""
    side = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)
    a = _box(rs, n, (1.5, 0.2, -0.8), (2.5, 1.8, 0.8))
    a[:, 0] *= side
    b = _box(rs, n, (0.2, 0.1, -0.9), (0.9, 2.3, 0.9))
    b[:, 0] *= side
    return _segments(a, b, True)


def in_the_box(rs, n):
    """Volume mode: points in the free space of the box and the direction the path came along"""
    a = _box(rs, n, (-0.9, 0.8, 0.0), (0.9, 1.9, 0.9))
    return _segments(a, a + rs.normal(size=(n, 3)), True)


# ---- groups -------------------------------------------------------------------------------------------------------------------------------------

def _group(scene, leg, rays, spp=(0, 2), seed=SEED, medium=None, media=None, bounce=1, light=None, skip=0, volume=False):
    return dict(scene=scene, leg=leg, rays=np.ascontiguousarray(rays, np.float32), spp=[int(spp[0]), int(spp[1])], seed=int(seed), medium=medium,
                media=media, bounce=int(bounce), light_name=light, skip=int(skip), volume=bool(volume))


def make_groups():
    rs = np.random.RandomState(SEED)
    g = []
    box = into_box(rs, 128)
    g.append(_group("dq_box", "box", box, spp=(0, 3)))
    g.append(_group("dq_box", "box_light_0", box, spp=(0, 3), light="light"))                    # one light: slot 0 and chooseLight are the same call
    g.append(_group("dq_box", "skip", into_box(rs, 64), spp=(2, 5), skip=3, seed=SEED + 7))
    two = into_box(rs, 96)
    g.append(_group("dq_two_lights", "two_lights", two))
    g.append(_group("dq_two_lights", "fixed_light", two, light="light2"))
    g.append(_group("dq_area_lights", "area_lights", into_box(rs, 96)))
    g.append(_group("dq_point_lights", "dirac", into_box(rs, 128)))
    g.append(_group("dq_mesh_light", "mesh", into_box(rs, 192)))
    g.append(_group("dq_caps", "caps", into_box(rs, 256), medium="fog"))
    g.append(_group("dq_sun_and_sky", "sun_and_sky", into_box(rs, 192)))
    g.append(_group("dq_light_corners", "sixteen_lights", into_box(rs, 320), spp=(0, 1)))
    g.append(_group("dq_bsdf_corners", "materials", into_box(rs, 320)))
    # under the pane stack (x -0.2 .. 0.8, z -0.3 .. 0.7, y 1.35 .. 1.65): the floor and the short block below it, and the panes themselves
    g.append(_group("dq_panes", "under_panes", at_region(rs, 160, (0.0, 0.0, -0.1), (0.6, 0.0, 0.5))))
    g.append(_group("dq_panes", "at_panes", at_region(rs, 96, (-0.1, 1.35, -0.2), (0.7, 1.65, 0.6))))
    g.append(_group("dq_panes_mb3", "max_bounces", at_region(rs, 192, (0.0, 0.0, -0.1), (0.6, 0.0, 0.5))))
    g.append(_group("dq_box", "back_sides", from_outside(rs, 96)))
    g.append(_group("dq_instances", "instances", into_box(rs, 256)))
    g.append(_group("dq_haze", "select_medium", at_region(rs, 128, (0.1, 0.1, 0.1), (0.55, 0.6, 0.65)), medium="fog"))
    # the ceiling around the mesh emitter (a dented ball under it): grazing views, where a dent's rim is nearer than the sampled point behind it
    g.append(_group("dq_mesh_light", "mesh_grazing", at_region(rs, 512, (-0.5, 2.0, -0.6), (0.7, 2.0, 0.6)), spp=(0, 3)))
    rays = into_box(rs, 96)
    g.append(_group("dq_fog_smoke", "media_per_ray", rays, medium="fog", media=[("fog", "-", "smoke")[i % 3] for i in range(len(rays))]))
    # volume mode: the three phase functions in the homogeneous fog, the exponential and the atmospheric medium
    for scene, leg in (("dq_fog", "volume_isotropic"), ("dq_fog_hg", "volume_henyey_greenstein"), ("dq_fog_rayleigh", "volume_rayleigh"),
                       ("dq_expfog", "volume_exponential"), ("dq_atmosphere", "volume_atmosphere")):
        g.append(_group(scene, leg, in_the_box(rs, 64), medium="fog", volume=True))
    rays = in_the_box(rs, 64)
    g.append(_group("dq_caps", "volume_caps", rays, medium="fog", volume=True, media=[("fog", "-")[i % 4 == 3] for i in range(len(rays))]))
    g.append(_group("dq_point_lights", "volume_dirac", in_the_box(rs, 64), medium=None, volume=True, media=["-"]*64))      # no medium: nothing is taken
    # the floor under the checkered light: half of the light samples end on a black square -- a transmittance is recorded, no light comes
    g.append(_group("dq_checker_light", "black_light_sample", at_region(rs, 128, (-0.4, 0.0, -0.4), (0.4, 0.0, 0.4)), spp=(0, 3)))
    return g


# ---- the golden ---------------------------------------------------------------------------------------------------------------------------------

PARTS = ("rays", "rgb", "transmittance", "recorded", "taken", "legs", "light", "hit")


def load_golden():
    """The groups with the reference's answers per ray and sample: rgb [n, spp, 3] and transmittance [n, spp] uint32 (the floats' bits), recorded,
    taken, legs (LEG_*), light and hit (primitive indices, -1 = none) [n, spp]"""
    z = np.load(GOLDEN, allow_pickle=False)
    table = json.loads(str(z["groups"]))
    groups = []
    for k, t in enumerate(table):
        g = dict(t)
        for part in PARTS:
            g[part] = z["g%03d_%s" % (k, part)]
        groups.append(g)
    return groups


def expected(g):
    """What tghip_query_direct answers for a group of the golden: rgb [n, 3] and visibility [n] float32 summed in sample order from zero, count and
    visibility_count [n]"""
    n, spp = g["taken"].shape
    rgb, vis = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    count, vcount = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for s in range(spp):
        rgb = (rgb + g["rgb"][:, s].view(np.float32)).astype(np.float32)
        rec = g["recorded"][:, s] != 0
        vis = np.where(rec, (vis + g["transmittance"][:, s].view(np.float32)).astype(np.float32), vis)
        vcount += rec
        count += g["taken"][:, s] != 0
    return rgb, vis, count, vcount


def census(groups, primitives):
    """leg -> number of (ray, sample) items that reach it.  primitives: scene name -> the scene file's primitives"""
    c = {}

    def add(leg, mask):
        c[leg] = c.get(leg, 0) + int(np.count_nonzero(mask))

    for g in groups:
        legs, leg, prims = g["legs"], g["leg"], primitives[g["scene"]]
        lit = (g["rgb"].view(np.float32) != 0).any(axis=2)
        kind = np.array([p["type"] for p in prims] + ["none"])[g["light"]]
        material = np.array([p.get("bsdf") if isinstance(p.get("bsdf"), str) else "" for p in prims] + [""])[g["hit"]]
        add("light_term", legs & LEG_LIGHT_TERM)
        add("bsdf_term", legs & LEG_BSDF_TERM)
        add("dirac_light", ((legs & LEG_DIRAC) != 0) & lit)
        add("mesh_accepted", legs & LEG_MESH_ACCEPTED)
        add("mesh_rejected", legs & LEG_MESH_REJECTED)
        if g["scene"] == "dq_caps" and not g["volume"]:
            for k in ("sphere", "cube", "disk"):
                add(k + "_emitter", (kind == k) & lit)
        if g["scene"] == "dq_sun_and_sky":
            add("infinite_emitter", (kind == "infinite_sphere") & lit)
            add("sun_cap", (kind == "infinite_sphere_cap") & lit)
        if g["scene"] == "dq_light_corners":
            add("choose_among_16", g["light"] >= 0)
        add("black_light_sample", (g["recorded"] != 0) & (g["transmittance"].view(np.float32) > 0) & ((legs & LEG_LIGHT_TERM) == 0))
        add("unknown_weight", legs & LEG_UNKNOWN_WEIGHT)
        add("pure_specular_return", legs & LEG_PURE_SPECULAR)
        add("forward_return", legs & LEG_FORWARD)
        add("inconsistent", legs & LEG_INCONSISTENT)
        add("flipped_frame", legs & LEG_FLIPPED)
        if g["scene"] == "dq_bsdf_corners":
            add("rough_material", np.isin(material, ROUGH) & lit)
            add("coated_material", np.isin(material, COATED) & lit)
            add("transparency_material", np.isin(material, TRANSPARENCY) & lit)
        add("shadow_crosses_forward", ((legs & LEG_CROSSED_FORWARD) != 0) & ((legs & LEG_LIGHT_TERM) != 0))
        add("shadow_crosses_fractional", ((legs & LEG_CROSSED_FRACTIONAL) != 0) & ((legs & LEG_LIGHT_TERM) != 0))
        add("shadow_ends_at_max_bounces", legs & LEG_MAX_BOUNCES)
        add("through_instance", ((legs & LEG_INSTANCE) != 0) & lit)
        add("select_medium", ((legs & LEG_MEDIUM_SELECTED) != 0) & lit)
        if leg.startswith("volume_") and leg[7:] in ("isotropic", "henyey_greenstein", "rayleigh", "exponential", "atmosphere"):
            add(leg, lit)
        if g["light_name"] is not None:
            add("fixed_light", lit)
        if g["skip"] > 0:
            add("skip", lit)
        if g["media"] is not None:
            add("media_per_ray", lit)
    return c


LEGS = ["light_term", "bsdf_term", "dirac_light", "mesh_accepted", "mesh_rejected", "sphere_emitter", "cube_emitter", "disk_emitter", "infinite_emitter",
        "sun_cap", "choose_among_16", "unknown_weight", "pure_specular_return", "forward_return", "inconsistent", "flipped_frame", "rough_material",
        "coated_material", "transparency_material", "shadow_crosses_forward", "shadow_crosses_fractional", "shadow_ends_at_max_bounces",
        "through_instance", "select_medium", "volume_isotropic", "volume_henyey_greenstein", "volume_rayleigh", "volume_exponential",
        "volume_atmosphere", "fixed_light", "skip", "media_per_ray", "black_light_sample"]
