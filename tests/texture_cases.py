"""Case table of the `disk`, `blade` and `ies` textures (textures/DiskTexture.cpp, BladeTexture.cpp, IesTexture.cpp of the reference): Cornell
box variants with those textures in every slot that takes one, and the builders that write them.  tests/test_textures_cpu.py and
tests/test_gpu_textures.py run them; tools/make_texture_golden.py renders tests/golden/<case>_samples.npz from them with the reference itself.

Every case is 48 x 27 at 8 spp (10 368 samples) on the Cornell box with both blocks a millimetre off the floor (no coincident faces: no tie
for the traversal order to decide, tests/scenes.py: LIFTED_CASES).  The .ies inputs are the small authored files under tests/golden/ies/."""
import math
import os
import shutil

import scenes
from scenes import _fog, _prim, _replace_bsdf

IES_DIR = os.path.join(scenes.GOLDEN, "ies")
IES_FILES = ("c0.ies", "c90.ies", "c180.ies", "c360.ies", "b_neg.ies", "tilt_commas.ies")
MISSING_IES = "no_such_profile.ies"          # a path that does not exist: texels of INV_TWO_PI
SIZE = dict(resolution=(48, 27), spp=8)


def _lift(scene):
    for p in scene["primitives"]:
        if p["type"] == "cube":
            p["transform"]["position"][1] += 1e-3


def _open_to_the_sky(scene):
    """No ceiling and no quad light: what lights the box comes in from above and through the open front."""
    scene["primitives"] = [p for p in scene["primitives"] if p["name"] not in ("ceiling", "light")]


def _albedo(scene):
    """Disk and blade as albedo, on quads and on a cube: 3, 5, 6 (the default, with its default angle) and 8 blades, angles of either sign,
    scalar and RGB values."""
    _replace_bsdf(scene, "floor", {"type": "lambert", "albedo": {"type": "disk", "value": [0.725, 0.4, 0.2]}})
    _replace_bsdf(scene, "ceiling", {"type": "lambert", "albedo": {"type": "disk", "value": 0.6}})
    _replace_bsdf(scene, "backWall", {"type": "lambert", "albedo": {"type": "blade", "blades": 5, "angle": 0.3, "value": 0.8}})
    _replace_bsdf(scene, "leftWall", {"type": "lambert", "albedo": {"type": "blade", "value": [0.63, 0.3, 0.05]}})
    _replace_bsdf(scene, "rightWall", {"type": "lambert", "albedo": {"type": "blade", "blades": 3, "angle": -0.7, "value": [0.14, 0.45, 0.6]}})
    _replace_bsdf(scene, "tallBox", {"type": "lambert", "albedo": {"type": "blade", "blades": 8, "angle": 1.9, "value": 0.7}})
    _replace_bsdf(scene, "shortBox", {"type": "lambert", "albedo": {"type": "disk"}})


def _slots(scene):
    """The scalar slots: disk as the roughness of two microfacet BSDFs, blade as the ratio of `mixed`, and bump slots that hold a disk and a
    blade -- no derivatives, but not constant either: the shading frame comes from the primitive's tangent space (Primitive.cpp:125-163)."""
    _replace_bsdf(scene, "floor", dict({"type": "rough_conductor", "distribution": "ggx", "albedo": [0.8, 0.75, 0.7],
                                        "roughness": {"type": "disk", "value": 0.35}}, **scenes._CU))
    _replace_bsdf(scene, "tallBox", {"type": "rough_plastic", "ior": 1.5, "distribution": "beckmann", "albedo": [0.3, 0.5, 0.7],
                                     "roughness": {"type": "disk", "value": 0.2}, "bump": {"type": "blade", "blades": 4, "angle": 0.4}})
    _replace_bsdf(scene, "backWall", {"type": "mixed", "albedo": 1, "ratio": {"type": "blade", "blades": 7, "angle": 0.15, "value": 0.75},
                                      "bsdf0": {"type": "lambert", "albedo": [0.7, 0.7, 0.2]}, "bsdf1": {"type": "mirror", "albedo": 0.9}})
    _replace_bsdf(scene, "leftWall", {"type": "rough_plastic", "ior": 1.4, "distribution": "ggx", "roughness": 0.2, "albedo": [0.63, 0.2, 0.1],
                                      "bump": {"type": "disk", "value": 0.5}})
    scene["bsdfs"].append(dict({"name": "ballMat", "type": "rough_conductor", "distribution": "beckmann", "roughness": 0.1, "albedo": 1,
                                "bump": {"type": "disk"}}, **scenes._CU))
    scene["primitives"].append({"name": "ball", "type": "sphere", "bsdf": "ballMat", "transform": {"position": [0.5, 1.2, 0.3], "scale": 0.22, "rotation": [20, 35, 10]}})


def _cutouts(scene):
    """`transparency` quads whose alpha is a disk and a blade, between the light and the floor: camera paths and shadow rays cross them
    (TraceBase::generalizedShadowRay, TraceBase.cpp:62-125, evaluates alpha on the way)."""
    scene["bsdfs"] += [
        {"name": "hole", "type": "transparency", "albedo": 1, "alpha": {"type": "disk", "value": 0.85}, "base": {"type": "lambert", "albedo": [0.3, 0.5, 0.7]}},
        {"name": "star", "type": "transparency", "albedo": 1, "alpha": {"type": "blade", "blades": 5, "angle": 0.6}, "base": {"type": "lambert", "albedo": [0.7, 0.6, 0.2]}}]
    scene["primitives"] += [
        {"name": "hole", "type": "quad", "bsdf": "hole", "transform": {"position": [0.05, 1.55, -0.1], "scale": [1.5, 1, 1.4], "rotation": [0, 15, 0]}},
        {"name": "star", "type": "quad", "bsdf": "star", "transform": {"position": [0.3, 0.9, 0.45], "scale": [0.8, 1, 0.7], "rotation": [8, 40, -6]}}]


def _cutouts_in_fog(scene):
    _cutouts(scene)
    _fog(scene)


def _lights(scene):
    """Two area lights: the ceiling light with a disk emission (a round lamp) and a quad on the left wall whose `power` is a blade texture
    (Primitive::prepareForRender clones it and scales its value): TraceBase::chooseLight weighs both by their textures' averages."""
    _prim(scene, "light")["emission"] = {"type": "disk", "value": [17, 12, 4]}
    scene["primitives"].append({"name": "light2", "type": "quad", "bsdf": "light", "power": {"type": "blade", "blades": 7, "angle": 0.2, "value": [3, 9, 14]},
                                "transform": {"position": [-0.98, 0.6, 0.2], "scale": [0.3, 0.3, 0.3], "rotation": [0, 0, -90]}})


def _environment(emission, sample, rotation):
    def edit(scene):
        _open_to_the_sky(scene)
        scene["primitives"].append({"name": "env", "type": "infinite_sphere", "emission": emission, "sample": sample, "transform": {"rotation": rotation}})
    return edit


def _ies_spheres(scene):
    """Five small sphere lights, one photometric profile each: type C files whose horizontal angles end at 0, 90, 180 and 360 degrees, and the
    file with TILT=INCLUDE and commas given as `power`.  The first uses the default resolution (256).  (The file that does not exist is held
    to its texels by tests/test_textures_cpu.py alone: the reference itself cannot render it -- IesTexture::loadResources hands wrapHorzAngles
    a photometric type it never read and, where that garbage is 1, the last element of an empty list.)"""
    _prim(scene, "light")["emission"] = [1.0, 0.8, 0.5]
    profiles = [{"type": "ies", "file": "c0.ies"}, {"type": "ies", "file": "c90.ies", "resolution": 32}, {"type": "ies", "file": "c180.ies", "resolution": 24},
                {"type": "ies", "file": "c360.ies", "resolution": 48}]
    spots = [[-0.6, 1.5, 0.3], [0.0, 1.6, 0.55], [0.6, 1.45, 0.2], [-0.45, 0.5, 0.65]]
    for i, (tex, pos) in enumerate(zip(profiles, spots)):
        scene["primitives"].append({"name": "lamp%d" % i, "type": "sphere", "bsdf": "light", "emission": tex,
                                    "transform": {"position": pos, "scale": 0.09, "rotation": [25*i, 40 + 10*i, 15]}})
    scene["primitives"].append({"name": "lamp4", "type": "sphere", "bsdf": "light", "power": {"type": "ies", "file": "tilt_commas.ies", "resolution": 20},
                                "transform": {"position": [0.1, 0.3, 0.8], "scale": 0.08, "rotation": [70, 0, 20]}})


def missing_ies(scene):
    """One sphere light whose profile is a path that does not exist (the loader's fall-back: 2R x R texels of INV_TWO_PI)."""
    scene["primitives"].append({"name": "lamp", "type": "sphere", "bsdf": "light", "emission": {"type": "ies", "file": MISSING_IES, "resolution": 8},
                                "transform": {"position": [0.7, 0.85, 0.7], "scale": 0.09}})


# The card: the camera looks straight at an emissive quad that nearly fills the frame, through the dirac filter, one bounce -- every sample is
# one lookup of the 32 x 16 bake at a pixel centre (u runs along the card's width), and the 47 x 26 pixel centres on the card reach every texel.
_CARD_DISTANCE = 3.8
_CARD_WIDTH = 0.98*2.0*_CARD_DISTANCE*math.tan(math.radians(35.0)/2.0)
_CARD_HEIGHT = _CARD_WIDTH*27.0/48.0


def _ies_card(scene):
    scene["camera"]["reconstruction_filter"] = "dirac"
    _prim(scene, "light")["emission"] = [1.0, 0.8, 0.5]
    scene["primitives"].append({"name": "card", "type": "quad", "bsdf": "light", "emission": {"type": "ies", "file": "tilt_commas.ies", "resolution": 16},
                                "transform": {"position": [0, 1, 6.8 - _CARD_DISTANCE], "scale": [_CARD_WIDTH, 1, _CARD_HEIGHT], "rotation": [90, 0, 0]}})


def build(tmpdir, edit=None, **kw):
    """Writes the Cornell box variant (blocks lifted) and puts the .ies fixtures next to it, where "file" looks for them."""
    tmpdir = str(tmpdir)
    for f in IES_FILES:
        dst = os.path.join(tmpdir, f)
        if not os.path.exists(dst):
            shutil.copyfile(os.path.join(IES_DIR, f), dst)

    def both(scene):
        _lift(scene)
        if edit:
            edit(scene)
    return scenes.cornell(tmpdir, **dict(kw, edit=both))


# name -> (builder, kwargs), the layout of scenes.GOLDEN_CASES: tests/golden/<name>_samples.npz
CASES = {
    "tex_albedo": (build, dict(SIZE, edit=_albedo)),
    "tex_slots": (build, dict(SIZE, edit=_slots)),
    "tex_slots_sobol": (build, dict(SIZE, edit=_slots, renderer={"stratified_sampler": True})),
    "tex_cutout": (build, dict(SIZE, edit=_cutouts)),
    "tex_cutout_fog": (build, dict(SIZE, edit=_cutouts_in_fog)),
    "tex_lights": (build, dict(SIZE, edit=_lights)),
    "tex_env_disk": (build, dict(SIZE, edit=_environment({"type": "disk", "value": [1.6, 1.3, 0.9]}, True, [70, 30, 0]))),
    "tex_env_blade": (build, dict(SIZE, edit=_environment({"type": "blade", "blades": 5, "angle": 0.25, "value": [0.8, 1.1, 1.7]}, True, [-60, 10, 25]))),
    "tex_env_disk_unsampled": (build, dict(SIZE, edit=_environment({"type": "disk", "value": 1.4}, False, [80, -20, 10]))),
    "tex_ies_spheres": (build, dict(SIZE, edit=_ies_spheres)),
    "tex_ies_env": (build, dict(SIZE, edit=_environment({"type": "ies", "file": "b_neg.ies", "resolution": 64}, True, [15, 50, -5]))),
    "tex_ies_card": (build, dict(SIZE, integrator={"max_bounces": 1}, edit=_ies_card)),
}
# the cases an unchanged CPU oracle renders too: an `ies` texture flattens to an ordinary scalar bitmap
IES_CASES = ("tex_ies_spheres", "tex_ies_env", "tex_ies_card")
# cases whose shadow rays are closest-hit walks that evaluate a disk / blade alpha on the way (k_trace_shadow_tex)
CUTOUT_CASES = ("tex_cutout", "tex_cutout_fog")


def declared_textures(scene):
    """Every {"type": "disk" | "blade" | "ies", ...} object of a scene's JSON, with the key it sits under, in document order."""
    out = []

    def walk(node, key):
        if isinstance(node, dict):
            if node.get("type") in ("disk", "blade", "ies") and key in ("albedo", "roughness", "ratio", "alpha", "bump", "emission", "power"):
                out.append((key, node))
            for k, v in node.items():
                walk(v, k)
        elif isinstance(node, list):
            for v in node:
                walk(v, key)
    walk(scene, None)
    return out
