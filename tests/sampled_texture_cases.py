"""Case table of the slots where the reference SAMPLES a texture -- the emission of a sampled infinite_sphere (primitives/InfiniteSphere.cpp:161-176,
218-229) and the aperture of a thin-lens camera (cameras/ThinlensCamera.cpp:85-97) -- with the texture types that were not sampled there before: a
checker environment, and constant, checker and `ies` apertures.  With them the cap that takes its direction from a named primitive
(primitives/InfiniteSphereCap.cpp:233-250).  tests/test_sampled_textures_cpu.py and tests/test_gpu_sampled_textures.py run the cases;
tools/make_sampled_texture_golden.py renders tests/golden/<case>_samples.npz from them with the reference itself.

Every case is 48 x 27 at 8 spp (10 368 samples) on the Cornell box with both blocks a millimetre off the floor (texture_cases.build)."""
import scenes
import texture_cases
from scenes import _fog, _replace_bsdf
from texture_cases import SIZE, _environment, build

CHECKER = {"type": "checker", "on_color": [1.7, 1.2, 0.6], "off_color": [0.25, 0.45, 0.9], "res_u": 6, "res_v": 3}
# off colour black: onProb == 1, every sample lands on an "on" cell; 5 x 3: both resolutions odd (rows of two and of one cell)
CHECKER_ODD = {"type": "checker", "on_color": [1.4, 1.5, 1.1], "off_color": 0.0, "res_u": 5, "res_v": 3}
# on colour black: onProb == 0, the second branch for every sample
CHECKER_ON_BLACK = {"type": "checker", "on_color": [0.0, 0.0, 0.0], "off_color": [0.9, 1.3, 1.6], "res_u": 6, "res_v": 4}
ROTATION = [65, 35, -10]

# The fog of scenes._fog has no boundary, and the transmittance of a homogeneous medium along a ray that never ends is exp(-inf) = 0: an
# environment seen from inside it is black, sampled or not.  So the fog case closes the fog of scenes._fog into a box around the scene and the
# camera (a cube with the `forward` BSDF whose interior is the fog: shadow rays cross it and pick up the transmittance of the part inside,
# TraceBase.cpp:62-125), off every face of the Cornell box.
FOG_BOUNDS = {"name": "fogBounds", "type": "cube", "bsdf": "fogWall", "int_medium": "fog",
              "transform": {"position": [0.13, 1.27, 3.1], "scale": [6.3, 5.1, 9.7]}}


def _checker_in_fog(scene):
    _environment(CHECKER, True, ROTATION)(scene)
    _fog(scene)
    scene["bsdfs"].append({"name": "fogWall", "type": "forward"})
    scene["primitives"].append(dict(FOG_BOUNDS))


def _lens(aperture, cateye=0.0):
    def edit(scene):
        scene["camera"].update(type="thinlens", focus_distance=6.0, aperture_size=0.12, cateye=cateye, aperture=aperture)
    return edit


LENS_CONSTANT = {"type": "constant", "value": [0.9, 0.6, 0.3]}
LENS_CHECKER = {"type": "checker", "on_color": [1.0, 0.8, 0.6], "off_color": 0.25, "res_u": 4, "res_v": 3}
LENS_IES = {"type": "ies", "file": "c90.ies", "resolution": 32}

# ---- the cap's pivot ----
SKY_ROTATION = [30, 10, -20]
SUN = {"name": "sun", "type": "infinite_sphere_cap", "emission": [60, 52, 40], "cap_angle": 8, "sample": True}
SUN_OWN_TRANSFORM = {"rotation": [25, 0, -20]}
# a small quad on the ground next to the box: the cap points along ITS normal
DIAL_TRANSFORM = {"position": [1.6, 0.3, 0.4], "scale": [0.3, 1, 0.4], "rotation": [35, 10, -25]}


def _mirror_block(scene):
    _replace_bsdf(scene, "tallBox", {"type": "mirror", "albedo": [0.9, 0.9, 0.95]})


def _sun_pivot(twin=False):
    """The procedural sky, rotated, and a cap that names it (how sun-and-sky set-ups are written); twin: the same scene with the sky's transform
    written out on the cap."""
    def edit(scene):
        scenes._skydome()(scene)
        sky = next(p for p in scene["primitives"] if p["name"] == "sky")
        assert sky["transform"] == {"rotation": SKY_ROTATION}
        scene["primitives"].append(dict(SUN, transform=dict(sky["transform"])) if twin else dict(SUN, skydome="sky", transform=dict(SUN_OWN_TRANSFORM)))
    return edit


def _sun_pivot_other(twin=False):
    """Any primitive's name counts (Scene::findPrimitive): the cap names a quad that is listed BEHIND it."""
    def edit(scene):
        texture_cases._open_to_the_sky(scene)
        _mirror_block(scene)
        scene["primitives"].append({"name": "env", "type": "infinite_sphere", "emission": [0.25, 0.35, 0.6], "sample": True})
        scene["primitives"].append(dict(SUN, transform=dict(DIAL_TRANSFORM)) if twin else dict(SUN, skydome="dial", transform=dict(SUN_OWN_TRANSFORM)))
        scene["primitives"].append({"name": "dial", "type": "quad", "bsdf": "floor", "transform": dict(DIAL_TRANSFORM)})
    return edit


def _sun_pivot_missing(twin=False):
    """A name that matches nothing: the cap's own transform, and a note on stderr."""
    def edit(scene):
        texture_cases._open_to_the_sky(scene)
        _mirror_block(scene)
        scene["primitives"].append({"name": "env", "type": "infinite_sphere", "emission": [0.25, 0.35, 0.6], "sample": True})
        scene["primitives"].append(dict(SUN, transform=dict(SUN_OWN_TRANSFORM)) if twin else dict(SUN, skydome="no_such_sky", transform=dict(SUN_OWN_TRANSFORM)))
    return edit


_SOBOL = {"stratified_sampler": True}

# name -> (builder, kwargs), the layout of scenes.GOLDEN_CASES: tests/golden/<name>_samples.npz
CASES = {
    "stex_env_checker": (build, dict(SIZE, edit=_environment(CHECKER, True, ROTATION))),
    "stex_env_checker_odd": (build, dict(SIZE, edit=_environment(CHECKER_ODD, True, ROTATION))),
    "stex_env_checker_on_black": (build, dict(SIZE, edit=_environment(CHECKER_ON_BLACK, True, ROTATION))),
    "stex_env_checker_sobol": (build, dict(SIZE, edit=_environment(CHECKER, True, ROTATION), renderer=_SOBOL)),
    "stex_env_checker_fog": (build, dict(SIZE, edit=_checker_in_fog)),
    "stex_env_checker_unsampled": (build, dict(SIZE, edit=_environment(CHECKER, False, ROTATION))),
    "stex_lens_constant": (build, dict(SIZE, edit=_lens(LENS_CONSTANT))),
    "stex_lens_checker": (build, dict(SIZE, edit=_lens(LENS_CHECKER, cateye=0.12))),
    "stex_lens_checker_sobol": (build, dict(SIZE, edit=_lens(LENS_CHECKER, cateye=0.12), renderer=_SOBOL)),
    "stex_lens_ies": (build, dict(SIZE, edit=_lens(LENS_IES))),
    "stex_sun_pivot": (build, dict(SIZE, edit=_sun_pivot())),
    "stex_sun_pivot_other": (build, dict(SIZE, edit=_sun_pivot_other())),
    "stex_sun_pivot_missing": (build, dict(SIZE, edit=_sun_pivot_missing())),
}
# the cases whose sampled environment is a checker: shaded by the all-features family throughout
SAMPLED_CHECKER_CASES = ("stex_env_checker", "stex_env_checker_odd", "stex_env_checker_on_black", "stex_env_checker_sobol", "stex_env_checker_fog")
# case -> the same scene with the pivot's transform written out on the cap
PIVOT_TWINS = {
    "stex_sun_pivot": (build, dict(SIZE, edit=_sun_pivot(twin=True))),
    "stex_sun_pivot_other": (build, dict(SIZE, edit=_sun_pivot_other(twin=True))),
    "stex_sun_pivot_missing": (build, dict(SIZE, edit=_sun_pivot_missing(twin=True))),
}
# case -> the JSON of its aperture
LENS_CASES = {
    "stex_lens_constant": LENS_CONSTANT,
    "stex_lens_checker": LENS_CHECKER,
    "stex_lens_checker_sobol": LENS_CHECKER,
    "stex_lens_ies": LENS_IES,
}
