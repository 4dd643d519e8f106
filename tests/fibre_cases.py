"""Case table of the fibre BCSDFs `lambertian_fiber` and `rough_wire` (bsdfs/LambertianFiberBcsdf.cpp, bsdfs/RoughWireBcsdf.cpp of the reference) on
every primitive that has a tangent space: their lobes are anisotropic, so the shading frame comes from Primitive::tangentSpace
(Primitive::setupTangentFrame, primitives/Primitive.cpp:125-163) with or without a bump map.  tests/test_fibres_cpu.py and tests/test_gpu_fibres.py
run the cases; tools/make_fibre_golden.py renders tests/golden/<case>_samples.npz and tests/golden/fibre_bsdf_cases.npz from them with the reference
itself (the CPU oracle does not know the two types).

Every case is 48 x 27 at 8 spp (10 368 samples) on the Cornell box; where the blocks stay they stand a millimetre off the floor
(texture_cases.build)."""
import os

import numpy as np

import bsdf_cases as bc
import scenes
import texture_cases
from scenes import _fog, _prim, _replace_bsdf
from texture_cases import SIZE, build

BSDF_GOLDEN = os.path.join(scenes.GOLDEN, "fibre_bsdf_cases.npz")
LAMBERT_FIBRE = {"type": "lambertian_fiber", "albedo": [0.75, 0.6, 0.45]}
# roughness -> _v = sqr(roughness*PI_HALF): 0.05 and 0.15 take M()'s v < 0.1 branch (0.15: v = 0.0555, cosThetaI*cosThetaO/v reaches both sides of
# logI0's x > 12), 0.35 and 1.0 the sinh branch at 1/v of about 3.3 and 0.405.  One case spells eta / k out, two name a material, one keeps the default.
WIRE = {
    "r005": {"type": "rough_wire", "albedo": 1, "roughness": 0.05, "eta": [0.27, 0.68, 1.32], "k": [3.6, 2.6, 2.3]},
    "r015": {"type": "rough_wire", "albedo": [0.95, 0.9, 0.85], "roughness": 0.15, "material": "Au"},
    "r035": {"type": "rough_wire", "albedo": 1, "roughness": 0.35},
    "r100": {"type": "rough_wire", "albedo": [0.9, 0.9, 0.95], "roughness": 1.0, "material": "Al"},
}
CHECKER_ALPHA = {"type": "checker", "on_color": 1.0, "off_color": 0.0, "res_u": 5, "res_v": 4}


def _no_blocks(scene):
    scene["primitives"] = [p for p in scene["primitives"] if p["name"] not in ("shortBox", "tallBox")]


def _lambert_prims(scene):
    """lambertian_fiber on a quad, both cubes, a sphere, a disk and a capped cylinder: every analytic tangentSpace (the cylinder's T is its axis)."""
    for name in ("backWall", "tallBox", "shortBox"):
        _replace_bsdf(scene, name, LAMBERT_FIBRE)
    scene["bsdfs"].append(dict(LAMBERT_FIBRE, name="fibre", albedo=[0.5, 0.7, 0.8]))
    scene["primitives"] += [
        {"name": "ball", "type": "sphere", "bsdf": "fibre", "transform": {"position": [0.55, 0.95, 0.45], "scale": 0.2, "rotation": [20, 35, 10]}},
        {"name": "plate", "type": "disk", "bsdf": "fibre", "transform": {"position": [-0.6, 0.55, 0.6], "scale": 0.3, "rotation": [60, 25, 10]}},
        {"name": "pillar", "type": "cylinder", "bsdf": "fibre", "capped": True,
         "transform": {"position": [0.1, 0.3, 0.75], "scale": [0.3, 0.6, 0.3], "rotation": [0, 0, 25]}}]


def _wire(bsdf):
    """rough_wire (or what stands in for it) on two rotated cylinders -- the reference's way to draw a cable -- and a sphere."""
    def edit(scene):
        _no_blocks(scene)
        scene["bsdfs"].append(dict(bsdf, name="wire"))
        scene["primitives"] += [
            {"name": "cable", "type": "cylinder", "bsdf": "wire", "transform": {"position": [-0.35, 0.7, -0.1], "scale": [0.28, 1.3, 0.28], "rotation": [25, 0, 40]}},
            {"name": "rod", "type": "cylinder", "bsdf": "wire", "capped": False,
             "transform": {"position": [0.45, 0.45, 0.4], "scale": [0.35, 0.8, 0.35], "rotation": [80, 30, 0]}},
            {"name": "bead", "type": "sphere", "bsdf": "wire", "transform": {"position": [0.5, 1.3, -0.2], "scale": 0.25, "rotation": [10, 50, 30]}}]
    return edit


def _wire_in_fog(scene):
    _wire(WIRE["r035"])(scene)
    _fog(scene)


def wire_meshes(tmpdir, **kw):
    """rough_wire on a smooth uv-mapped triangle mesh, and on a second mesh whose uvs are all equal: there TriangleMesh::tangentSpace fails (its uv
    determinant is zero, TriangleMesh.cpp:362-384) and the frame falls back to the normal's."""
    tmpdir = str(tmpdir)
    verts, tris = scenes.displaced_sphere(9, 12, seed=7)
    scenes.write_wo3(os.path.join(tmpdir, "fibre_blob.wo3"), verts, tris)
    flat_uv = verts.copy()
    flat_uv[:, 6:8] = 0.5
    scenes.write_wo3(os.path.join(tmpdir, "fibre_blob_no_uv.wo3"), flat_uv, tris)

    def edit(scene):
        _no_blocks(scene)
        scene["bsdfs"].append(dict(WIRE["r035"], name="wire"))
        scene["primitives"] += [
            {"name": "blob", "type": "mesh", "file": "fibre_blob.wo3", "smooth": True, "bsdf": "wire",
             "transform": {"position": [-0.4, 0.3, 0.2], "scale": 0.9, "rotation": [10, 50, 0]}},
            {"name": "blobNoUv", "type": "mesh", "file": "fibre_blob_no_uv.wo3", "smooth": True, "bsdf": "wire",
             "transform": {"position": [0.45, 0.15, 0.45], "scale": 0.7, "rotation": [40, 0, 20]}}]
    return build(tmpdir, **dict(kw, edit=edit))


NESTED = {
    # the Lambert half is shaded in the tangent-space frame too: the wrapper's lobes carry the anisotropic bit (MixedBsdf.cpp:132-135)
    "mix": {"type": "mixed", "albedo": 1, "ratio": 0.4, "bsdf0": dict(LAMBERT_FIBRE), "bsdf1": {"type": "lambert", "albedo": [0.2, 0.5, 0.7]}},
    # (the base is NAMED: the reference prepares the bsdfs of the scene's list and the unnamed ones primitives hold, TraceableScene.hpp:76-84, so a
    # rough_wire written inline inside a wrapper never runs prepareForRender and scatters with an uninitialised _v -- NaN samples, another image per run)
    "cut": {"type": "transparency", "albedo": 1, "alpha": dict(CHECKER_ALPHA), "base": "cutWire"},
    "coat": {"type": "smooth_coat", "albedo": 1, "ior": 1.4, "thickness": 0.6, "sigma_a": [0.3, 0.1, 0.05], "substrate": dict(LAMBERT_FIBRE)},
}


CUT_WIRE = dict(WIRE["r035"], name="cutWire")


def _nested(scene):
    scene["bsdfs"].insert(0, dict(CUT_WIRE))         # (in front of the bsdf that names it)
    _replace_bsdf(scene, "tallBox", NESTED["mix"])
    _replace_bsdf(scene, "shortBox", NESTED["cut"])
    scene["bsdfs"].append(dict(NESTED["coat"], name="coat"))
    scene["primitives"].append({"name": "ball", "type": "sphere", "bsdf": "coat", "transform": {"position": [0.55, 0.95, 0.45], "scale": 0.22, "rotation": [20, 35, 10]}})


def fibre_bump(tmpdir, **kw):
    """lambertian_fiber WITH a non-constant bitmap bump map, on a quad and a cube: both reasons for the long way of setupTangentFrame together.  The
    bump map is the one scenes.cornell_bump writes (and the rest of that scene stays: its ball and its mesh)."""
    def edit(scene):
        texture_cases._lift(scene)
        _replace_bsdf(scene, "floor", dict(LAMBERT_FIBRE, bump={"type": "bitmap", "file": "bump.png", "scale": 1.5}))
        _replace_bsdf(scene, "tallBox", dict(LAMBERT_FIBRE, albedo=[0.3, 0.5, 0.7], bump="bump.png"))
    return scenes.cornell_bump(tmpdir, **dict(kw, edit=edit))


def fibre_instances(tmpdir, **kw):
    """rough_wire on the master mesh of an `instances` primitive: an instance refuses a tangent space (Instance.cpp:348-351), so the frame is the
    normal's.  The masters of scenes.cornell_instances."""
    def edit(scene):
        _replace_bsdf(scene, "copper", WIRE["r035"])
    return scenes.cornell_instances(tmpdir, **dict(kw, edit=edit))


_SOBOL = {"stratified_sampler": True}

# name -> (builder, kwargs), the layout of scenes.GOLDEN_CASES: tests/golden/<name>_samples.npz
CASES = {
    "fibre_lambert_prims": (build, dict(SIZE, edit=_lambert_prims)),
    "fibre_wire_r005": (build, dict(SIZE, edit=_wire(WIRE["r005"]))),
    "fibre_wire_r015": (build, dict(SIZE, edit=_wire(WIRE["r015"]))),
    "fibre_wire_r035": (build, dict(SIZE, edit=_wire(WIRE["r035"]))),
    "fibre_wire_r100": (build, dict(SIZE, edit=_wire(WIRE["r100"]))),
    "fibre_wire_mesh": (wire_meshes, dict(SIZE)),
    "fibre_nested": (build, dict(SIZE, edit=_nested)),
    "fibre_bump": (fibre_bump, dict(SIZE)),
    "fibre_instances": (fibre_instances, dict(SIZE)),
    "fibre_sobol_fog": (build, dict(SIZE, edit=_wire_in_fog, renderer=_SOBOL)),
}
ROUGHNESS_CASES = ("fibre_wire_r005", "fibre_wire_r015", "fibre_wire_r035", "fibre_wire_r100")
# case -> the same scene with `lambert` in the fibres' place: what a golden must differ from (tools/make_fibre_golden.py records in how many samples)
LAMBERT = {"type": "lambert", "albedo": [0.75, 0.6, 0.45]}


def lambert_twin(name):
    """(builder, kwargs) of case `name` with every fibre BCSDF of its JSON replaced by a Lambert BSDF."""
    mk, kw = CASES[name]

    def swap(node):
        if isinstance(node, dict):
            if node.get("type") in ("lambertian_fiber", "rough_wire"):
                keep = {k: v for k, v in node.items() if k in ("name", "bump")}
                node.clear()
                node.update(dict(LAMBERT, **keep))
            for v in node.values():
                swap(v)
        elif isinstance(node, list):
            for v in node:
                swap(v)

    def twin(tmpdir, **kw2):
        path = mk(tmpdir, **kw2)
        import json
        with open(path) as f:
            sc = json.load(f)
        swap(sc["bsdfs"])
        with open(path, "w") as f:
            json.dump(sc, f)
        return path
    return twin, kw


# ---- single BSDF calls: one scene that holds every BSDF of the cases above, a few hundred calls each ----
def bsdf_list():
    """The named bsdfs of the per-call fixture, in the order of the fixture's blocks."""
    out = [dict(LAMBERT_FIBRE, name="lambertian_fiber")]
    out += [dict(WIRE[r], name="wire_" + r) for r in ("r005", "r015", "r035", "r100")]
    out.append(dict(CUT_WIRE))
    out += [dict(NESTED[k], name=k) for k in ("mix", "cut", "coat")]
    out.append(dict(LAMBERT_FIBRE, name="fibre_bumped", bump=dict(CHECKER_ALPHA)))    # (a bump map is no part of a BSDF call: the answers of the first)
    return out


def bsdf_scene(tmpdir, **kw):
    def edit(scene):
        scene["bsdfs"] += bsdf_list()
        scene["primitives"].append({"name": "bead", "type": "sphere", "bsdf": "wire_r035", "transform": {"position": [0.5, 1.3, -0.2], "scale": 0.25}})
    return build(tmpdir, **dict(SIZE, name="fibre_bsdfs.json", edit=edit, **kw))


GENERAL_CASES = 256          # bsdf_cases.make_cases: the crafted period (every wi x wo kind x ulp step, every requested set) and a random tail
STREAM_BASE = 64             # the fixture's sampler streams: bsdf_cases.stream_index(STREAM_BASE + position, case)


def _corner_cases():
    """The fibres' own corners: wo.z == 0 (rough_wire's eval is black there, its pdf divides by sqrt(wo.x^2)), wo along +-y (cosThetaO == 0 and
    cosPhi = 0/0), wi.y = +-1 (cosThetaI == 0), wo in the z == 0 plane with x == 0 too, each under the lobe sets that switch a branch."""
    f32 = np.float32
    wis = [bc._unit([0.3, -0.2, 0.9]), np.array([0, 1, 0], f32), np.array([0, -1, 0], f32), bc._unit([-0.5, 0.4, -0.7]), np.array([0, 0, 1], f32)]
    wos = [bc._at_height(f32(0.0), 0.9), bc._at_height(f32(-0.0), 2.1), np.array([0, 1, 0], f32), np.array([0, -1, 0], f32), np.array([1, 0, 0], f32),
           np.array([-1, 0, 0], f32), bc._unit([0.0, 0.6, 0.8]), bc._unit([0.6, 0.0, -0.8]), np.array([0, 0, -1], f32)]
    reqs = [bc.ALL_LOBES, bc.ALL_BUT_SPECULAR, 1, 2, 4, 8, 3, 12, 64, 128, 0]
    wi, wo, req = [], [], []
    k = 0
    for a in wis:
        for b in wos:
            wi.append(a); wo.append(b); req.append(reqs[k % len(reqs)])
            k += 1
    n = len(wi)
    uv = np.stack([(np.arange(n)*0.37) % 1.0, (np.arange(n)*0.61) % 1.0], axis=1).astype(f32)
    return {"wi": np.stack(wi).astype(f32), "wo": np.stack(wo).astype(f32), "uv": uv, "requested": np.array(req, np.uint32)}


def bsdf_fixture_cases():
    """(names, position of each case's bsdf in bsdf_list() [N], cases dict of [N, ...], sampler stream index [N], cases per bsdf)."""
    names = [b["name"] for b in bsdf_list()]
    corners = _corner_cases()
    parts, position, stream = [], [], []
    for pos, b in enumerate(bsdf_list()):
        general = bc.make_cases(b, GENERAL_CASES, (CHECKER_ALPHA["res_u"], CHECKER_ALPHA["res_v"]))
        part = {k: np.concatenate([general[k], corners[k]]) for k in general}
        n = part["wi"].shape[0]
        parts.append(part)
        position += [pos]*n
        stream.append(bc.stream_index(STREAM_BASE + pos, 0) + np.arange(n))
    cases = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    return names, np.array(position, np.int32), cases, np.concatenate(stream).astype(np.uint32), parts[0]["wi"].shape[0]
