"""The cases of the launched-kernel inventory (tests/golden/launch_inventory.json): scenes of tests/scenes.py, each under the default options and under
every single option toggle its branch of the launch choice can see.  Read by tools/launch_inventory.py, which records the inventory from kernel traces
of renders, and by the tests that hold the launch choice (tungsten_amd/csrc/host/LaunchChoice.cpp) and the context's launch plan to it."""
import os

import scenes


def _blob(scene):
    """A Lambert 168-triangle blob in the box: more than TGHIP_FLAT_MAX_RECS records, so the scene is walked through its BVH."""
    scene["primitives"].append({"name": "blob", "type": "mesh", "file": "blob.wo3", "smooth": True, "bsdf": "ceiling",
                                "transform": {"position": [0.1, 1.2, 0.0]}})


def _with_blob(make):
    def build(tmpdir, **kw):
        verts, tris = scenes.displaced_sphere(8, 12, seed=3)
        verts = verts.copy()
        verts[:, 0:3] = (verts[:, 0:3] - [0, 0.5, 0])*0.5
        scenes.write_wo3(os.path.join(str(tmpdir), "blob.wo3"), verts, tris[:, [0, 2, 1, 3]])
        user = kw.pop("edit", None)

        def edit(scene):
            if user:
                user(scene)
            _blob(scene)
        return make(tmpdir, edit=edit, **kw)
    return build


def _instances_zoo(scene):
    """The instanced Cornell box with a dielectric and a plastic inside the two-material master and a sphere beside the swarm: every class of an instanced
    scene, and solids."""
    scenes._replace_bsdf(scene, "leftWall", {"type": "dielectric", "ior": 1.5, "albedo": 1})
    scenes._replace_bsdf(scene, "rightWall", {"type": "plastic", "ior": 1.5, "thickness": 1.0, "sigma_a": [0.2, 0.4, 0.1], "albedo": [0.3, 0.5, 0.7]})
    scene["primitives"].append({"name": "ball", "type": "sphere", "bsdf": "floor", "transform": {"position": [0.6, 0.2, 0.6], "scale": 0.2}})


def _instances_forward(scene):
    scenes._replace_bsdf(scene, "backWall", {"type": "transparency", "alpha": 0.6, "albedo": 1, "base": {"type": "lambert", "albedo": [0.63, 0.065, 0.05]}})


def _blade_wall(scene):
    scenes._replace_bsdf(scene, "rightWall", {"type": "lambert", "albedo": {"type": "blade", "blades": 5, "angle": 0.25, "value": [0.14, 0.45, 0.091]}})


def _zoo(which):
    return lambda t, **kw: scenes.cornell_zoo(t, which, **kw)


_G, _I, _O = scenes.GOLDEN_CASES, scenes.INTEGRATE_CASES, scenes.OUTPUT_CASES
_SMALL = dict(resolution=(48, 27), spp=8)
# name -> (builder, keyword arguments): renders at the goldens' sizes
SCENES = {
    "cornell": _G["cornell"],
    "zoo_a": _G["zoo_a"],                                              # a flat list with further classes
    "cornell_mesh_light_flat": _G["cornell_mesh_light_flat"],
    "cornell_mesh_light": _G["cornell_mesh_light"],
    "materialtest": _G["materialtest"],
    "materialtest_dielectric": _G["materialtest_dielectric"],
    "materialtest_plastic": (scenes.materialtest, dict(resolution=(48, 27), spp=4, edit=scenes._mt_material(
        {"type": "plastic", "ior": 1.5, "thickness": 1.0, "sigma_a": [0.2, 0.4, 0.1], "albedo": [0.3, 0.5, 0.7]}))),
    # (no zoo scene of tests/scenes.py is walked through a BVH: zoo_a and zoo_b with a triangle blob added have three further shading classes on one)
    "zoo_a_blob": (_with_blob(_zoo("zoo_a")), _SMALL),
    "zoo_b_blob": (_with_blob(_zoo("zoo_b")), _SMALL),                 # ... class 3 not covered by the plastic family, and a forward lobe
    "cornell_many_cubes": _G["cornell_many_cubes"],                    # tables too large for the shading kernels' LDS copy
    "cornell_instances": _G["cornell_instances"],
    "cornell_instances_zoo": (scenes.cornell_instances, dict(_SMALL, edit=_instances_zoo)),
    "cornell_instances_forward": (scenes.cornell_instances, dict(_SMALL, edit=_instances_forward)),
    "cornell_crowd": _G["cornell_crowd"],
    "cornell_fog": _G["cornell_fog"],
    "zoo_a_fog": (_zoo("zoo_a"), dict(_SMALL, edit=scenes._fog)),     # media with surfaces MASK_MEDIA does not cover
    "cornell_bump": _G["cornell_bump"],
    "zoo_b_blade": (_zoo("zoo_b"), dict(_SMALL, edit=_blade_wall)),   # a blade texture and a forward lobe
    "zoo_b_blade_blob": (_with_blob(_zoo("zoo_b")), dict(_SMALL, edit=_blade_wall)),
    "cornell_instances_blade": (scenes.cornell_instances, dict(_SMALL, edit=lambda s: (_instances_forward(s), _blade_wall(s)))),
    "cornell_cubemap_cross": _G["cornell_cubemap_cross"],
    "zoo_a_outputs": _O["zoo_a_outputs"],                              # auxiliary passes
    "cornell_adaptive_sobol": _I["cornell_adaptive_sobol"],
    "materialtest_as_shipped": _I["materialtest_as_shipped"],
}

ALWAYS = ({}, {"count_traversal": 1}, {"max_slots": 8192}, {"blocks_per_cu": 4}, {"lds_tables": 0})
FLAT = ({"fuse_flat": 0}, {"run_to_completion": 0})
LOOP = ({"streams": 1}, {"merge_miss": 0})                             # every scene whose loop is not fused into k_shade
SINGLE_LEVEL = ({"wide_bvh": 0}, {"wide_shadow": 0}, {"wide_closest": 0}, {"dynamic_fetch": 0}, {"decouple": 0}, {"fold_finish": 0}, {"shade_fused": 0},
                {"tail_kernel": 0}, {"tail_family": 0})
INSTANCED = ({"wide_bvh": 0}, {"wide_shadow": 0}, {"wide_closest": 1}, {"dynamic_fetch": 0}, {"inst_dyn": 0}, {"inst_wide": 0}, {"inst_simple": 0},
             {"inst_shadow_fast": 0})
MEDIA = ({"media_lean": 0},)


# scenes that are here for one branch no other scene reaches: the default and the toggles that reach it, not the whole list
ONLY = {
    "materialtest_plastic": ({},),                                     # the plastic family's pair of k_shade_fused
    "zoo_b_blob": ({},),                                               # FULL for class 3 next to the class families, the closest-hit shadow walk on a BVH
    "cornell_many_cubes": ({},),                                       # GLOBAL_TABLES without "lds_tables" = 0
    "cornell_instances_zoo": ({}, {"inst_dyn": 0}, {"inst_simple": 0}),   # the _INST twins of every class; k_trace_closest<., false, 1>
    "cornell_instances_forward": ({}, {"inst_dyn": 0}),               # k_trace_shadow<., true, false, 2>
    "cornell_instances_blade": ({},),                                  # k_trace_shadow<., true, false, 2, BSDF_MASK_ALL>
    "zoo_b_blade_blob": ({},),                                         # k_trace_shadow<., true, false, 0, BSDF_MASK_ALL>
}


def option_sets(scene, num_recs, traits):
    """The option sets of a scene with the traits `traits` (capi.TgHostSceneTraits): the toggles its branch of the launch choice can see.  (Which toggles
    are worth a traced render, no more: a set too many or too few changes the inventory's size, not what is asserted about a case in it.)"""
    if scene in ONLY:
        return list(ONLY[scene])
    flat = num_recs <= 16 and not traits.have_instances
    fused = flat and not (traits.have_forward or traits.have_mesh_light or traits.all_features_shading or traits.camera_fix) and traits.tables_fit
    sets = list(ALWAYS)
    if flat:
        sets += FLAT
    if not fused:
        sets += LOOP
    if traits.have_instances:
        sets += INSTANCED
    elif not flat:
        sets += SINGLE_LEVEL
    if traits.have_media:
        sets += MEDIA
    return sets


def case_name(scene, options):
    return scene + "".join(":%s=%d" % kv for kv in sorted(options.items()))


def have(scene):
    """Can the scene be built here?  (materialtest needs the unpacked scene files.)"""
    return scenes.have_materialtest() or not scene.startswith("materialtest")


def build(scene, tmpdir):
    make, kw = SCENES[scene]
    return make(tmpdir, **kw)


def cases(tmpdir, lib):
    """[(case name, scene, options, scene file)] of every case that can be built here."""
    import ctypes as C
    import tungsten_amd as tg
    from tungsten_amd import capi
    out = []
    for scene in SCENES:
        if not have(scene):
            continue
        sub = os.path.join(str(tmpdir), scene)
        os.makedirs(sub, exist_ok=True)
        path = build(scene, sub)
        flat = tg.FlattenedScene(path)
        traits = capi.TgHostSceneTraits()
        assert lib.tgh_scene_check(flat.desc, C.byref(traits), None, 0) == 0, scene
        num_recs = flat.desc.contents.num_recs
        flat.close()
        for options in option_sets(scene, num_recs, traits):
            out.append((case_name(scene, options), scene, options, path))
    return out
