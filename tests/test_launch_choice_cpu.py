"""The choice of a pass's kernels (tungsten_amd/csrc/host/LaunchChoice.cpp, through tgh_launch_choice) against the launched-kernel inventory
tests/golden/launch_inventory.json: kernel traces of renders of the cases of tests/launch_cases.py, recorded by tools/launch_inventory.py with the library of
the commit BEFORE the choice became host code -- so what is checked here is that the one statement of the decision names the kernels the three
hand-kept copies launched.  No GPU: the choice is plain host arithmetic."""
import json
import os
import re

import pytest

import launch_cases
import light_cases
import scenes
import tungsten_amd as tg
from tungsten_amd import capi

with open(os.path.join(scenes.GOLDEN, "launch_inventory.json")) as f:
    INVENTORY = json.load(f)


@pytest.fixture(scope="module")
def descs(tmp_path_factory):
    """scene name -> FlattenedScene of every inventory scene that can be built here"""
    out = {}
    for scene in launch_cases.SCENES:
        if launch_cases.have(scene):
            out[scene] = tg.FlattenedScene(launch_cases.build(scene, tmp_path_factory.mktemp(scene)))
    yield out
    for flat in out.values():
        flat.close()


def choices_of(flat, case):
    """The choice of every kind of pass the case's render ran (the inventory's `passes`: flags, short or not)."""
    options = {k: v for k, v in case["options"].items() if k != "max_slots"}      # ("max_slots" only makes the batch long: `passes` has what came of it)
    return [capi.launch_choice(tg.lib, flat.desc, options, flags, short) for flags, short in case["passes"]]


def buildable_cases():
    return [(name, case) for name, case in INVENTORY.items() if launch_cases.have(case["scene"])]


def test_inventory_holds_every_case_of_the_list(descs):
    import ctypes as C
    want = set()
    for scene, flat in descs.items():
        traits = capi.TgHostSceneTraits()
        assert tg.lib.tgh_scene_check(flat.desc, C.byref(traits), None, 0) == 0
        want |= {launch_cases.case_name(scene, o) for o in launch_cases.option_sets(scene, flat.desc.contents.num_recs, traits)}
    assert want == {name for name, _ in buildable_cases()}


def test_choice_names_the_kernels_the_parent_launched(descs):
    """For every case: the kernels of the choice -- over the kinds of passes the render ran -- are the kernels of the trace, name for name."""
    assert buildable_cases()
    wrong = {}
    for name, case in buildable_cases():
        got = set().union(*[c.kernel_names() for c in choices_of(descs[case["scene"]], case)])
        traced = {l[0] for l in case["launches"]}
        if got != traced:
            wrong[name] = {"choice only": sorted(got - traced), "trace only": sorted(traced - got)}
    assert not wrong, json.dumps(wrong, indent=1)


# every launch family of the shim, as a pattern over canonical kernel names: each must be chosen in at least one case, so that the inventory cannot
# hide a branch no case reaches.  (Masks: csrc/hip/pt_variants.h; the FEAT_QMC twin of a family is the same family.)
QMC = 1 << 30
MASKS = {"LEAN": 8195, "SIMPLE": 520101891, "SIMPLE_INST": 2667585539, "COAT": 520102095, "GLASS": 520102003, "PLASTIC": 520102659,
         "COAT_INST": 2667585743, "GLASS_INST": 2667585651, "PLASTIC_INST": 2667586307, "FULL": 3205496831, "MEDIA": 1602236499, "ALL": 4294967295,
         "TAIL": 520634367}


def _either(mask):
    return "(%d|%d)" % (mask, mask | QMC)


FAMILIES = [r"k_trace_closest<\w+,true,0>", r"k_trace_closest<\w+,false,1>", r"k_trace_closest<\w+,false,2>", r"k_trace_closest<\w+,false,0>",
            r"k_trace_closest_dyn<", r"k_trace_closest_inst<", r"k_trace_closest_instw<",
            r"k_trace_closest_wide<\w+,\w+,true,false>", r"k_trace_closest_wide<\w+,\w+,false,true>", r"k_trace_closest_wide<\w+,\w+,false,false>",
            r"k_finish_trace_closest_wide<",
            r"k_trace_shadow<\w+,true,\w+,0,4290772991>", r"k_trace_shadow<\w+,\w+,true,0,", r"k_trace_shadow<\w+,\w+,false,[12],4290772991>",
            r"k_trace_shadow<\w+,true,\w+,\d,4294967295>",
            r"k_trace_shadow_dyn<", r"k_trace_shadow_wide<", r"k_trace_shadow_fast<", r"k_trace_shadow_fast_inst<"] + \
           [r"k_shade<%s,\d,\d,false>" % _either(MASKS[m]) for m in ("LEAN", "SIMPLE", "SIMPLE_INST", "COAT", "GLASS", "PLASTIC", "COAT_INST", "GLASS_INST",
                                                                    "PLASTIC_INST", "FULL")] + \
           [r"k_shade<%d,2,0,false>" % MASKS["MEDIA"], r"k_shade<%d,2,0,false>" % MASKS["ALL"], r"k_shade<%d,2,0,true>" % MASKS["ALL"]] + \
           [r"k_shade_fused<%s," % _either(MASKS[m]) for m in ("COAT", "GLASS", "PLASTIC")] + \
           [r"k_tail<%s," % _either(MASKS["COAT"]), r"k_tail<%s," % _either(MASKS["TAIL"]), r"k_camera_rays$"]


def test_every_launch_family_is_chosen_in_some_case(descs):
    chosen = set()
    for name, case in buildable_cases():
        for c in choices_of(descs[case["scene"]], case):
            chosen |= c.kernel_names()
    missing = [f for f in FAMILIES if not any(re.match(f, k) for k in chosen)]
    if not scenes.have_materialtest():       # (only materialtest shades in k_shade_fused and ends in the conductor-family k_tail: it needs the unpacked scene files)
        missing = [f for f in missing if not f.startswith(("k_shade_fused<", "k_tail<%s," % _either(MASKS["COAT"])))]
    assert not missing, missing


def test_masks_are_those_of_the_kernel_headers():
    """MASKS above against familyMask (tgh_light_needs reports it), so that a changed mask cannot leave the family patterns matching nothing new."""
    import ctypes as C
    flat = tg.FlattenedScene(scenes.CORNELL)
    for variant, name in ((light_cases.LEAN, "LEAN"), (light_cases.SIMPLE, "SIMPLE"), (light_cases.COAT, "COAT"), (light_cases.GLASS, "GLASS"),
                          (light_cases.PLASTIC, "PLASTIC"), (light_cases.MEDIA, "MEDIA"), (light_cases.TAIL, "TAIL"), (light_cases.FULL, "FULL"),
                          (light_cases.ALL, "ALL")):
        mask = C.c_uint32(0)
        assert tg.lib.tgh_light_needs(flat.desc, variant, None, None, C.byref(mask)) == 0
        assert mask.value == MASKS[name] & ~QMC, name          # (familyMask: without the Sobol' sampler's bit, which MASK_MEDIA always carries)
    flat.close()


def test_families_of_the_choice_are_families_of_the_light_rule(descs, tmp_path):
    """light_cases.families_for -- the families whose masks the lights' feature bits are checked against (tests/test_light_units_cpu.py) -- holds every
    family the choice launches: for every inventory scene and every scene of the light corner cases, on normal, auxiliary and Sobol' passes, under the
    default options and every toggle of the inventory."""
    import ctypes as C
    flats = dict(descs)
    for which in scenes.LIGHT_CORNER_SCENES:
        flats["light_corners_" + which] = tg.FlattenedScene(scenes.light_corners(tmp_path, which))
    toggles = launch_cases.ALWAYS + launch_cases.FLAT + launch_cases.LOOP + launch_cases.SINGLE_LEVEL + launch_cases.INSTANCED + launch_cases.MEDIA
    for scene, flat in flats.items():
        traits = capi.TgHostSceneTraits()
        assert tg.lib.tgh_scene_check(flat.desc, C.byref(traits), None, 0) == 0, scene
        allowed = light_cases.families_for(traits)
        for options in toggles:
            options = {k: v for k, v in options.items() if k != "max_slots"}
            for flags in (0, 1, 4, 5):                                # TGHIP_PASS_SOBOL = 1, TGHIP_PASS_AUX = 4
                for short in (0, 1):
                    c = capi.launch_choice(tg.lib, flat.desc, options, flags, short)
                    fams = {l.variant for l in c.shade[:c.num_shade]}
                    if c.tail_eligible:
                        fams.add(light_cases.TAIL)
                    assert fams <= allowed, (scene, options, flags, sorted(fams - allowed))
    for which in scenes.LIGHT_CORNER_SCENES:
        flats["light_corners_" + which].close()


def test_refusals():
    flat = tg.FlattenedScene(scenes.CORNELL)
    with pytest.raises(ValueError, match="no option"):
        capi.launch_choice(tg.lib, flat.desc, {"max_slots": 8192})
    assert tg.lib.tgh_launch_choice(None, None, None, 0, 0, 0, None, None, 0) != 0
    flat.close()
