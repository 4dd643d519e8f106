"""What a context would launch (tghip_debug_launch_plan: the launch choice resolved on the device -- workgroup sizes from the occupancy of the kernels,
dynamic LDS bytes, grid, parts) against the launched-kernel inventory tests/golden/launch_inventory.json, which kernel traces of renders with the library of
the commit before the plan existed recorded (tools/launch_inventory.py).  Uploads only: nothing is rendered."""
import collections
import ctypes as C
import json
import os

import numpy as np
import pytest

import launch_cases
import scenes
import tungsten_amd as tg
from tungsten_amd import capi

pytestmark = pytest.mark.gpu

with open(os.path.join(scenes.GOLDEN, "launch_inventory.json")) as f:
    INVENTORY = json.load(f)
SOBOL, RECORDS, AUX = 1, 2, 4
ITEM_GROUP = 64                      # PT_ITEM_GROUP: a part of the loop needs two groups of work items
DEFAULT = collections.defaultdict(lambda: 1, count_traversal=0, streams=0, blocks_per_cu=0, wide_closest=-1, max_slots=1 << 23)   # the options' defaults


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return {scene: launch_cases.build(scene, tmp_path_factory.mktemp(scene)) for scene in launch_cases.SCENES if launch_cases.have(scene)}


class Pass(object):
    """A pass description of the kind (flags, short) for the scene of `renderer`, and the host-side plan of its batches."""

    def __init__(self, renderer, flags, max_slots, spp=16, whole=True):
        """spp samples of every pixel -- the passes the integrator makes of a render: spp_step samples each, the first pass of an adaptive render too --, or
        (whole = False) one sample per pixel of one record, as small as a late adaptive pass gets."""
        w, h = renderer.width, renderer.height
        records = ((w + 3)//4)*((h + 3)//4)
        self.keep = [np.zeros(((w + 15)//16)*((h + 15)//16), np.uint32), np.zeros(records, np.uint32), np.full(records, spp if whole else 1, np.uint32)]
        if not whole:
            self.keep[2][1:] = 0
        u32p = C.POINTER(C.c_uint32)
        self.desc = capi.TgHipPassDesc(0, spp if whole else 1, tg.DEFAULT_SEED, 0, 1, flags,
                                       self.keep[0].ctypes.data_as(u32p) if flags & SOBOL else None,
                                       self.keep[1].ctypes.data_as(u32p) if flags & RECORDS else None,
                                       self.keep[2].ctypes.data_as(u32p) if flags & RECORDS else None)
        rc = C.c_int(0)
        p = tg.lib.tgh_pass_plan_create(C.byref(self.desc), w, h, 1, 1 << 26, max_slots, 0, C.byref(rc), None, 0)
        assert p, rc.value
        info = capi.TgHostPassPlan()
        tg.lib.tgh_pass_plan_info(p, C.byref(info))
        n = C.c_uint32(0)
        b = tg.lib.tgh_pass_plan_batches(p, C.byref(n))
        self.short, self.batch_items = int(info.short_batch), [int(b[i].total_items) for i in range(n.value)]
        tg.lib.tgh_pass_plan_free(p)


def plan_of(renderer, desc):
    plan = capi.TgHipLaunchPlan()
    assert tg.lib.tghip_debug_launch_plan(renderer.context(), C.byref(desc), C.byref(plan)) == 0, tg.lib.tghip_last_error(renderer.context())
    return plan


def lds_bytes(formula, threads, choice, traits):
    """The dynamic LDS of a walk launch, restated from the kernels' use of it (csrc/hip/pt_wavefront.h): formula 1, the BVH2 walks -- one stack word per tree level
    and thread, over the expanded queue of two bytes per slot that is consumed first (a flat list has no stack); 2, the dynamic-fetch walks -- queue and stacks
    side by side; 3, the wide walks -- queue + one 8-byte group entry per level of the wide tree and thread; 4, k_trace_closest_instw -- half a word per slot,
    the BVH2 stack of the levels above the masters, rounded to 8 bytes, + the masters' group stacks."""
    queue = 2*choice.slot_cap
    if formula == 1:
        return max(0 if choice.flat else 4*max(traits.bvh_depth, 1)*threads, queue)
    if formula == 2:
        return queue + 4*max(traits.bvh_depth, 1)*threads
    if formula == 3:
        return queue + 8*max(traits.wide_depth, 1)*threads
    if formula == 4:
        words = (choice.slot_cap//2 + max(traits.bvh_depth - traits.bvh_master_depth, 1)*threads + 1)//2*2
        return 4*words + 8*max(traits.wide_master_depth, 1)*threads
    return 0


def launches_of(plan, batch_items):
    """{(kernel, workgroup size, grid): dynamic LDS bytes} of the plan's launches, for batches of `batch_items` work items."""
    c = plan.choice
    out = {}
    for items in batch_items:
        parts = plan.parts if items >= 2*plan.parts*ITEM_GROUP else 1
        grid = plan.grid//parts
        for l in c.shade[:c.num_shade]:
            out[(l.name.decode(), plan.threads_shade[l.size], grid)] = 0
        if not c.fused_flat:
            out[(c.closest.name.decode(), plan.threads_closest, grid)] = plan.lds_closest
            out[(c.shadow.name.decode(), plan.threads_shadow, grid)] = plan.lds_shadow
        if c.camera_rays:
            out[("k_camera_rays", 256, grid)] = 0
        if plan.tail_fits:
            out[(c.tail.decode(), plan.threads_tail, grid)] = plan.lds_tail
    return out


def test_plan_gives_the_launches_of_the_inventory(paths):
    """Per case: the (kernel, workgroup size, grid) of the plan, for the passes the traced render made, are those of the trace; the plan's choice is
    tgh_launch_choice's for the same inputs; and the plan's dynamic LDS bytes are those of the formula the choice names, restated in lds_bytes above (the trace's
    LDS column is a kernel's static LDS: a kernel trace does not show the dynamic bytes of a launch, so the golden cannot carry them)."""
    wrong, open_scene, traits = {}, [None, None, None], capi.TgHostSceneTraits()
    for name, case in INVENTORY.items():
        if case["scene"] not in paths:
            continue
        if open_scene[0] != case["scene"]:                             # (one upload per scene: the cases of a scene follow each other)
            if open_scene[0]:
                open_scene[1].close()
                open_scene[2].close()
            open_scene = [case["scene"], tg.Renderer(paths[case["scene"]]), tg.FlattenedScene(paths[case["scene"]])]
            assert tg.lib.tgh_scene_check(open_scene[2].desc, C.byref(traits), None, 0) == 0
        r, flat = open_scene[1:]
        kw = launch_cases.SCENES[case["scene"]][1]
        spp = min(kw["spp"], kw.get("spp_step", kw["spp"]))              # (the integrator renders spp_step samples per pass)
        for k, v in case["options"].items():
            r.set_option(k, v)
        max_slots = case["options"].get("max_slots", 1 << 23)
        choice_options = {k: v for k, v in case["options"].items() if k != "max_slots"}
        got, grids, adaptive = {}, collections.defaultdict(set), False
        for flags, short in case["passes"]:
            # (the later passes of an adaptive render sample the records its error estimate picks: the pass made here is the first one, or the smallest)
            adaptive = adaptive or bool(flags & RECORDS)
            kinds = [p for p in [Pass(r, flags, max_slots, spp)] + ([Pass(r, flags, max_slots, whole=False)] if flags & RECORDS else []) if p.short == short]
            assert kinds, (name, flags, short)
            plan = plan_of(r, kinds[0].desc)
            c = plan.choice
            assert bytes(c) == bytes(capi.launch_choice(tg.lib, flat.desc, choice_options, flags, short)), name
            assert plan.lds_closest == lds_bytes(c.closest.lds_formula, plan.threads_closest, c, traits), name
            assert plan.lds_shadow == lds_bytes(c.shadow.lds_formula, plan.threads_shadow, c, traits), name
            assert plan.lds_tail == lds_bytes(3, 256, c, traits) and plan.threads_tail == 256, name
            launches = launches_of(plan, kinds[0].batch_items)
            got.update(launches)
            for key in launches:
                grids[key[:2]] |= {plan.grid, plan.grid//plan.parts}
        for k in case["options"]:
            r.set_option(k, DEFAULT[k])
        traced = {(l[0], l[1], l[3]): l[2] for l in case["launches"]}
        # the tuples are the trace's; of an adaptive render, whose later passes are not the ones described here, the kernels and workgroup sizes are, and every
        # traced grid of a kernel is that kernel's whole grid or a part's
        if adaptive:
            same = {k[:2] for k in got} == {k[:2] for k in traced} and all(k[2] in grids[k[:2]] for k in traced)
        else:
            same = set(got) == set(traced)
        if not same:
            wrong[name] = {"plan": sorted(got), "trace": sorted(traced)}
    open_scene[1].close()
    open_scene[2].close()
    assert not wrong, json.dumps(wrong, indent=1)


TOGGLES = [("cornell", "fuse_flat", 0), ("cornell_instances", "inst_dyn", 0), ("cornell_instances", "wide_shadow", 0), ("zoo_a_blob", "decouple", 0),
           ("zoo_a_blob", "blocks_per_cu", 2), ("zoo_a_blob", "count_traversal", 1), ("zoo_a_blob", "streams", 2), ("cornell_fog", "media_lean", 0)]


@pytest.mark.parametrize("scene,key,value", TOGGLES, ids=["%s-%s" % t[:2] for t in TOGGLES])
def test_option_on_a_live_context_plans_like_a_fresh_one(paths, scene, key, value):
    """An option set after a plan was made (upload, and a first look at the plan) gives the plan of a context that never planned without it; switching it back
    gives the first plan again."""
    live, fresh = tg.Renderer(paths[scene]), tg.Renderer(paths[scene])
    for flags in (0, AUX):
        kind = Pass(live, flags, 1 << 23)                       # (owns the arrays its description points to)
        desc = kind.desc
        before = bytes(plan_of(live, desc))
        live.set_option(key, value)
        fresh.set_option(key, value)
        toggled = bytes(plan_of(live, desc))
        assert toggled == bytes(plan_of(fresh, desc))
        assert toggled != before or flags == AUX                       # (an auxiliary pass keeps to the all-features kernels whatever most options say)
        live.set_option(key, DEFAULT[key])
        fresh.set_option(key, DEFAULT[key])
        assert bytes(plan_of(live, desc)) == before
    live.close()
    fresh.close()
