"""The decoupled single-level closest-hit walk with the refill and the publish under the turn's one memory wait (pt_wavefront.h:
traceClosestWideBody): a lane that takes a ray fetches the root in the turn it takes it, before its ray has arrived, and a finished
walk is binned a turn's wait after its hit was stored.  What could go wrong is the order of things, so the shapes are the smallest at which the
order matters -- a queue of one (63 lanes claim nothing and must not visit a root), exactly one wave, a queue that ends one lane into a wave, and
a pool so small against the work that nearly every turn refills and publishes, with and without suspended walks among the fresh ones (a walk
suspended after ONE turn per launch must still advance in every launch).  The shadow walk (traceShadowFastBody), whose slots the same passes
resolve, is held to the same counters.

The yardstick is never the changed kernels:
  * the image is the oracle's render of the same pass (tests/oracle_lib.py, as tests/test_gpu_parity.py uses it): `sum` and `count` bit for bit on
    EVERY pixel (the passes are a single chunk of at most four samples per pixel, which the device sums in the oracle's order), `samples` equal;
  * `closest_rays`, `shadow_rays`, `shadow_slots` and, under count_traversal=1, the four visit counters are those of the library of the commit
    before the change, recorded once on the GPU (tools/make_walk_refill_golden.py -> tests/golden/walk_refill_counts.json); they depend on the
    scene and the pass alone, not on pool geometry, suspension or the tail kernel (a walk is a pure function of its ray)."""
import functools
import json
import os

import numpy as np
import pytest

import oracle_lib
import scenes
import tungsten_amd as tg

pytestmark = pytest.mark.gpu

SEED = tg.DEFAULT_SEED
GOLDEN = os.path.join(scenes.GOLDEN, "walk_refill_counts.json")
COUNTERS = ("samples", "closest_rays", "shadow_rays", "shadow_slots", "nodes_visited", "prims_tested", "nodes_visited_shadow", "prims_tested_shadow")

# scene kinds: materialtest is the only one that runs the hoisted quad; tile_terraces is a wide tree without one
SCENES = {
    "materialtest": (lambda t, **kw: scenes.materialtest(t, **kw), {}),
    "materialtest_no_hoist": (lambda t, **kw: scenes.materialtest(t, **kw), dict(hoist_quad=0)),
    "tile_terraces": (lambda t, **kw: scenes.tile_terraces(t, **kw), {}),
}
# the smallest pool the options accept: max_slots >= 256, slots_per_block a multiple of 64
SMALL_POOL = dict(max_slots=256, slots_per_block=64)
SUSPEND = dict(suspend_lanes=63, suspend_turns=1, suspend_min_queue=0)
# (width, height, spp, options, label)
SHAPES = [
    (1, 1, 1, {}, "one"),
    (8, 8, 1, {}, "wave"),
    (13, 5, 1, {}, "wave_plus_one"),
    (64, 36, 4, SMALL_POOL, "small_pool"),
    (64, 36, 4, dict(SMALL_POOL, **SUSPEND), "suspend"),
    (64, 36, 4, dict(SMALL_POOL, tail_kernel=0, **SUSPEND), "suspend_no_tail"),
    (64, 36, 4, dict(SMALL_POOL, suspend_lanes=0), "no_suspend"),
    (64, 36, 4, dict(SMALL_POOL, suspend_lanes=0, tail_kernel=0), "no_suspend_no_tail"),
]


def golden_key(scene, w, h, spp):
    return "%s-%dx%dx%d" % (scene, w, h, spp)


def scene_path(scene, w, h, spp, tmpdir):
    mk, _ = SCENES[scene]
    return mk(tmpdir, name="%s_%dx%dx%d.json" % (scene, w, h, spp), resolution=(w, h), spp=spp)


def render(path, count_traversal, opts):
    r = tg.Renderer(path, seed=SEED)
    for k, v in opts.items():
        r.set_option(k, v)
    r.set_option("count_traversal", 1 if count_traversal else 0)
    r.render()
    _, ssum, count = r.image()
    c = r.counters()
    counters = {k: int(getattr(c, k)) for k in COUNTERS}
    r.close()
    return ssum.copy(), count.copy(), counters


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """The oracle's (sum, count, samples) of a pass, computed once per scene file and shape and shared by the cases that need it."""
    tmp = tmp_path_factory.mktemp("walk_refill_oracle")

    @functools.lru_cache(maxsize=None)
    def get(scene, w, h, spp):
        # (hoisting the quad is the device's business: the oracle renders the same scene either way)
        path = scene_path(scene, w, h, spp, tmp)
        flat = tg.FlattenedScene(path)
        oc = oracle_lib.OracleCounters()
        osum, ocount = oracle_lib.render(flat.desc, flat.width, flat.height, 0, spp, SEED, counters=oc)
        flat.close()
        osum.setflags(write=False)
        ocount.setflags(write=False)
        return osum, ocount, int(oc.samples)
    return get


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["counters"]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[4] for s in SHAPES])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_refilled_and_published_walks_render_the_oracles_pass(scene, shape, oracle, golden, tmp_path):
    if "materialtest" in scene and not scenes.have_materialtest():
        pytest.skip("materialtest assets (assets/) not present")
    w, h, spp, opts, _ = shape
    opts = dict(opts, **SCENES[scene][1])
    path = scene_path(scene, w, h, spp, tmp_path)
    osum, ocount, osamples = oracle(scene, w, h, spp)
    want = golden[golden_key(scene, w, h, spp)]
    for counting in (False, True):
        ssum, count, c = render(path, counting, opts)
        bad = int((ssum.view(np.uint32) != osum.view(np.uint32)).any(axis=-1).sum())
        print("%s %s counting=%d: pixels whose sum differs from the oracle's in any bit: %d of %d; counters %s" % (scene, shape[4], counting, bad, w*h, c))
        assert (count == ocount).all(), "sample counts differ from the oracle's"
        assert bad == 0, "%d of %d pixels differ from the oracle's sum" % (bad, w*h)
        assert c["samples"] == osamples == w*h*spp
        for k in ("samples", "closest_rays", "shadow_rays", "shadow_slots"):
            assert c[k] == want[k], (k, c[k], want[k])
        if counting:
            for k in ("nodes_visited", "prims_tested", "nodes_visited_shadow", "prims_tested_shadow"):
                assert c[k] == want[k], (k, c[k], want[k])
