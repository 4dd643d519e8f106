"""Single light calls ON THE DEVICE (tghip_debug_light: chooseLight / lightSampleDirect / lightApproximateRadiance / lightIntersect / lightEvalDirect /
lightDirectPdf as k_shade's next-event estimation calls them, csrc/hip/debug_units.hip) against the oracle, word for word, on the cases of
tests/light_cases.py: every sampled light of scenes.light_corners("all") -- quads, a cube, a sphere, a disk with its cone, a point light, a mesh,
capped and uncapped cylinders, a sphere cap, the skydome and infinite spheres with constant, bitmap, checker, disk and blade emission -- times 4096
cases of shading points in the emitter's plane, on and inside it, at a point light's own position, 1e4 and 1e6 units away, and directions through a
quad's corners and edges, across its plane, at the poles, the seam and the texel boundaries of the environment maps.  The first FIXTURE_CASES cases
of every light are also held to the reference's recorded answers (tests/golden/light_corners.npz).

Compared as bit patterns: the chosen light, sample_ok, approximateRadiance and hit always; the weight where a light was chosen; d, dist and pdf where
the sample succeeded; t, u, v, back_side, the emission and directPdf where the ray hit (directPdf always for the point light); a NaN matches a NaN.
The counts of numbers chooseLight and sampleDirect consumed are checked through the two streams' next numbers where the call succeeded.  The numbers
themselves come from each case's counter-based streams: the device's Rng replays nothing, so crafted sampling numbers (xi of exactly 0, or 1 - ulp)
are out of scope.

The two lights each of `backs` and `unknown` are held the same way: there chooseLight answers "no light" (every weight 0) and weighs lights that are
all "unknown".  Then every shading family's instantiation on each of the six scenes: bit for bit the all-features variant's answers on every light whose feature
bits the family's mask holds (SceneCheck.cpp: lightNeeds) -- chooseLight included where it holds those of ALL the scene's lights --, and every
family the launch code may pick for a scene covers all of that scene's lights.

One renderer per scene serves the module; cases and oracle answers are computed once per light and shared."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import light_cases as lc
import scenes
import tungsten_amd as tg
from tungsten_amd import capi

pytestmark = pytest.mark.gpu

SCENES = scenes.LIGHT_CORNER_SCENES
N = lc.CASES_PER_LIGHT
VARIANTS = list(range(capi.TGHIP_BSDF_VARIANT_COUNT))
ALL_NAMES = [name for name, _, _ in scenes.light_corner_list("all")]
# the lights held to the oracle and the reference: those of `all`, and of the two scenes that reach chooseLight's "no light" and all-unknown legs
ORACLE_LIGHTS = [(which, name) for which in ("all", "backs", "unknown") for name, _, _ in scenes.light_corner_list(which)]
T0 = time.time()


class Corner(object):
    def __init__(self, tmp, which):
        self.which = which
        self.position = SCENES.index(which)
        self.names = [name for name, _, _ in scenes.light_corner_list(which)]
        self.path = scenes.light_corners(tmp, which)
        self.flat = tg.FlattenedScene(self.path)
        self.renderer = tg.Renderer(self.path)
        self.info = {v: self.renderer.debug_light_info(v) for v in VARIANTS}
        d = self.flat.desc.contents
        self.dirac = [d.objects[d.lights[s]].type == lc.POINT for s in range(d.num_lights)]
        traits = capi.TgHostSceneTraits()
        assert tg.lib.tgh_scene_check(self.flat.desc, C.byref(traits), None, 0) == 0
        self.families = lc.families_for(traits)

    @functools.lru_cache(maxsize=None)
    def cases(self, slot):
        return lc.make_cases(lc.light_geometry(self.flat.desc, slot), self.names[slot], N)

    @functools.lru_cache(maxsize=None)
    def streams(self, slot):
        return lc.streams(self.position, slot, N, extra=1)

    def device(self, slots, variant, n=N):
        """The device's answers for the first n cases of each light of `slots` under `variant`: (words [len(slots)*n, 18], next numbers [.., 2])."""
        dc = np.zeros(len(slots)*n, tg.LIGHT_CASE_DTYPE)
        for i, slot in enumerate(slots):
            c, s = self.cases(slot), slice(i*n, (i + 1)*n)
            dc["light"][s] = slot
            dc["p"][s], dc["w"][s] = c["p"][:n], c["w"][:n]
            dc["stream"][s] = lc.stream_index(self.position, slot) + np.arange(n)
        dc["seed"], dc["variant"] = lc.SEED, variant
        return lc.device_words(self.renderer.debug_light(dc))

    def close(self):
        self.renderer.close()
        self.flat.close()


@pytest.fixture(scope="module")
def corners(tmp_path_factory):
    made = {}

    def get(which):
        if which not in made:
            made[which] = Corner(tmp_path_factory.mktemp("light_corners_" + which), which)
        return made[which]
    yield get
    for c in made.values():
        c.close()
    print("tests/test_gpu_light_units.py: %.1f s since import" % (time.time() - T0))


def _pad(words):
    return np.concatenate([words[:, :18], np.zeros((words.shape[0], 2), np.uint32)], axis=1)


def _bad_draws(nxt, xc, xs, want):
    """Cases whose streams stand elsewhere than the oracle's (or the reference's) counts say: the next number of the choose stream where a light was
    chosen, of the sample stream where the sample succeeded."""
    rows = np.arange(want.shape[0])
    chose, ok = want[:, 0].view(np.int32) >= 0, want[:, 2] == 1
    bad_c = chose & (nxt[:, 0].view(np.uint32) != xc[rows, np.minimum(want[:, 18], xc.shape[1] - 1)].view(np.uint32))
    bad_s = ok & (nxt[:, 1].view(np.uint32) != xs[rows, np.minimum(want[:, 19], xs.shape[1] - 1)].view(np.uint32))
    return np.nonzero(bad_c | bad_s)[0]


@pytest.mark.parametrize("which,name", ORACLE_LIGHTS, ids=[n if w == "all" else "%s/%s" % (w, n) for w, n in ORACLE_LIGHTS])
def test_device_is_the_oracle_in_every_word(which, name, corners):
    corner = corners(which)
    slot = corner.names.index(name)
    c = corner.cases(slot)
    xc, xs = corner.streams(slot)
    want = lc.oracle_words(corner.flat.desc, slot, c, xc, xs)
    assert int(want[:, 18].max()) <= lc.NXC and int(want[:, 19].max()) <= lc.NXS
    got, nxt = corner.device([slot], capi.TGHIP_BSDF_VARIANT_ALL)
    dirac = corner.dirac[slot]
    bad = np.nonzero(lc.differing(_pad(got), _pad(want), dirac=dirac))[0]
    bad_draw = _bad_draws(nxt, xc, xs, want)
    print("%s: %d of %d cases differ from the oracle, %d consumed another count of numbers; chosen %d, sampled %d, hit %d, unknown weight %d"
          % (name, len(bad), N, len(bad_draw), int((want[:, 0].view(np.int32) >= 0).sum()), int((want[:, 2] == 1).sum()), int((want[:, 9] == 1).sum()),
             int((want[:, 8].view(np.float32) < 0).sum())))
    assert len(bad) == 0, "%s: cases %s, e.g. case %d (p %s, w %s): %s" % (
        name, bad[:8], bad[0], c["p_kind"][bad[0]], c["w_kind"][bad[0]],
        [(lc.WORDS[w], hex(got[bad[0], w]), hex(want[bad[0], w])) for w in np.nonzero(got[bad[0]] != want[bad[0], :18])[0]])
    assert len(bad_draw) == 0, "%s: cases %s consumed another count of random numbers than the oracle's %s" % (name, bad_draw[:8], want[bad_draw[:8], 18:20])
    # ... and the reference's recorded words on the fixture's cases
    gold = np.load(lc.GOLDEN)
    n = int(gold["cases_per_light"])
    assert list(gold[which + "_names"]) == corner.names
    ref = lc.chosen_as_objects(gold[which + "_ref"][slot*n:(slot + 1)*n], corner.flat.desc)
    for key in ("p", "w"):                       # the recorded answers are answers to these very cases
        assert (gold["%s_%s" % (which, key)][slot*n:(slot + 1)*n].view(np.uint32) == c[key][:n].view(np.uint32)).all(), key
    bad_ref = np.nonzero(lc.differing(_pad(got[:n]), _pad(ref), dirac=dirac))[0]
    assert len(bad_ref) == 0, "%s: cases %s differ from the reference's recorded words" % (name, bad_ref[:8])
    assert len(_bad_draws(nxt[:n], xc[:n], xs[:n], ref)) == 0


@pytest.mark.parametrize("which", SCENES)
@pytest.mark.parametrize("variant", VARIANTS, ids=capi.TGHIP_BSDF_VARIANT_NAMES)
def test_family_is_the_full_variant_where_it_covers(variant, which, corners):
    """On the lights whose feature bits the family's mask holds, its instantiation answers bit for bit what the all-features variant answers -- the
    chooseLight words too where the mask holds the bits of every light of the scene (it weighs them all).  A family the launch code may pick for
    the scene covers every light of it."""
    corner = corners(which)
    needs, covered, mask = corner.info[variant]
    slots = [s for s in range(len(corner.names)) if covered[s]]
    print("%s on %s covers %d of %d lights: %s" % (capi.TGHIP_BSDF_VARIANT_NAMES[variant], which, len(slots), len(corner.names), [corner.names[s] for s in slots]))
    if variant in corner.families:
        assert len(slots) == len(corner.names) >= 1, "a family this scene may be shaded by does not cover all of its lights"
    if not slots:
        return
    got, nxt = corner.device(slots, variant)
    want, wnxt = corner.device(slots, capi.TGHIP_BSDF_VARIANT_ALL)
    g, w = _pad(got), _pad(want)
    if not covered.all():                        # chooseLight evaluated a light this family folds away: its words are not this family's to answer
        g[:, [0, 1]] = w[:, [0, 1]]
    dirac = np.repeat([corner.dirac[s] for s in slots], N)
    bad = lc.differing(g, w) | (dirac & lc.differing(g, w, dirac=True))
    bad |= (want[:, 2] == 1) & (nxt[:, 1].view(np.uint32) != wnxt[:, 1].view(np.uint32))
    if covered.all():
        bad |= (want[:, 0].view(np.int32) >= 0) & (nxt[:, 0].view(np.uint32) != wnxt[:, 0].view(np.uint32))
    bad = np.nonzero(bad)[0]
    assert len(bad) == 0, "%d cases differ, first: light %s case %d: %s" % (
        len(bad), corner.names[slots[bad[0]//N]], bad[0] % N, [(lc.WORDS[k], hex(got[bad[0], k]), hex(want[bad[0], k])) for k in np.nonzero(got[bad[0]] != want[bad[0]])[0]])


def test_every_scene_keeps_a_covered_light_for_each_of_its_families(corners):
    """No family drops out of the comparison above: each of the four scenes has a covered light under every family meant for it, the device's masks
    are the host rule's (tgh_light_needs), and none holds the Sobol' sampler."""
    seen = set()
    for which in SCENES:
        corner = corners(which)
        for v in sorted(corner.families):
            assert corner.info[v][1].any(), (which, capi.TGHIP_BSDF_VARIANT_NAMES[v])
        seen |= corner.families
        n = len(corner.names)
        for v in VARIANTS:
            needs, covered, mask = np.zeros(n, np.uint32), np.zeros(n, np.uint32), C.c_uint32(0)
            assert tg.lib.tgh_light_needs(corner.flat.desc, v, needs.ctypes.data, covered.ctypes.data, C.addressof(mask)) == 0
            assert (needs == corner.info[v][0]).all() and (covered.astype(bool) == corner.info[v][1]).all() and mask.value == corner.info[v][2]
            assert mask.value & (1 << 30) == 0
    assert seen == set(VARIANTS) - {lc.MEDIA}          # (the lean media family shades media scenes only; its light bits are SIMPLE's, compared above)
    # a mask without the bits answers as another emitter would: LEAN takes every light for a quad -- the cube of `solids` is not covered, and differs
    corner = corners("solids")
    slot = corner.names.index("brick")
    assert not corner.info[capi.TGHIP_BSDF_VARIANT_LEAN][1][slot]
    got, _ = corner.device([slot], capi.TGHIP_BSDF_VARIANT_LEAN, 256)
    want, _ = corner.device([slot], capi.TGHIP_BSDF_VARIANT_ALL, 256)
    assert lc.differing(_pad(got), _pad(want)).any()


def test_a_context_without_a_scene_refuses(corners):
    """Both entries answer TGHIP_E_INVALID, with a message, on a context nothing was uploaded to -- and the context can still be destroyed."""
    corners("lean")                                            # (a device is there and initialised)
    lib = tg.lib
    ctx = lib.tghip_create(0)
    assert ctx
    one = np.zeros(2, tg.LIGHT_CASE_DTYPE)
    one["variant"] = capi.TGHIP_BSDF_VARIANT_ALL
    one["w"] = (0.0, 1.0, 0.0)
    out = np.zeros(2, tg.LIGHT_RESULT_DTYPE)
    needs = np.zeros(16, np.uint32)
    try:
        assert lib.tghip_debug_light(ctx, one.ctypes.data, out.ctypes.data, 2) == capi.TGHIP_E_INVALID
        assert b"scene" in lib.tghip_last_error(ctx)
        assert lib.tghip_debug_light_info(ctx, capi.TGHIP_BSDF_VARIANT_ALL, needs.ctypes.data, None, None) == capi.TGHIP_E_INVALID
        assert b"scene" in lib.tghip_last_error(ctx)
        assert lib.tghip_debug_light(ctx, None, None, 0) == capi.TGHIP_OK          # n == 0 asks for nothing
        assert not out.view(np.uint32).any() and not needs.any()
    finally:
        lib.tghip_destroy(ctx)


def test_invalid_arguments_leave_the_context_usable(corners):
    corner = corners("all")
    r, lib = corner.renderer, tg.lib
    ctx = r.context()
    slots = [ALL_NAMES.index("env"), ALL_NAMES.index("shard")]
    before, nb = corner.device(slots, capi.TGHIP_BSDF_VARIANT_ALL, 256)
    image = r.trace_samples(0, 2)
    one = np.zeros(4, tg.LIGHT_CASE_DTYPE)
    one["variant"] = capi.TGHIP_BSDF_VARIANT_ALL
    one["w"] = (0.0, 1.0, 0.0)
    out = np.zeros(4, tg.LIGHT_RESULT_DTYPE)
    assert lib.tghip_debug_light(ctx, None, None, 0) == capi.TGHIP_OK                                  # n == 0 succeeds
    assert lib.tghip_debug_light(ctx, one.ctypes.data, out.ctypes.data, 0) == capi.TGHIP_OK
    assert lib.tghip_debug_light(ctx, None, out.ctypes.data, 4) == capi.TGHIP_E_INVALID
    assert lib.tghip_debug_light(ctx, one.ctypes.data, None, 4) == capi.TGHIP_E_INVALID
    assert b"light" in lib.tghip_last_error(ctx)
    for field, value in (("light", -1), ("light", len(ALL_NAMES)), ("variant", capi.TGHIP_BSDF_VARIANT_COUNT), ("variant", 0xFFFFFFFF)):
        bad = one.copy()
        bad[field][2] = value
        assert lib.tghip_debug_light(ctx, bad.ctypes.data, out.ctypes.data, 4) == capi.TGHIP_E_INVALID, (field, value)
        assert lib.tghip_last_error(ctx)
    assert lib.tghip_debug_light_info(ctx, capi.TGHIP_BSDF_VARIANT_COUNT, None, None, None) == capi.TGHIP_E_INVALID
    assert lib.tghip_debug_light_info(ctx, -1, None, None, None) == capi.TGHIP_E_INVALID
    assert lib.tghip_debug_light_info(ctx, 0, None, None, None) == capi.TGHIP_OK
    assert lib.tghip_debug_light(ctx, one.ctypes.data, out.ctypes.data, 4) == capi.TGHIP_OK
    after, na = corner.device(slots, capi.TGHIP_BSDF_VARIANT_ALL, 256)
    assert (after == before).all() and (na.view(np.uint32) == nb.view(np.uint32)).all()
    assert (r.trace_samples(0, 2).view(np.uint32) == image.view(np.uint32)).all()
