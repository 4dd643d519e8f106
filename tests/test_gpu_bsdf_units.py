"""Single BSDF calls ON THE DEVICE (tghip_debug_bsdf: bsdfEval / bsdfPdf / bsdfSample as the shading kernels call them, csrc/hip/debug_units.hip)
against the oracle, word for word, on the cases of tests/bsdf_cases.py: every named bsdf of scenes.bsdf_corners -- parameters at and beyond their
clamps, ior of exactly one and below one, absorbing and empty layers, mixtures at 0 and 1, the deepest nesting -- times 4096 cases of directions in
and next to the surface plane, exact mirror / reverse / refracted directions and their one-ulp neighbours, uv on checker and texel boundaries, every
`requested` set.  The first 96 cases of every bsdf are also held to the reference's recorded answers (tests/golden/bsdf_corners.npz).

Compared as bit patterns: f, pdf, sample_ok and -- where the sample succeeded -- wo, weight, pdf and the sampled lobe; a NaN matches a NaN.  The
count of numbers a sample consumed is checked through the stream's next number where the sample succeeded; after a failed sample -- the path ends
there, and its outputs are not compared either -- the count is only printed, not checked.  The numbers themselves come from each case's counter-based
stream: the device's Rng replays nothing, so crafted sampling numbers (xi of exactly 0, or 1 - ulp) are out of scope.

Then every shading family's instantiation: bit for bit the full variant's answer on every bsdf the product's rule lets that family shade, and black
on a bsdf whose own type the family's mask does not hold.

One renderer serves the module; cases and oracle answers are computed once per bsdf and shared."""
import functools
import json
import time

import numpy as np
import pytest

import bsdf_cases as bc
import oracle_lib
import scenes
import tungsten_amd as tg
from tungsten_amd import capi
from test_oracle_golden import flat_bsdf_index

pytestmark = pytest.mark.gpu

CORNERS = scenes.bsdf_corner_list()
NAMES = [b["name"] for b in CORNERS]
N = bc.CASES_PER_BSDF
FAMILY_CASES = N              # per bsdf in the family comparisons
VARIANTS = list(range(capi.TGHIP_BSDF_VARIANT_COUNT))
T0 = time.time()


class Corner(object):
    def __init__(self, tmp):
        self.path = scenes.bsdf_corners(tmp)
        with open(self.path) as f:
            self.json = json.load(f)
        self.flat = tg.FlattenedScene(self.path)
        self.renderer = tg.Renderer(self.path)
        self.flat_index = {n: flat_bsdf_index(self.json, bc.scene_index(self.json, n)) for n in NAMES}
        self.info = {v: self.renderer.debug_bsdf_info(v) for v in VARIANTS}

    @functools.lru_cache(maxsize=None)
    def cases(self, name):
        return bc.make_cases(CORNERS[NAMES.index(name)], N, scenes.CORNER_TEXTURE_SIZE)

    @functools.lru_cache(maxsize=None)
    def stream(self, name):
        return bc.streams(NAMES.index(name), N, extra=1)

    def device(self, names, variant, n):
        """The device's answers for the first n cases of each of `names` under `variant`: (words [len(names)*n, 13], next [len(names)*n])."""
        dc = np.zeros(len(names)*n, tg.BSDF_CASE_DTYPE)
        for i, name in enumerate(names):
            c, s = self.cases(name), slice(i*n, (i + 1)*n)
            dc["bsdf"][s] = self.flat_index[name]
            dc["wi"][s], dc["wo"][s], dc["uv"][s], dc["requested"][s] = c["wi"][:n], c["wo"][:n], c["uv"][:n], c["requested"][:n]
            dc["stream"][s] = bc.stream_index(NAMES.index(name), 0) + np.arange(n)
        dc["seed"], dc["variant"] = bc.SEED, variant
        r = self.renderer.debug_bsdf(dc)
        words = np.concatenate([r["f"].view(np.uint32), r["pdf"].view(np.uint32)[:, None], r["sample_ok"][:, None], r["sample_wo"].view(np.uint32),
                                r["sample_weight"].view(np.uint32), r["sample_pdf"].view(np.uint32)[:, None], r["sampled"][:, None]], axis=1)
        return words, r["next"].copy()


@pytest.fixture(scope="module")
def corner(tmp_path_factory):
    c = Corner(tmp_path_factory.mktemp("bsdf_corners"))
    yield c
    c.renderer.close()
    c.flat.close()
    print("tests/test_gpu_bsdf_units.py: %.1f s since import" % (time.time() - T0))


def _differing13(got, want):
    """bc.differing on the 13 words the device returns (no consumed count)."""
    pad = np.zeros((got.shape[0], 1), np.uint32)
    return bc.differing(np.concatenate([got, pad], axis=1), np.concatenate([want[:, :13], pad], axis=1))


@pytest.mark.parametrize("name", NAMES)
def test_device_is_the_oracle_in_every_word(name, corner):
    c, xi = corner.cases(name), corner.stream(name)
    want = bc.oracle_words(corner.flat.desc, corner.flat_index[name], c, xi)
    got, nxt = corner.device([name], capi.TGHIP_BSDF_VARIANT_ALL, N)
    bad = np.nonzero(_differing13(got, want))[0]
    ok = want[:, 4] == 1
    assert int(want[:, 13].max()) <= bc.NXI
    drawn = xi[np.arange(N), want[:, 13]]                      # stream[consumed]
    bad_draw = np.nonzero(ok & (nxt.view(np.uint32) != drawn.view(np.uint32)))[0]
    print("%s: %d of %d cases differ from the oracle, %d consumed another count of numbers; %d samples succeeded; after a failed sample %d counts differ"
          % (name, len(bad), N, len(bad_draw), int(ok.sum()), int((~ok & (nxt.view(np.uint32) != drawn.view(np.uint32))).sum())))
    assert len(bad) == 0, "%s: cases %s, e.g. case %d: %s" % (
        name, bad[:8], bad[0], [(bc.WORDS[w], hex(got[bad[0], w]), hex(want[bad[0], w])) for w in np.nonzero(got[bad[0]] != want[bad[0], :13])[0]])
    assert len(bad_draw) == 0, "%s: cases %s consumed another count of random numbers than the oracle's %s" % (name, bad_draw[:8], want[bad_draw[:8], 13])
    # ... and the reference's recorded words on the fixture's cases
    gold = np.load(bc.GOLDEN)
    n, pos = int(gold["cases_per_bsdf"]), NAMES.index(name)
    assert list(gold["names"]) == NAMES
    ref = gold["ref"][pos*n:(pos + 1)*n]
    bad_ref = np.nonzero(_differing13(got[:n], ref))[0]
    assert len(bad_ref) == 0, "%s: cases %s differ from the reference's recorded words" % (name, bad_ref[:8])
    okr = ref[:, 4] == 1
    assert (nxt[:n].view(np.uint32)[okr] == xi[np.arange(n), ref[:, 13]].view(np.uint32)[okr]).all()


@pytest.mark.parametrize("variant", VARIANTS, ids=capi.TGHIP_BSDF_VARIANT_NAMES)
def test_family_is_the_full_variant_where_it_covers(variant, corner):
    """Covered by the product's own rule (tghip_debug_bsdf_info: the type set inside the material within the family's mask, no forward lobe where the
    shading-class rule excludes one): then the family's instantiation answers bit for bit what the all-types variant answers."""
    covered = corner.info[variant][2]
    names = [n for n in NAMES if covered[corner.flat_index[n]]]
    print("%s covers %d of %d bsdfs: %s" % (capi.TGHIP_BSDF_VARIANT_NAMES[variant], len(names), len(NAMES), names[:6]))
    assert len(names) >= 1, "no bsdf of the corner scene is covered by this family: it would drop out of the test"
    got, nxt = corner.device(names, variant, FAMILY_CASES)
    want, wnxt = corner.device(names, capi.TGHIP_BSDF_VARIANT_ALL, FAMILY_CASES)
    bad = np.nonzero(_differing13(got, want) | ((nxt.view(np.uint32) != wnxt.view(np.uint32)) & (want[:, 4] == 1)))[0]
    assert len(bad) == 0, "%d cases differ, first: bsdf %s case %d" % (len(bad), names[bad[0]//FAMILY_CASES], bad[0] % FAMILY_CASES)


@pytest.mark.parametrize("variant", VARIANTS, ids=capi.TGHIP_BSDF_VARIANT_NAMES)
def test_family_is_black_on_a_type_outside_its_mask(variant, corner):
    """A top-level bsdf whose own type bit the family's mask lacks: f = 0, pdf = 0, the sample fails -- never another material's numbers."""
    mask = corner.info[variant][3]
    desc = corner.flat.desc.contents
    names = [n for n in NAMES if not (mask >> desc.bsdfs[corner.flat_index[n]].type) & 1]
    if variant in (capi.TGHIP_BSDF_VARIANT_FULL, capi.TGHIP_BSDF_VARIANT_ALL):
        assert names == []                                   # every type is inside
        return
    assert len(names) >= 1
    got, _ = corner.device(names, variant, FAMILY_CASES)
    black = (got[:, :5] & np.array([0x7FFFFFFF]*4 + [0xFFFFFFFF], np.uint32) == 0).all(axis=1)     # +-0, +-0, +-0, +-0, not ok
    bad = np.nonzero(~black)[0]
    assert len(bad) == 0, "%d cases are not black, first: bsdf %s case %d: %s" % (len(bad), names[bad[0]//FAMILY_CASES], bad[0] % FAMILY_CASES, got[bad[0], :5])


def test_type_sets_and_forward_lobes_reported(corner):
    tm, fwd, cov, mask = corner.info[capi.TGHIP_BSDF_VARIANT_ALL]
    desc = corner.flat.desc.contents
    assert cov.all() and mask & (1 << 30) == 0                # no instantiation holds the Sobol' sampler
    for v in VARIANTS:
        assert corner.info[v][3] & (1 << 30) == 0
    for n in NAMES:
        i = corner.flat_index[n]
        assert (tm[i] >> desc.bsdfs[i].type) & 1
        assert bool(fwd[i]) == bool(desc.bsdfs[i].lobes & 128)
    i = corner.flat_index["deep_mixed_coat_cut"]              # mixed(smooth_coat(lambert), transparency(rough_dielectric))
    assert tm[i] & 0x7FFFF == (1 << 10) | (1 << 3) | (1 << 0) | (1 << 11) | (1 << 5)
    assert tm[corner.flat_index["rc_phong_0.05"]] & (1 << 19) and not tm[corner.flat_index["rc_ggx_0.05"]] & (1 << 19)
    assert tm[corner.flat_index["tex_albedo"]] & (1 << 24) and not tm[corner.flat_index["plain_lambert"]] & (1 << 24)


def test_invalid_arguments_leave_the_context_usable(corner):
    r, lib = corner.renderer, tg.lib
    ctx = r.context()
    names = ["plain_rough_dielectric", "deep_coat_mixed_glass"]
    before, nb = corner.device(names, capi.TGHIP_BSDF_VARIANT_ALL, 256)
    image = r.trace_samples(0, 2)
    one = np.zeros(4, tg.BSDF_CASE_DTYPE)
    one["variant"] = capi.TGHIP_BSDF_VARIANT_ALL
    out = np.zeros(4, tg.BSDF_RESULT_DTYPE)
    assert lib.tghip_debug_bsdf(ctx, None, None, 0) == capi.TGHIP_OK                                  # n == 0 succeeds
    assert lib.tghip_debug_bsdf(ctx, one.ctypes.data, out.ctypes.data, 0) == capi.TGHIP_OK
    assert lib.tghip_debug_bsdf(ctx, None, out.ctypes.data, 4) == capi.TGHIP_E_INVALID
    assert lib.tghip_debug_bsdf(ctx, one.ctypes.data, None, 4) == capi.TGHIP_E_INVALID
    assert b"bsdf" in lib.tghip_last_error(ctx)
    for field, value in (("bsdf", -1), ("bsdf", int(corner.flat.info.num_bsdfs)), ("variant", capi.TGHIP_BSDF_VARIANT_COUNT), ("variant", 0xFFFFFFFF)):
        bad = one.copy()
        bad[field][2] = value
        assert lib.tghip_debug_bsdf(ctx, bad.ctypes.data, out.ctypes.data, 4) == capi.TGHIP_E_INVALID, (field, value)
        assert lib.tghip_last_error(ctx)
    assert lib.tghip_debug_bsdf_info(ctx, capi.TGHIP_BSDF_VARIANT_COUNT, None, None, None, None) == capi.TGHIP_E_INVALID
    assert lib.tghip_debug_bsdf_info(ctx, -1, None, None, None, None) == capi.TGHIP_E_INVALID
    assert lib.tghip_debug_bsdf_info(ctx, 0, None, None, None, None) == capi.TGHIP_OK
    after, na = corner.device(names, capi.TGHIP_BSDF_VARIANT_ALL, 256)
    assert (after == before).all() and (na.view(np.uint32) == nb.view(np.uint32)).all()
    assert (r.trace_samples(0, 2).view(np.uint32) == image.view(np.uint32)).all()
