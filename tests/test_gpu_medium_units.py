"""Single medium calls ON THE DEVICE (tghip_debug_medium: mediumSampleDistance / mediumTransmittance / phaseEval / phaseSample as k_shade and the shadow
walks call them, csrc/hip/debug_units.hip) against the oracle, word for word, on the cases of tests/medium_cases.py: every medium of
scenes.medium_corners -- the nine transmittances and their corners, absorption-only media, a channel that never scatters, extinctions three orders of
magnitude apart, bounce limits of 0, 1 and 3, the Rayleigh and seven Henyey-Greenstein phase functions, exponential and atmospheric media -- times 2048
cases: max_t at, a float32 step from and 9e-4 from every edge of a kernel, +inf, bounce counts around the medium's limit, rays across, along and against
a falloff, through, tangent to and far outside a ball, wo along and against d.  The first FIXTURE_CASES cases of every medium are also held to the
reference's recorded answers (tests/golden/medium_corners.npz).

Compared as bit patterns, without a tolerance and without an allowance of differing cases: ok, the four transmittances and the phase function's value
always; t, the weight, exited, the bounce count and the distance stream's next number where sampleDistance succeeded; the sampled direction, its pdf and
the phase stream's next number always.  A NaN matches a NaN; +-inf and -0 match only themselves.  The numbers themselves come from each case's
counter-based streams: the device's Rng replays nothing, so crafted sampling numbers are out of scope.

Then the two instantiations that carry the media code -- which they are is read from tghip_debug_bsdf_info's variant_mask -- against each other on
every case of every medium, and the refusals.

One renderer serves the module; cases and oracle answers are computed once per medium and shared."""
import functools
import time

import numpy as np
import pytest

import medium_cases as mc
import scenes
import tungsten_amd as tg
from tungsten_amd import capi

pytestmark = pytest.mark.gpu

MEDIA = [name for name, _ in scenes.medium_corner_list()]
N = mc.CASES_PER_MEDIUM
T0 = time.time()


class Corner(object):
    def __init__(self, tmp):
        self.path = scenes.medium_corners(tmp)
        self.flat = tg.FlattenedScene(self.path)
        self.renderer = tg.Renderer(self.path)
        self.indices = mc.medium_indices(self.flat.desc)
        self.families = mc.variant_masks(self.renderer, capi)

    @functools.lru_cache(maxsize=None)
    def cases(self, pos):
        return mc.make_cases(mc.medium_geometry(self.flat.desc, self.indices[pos]), MEDIA[pos], N)

    @functools.lru_cache(maxsize=None)
    def streams(self, pos):
        return mc.streams(pos, N, extra=1)

    def device(self, positions, variant, n=N):
        """The device's answers for the first n cases of each medium of `positions` under `variant`: (words [len(positions)*n, 24], next numbers [.., 2])."""
        dc = np.zeros(len(positions)*n, tg.MEDIUM_CASE_DTYPE)
        for i, pos in enumerate(positions):
            c, s = self.cases(pos), slice(i*n, (i + 1)*n)
            dc["medium"][s] = self.indices[pos]
            dc["p"][s], dc["d"][s], dc["max_t"][s], dc["wo"][s], dc["state_bounce"][s] = c["p"][:n], c["d"][:n], c["max_t"][:n], c["wo"][:n], c["bounce"][:n]
            dc["stream"][s] = mc.stream_index(pos) + np.arange(n)
        dc["seed"], dc["variant"] = mc.SEED, variant
        r = self.renderer.debug_medium(dc)
        assert not r["reserved"].any()
        return mc.device_words(r)

    def close(self):
        self.renderer.close()
        self.flat.close()


@pytest.fixture(scope="module")
def corner(tmp_path_factory):
    c = Corner(tmp_path_factory.mktemp("medium_corners"))
    yield c
    c.close()
    print("tests/test_gpu_medium_units.py: %.1f s since import" % (time.time() - T0))


def _pad(words):
    return np.concatenate([words[:, :24], np.zeros((words.shape[0], 2), np.uint32)], axis=1)


def _counts_out(words):
    w = np.array(words, np.uint32, copy=True)
    w[:, 24:26] = 0
    return w


def _bad_draws(nxt, xd, xp, want):
    """Cases whose streams stand elsewhere than the oracle's (or the reference's) counts say: the next number of the distance stream where
    sampleDistance succeeded, of the phase stream always."""
    rows = np.arange(want.shape[0])
    ok = want[:, 0] == 1
    bad_d = ok & (nxt[:, 0].view(np.uint32) != xd[rows, np.minimum(want[:, 24], xd.shape[1] - 1)].view(np.uint32))
    bad_p = nxt[:, 1].view(np.uint32) != xp[rows, np.minimum(want[:, 25], xp.shape[1] - 1)].view(np.uint32)
    return np.nonzero(bad_d | bad_p)[0]


@pytest.mark.parametrize("name", MEDIA)
def test_device_is_the_oracle_in_every_word(name, corner):
    pos = MEDIA.index(name)
    c = corner.cases(pos)
    xd, xp = corner.streams(pos)
    want = mc.oracle_words(corner.flat.desc, corner.indices[pos], c, xd, xp)
    assert int(want[:, 24].max()) <= mc.NXD and int(want[:, 25].max()) <= mc.NXP
    got, nxt = corner.device([pos], capi.TGHIP_BSDF_VARIANT_ALL)
    bad = np.nonzero(mc.differing(_pad(got), _counts_out(want)))[0]
    bad_draw = _bad_draws(nxt, xd, xp, want)
    print("%s: %d of %d cases differ from the oracle, %d consumed another count of numbers; ok %d, exited %d, infinite t %d"
          % (name, len(bad), N, len(bad_draw), int((want[:, 0] == 1).sum()), int((want[:, 5] == 1).sum()), int(np.isinf(want[:, 1].view(np.float32)).sum())))
    assert len(bad) == 0, "%s: cases %s, e.g. case %d (max_t %s %r, bounce %s, ray %s, wo %s): %s" % (
        name, bad[:8], bad[0], c["t_kind"][bad[0]], float(c["max_t"][bad[0]]), c["bounce"][bad[0]], c["r_kind"][bad[0]], c["w_kind"][bad[0]],
        [(mc.WORDS[w], hex(got[bad[0], w]), hex(want[bad[0], w])) for w in np.nonzero(got[bad[0]] != want[bad[0], :24])[0]])
    assert len(bad_draw) == 0, "%s: cases %s consumed another count of random numbers than the oracle's %s" % (name, bad_draw[:8], want[bad_draw[:8], 24:26])
    # ... and the reference's recorded words on the fixture's cases
    gold = np.load(mc.GOLDEN)
    n = int(gold["cases_per_medium"])
    assert list(gold["names"]) == MEDIA
    ref = gold["ref"][pos*n:(pos + 1)*n]
    for key in mc.CASE_KEYS:                      # the recorded answers are answers to these very cases
        assert (gold[key][pos*n:(pos + 1)*n].view(np.uint32) == c[key][:n].view(np.uint32)).all(), key
    bad_ref = np.nonzero(mc.differing(_pad(got[:n]), _counts_out(ref)))[0]
    assert len(bad_ref) == 0, "%s: cases %s differ from the reference's recorded words" % (name, bad_ref[:8])
    assert len(_bad_draws(nxt[:n], xd[:n], xp[:n], ref)) == 0


def test_the_media_families_answer_alike(corner):
    """MASK_MEDIA is BSDF_MASK_ALL, word for word on every case of every medium: which families carry the media code is read from the masks."""
    FEAT_QMC = 1 << 30
    assert set(corner.families) == {capi.TGHIP_BSDF_VARIANT_MEDIA, capi.TGHIP_BSDF_VARIANT_ALL}, "a family gained or lost FEAT_MEDIA: the debug kernel is instantiated per family"
    assert all(m & FEAT_QMC == 0 for m in corner.families.values())
    positions = list(range(len(MEDIA)))
    want, wnxt = corner.device(positions, capi.TGHIP_BSDF_VARIANT_ALL)
    for v in sorted(set(corner.families) - {capi.TGHIP_BSDF_VARIANT_ALL}):
        got, nxt = corner.device(positions, v)
        bad = mc.differing(_pad(got), _pad(want))
        bad |= ((want[:, 0] == 1) & (nxt[:, 0].view(np.uint32) != wnxt[:, 0].view(np.uint32))) | (nxt[:, 1].view(np.uint32) != wnxt[:, 1].view(np.uint32))
        bad = np.nonzero(bad)[0]
        assert len(bad) == 0, "%s: %d cases differ, first: medium %s case %d: %s" % (
            capi.TGHIP_BSDF_VARIANT_NAMES[v], len(bad), MEDIA[bad[0]//N], bad[0] % N,
            [(mc.WORDS[k], hex(got[bad[0], k]), hex(want[bad[0], k])) for k in np.nonzero(got[bad[0]] != want[bad[0]])[0]])


def test_a_context_without_a_scene_refuses(corner):
    lib = tg.lib
    ctx = lib.tghip_create(0)
    assert ctx
    one = np.zeros(2, tg.MEDIUM_CASE_DTYPE)
    one["variant"], one["d"], one["wo"], one["max_t"] = capi.TGHIP_BSDF_VARIANT_ALL, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 1.0
    out = np.zeros(2, tg.MEDIUM_RESULT_DTYPE)
    try:
        assert lib.tghip_debug_medium(ctx, one.ctypes.data, out.ctypes.data, 2) == capi.TGHIP_E_INVALID
        assert b"scene" in lib.tghip_last_error(ctx)
        assert lib.tghip_debug_medium(ctx, None, None, 0) == capi.TGHIP_OK          # n == 0 asks for nothing
        assert not out.view(np.uint32).any()
    finally:
        lib.tghip_destroy(ctx)


def test_a_scene_without_media_refuses(tmp_path, corner):
    r = tg.Renderer(scenes.cornell(tmp_path, resolution=(32, 18), spp=1))
    one = np.zeros(2, tg.MEDIUM_CASE_DTYPE)
    one["variant"], one["d"], one["wo"], one["max_t"] = capi.TGHIP_BSDF_VARIANT_ALL, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 1.0
    out = np.zeros(2, tg.MEDIUM_RESULT_DTYPE)
    try:
        assert tg.lib.tghip_debug_medium(r.context(), one.ctypes.data, out.ctypes.data, 2) == capi.TGHIP_E_INVALID
        assert b"no media" in tg.lib.tghip_last_error(r.context()) and not out.view(np.uint32).any()
    finally:
        r.close()


def test_invalid_arguments_leave_the_context_usable(corner):
    r, lib = corner.renderer, tg.lib
    ctx = r.context()
    positions = [MEDIA.index("t_interpolated"), MEDIA.index("h_golden")]
    before, nb = corner.device(positions, capi.TGHIP_BSDF_VARIANT_ALL, 256)
    image = r.trace_samples(0, 2)
    one = np.zeros(4, tg.MEDIUM_CASE_DTYPE)
    one["variant"], one["d"], one["wo"], one["max_t"] = capi.TGHIP_BSDF_VARIANT_ALL, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 1.0
    out = np.zeros(4, tg.MEDIUM_RESULT_DTYPE)
    assert lib.tghip_debug_medium(ctx, None, None, 0) == capi.TGHIP_OK                                  # n == 0 succeeds, and launches nothing
    assert lib.tghip_debug_medium(ctx, one.ctypes.data, out.ctypes.data, 0) == capi.TGHIP_OK
    assert lib.tghip_debug_medium(ctx, None, out.ctypes.data, 4) == capi.TGHIP_E_INVALID
    assert lib.tghip_debug_medium(ctx, one.ctypes.data, None, 4) == capi.TGHIP_E_INVALID
    assert b"medium" in lib.tghip_last_error(ctx)
    operand = corner.indices[MEDIA.index("t_interpolated")] + 1
    lacking = [v for v in range(capi.TGHIP_BSDF_VARIANT_COUNT) if v not in corner.families]
    assert len(lacking) == capi.TGHIP_BSDF_VARIANT_COUNT - 2
    for field, value in [("medium", -1), ("medium", int(corner.flat.desc.contents.num_media)), ("medium", operand), ("medium", operand + 1),
                         ("variant", capi.TGHIP_BSDF_VARIANT_COUNT), ("variant", 0xFFFFFFFF)] + [("variant", v) for v in lacking]:
        bad = one.copy()
        bad[field][2] = value
        assert lib.tghip_debug_medium(ctx, bad.ctypes.data, out.ctypes.data, 4) == capi.TGHIP_E_INVALID, (field, value)
        assert lib.tghip_last_error(ctx)
    assert not out.view(np.uint32).any()                      # no refusal wrote a result: nothing was launched
    assert lib.tghip_debug_medium(ctx, one.ctypes.data, out.ctypes.data, 4) == capi.TGHIP_OK
    after, na = corner.device(positions, capi.TGHIP_BSDF_VARIANT_ALL, 256)
    assert (after == before).all() and (na.view(np.uint32) == nb.view(np.uint32)).all()
    assert (r.trace_samples(0, 2).view(np.uint32) == image.view(np.uint32)).all()
