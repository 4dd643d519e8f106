"""Single medium calls, CPU side: the oracle's medium_sampleDistance / medium_transmittance / phase_eval / phase_sample (through oracle_medium_cases)
against the answers of the reference's own Medium::sampleDistance, Medium::transmittance, PhaseFunction::eval and PhaseFunction::sample, recorded in
tests/golden/medium_corners.npz (tools/make_medium_golden.py) for the first FIXTURE_CASES cases of every medium of scenes.medium_corners -- max_t at,
one float32 step from and 9e-4 from every edge of the linear, quadratic and pulse transmittances, +inf, state_bounce around the medium's limit, rays
across, along and against an exponential medium's falloff and 200 units up and down it, rays through, tangent to, inside and 1e3 radii outside an
atmosphere, wo along and against d and a hair off perpendicular (tests/medium_cases.py).

Every word is compared as a bit pattern: ok, the four (startOnSurface, endOnSurface) transmittances, the phase function's value, the sampled
direction and its pdf always; t, the weight, exited and the bounce count where sampleDistance succeeded; and the counts of random numbers the two
samplers consumed.  A NaN matches a NaN.  Crafted sampling numbers are out of scope here, because the device, which is held to the same cases
(tests/test_gpu_medium_units.py), replays nothing.

A residual would be pinned case by case in tests/golden/medium_corners_residual.json; there is none: 0 of 5 376 cases differ (and 0 of the 86 016 of
the device test's full lists: `python tools/make_medium_golden.py --cases 2048` measures that).

The census (medium_cases.census) keeps the case list from going vacuous: per medium it counts, from the oracle's answers, the legs the cases reach,
and every leg the medium's kind can reach must have a case."""
import hashlib
import json
import os

import numpy as np
import pytest

import medium_cases as mc
import scenes
import tungsten_amd as tg

MEDIA = [name for name, _ in scenes.medium_corner_list()]
N = mc.CASES_PER_MEDIUM
PINNED = json.load(open(mc.RESIDUAL)) if os.path.exists(mc.RESIDUAL) else {}
# sha256 over the inputs of all CASES_PER_MEDIUM cases of every medium, in scene order: the list is deterministic, here and on every other machine
DIGEST = "4bf52b3386f3bd55e866601948276a4eef336b0cbfd472116aa99306e965dbe1"


@pytest.fixture(scope="module")
def gold():
    return np.load(mc.GOLDEN)


@pytest.fixture(scope="module")
def corner(tmp_path_factory):
    flat = tg.FlattenedScene(scenes.medium_corners(tmp_path_factory.mktemp("medium_corners")))
    yield flat
    flat.close()


@pytest.fixture(scope="module")
def everything(corner):
    """Per medium: (geometry, all N cases, (xi_dist, xi_phase), the oracle's words) -- computed once."""
    indices = mc.medium_indices(corner.desc)
    out = {}
    for pos, name in enumerate(MEDIA):
        g = mc.medium_geometry(corner.desc, indices[pos])
        c = mc.make_cases(g, name, N)
        xd, xp = mc.streams(pos, N, extra=0)
        out[name] = (g, c, (xd, xp), mc.oracle_words(corner.desc, indices[pos], c, xd, xp))
    return out


def test_scene_holds_the_listed_media_in_order(corner):
    d = corner.desc.contents
    indices = mc.medium_indices(corner.desc)
    assert len(indices) == len(MEDIA) <= mc.MAX_MEDIA and d.num_media == len(MEDIA) + 2*sum(1 for n in MEDIA if "interpolated" in n) <= 126
    kinds = {name: (d.media[i].medium_type, d.media[i].trans_type, d.media[i].phase_type, bool(d.media[i].absorption_only)) for name, i in zip(MEDIA, indices)}
    assert [kinds["t_" + t][1] for t in ("exponential", "linear", "quadratic", "double_exponential", "pulse", "erlang", "davis", "davis_weinstein",
                                         "interpolated")] == list(range(9))
    assert all(kinds[n][3] == (n.endswith("absorbing") or n.startswith("a_")) for n in MEDIA)
    assert kinds["e_axis"][0] == mc.EXP_MEDIUM and kinds["h_small"][0] == mc.ATMOSPHERE and kinds["p_rayleigh"][2] == mc.RAYLEIGH
    assert [d.media[indices[MEDIA.index("b_%d" % b)]].max_bounce for b in (0, 1, 3)] == [0, 1, 3]
    assert d.media[indices[MEDIA.index("t_davis_clamped")]].trans_p[0] == np.float32(1 + 1e-6)      # davis: alpha below 1 is clamped by both loaders
    assert d.media[indices[MEDIA.index("t_davis_weinstein_half")]].trans_p[0] == 0.5
    assert list(d.media[indices[MEDIA.index("c_wide")]].sigma_t) == [np.float32(1e-3), 1.0, 50.0]
    assert list(d.media[indices[MEDIA.index("c_zero_channel")]].sigma_s)[1] == 0.0 and not d.media[indices[MEDIA.index("c_zero_channel")]].absorption_only


def test_case_list_is_deterministic(everything):
    h = hashlib.sha256()
    for name in MEDIA:
        c = everything[name][1]
        for key in mc.CASE_KEYS:
            h.update(np.ascontiguousarray(c[key]).tobytes())
    assert h.hexdigest() == DIGEST


def test_fixture_inputs_are_what_the_generator_produces(gold, corner, everything):
    n = int(gold["cases_per_medium"])
    assert list(gold["names"]) == MEDIA
    assert n == mc.FIXTURE_CASES and int(gold["seed"]) == mc.SEED and int(gold["nxd"]) == mc.NXD and int(gold["nxp"]) == mc.NXP
    assert gold["ref"].shape == (len(MEDIA)*n, 26)
    indices = mc.medium_indices(corner.desc)
    for pos, name in enumerate(MEDIA):
        short = mc.make_cases(mc.medium_geometry(corner.desc, indices[pos]), name, n)
        for key in mc.CASE_KEYS:                                     # a prefix of the device test's longer list, and the recording's inputs
            assert (short[key].view(np.uint32) == everything[name][1][key][:n].view(np.uint32)).all(), (name, key)
            assert (gold[key][pos*n:(pos + 1)*n].view(np.uint32) == short[key].view(np.uint32)).all(), (name, key)


def test_fixture_cases_hold_every_crafted_value(everything):
    """Every crafted ray, wo, bounce class and max_t lies among the first FIXTURE_CASES -- for the three media with `pulse` cells the max_t list is
    longer than that: its first three priority groups do, the rest follows at once (tests/medium_cases.py)."""
    n = mc.FIXTURE_CASES
    for name in MEDIA:
        g, c = everything[name][:2]
        MT, RAYS = mc.crafted_max_t(g), mc.crafted_rays(g)
        assert {k for k, _, _ in RAYS} <= set(c["r_kind"][:n]), name
        assert {"+d", "-d", "dot+1e-7", "dot-1e-7", "general"} <= set(c["w_kind"][:n]), name
        assert set(mc.BOUNCE_KINDS) <= set(c["b_kind"][:n]), name
        assert {"+x", "-x", "+y", "-y", "+z", "-z"} <= set(c["r_kind"][:n]), name
        assert {"%g" % v for v in mc.BASE_MAX_T} <= set(c["t_kind"][:n]), name
        assert np.isinf(c["max_t"][:n]).any() and (c["max_t"][:n] == np.float32(1e-6)).any(), name
        assert {k for k, _ in MT} <= set(c["t_kind"][:max(n, len(MT))]), name
        th = mc.thresholds(g)
        first = 6 + 3*len(th) + 4*len(th)            # the six values, "at" per threshold and channel, +-ulp and +-9e-4 on one channel per threshold
        if len(MT) <= n:
            assert "pulse" not in name and name != "t_interpolated_dirac", name
        else:
            assert first <= n and {k for k, _ in MT[:first]} <= set(c["t_kind"][:n]), name
        if th:
            kinds = set(c["t_kind"][:n])
            for tag, _ in th:
                assert {"c%d:%s:at" % (ch, tag) for ch in range(3)} <= kinds, (name, tag)
                assert any({"c%d:%s:%s" % (ch, tag, v) for v in ("+ulp", "-ulp", "+9e-4", "-9e-4")} <= kinds for ch in range(3)), (name, tag)
    # the crafted rays of the two inhomogeneous kinds, by name
    assert {"across", "along", "against", "p+50", "p-50", "p+200", "p-200"} <= set(everything["e_axis"][1]["r_kind"][:n])
    assert {"through", "tangent", "h_6", "inside", "from_10_at", "from_10_away", "from_1000_at", "from_1000_away"} <= set(everything["h_golden"][1]["r_kind"][:n])
    e = everything["e_axis"]
    dx = e[1]["d"].astype(np.float64) @ e[0]["falloff_dir"]
    assert ((dx == 0.0) & np.isinf(e[1]["max_t"]))[:n].any() and ((dx < 0.0) & np.isinf(e[1]["max_t"]))[:n].any() and ((dx > 0.0) & np.isinf(e[1]["max_t"]))[:n].any()


@pytest.mark.parametrize("name", MEDIA)
def test_oracle_is_the_reference_in_every_word(name, gold, everything):
    pos, n = MEDIA.index(name), mc.FIXTURE_CASES
    ref = gold["ref"][pos*n:(pos + 1)*n]
    got = everything[name][3][:n]
    assert int(ref[:, 24].max()) <= mc.NXD and int(ref[:, 25].max()) <= mc.NXP
    bad = [int(i) for i in np.nonzero(mc.differing(got, ref))[0]]
    print("%s: %d of %d cases differ; ok %d, exited %d" % (name, len(bad), n, int((ref[:, 0] == 1).sum()), int((ref[:, 5] == 1).sum())))
    assert bad == [e["case"] for e in PINNED.get(name, [])], "%s: cases %s differ from the reference, e.g. %s" % (
        name, bad[:8], [(mc.WORDS[w], hex(got[bad[0], w]), hex(ref[bad[0], w])) for w in np.nonzero(got[bad[0]] != ref[bad[0]])[0]] if bad else None)


def test_residual_is_within_its_cap():
    assert sum(len(v) for v in PINNED.values()) <= 0.001*len(MEDIA)*mc.FIXTURE_CASES
    assert set(PINNED) <= set(MEDIA)


@pytest.mark.parametrize("name", MEDIA)
def test_no_call_consumes_more_numbers_than_it_was_given(name, everything):
    w = everything[name][3]
    g = everything[name][0]
    assert int(w[:, 24].max()) <= mc.NXD and int(w[:, 25].max()) == mc.NXP
    if g["absorption_only"]:
        assert int(w[:, 24].max()) == 0                              # an absorption-only medium draws nothing
    else:
        assert int(w[w[:, 0] == 1, 24].min()) >= 1                   # the channel; `linear` from the medium draws no more
    if name in ("t_pulse", "t_erlang", "t_interpolated", "t_interpolated_dirac"):
        assert int(w[:, 24].max()) >= 3                              # pulse from a surface, erlang from the medium: two draws; interpolated: a boolean more
    assert int(everything["t_interpolated"][3][:, 24].max()) == mc.NXD


@pytest.mark.parametrize("name", MEDIA)
def test_census_every_reachable_leg_has_a_case(name, everything):
    g, c, (xd, _), w = everything[name]
    got = mc.census(w, c, g, xd)
    print(name, got)
    for n_cases, label in ((mc.FIXTURE_CASES, "fixture"), (N, "all")):
        cc = mc.census(w[:n_cases], {k: v[:n_cases] for k, v in c.items()}, g, xd[:n_cases])
        assert cc["ends"] >= 1 and all(cc["bounce_" + k] >= 1 for k in mc.BOUNCE_KINDS), (label, cc)
        assert np.isinf(c["max_t"][:n_cases]).any()
        if not g["absorption_only"]:
            # per chosen channel over the whole list; the fixture of a medium that ends three paths in four (b_0) need not hold all six
            assert all(cc["exit_%d" % ch] >= 1 and cc["scatter_%d" % ch] >= 1 for ch in range(3)) or label == "fixture", (label, cc)
            assert sum(cc["exit_%d" % ch] for ch in range(3)) >= 1 and sum(cc["scatter_%d" % ch] for ch in range(3)) >= 1, (label, cc)
        if g["medium_type"] != mc.ATMOSPHERE:
            assert cc["clamped"] >= 1, (label, cc)                   # (the atmosphere's t is maxT + t0 - t0)
        if g["medium_type"] == mc.HOMOGENEOUS or g["falloff_scale"] == 0.0:
            assert cc["infinite_t"] == 0                             # a medium of constant density never answers an infinite distance
        else:
            assert cc["infinite_t"] >= 1, (label, cc)
        for leg in ("ss", "sm", "ms", "mm"):
            if "dirac_" + leg in cc:
                assert cc["dirac_" + leg] >= 1, (label, leg, cc)
        if "inner_ge_1" in cc:
            assert cc["inner_ge_1"] >= 1, (label, cc)
    assert ("dirac_mm" in got) == (name in ("t_linear", "t_pulse", "t_pulse_7", "t_interpolated", "t_interpolated_dirac", "a_linear", "a_pulse", "a_interpolated"))
    if "erfinv_1" in got:
        # Of the seven branches of erfInv, q = 1 - |inner| in double reaches the first four anywhere; 6 <= x < 18 only where q is 2^-52 or 2^-53,
        # and x >= 44 only where q is 0 (x = inf) -- both need erf(s t0) alone to decide `inner`, which takes a ball as steep as h_steep's and a
        # start outside it.  18 <= x < 44 (the sixth branch) would need 0 < q < exp(-324): no double 1 - p is that small.  Unreachable.
        # The fourth (3 <= x < 6: |inner| within 1.2e-4 of 1) is met without crafted sampling numbers only where a ray starts past the ball
        # (erf(s t0) that close to 1) on a line along which the density adds less than that: exp(-falloff_scale^2) small, h_small and h_steep.
        assert all(got["erfinv_%d" % b] >= 1 for b in (1, 2, 3)), got
        if g["falloff_scale"]*g["falloff_dir"][0] > 2.9:
            assert got["erfinv_4"] >= 1, got
        assert got["erfinv_6"] == 0
        if name == "h_steep":
            assert got["erfinv_5"] >= 1 and got["erfinv_7"] >= 1, got


def test_every_pair_and_every_bounce_class_occurs(everything):
    """All four (startOnSurface, endOnSurface) pairs are answered for every case; where the transmittance looks at them they give different answers.
    sampleDistance sees both firstScatter values on both of its legs."""
    for name in MEDIA:
        g, c, _, w = everything[name]
        tr = w[:, 7:19].reshape(-1, 4, 3)
        looks = g["medium_type"] == mc.HOMOGENEOUS and g["trans_type"] != mc.EXPONENTIAL
        if name == "t_double_equal":                # two equal rates: all four kernels are the one exponential (times sigmaBar, which eval divides out)
            continue
        finite = ~np.isinf(c["max_t"])
        for a in range(4):
            for b in range(a + 1, 4):
                differs = (tr[finite, a] != tr[finite, b]).any()
                assert differs == (looks and (a, b) != (1, 2)), (name, a, b)      # (1, 0) and (0, 1) are the same kernel
        ok, exited, first = w[:, 0] == 1, w[:, 5] == 1, c["bounce"] == 0
        for f in (True, False) if g["max_bounce"] >= 1 else (True,):
            assert (ok & exited & (first == f)).any(), (name, f)
            if not g["absorption_only"]:
                assert (ok & ~exited & (first == f)).any(), (name, f)
        past = c["bounce"] > g["max_bounce"]
        assert past.any() and not ok[past].any()
        if not g["absorption_only"]:
            assert (w[ok, 6].view(np.int32) == c["bounce"][ok] + 1).all()
        else:
            assert (w[ok, 6].view(np.int32) == c["bounce"][ok]).all()


@pytest.mark.skipif(not os.path.exists(os.path.join(scenes.ROOT, "oracle", "_ref", "ref_harness")), reason="reference harness (oracle/_ref) not built")
def test_reference_harness_reproduces_the_medium_fixture(gold, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(scenes.ROOT, "tools"))
    import make_medium_golden
    path = scenes.medium_corners(tmp_path)
    flat = tg.FlattenedScene(path)
    names, which, index, cases, xd, xp = make_medium_golden.scene_cases(flat.desc, mc.FIXTURE_CASES)
    flat.close()
    ref = make_medium_golden.reference_words(path, names, which, cases, xd, xp, str(tmp_path))
    same = (ref == gold["ref"]) | (np.isnan(ref.view(np.float32)) & np.isnan(gold["ref"].view(np.float32)))
    assert same.all()


def test_refusals_are_made_on_the_host(corner, tmp_path):
    """checkMediumCases (csrc/host/SceneCheck.cpp), the rule tghip_debug_medium applies before it launches anything, through tgh_medium_cases_check."""
    import ctypes as C
    from tungsten_amd import capi
    lib = tg.lib
    indices = mc.medium_indices(corner.desc)
    operand = indices[MEDIA.index("t_interpolated")] + 1
    cases = np.zeros(4, tg.MEDIUM_CASE_DTYPE)
    cases["variant"], cases["d"], cases["wo"], cases["max_t"] = capi.TGHIP_BSDF_VARIANT_ALL, (0, 1, 0), (0, 1, 0), 1.0
    out = np.zeros(4, tg.MEDIUM_RESULT_DTYPE)
    err = C.create_string_buffer(256)

    def check(c, cp=True, op=True, n=4, desc=corner.desc):
        err.value = b""
        return lib.tgh_medium_cases_check(desc, c.ctypes.data if cp else None, out.ctypes.data if op else None, n, err, len(err))
    assert check(cases) == capi.TGHIP_OK and err.value == b""
    assert check(cases, n=0) == capi.TGHIP_OK and check(cases, cp=False, op=False, n=0) == capi.TGHIP_OK      # n == 0 asks for nothing
    assert check(cases, cp=False) == capi.TGHIP_E_INVALID and check(cases, op=False) == capi.TGHIP_E_INVALID and b"arguments" in err.value
    media_families = [v for v in range(capi.TGHIP_BSDF_VARIANT_COUNT) if v in (capi.TGHIP_BSDF_VARIANT_MEDIA, capi.TGHIP_BSDF_VARIANT_ALL)]
    for field, value, text in [("medium", -1, b"outside"), ("medium", corner.desc.contents.num_media, b"outside"), ("medium", operand, b"operand"),
                               ("medium", operand + 1, b"operand"), ("variant", capi.TGHIP_BSDF_VARIANT_COUNT, b"unknown variant"),
                               ("variant", 0xFFFFFFFF, b"unknown variant")] + \
                              [("variant", v, b"no medium code") for v in range(capi.TGHIP_BSDF_VARIANT_COUNT) if v not in media_families]:
        bad = cases.copy()
        bad[field][2] = value
        assert check(bad) == capi.TGHIP_E_INVALID and text in err.value, (field, value, err.value)
    for v in media_families:
        good = cases.copy()
        good["variant"] = v
        good["medium"] = indices[-1]
        assert check(good) == capi.TGHIP_OK
    # a scene without media
    plain = tg.FlattenedScene(scenes.cornell(tmp_path, name="plain.json", resolution=(32, 18), spp=1))
    zero = cases.copy()
    zero["medium"] = 0
    assert check(zero, desc=plain.desc) == capi.TGHIP_E_INVALID and b"no media" in err.value
    plain.close()
