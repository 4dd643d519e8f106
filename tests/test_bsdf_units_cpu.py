"""Single BSDF calls, CPU side: the oracle's bsdf_eval / bsdf_sample against the answers of the reference's own Bsdf::eval / pdf / sample recorded in
tests/golden/bsdf_corners.npz (tools/make_bsdf_golden.py) for the first FIXTURE_CASES cases of every bsdf of scenes.bsdf_corners -- materials at and
beyond the edges of their parameters, directions in and next to the surface plane, exact mirror / reverse / refracted directions (tests/bsdf_cases.py).

Every word is compared as a bit pattern: f, pdf, sample_ok, and -- where the sample succeeded -- wo, weight, pdf, the sampled lobe and the count of
random numbers consumed.  A NaN matches a NaN.  The numbers a sample draws come from the counter-based stream of each case; crafted sampling numbers
(xi of exactly 0, or 1 - ulp) are out of scope here, because the device, which is held to the same cases (tests/test_gpu_bsdf_units.py), replays nothing.

A residual would be pinned case by case in tests/golden/bsdf_corners_residual.json; there is none: 0 of 11 040 cases differ."""
import json
import os

import numpy as np
import pytest

import bsdf_cases as bc
import oracle_lib
import scenes
import tungsten_amd as tg
from test_oracle_golden import flat_bsdf_index

CORNERS = scenes.bsdf_corner_list()
NAMES = [b["name"] for b in CORNERS]
PINNED = json.load(open(bc.RESIDUAL)) if os.path.exists(bc.RESIDUAL) else {}


@pytest.fixture(scope="module")
def gold():
    return np.load(bc.GOLDEN)


@pytest.fixture(scope="module")
def corner_scene(tmp_path_factory):
    path = scenes.bsdf_corners(tmp_path_factory.mktemp("bsdf_corners"))
    with open(path) as f:
        sj = json.load(f)
    flat = tg.FlattenedScene(path)
    yield path, sj, flat
    flat.close()


def test_scene_holds_every_bsdf_type_and_every_named_bsdf_is_flattened(corner_scene):
    _, sj, flat = corner_scene
    assert flat.info.num_bsdfs == len(sj["bsdfs"])                      # named references are shared, nothing is dropped
    types = {flat.desc.contents.bsdfs[flat_bsdf_index(sj, bc.scene_index(sj, n))].type for n in NAMES}
    assert types == set(range(19)) - {13}                               # (TGHIP_BSDF_ERROR has no scene-file spelling)
    assert len(set(NAMES)) == len(NAMES)


def test_fixture_inputs_are_what_the_generator_produces(gold):
    assert list(gold["names"]) == NAMES
    n = int(gold["cases_per_bsdf"])
    assert n == bc.FIXTURE_CASES and int(gold["seed"]) == bc.SEED and int(gold["nxi"]) == bc.NXI
    assert gold["ref"].shape == (len(NAMES)*n, 14)
    for pos, b in enumerate(CORNERS):
        c = bc.make_cases(b, n, scenes.CORNER_TEXTURE_SIZE)
        for key in ("wi", "wo", "uv", "requested"):
            assert (gold[key][pos*n:(pos + 1)*n].view(np.uint32) == c[key].view(np.uint32)).all(), (b["name"], key)
        # a prefix of the device test's longer list
        long = bc.make_cases(b, 4*n, scenes.CORNER_TEXTURE_SIZE)
        assert all((long[key][:n].view(np.uint32) == c[key].view(np.uint32)).all() for key in c)


def test_fixture_cases_hold_every_crafted_direction(gold):
    n = bc.FIXTURE_CASES
    c = bc.make_cases(CORNERS[7], n, scenes.CORNER_TEXTURE_SIZE)        # plain_dielectric
    wi = {tuple(r) for r in c["wi"].view(np.uint32)}
    assert wi == {tuple(np.asarray(w, np.float32).view(np.uint32)) for w in bc.crafted_wi()}
    k = np.arange(n)
    assert len(set(zip((k % 15) % 5, (k % 15)//5))) == 15               # every wo kind with both one-ulp neighbours
    assert set(c["requested"]) == set(np.array(bc.REQUESTED, np.uint32))
    mirror = (c["wo"][:, 0] == -c["wi"][:, 0]) & (c["wo"][:, 1] == -c["wi"][:, 1]) & (c["wo"][:, 2] == c["wi"][:, 2])
    reverse = (c["wo"] == -c["wi"]).all(axis=1)
    assert mirror.sum() >= 4 and reverse.sum() >= 4
    assert ((c["wi"][:, 2] == 0) & ~np.signbit(c["wi"][:, 2])).any() and ((c["wi"][:, 2] == 0) & np.signbit(c["wi"][:, 2])).any()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_is_the_reference_in_every_word(name, gold, corner_scene):
    _, sj, flat = corner_scene
    pos, n = NAMES.index(name), bc.FIXTURE_CASES
    c = {k: gold[k][pos*n:(pos + 1)*n] for k in ("wi", "wo", "uv", "requested")}
    ref = gold["ref"][pos*n:(pos + 1)*n]
    xi = bc.streams(pos, n, extra=0)
    got = bc.oracle_words(flat.desc, flat_bsdf_index(sj, bc.scene_index(sj, name)), c, xi)
    bad = [int(i) for i in np.nonzero(bc.differing(got, ref))[0]]
    print("%s: %d of %d cases differ" % (name, len(bad), n))
    assert bad == PINNED.get(name, []), "%s: cases %s differ from the reference, e.g. %s" % (
        name, bad[:8], [(bc.WORDS[w], hex(got[bad[0], w]), hex(ref[bad[0], w])) for w in np.nonzero(got[bad[0]] != ref[bad[0]])[0]] if bad else None)


def test_residual_is_within_its_cap():
    assert sum(len(v) for v in PINNED.values()) <= 0.001*len(NAMES)*bc.FIXTURE_CASES
    assert set(PINNED) <= set(NAMES)


def test_batched_entry_is_the_per_case_entry(gold, corner_scene):
    """oracle_bsdf_cases only loops over oracle_bsdf_eval / oracle_bsdf_sample."""
    _, sj, flat = corner_scene
    pos = NAMES.index("deep_mixed_coat_cut")
    bi = flat_bsdf_index(sj, bc.scene_index(sj, NAMES[pos]))
    n = 24
    c = bc.make_cases(CORNERS[pos], n, scenes.CORNER_TEXTURE_SIZE)
    xi = bc.streams(pos, n, extra=0)
    got = bc.oracle_words(flat.desc, bi, c, xi)
    for k in range(n):
        f, pdf = oracle_lib.bsdf_eval(flat.desc, bi, c["wi"][k], c["wo"][k], c["uv"][k], int(c["requested"][k]))
        ok, wo, weight, spdf, lobe, consumed = oracle_lib.bsdf_sample(flat.desc, bi, c["wi"][k], c["uv"][k], int(c["requested"][k]), xi[k])
        want = np.concatenate([f.view(np.uint32), np.float32([pdf]).view(np.uint32), [int(ok)], wo.view(np.uint32), weight.view(np.uint32),
                               np.float32([spdf]).view(np.uint32), [lobe, consumed]]).astype(np.uint32)
        assert not bc.differing(got[k:k + 1], want[None]).any(), k


@pytest.mark.skipif(not os.path.exists(os.path.join(scenes.ROOT, "oracle", "_ref", "ref_harness")), reason="reference harness (oracle/_ref) not built")
def test_reference_harness_reproduces_the_bsdf_fixture(gold, corner_scene, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(scenes.ROOT, "tools"))
    import make_bsdf_golden
    path, sj, _ = corner_scene
    names, index, cases, xi = make_bsdf_golden.fixture_cases(sj)
    ref = make_bsdf_golden.reference_words(path, index, cases, xi, str(tmp_path))
    assert not bc.differing(ref, gold["ref"]).any()
