"""The fibre BCSDFs on the device: every case of tests/fibre_cases.py through Renderer.trace_samples against the reference's own per-sample radiance
(tests/golden/fibre_*_samples.npz, tools/make_fibre_golden.py) -- float32 == in all three channels of every sample, the project's standing norm; no
case is exempt and none has a divergence allowance.  Each case is rendered once (10 368 samples) and shared by the tests below.  Then single BSDF
calls (tghip_debug_bsdf under the all-features variant) against the reference's recorded words, the device's sinhf against the host libm's, and
one control: a scene without a fibre launches what it launched before.

fibre_nested holds the path that found a tie rule: the reference's smooth_coat, handed a TRANSMITTED substrate direction by lambertian_fiber, returns
an unnormalised direction; two bounces on, rough_wire (cosThetaI = cosThetaO = 0) samples wo exactly along the cube's tangent, the ray runs IN the face
it starts on and leaves the block through its lower edge, where the hit point lies on two faces to the bit.  Vec::maxDim gives that tie to the first of
the equal components (pt_scene.h: cubeSurface<REF_TIES>); sample 3 of pixel (27, 9) is on another path otherwise.

The two types are compiled into the all-features shading family only (pt_variants.h: HAS_FIBRE), so a scene that holds one is shaded by that
family throughout and keeps the loop to the end (no tail kernel)."""
import ctypes as C
import ctypes.util
import json
import os

import numpy as np
import pytest

import bsdf_cases as bc
import fibre_cases as fc
import oracle_lib
import scenes
import tungsten_amd as tg
from tungsten_amd import capi
from test_oracle_golden import flat_bsdf_index

pytestmark = pytest.mark.gpu

FAMILY_MARKER = 0xF << 20                 # FEAT_BUMP | FEAT_CYLINDER | FEAT_AUX | FEAT_MEDIA: together only in the all-features family's mask
OTHER_FAMILIES = [v for v in range(capi.TGHIP_BSDF_VARIANT_COUNT) if v != capi.TGHIP_BSDF_VARIANT_ALL]

_rendered = {}


def _launches(c):
    return (int(c.launches_trace_closest), int(c.launches_trace_shadow), int(c.launches_shade), int(c.tail_launches))


def _render(name, tmp_path_factory):
    if name not in _rendered:
        mk, kw = fc.CASES[name]
        gold = np.load(os.path.join(scenes.GOLDEN, name + "_samples.npz"))
        ref, seed = gold["samples"], int(gold["seed"])
        h, w, spp, _ = ref.shape
        path = mk(tmp_path_factory.mktemp(name), name=name + ".json", **kw)
        r = tg.Renderer(path, seed=seed)
        try:
            assert (r.width, r.height) == (w, h)
            r.set_option("time_kernels", 1)
            sobol = bool(r.info.stratified_sampler)
            got = r.trace_samples(0, spp, seed=seed, tile_seeds=oracle_lib.dice_tiles(w, h, seed)[0] if sobol else None)
            _, ssum, count = r.image()
            c = r.counters()
            tm, _, covered_all, mask_all = r.debug_bsdf_info(capi.TGHIP_BSDF_VARIANT_ALL)
            others = {v: r.debug_bsdf_info(v)[2] for v in OTHER_FAMILIES}
            _rendered[name] = dict(got=got, ref=ref, ssum=ssum.copy(), count=count.copy(), family=(tm, covered_all, mask_all, others),
                                   launches=_launches(c), shadow_rays=int(c.shadow_rays))
        finally:
            r.close()
    return _rendered[name]


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_device_samples_are_the_reference_bit_for_bit(name, tmp_path_factory):
    res = _render(name, tmp_path_factory)
    got, ref = res["got"], res["ref"]
    equal = (got == ref).all(axis=-1)
    off = np.abs(got - ref).max(axis=-1) > 1e-3*(np.abs(ref).max(axis=-1) + 1e-3)
    print("%s: %d of %d samples equal, %d on another path, launches (closest, shadow, shade, tail) %s" % (
        name, int(equal.sum()), equal.size, int(off.sum()), res["launches"]))
    assert np.isfinite(got).all() and ref.max() > 0
    assert equal.all(), "%s: %d of %d device samples are not the reference's (%d of them on another path); first at (y, x, sample) %s" % (
        name, int((~equal).sum()), equal.size, int(off.sum()), np.argwhere(~equal)[:4].tolist())


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_framebuffer_is_the_sum_of_the_samples(name, tmp_path_factory):
    res = _render(name, tmp_path_factory)
    assert (res["count"] == res["ref"].shape[2]).all()
    assert np.allclose(res["got"].sum(axis=2), res["ssum"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_fibre_scenes_take_the_all_features_family(name, tmp_path_factory):
    res = _render(name, tmp_path_factory)
    tm, covered_all, mask_all, others = res["family"]
    assert mask_all == 0xFFFFFFFF & ~(1 << 30)                    # (the debug instantiation: BSDF_MASK_ALL without the Sobol' sampler)
    assert len(tm) > 0 and ((tm & FAMILY_MARKER) == FAMILY_MARKER).all() and covered_all.all()
    for v, covered in others.items():
        assert not covered.any(), "%s: family %s would shade a material of a scene that holds a fibre BCSDF" % (name, capi.TGHIP_BSDF_VARIANT_NAMES[v])
    closest, shadow, shade, tail = res["launches"]
    assert shade > 0 and tail == 0 and closest > 0 and res["shadow_rays"] > 0


# ---- single calls ----
@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    path = fc.bsdf_scene(tmp_path_factory.mktemp("fibre_bsdfs"))
    with open(path) as f:
        sj = json.load(f)
    r = tg.Renderer(path)
    yield sj, r
    r.close()


def test_device_bsdf_calls_are_the_references_word_for_word(fixture):
    """f, pdf, sample_ok and -- where the sample succeeded -- wo, weight, pdf and the sampled lobe as bit patterns (a NaN would match a NaN; the
    golden holds none), and the count of numbers the sample consumed through the stream's next number."""
    sj, r = fixture
    g = np.load(fc.BSDF_GOLDEN)
    names, per, ref = list(g["names"]), int(g["cases_per_bsdf"]), g["ref"]
    n = len(names)*per
    dc = np.zeros(n, tg.BSDF_CASE_DTYPE)
    for pos, name in enumerate(names):
        dc["bsdf"][pos*per:(pos + 1)*per] = flat_bsdf_index(sj, bc.scene_index(sj, name))
    dc["wi"], dc["wo"], dc["uv"], dc["requested"], dc["stream"] = g["wi"], g["wo"], g["uv"], g["requested"], g["stream"]
    dc["seed"], dc["variant"] = int(g["seed"]), capi.TGHIP_BSDF_VARIANT_ALL
    out = r.debug_bsdf(dc)
    got = np.concatenate([out["f"].view(np.uint32), out["pdf"].view(np.uint32)[:, None], out["sample_ok"][:, None], out["sample_wo"].view(np.uint32),
                          out["sample_weight"].view(np.uint32), out["sample_pdf"].view(np.uint32)[:, None], out["sampled"][:, None],
                          np.zeros((n, 1), np.uint32)], axis=1)
    want = ref.copy()
    want[:, 13] = 0
    bad = np.nonzero(bc.differing(got, want))[0]
    for pos, name in enumerate(names):
        print("%s: %d of %d cases differ from the reference" % (name, int(((bad >= pos*per) & (bad < (pos + 1)*per)).sum()), per))
    assert len(bad) == 0, "cases %s, e.g. %s case %d: %s" % (
        bad[:8], names[bad[0]//per], bad[0] % per, [(bc.WORDS[w], hex(got[bad[0], w]), hex(want[bad[0], w])) for w in np.nonzero(got[bad[0]] != want[bad[0]])[0]])
    assert (got[:, 4] == ref[:, 4]).all() and ref[:, 4].sum() > 1000
    # the numbers consumed: next1D, then next2D -- three -- wherever a fibre's sample ran (more under a wrapper that draws its own)
    ok = ref[:, 4] == 1
    xi = np.concatenate([oracle_lib.rng_streams(int(g["seed"]), int(g["stream"][pos*per]), per, bc.NXI + 1) for pos in range(len(names))])
    drawn = xi[np.arange(n), ref[:, 13]]
    assert (out["next"].view(np.uint32)[ok] == drawn.view(np.uint32)[ok]).all()
    plain = np.isin(np.arange(n)//per, [names.index(x) for x in names if x.startswith("wire_") or x in ("lambertian_fiber", "fibre_bumped", "cutWire", "cut")])
    assert (ref[ok & plain, 13] == 3).all()


def test_other_families_are_black_on_a_fibre(fixture):
    """The two types have no bit in any mask: every family but the all-features one folds them away (black, zero pdf, failed sample)."""
    sj, r = fixture
    idx = flat_bsdf_index(sj, bc.scene_index(sj, "wire_r035")), flat_bsdf_index(sj, bc.scene_index(sj, "lambertian_fiber"))
    for variant in OTHER_FAMILIES:
        dc = np.zeros(64, tg.BSDF_CASE_DTYPE)
        dc["bsdf"] = np.where(np.arange(64) % 2 == 0, idx[0], idx[1])
        dc["wi"], dc["wo"] = bc._unit([0.3, -0.2, 0.9]), bc._unit([-0.4, 0.5, 0.6])
        dc["requested"], dc["stream"], dc["seed"], dc["variant"] = bc.ALL_LOBES, np.arange(64), bc.SEED, variant
        out = r.debug_bsdf(dc)
        assert (out["f"] == 0).all() and (out["pdf"] == 0).all() and (out["sample_ok"] == 0).all(), capi.TGHIP_BSDF_VARIANT_NAMES[variant]


def test_device_sinhf_is_the_host_libms(fixture):
    """2^20 bit patterns spread evenly over [2^-30, 10] and both ends, bit-equal to sinhf of the host's libm.so.6."""
    _, r = fixture
    lo, hi = int(np.float32(2.0**-30).view(np.uint32)), int(np.float32(10.0).view(np.uint32))
    bits = np.unique(np.concatenate([np.linspace(lo, hi, 1 << 20).astype(np.uint64), [lo, hi]])).astype(np.uint32)
    x = bits.view(np.float32)
    assert x[0] == np.float32(2.0**-30) and x[-1] == np.float32(10.0) and x.size > (1 << 20) - 8
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.sinhf.restype, libm.sinhf.argtypes = C.c_float, [C.c_float]
    want = np.fromiter((libm.sinhf(float(v)) for v in x), np.float32, x.size)
    got = r.debug_libm(capi.TGHIP_LIBM_SINHF, x)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert len(bad) == 0, "%d of %d differ, first x = %r: device %r, libm %r" % (len(bad), x.size, x[bad[0]], got[bad[0]], want[bad[0]])
    outside = r.debug_libm(capi.TGHIP_LIBM_SINHF, np.array([0.0, -1.0, 10.000001, np.inf, np.nan], np.float32))
    assert np.isnan(outside).all()                          # outside the restated domain: NaN, never a wrong number


# ---- control ----
# (launches_trace_closest, launches_trace_shadow, launches_shade, tail_launches) of a whole render of the 48 x 27, 8 spp Cornell box with
# "time_kernels", as recorded before the fibre BCSDFs existed (tests/test_gpu_sampled_textures.py holds the same figures): one run-to-completion launch
CORNELL_LAUNCHES_BEFORE = (1, 1, 1, 0)


def test_a_scene_without_a_fibre_launches_what_it_did(tmp_path):
    mk, kw = scenes.GOLDEN_CASES["cornell"]
    r = tg.Renderer(mk(tmp_path, name="cornell.json", **kw), seed=tg.DEFAULT_SEED)
    try:
        r.set_option("time_kernels", 1)
        r.render()
        launches = _launches(r.counters())
        tm, _, _, _ = r.debug_bsdf_info(capi.TGHIP_BSDF_VARIANT_ALL)
        lean = r.debug_bsdf_info(capi.TGHIP_BSDF_VARIANT_LEAN)[2]
    finally:
        r.close()
    flat = tg.FlattenedScene(mk(tmp_path, name="cornell_check.json", **kw))
    traits = capi.TgHostSceneTraits()
    assert tg.lib.tgh_scene_check(flat.desc, C.byref(traits), None, 0) == 0
    flat.close()
    assert traits.have_fibre == 0 and traits.all_features_shading == 0 and traits.lean_scene == 1
    assert ((tm & FAMILY_MARKER) == 0).all() and lean.all()          # the lean family, as before
    assert launches == CORNELL_LAUNCHES_BEFORE
