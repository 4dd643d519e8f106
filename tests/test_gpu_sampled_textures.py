"""The sampled-texture cases on the device: every case of tests/sampled_texture_cases.py through Renderer.trace_samples against the reference's own
per-sample radiance (tests/golden/stex_*_samples.npz, tools/make_sampled_texture_golden.py) -- bit for bit in every sample, the project's standing
norm; no case is exempt and none has a divergence allowance.  Each case is rendered once (10 368 samples) and shared by the tests below.

A checker's sample / pdf are compiled into the all-features shading family only (pt_scene.h: HAS_PROCTEX), so a scene whose SAMPLED environment is a
checker is shaded by that family throughout; the new apertures are branches of cameraRay<LENS> alone.  Scenes with none of the new forms launch
what they launched before."""
import os

import numpy as np
import pytest

import oracle_lib
import sampled_texture_cases as stc
import scenes
import texture_cases
import tungsten_amd as tg
from tungsten_amd import capi

pytestmark = pytest.mark.gpu

FAMILY_MARKER = 0xF << 20                 # FEAT_BUMP | FEAT_CYLINDER | FEAT_AUX | FEAT_MEDIA: together only in the all-features family's mask
OTHER_FAMILIES = [v for v in range(capi.TGHIP_BSDF_VARIANT_COUNT) if v != capi.TGHIP_BSDF_VARIANT_ALL]

_rendered = {}


def _launches(c):
    return (int(c.launches_trace_closest), int(c.launches_trace_shadow), int(c.launches_shade), int(c.tail_launches))


def _render(name, tmp_path_factory):
    if name not in _rendered:
        mk, kw = stc.CASES[name]
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


@pytest.mark.parametrize("name", sorted(stc.CASES))
def test_device_samples_are_the_reference_bit_for_bit(name, tmp_path_factory):
    res = _render(name, tmp_path_factory)
    got, ref = res["got"], res["ref"]
    equal = (got.view(np.uint32) == ref.view(np.uint32)).all(axis=-1)
    off = np.abs(got - ref).max(axis=-1) > 1e-3*(np.abs(ref).max(axis=-1) + 1e-3)
    print("%s: %d of %d samples bit-equal, %d on another path, launches (closest, shadow, shade, tail) %s" % (
        name, int(equal.sum()), equal.size, int(off.sum()), res["launches"]))
    assert np.isfinite(got).all() and ref.max() > 0
    assert equal.all(), "%s: %d of %d device samples are not the reference's bit for bit (%d of them on another path); first at (y, x, sample) %s" % (
        name, int((~equal).sum()), equal.size, int(off.sum()), np.argwhere(~equal)[:4].tolist())


@pytest.mark.parametrize("name", sorted(stc.CASES))
def test_framebuffer_is_the_sum_of_the_samples(name, tmp_path_factory):
    res = _render(name, tmp_path_factory)
    assert (res["count"] == res["ref"].shape[2]).all()
    assert np.allclose(res["got"].sum(axis=2), res["ssum"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", stc.SAMPLED_CHECKER_CASES)
def test_sampled_checker_environments_take_the_all_features_family(name, tmp_path_factory):
    res = _render(name, tmp_path_factory)
    tm, covered_all, mask_all, others = res["family"]
    assert mask_all == 0xFFFFFFFF & ~(1 << 30)                    # (the debug instantiation: BSDF_MASK_ALL without the Sobol' sampler)
    assert len(tm) > 0 and ((tm & FAMILY_MARKER) == FAMILY_MARKER).all() and covered_all.all()
    for v, covered in others.items():
        assert not covered.any(), "%s: family %s would shade a material of a scene that samples a checker environment" % (name, capi.TGHIP_BSDF_VARIANT_NAMES[v])
    closest, shadow, shade, tail = res["launches"]
    assert shade > 0 and tail == 0 and closest > 0 and res["shadow_rays"] > 0


def test_an_unsampled_checker_environment_keeps_its_family(tmp_path_factory):
    tm, covered_all, _, others = _render("stex_env_checker_unsampled", tmp_path_factory)["family"]
    assert ((tm & FAMILY_MARKER) == 0).all() and covered_all.all()
    assert others[capi.TGHIP_BSDF_VARIANT_SIMPLE].all()           # Lambert throughout: the class-0 family, as before


def test_the_cateye_checker_lens_has_failed_direction_samples(tmp_path_factory):
    """stex_lens_checker: cat-eye vignetting makes some direction samples fail -- black samples (PathTracer.cpp:27-28) --, in the golden as on the device."""
    for name in ("stex_lens_checker", "stex_lens_checker_sobol"):
        ref = _render(name, tmp_path_factory)["ref"]
        black = (ref == 0).all(axis=-1)
        assert 0 < black.sum() < black.size


# (launches_trace_closest, launches_trace_shadow, launches_shade, tail_launches) of a whole render with "time_kernels" on the commit before
# checker environments, the new apertures and cap pivots existed, recorded there: the Cornell box (one run-to-completion launch, counted once in
# each), the thin lens with its default disk, a sampled disk environment (the all-features family) and the sun-and-sky box (two infinite lights)
LAUNCHES_BEFORE = {
    "cornell": (1, 1, 1, 0),
    "cornell_thinlens": (1, 1, 1, 0),
    "tex_env_disk": (16, 16, 16, 0),
    "cornell_sun_sky": (24, 24, 48, 0),
}


@pytest.mark.parametrize("name", sorted(LAUNCHES_BEFORE))
def test_a_scene_without_the_new_forms_launches_what_it_did(name, tmp_path):
    mk, kw = scenes.GOLDEN_CASES[name] if name in scenes.GOLDEN_CASES else texture_cases.CASES[name]
    r = tg.Renderer(mk(tmp_path, name=name + ".json", **kw), seed=tg.DEFAULT_SEED)
    try:
        r.set_option("time_kernels", 1)
        r.render()
        launches = _launches(r.counters())
        tm = r.debug_bsdf_info(capi.TGHIP_BSDF_VARIANT_ALL)[0]
    finally:
        r.close()
    print("%s: launches (closest, shadow, shade, tail) %s" % (name, launches))
    assert (((tm & FAMILY_MARKER) == FAMILY_MARKER).all() if name == "tex_env_disk" else ((tm & FAMILY_MARKER) == 0).all())
    assert launches == LAUNCHES_BEFORE[name]
