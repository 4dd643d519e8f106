"""The `disk`, `blade` and `ies` textures on the device: every case of tests/texture_cases.py through Renderer.trace_samples against the reference's
own per-sample radiance (tests/golden/tex_*_samples.npz, tools/make_texture_golden.py) -- bit for bit in every sample, the project's standing norm;
no case is exempt and none has a divergence allowance.  Each case is rendered once (10 368 samples) and shared by the tests below.

Disk and blade are evaluated by the all-features shading family only (pt_scene.h: HAS_PROCTEX), so a scene that holds one is shaded by that family
throughout: tghip_debug_bsdf_info then reports the family's marker bits in every material's mask and no other family as covering it.  An `ies`
texture is a scalar bitmap by the time it reaches the device: those scenes keep the kernels they would have had with any other bitmap."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib
import scenes
import texture_cases
import tungsten_amd as tg
from tungsten_amd import capi

pytestmark = pytest.mark.gpu

FAMILY_MARKER = 0xF << 20                 # FEAT_BUMP | FEAT_CYLINDER | FEAT_AUX | FEAT_MEDIA: together only in the all-features family's mask
OTHER_FAMILIES = [v for v in range(capi.TGHIP_BSDF_VARIANT_COUNT) if v != capi.TGHIP_BSDF_VARIANT_ALL]
PROCEDURAL = sorted(set(texture_cases.CASES) - set(texture_cases.IES_CASES))

_rendered = {}


def _family_info(r):
    tm, _, covered_all, mask_all = r.debug_bsdf_info(capi.TGHIP_BSDF_VARIANT_ALL)
    others = {v: r.debug_bsdf_info(v)[2] for v in OTHER_FAMILIES}
    return tm, covered_all, mask_all, others


def _render(name, tmp_path_factory):
    if name not in _rendered:
        mk, kw = texture_cases.CASES[name]
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
            _rendered[name] = dict(got=got, ref=ref, ssum=ssum.copy(), count=count.copy(), family=_family_info(r),
                                   launches=(int(c.launches_trace_closest), int(c.launches_trace_shadow), int(c.launches_shade), int(c.tail_launches)),
                                   shadow_rays=int(c.shadow_rays))
        finally:
            r.close()
    return _rendered[name]


@pytest.mark.parametrize("name", sorted(texture_cases.CASES))
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


@pytest.mark.parametrize("name", sorted(texture_cases.CASES))
def test_framebuffer_is_the_sum_of_the_samples(name, tmp_path_factory):
    res = _render(name, tmp_path_factory)
    assert (res["count"] == res["ref"].shape[2]).all()
    assert np.allclose(res["got"].sum(axis=2), res["ssum"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", PROCEDURAL)
def test_disk_and_blade_scenes_take_the_all_features_family(name, tmp_path_factory):
    res = _render(name, tmp_path_factory)
    tm, covered_all, mask_all, others = res["family"]
    assert mask_all == 0xFFFFFFFF & ~(1 << 30)                    # (the debug instantiation: BSDF_MASK_ALL without the Sobol' sampler)
    assert len(tm) > 0 and ((tm & FAMILY_MARKER) == FAMILY_MARKER).all() and covered_all.all()
    for v, covered in others.items():
        assert not covered.any(), "%s: family %s would shade a material of a scene with a disk / blade texture" % (name, capi.TGHIP_BSDF_VARIANT_NAMES[v])
    closest, shadow, shade, tail = res["launches"]
    assert shade > 0 and tail == 0 and closest > 0                # the wavefront loop's per-class launches: never fused, never k_tail
    if name in texture_cases.CUTOUT_CASES:
        assert shadow > 0 and res["shadow_rays"] > 0              # the closest-hit shadow walk that evaluates alpha on the way


@pytest.mark.parametrize("name", texture_cases.IES_CASES)
def test_ies_scenes_are_bitmap_scenes(name, tmp_path_factory):
    tm, covered_all, _, others = _render(name, tmp_path_factory)["family"]
    assert ((tm & FAMILY_MARKER) == 0).all() and covered_all.all()
    assert others[capi.TGHIP_BSDF_VARIANT_SIMPLE].any()           # the Lambert walls: the class-0 family, as with any other bitmap in the scene


def _plain(name, tmp_path):
    mk, kw = scenes.GOLDEN_CASES[name]
    r = tg.Renderer(mk(tmp_path, name=name + ".json", **kw), seed=tg.DEFAULT_SEED)
    try:
        r.set_option("time_kernels", 1)
        r.render()
        c = r.counters()
        tm = r.debug_bsdf_info(capi.TGHIP_BSDF_VARIANT_ALL)[0]
        cover = {v: r.debug_bsdf_info(v)[2] for v in range(capi.TGHIP_BSDF_VARIANT_COUNT)}
        return tm, cover, (int(c.launches_trace_closest), int(c.launches_trace_shadow), int(c.launches_shade), int(c.tail_launches))
    finally:
        r.close()


# (launches_trace_closest, launches_trace_shadow, launches_shade, tail_launches) of a whole render with "time_kernels" on the commit before these
# textures existed, recorded there: the Cornell box (one run-to-completion launch, counted once in each), zoo_c (checker alpha: the
# closest-hit shadow walk with MASK_ALL_NO_PROCTEX) and cornell_bump (the all-features family without a disk or blade)
LAUNCHES_BEFORE = {
    "cornell": (1, 1, 1, 0),
    "zoo_c": (16, 16, 48, 0),
    "cornell_bump": (24, 24, 96, 0),
}


@pytest.mark.parametrize("name", sorted(LAUNCHES_BEFORE))
def test_a_scene_without_the_new_textures_launches_what_it_did(name, tmp_path):
    tm, cover, launches = _plain(name, tmp_path)
    print("%s: launches (closest, shadow, shade, tail) %s" % (name, launches))
    assert ((tm & FAMILY_MARKER) == 0).all()
    assert cover[capi.TGHIP_BSDF_VARIANT_ALL].all() and cover[capi.TGHIP_BSDF_VARIANT_FULL].all()
    if name == "cornell":
        assert cover[capi.TGHIP_BSDF_VARIANT_LEAN].all() and cover[capi.TGHIP_BSDF_VARIANT_SIMPLE].all()
    assert launches == LAUNCHES_BEFORE[name]


def test_upload_refuses_an_unknown_texture_type(tmp_path):
    flat = tg.FlattenedScene(texture_cases.build(tmp_path, name="albedo.json", edit=texture_cases._albedo, **texture_cases.SIZE))
    d = flat.desc.contents
    ctx = tg.lib.tghip_create(0)
    assert ctx
    try:
        textures = (capi.TgHipTexture*d.num_textures)()
        C.memmove(textures, d.textures, C.sizeof(textures))
        procedural = [i for i in range(d.num_textures) if textures[i].type in (capi.TGHIP_TEX_DISK, capi.TGHIP_TEX_BLADE)]
        assert procedural
        textures[procedural[0]].type = 5
        bad = tg.TgHipSceneDesc.from_buffer_copy(d)
        bad.textures = C.cast(textures, C.POINTER(capi.TgHipTexture))
        assert tg.lib.tghip_upload_scene(ctx, C.byref(bad)) == -6     # TGHIP_E_UNSUPPORTED
        assert b"texture type" in tg.lib.tghip_last_error(ctx)
        textures[procedural[0]].type = -1
        assert tg.lib.tghip_upload_scene(ctx, C.byref(bad)) == -6
        assert tg.lib.tghip_upload_scene(ctx, flat.desc) == 0         # disk (3) and blade (4) are accepted
    finally:
        tg.lib.tghip_destroy(ctx)
        flat.close()
