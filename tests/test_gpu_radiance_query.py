"""tghip_query_radiance on the device (csrc/hip/radiance_query.hip in front of the wavefront loop's own kernels): a query on a pinhole camera's own
rays returns that camera's samples -- the oracle's AND the reference's (tests/golden/*_samples.npz), float32 == in every channel of every ray, no
tolerance and no ray left out --; several samples in one call add up in index order whatever the options; the Sobol' sampler; the scene's camera
type changes nothing; closed-form rays on a one-bounce Cornell box, independent of the oracle; the context's state is left alone; the refusals;
torch tensors on the device.  tests/test_radiance_query_cpu.py checks, without a device, the two facts about the oracle and the goldens used here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import scenes
import tungsten_amd as tg
from tungsten_amd import capi
from test_oracle_golden import _oracle_samples

pytestmark = pytest.mark.gpu

INVALID, NOSCENE, UNSUPPORTED = capi.TGHIP_E_INVALID, capi.TGHIP_E_NOSCENE, capi.TGHIP_E_UNSUPPORTED
DEVICE, SOBOL = capi.TGHIP_DEVELOP_DEVICE_POINTERS, capi.TGHIP_RADIANCE_SOBOL
# the pinhole golden cases: the flat list that a pass fuses into k_shade, the 8-wide walk whose pass folds its finish and ends in k_tail, a mesh
# emitter (closest-hit shadow walks), every shading class, instances, media, and the metric's scene
CAMERA_CASES = ("cornell", "cornell_nee_off", "cornell_minb2", "cornell_box_filter", "cornell_mesh_light", "zoo_d", "cornell_instances", "cornell_fog",
                "materialtest")

_lib = oracle_lib._lib
_lib.oracle_trace_sample_log.argtypes = [oracle_lib.DESC_P, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]
_lib.oracle_trace_sample_log.restype = C.c_int


def camera_rays(flat, w, h, seed, s):
    """The rays of sample s of every pixel, in pixel order: oracle_lib.camera_ray of the two numbers the pixel's stream starts with."""
    rays = np.empty((w*h, 8), np.float32)
    for pixel in range(w*h):
        xi = oracle_lib.rng_stream(seed, pixel, s, 2)
        o, d = oracle_lib.camera_ray(flat.desc, pixel % w, pixel//w, xi[0], xi[1])
        rays[pixel] = [o[0], o[1], o[2], 1e-4, d[0], d[1], d[2], np.inf]
    return rays


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def in_order(parts):
    """float32 sums and counts of single-sample answers added in index order, starting from zero"""
    ssum, count = np.zeros_like(parts[0][0]), np.zeros_like(parts[0][1])
    for s, c in parts:
        ssum = (ssum + s).astype(np.float32)
        count = count + c
    return ssum, count


# ---- 1. the camera's own rays give the camera's own samples ----

@pytest.mark.parametrize("name", CAMERA_CASES)
def test_the_cameras_own_rays_give_the_cameras_own_samples(name, tmp_path):
    if "materialtest" in name and not scenes.have_materialtest():
        pytest.skip("materialtest assets (assets/) not present")
    mk, kw = scenes.GOLDEN_CASES[name]
    gold = np.load(os.path.join(scenes.GOLDEN, name + "_samples.npz"))
    ref, seed = gold["samples"], int(gold["seed"])
    h, w, spp, _ = ref.shape
    assert w*h in (576, 1296, 2304)
    ora = _oracle_samples(mk, kw, name, tmp_path, ref, seed)
    assert (ora == ref).all()                                 # (the oracle is the reference on these cases: tests/test_oracle_golden.py)
    path = mk(tmp_path, name=name + "_q.json", **kw)
    flat = tg.FlattenedScene(path)
    assert flat.desc.contents.camera.type == 0 and not flat.info.stratified_sampler
    r = tg.Renderer(path, seed=seed)
    try:
        for s in range(spp):
            rays = camera_rays(flat, w, h, seed, s)
            ssum, count = r.query_radiance(rays, s, s + 1, seed=seed)
            want_ora, want_ref = ora[:, :, s].reshape(-1, 3), ref[:, :, s].reshape(-1, 3)
            print("%s sample %d: %d of %d rays differ from the oracle, %d from the reference" % (
                name, s, int((ssum != want_ora).any(axis=-1).sum()), w*h, int((ssum != want_ref).any(axis=-1).sum())))
            assert np.isfinite(want_ref).all()
            assert (ssum == want_ora).all() and (ssum == want_ref).all()
            assert count.dtype == np.uint32 and (count == 1).all()
    finally:
        r.close()
        flat.close()


# ---- 2. several samples in one call ----

@pytest.mark.parametrize("name", ["cornell", "zoo_d"])
def test_several_samples_in_one_call_add_up_in_index_order(name, tmp_path):
    mk, kw = scenes.GOLDEN_CASES[name]
    w, h = kw["resolution"]
    path = mk(tmp_path, name=name + ".json", **kw)
    flat = tg.FlattenedScene(path)
    rays = camera_rays(flat, w, h, tg.DEFAULT_SEED, 0)       # held fixed: the rays of sample 0
    flat.close()
    r = tg.Renderer(path)
    try:
        singles = [r.query_radiance(rays, s, s + 1) for s in range(8)]
        want = in_order(singles)
        assert (want[1] == 8).all() and len({p[0].tobytes() for p in singles}) == 8
        got = r.query_radiance(rays, 0, 8)
        assert same_bytes(got[0], want[0]) and same_bytes(got[1], want[1])
        tail = r.query_radiance(rays, 3, 8)
        want_tail = in_order(singles[3:])
        assert same_bytes(tail[0], want_tail[0]) and same_bytes(tail[1], want_tail[1])
        # every slot regenerates several times (10 368 items on a few hundred slots); batches cut by sample range and by tile; items of any size asked for
        for options in ({"max_slots": 256}, {"max_slots": 1024, "max_items": 1024}, {"chunk_samples": 1}, {"chunk_samples": 4},
                        {"chunk_samples": 4, "max_slots": 512, "max_items": 4096}, {"streams": 1}, {"check_interval": 1}):
            for k, v in options.items():
                r.set_option(k, v)
            try:
                again = r.query_radiance(rays, 0, 8)
                assert same_bytes(again[0], want[0]) and same_bytes(again[1], want[1]), options
            finally:
                for k in options:
                    r.set_option(k, {"max_slots": 1 << 23, "max_items": 1 << 26, "chunk_samples": 0, "streams": 0, "check_interval": 0}[k])
        # a part of the batch: ray i draws from stream i whatever follows it (997 rays: 11 padding pixels behind them)
        part = r.query_radiance(rays[:997], 0, 8)
        assert same_bytes(part[0], want[0][:997]) and same_bytes(part[1], want[1][:997])
    finally:
        r.close()


# ---- 3. the Sobol' sampler ----

def test_sobol_queries_match_the_oracles_sobol_sampler(tmp_path):
    w, h, spp, seed, T = 32, 18, 4, tg.DEFAULT_SEED, 0x5EED1234
    path = scenes.cornell(tmp_path, resolution=(w, h), spp=spp, renderer={"stratified_sampler": True})
    flat = tg.FlattenedScene(path)
    assert flat.desc.contents.num_sobol_words > 0
    rgb, log = (C.c_float*3)(), (C.c_float*8)()
    rays, want = np.empty((spp, w*h, 8), np.float32), np.empty((spp, w*h, 3), np.float32)
    for s in range(spp):
        for pixel in range(w*h):
            px, py = pixel % w, pixel//w
            assert _lib.oracle_trace_sample_log(flat.desc, seed, T, 1, px, py, s, rgb, log, 8) >= 2
            o, d = oracle_lib.camera_ray(flat.desc, px, py, log[0], log[1])
            rays[s, pixel] = [o[0], o[1], o[2], 1e-4, d[0], d[1], d[2], np.inf]
            want[s, pixel] = oracle_lib.trace_sample(flat.desc, seed, px, py, s, tile_seed=T)
            assert (want[s, pixel] == np.array(rgb[:], np.float32)).all()
    flat.close()
    r = tg.Renderer(path, seed=seed)
    try:
        for s in range(spp):
            ssum, count = r.query_radiance(rays[s], s, s + 1, seed=seed, sobol_seed=T)
            print("sobol sample %d: %d of %d rays differ from the oracle" % (s, int((ssum != want[s]).any(axis=-1).sum()), w*h))
            assert (ssum == want[s]).all() and (count == 1).all()
        other = r.query_radiance(rays[0], 0, 1, seed=seed, sobol_seed=T + 1)[0]
        plain = r.query_radiance(rays[0], 0, 1, seed=seed)[0]
        assert not same_bytes(other, want[0]) and not same_bytes(plain, want[0])
    finally:
        r.close()


# ---- 4. the scene's camera does not matter ----

def test_the_scenes_camera_does_not_matter(tmp_path):
    w, h, seed = 32, 18, 77
    paths = {"pinhole": scenes.cornell(tmp_path, resolution=(w, h), spp=1, name="pinhole.json"),
             "thinlens": scenes.cornell(tmp_path, resolution=(w, h), spp=1, name="thinlens.json", edit=scenes._thinlens(0.35)),
             "equirectangular": scenes.cornell(tmp_path, resolution=(48, 27), spp=1, name="equi.json", edit=scenes._equirectangular),
             "cubemap": scenes.cornell(tmp_path, resolution=(48, 36), spp=1, name="cube.json", edit=scenes._cubemap("horizontal_cross"))}
    flat = tg.FlattenedScene(paths["pinhole"])
    rays = camera_rays(flat, w, h, seed, 0)
    flat.close()
    answers = {}
    for which, path in paths.items():
        r = tg.Renderer(path)
        answers[which] = r.query_radiance(rays, 2, 6, seed=seed)
        r.close()
    assert (answers["pinhole"][1] == 4).all() and answers["pinhole"][0].max() > 0
    for which in ("thinlens", "equirectangular", "cubemap"):
        assert same_bytes(answers[which][0], answers["pinhole"][0]) and same_bytes(answers[which][1], answers["pinhole"][1]), which


# ---- 5. closed form, independent of the oracle ----

def test_closed_form_rays_on_the_one_bounce_cornell_box(tmp_path):
    """max_bounces 1: a path ends at its first hit -- the light's emission when that is the light's front, nothing otherwise (no next-event estimation
    at the last bounce, no infinite emitter in the scene).  tests/test_radiance_query_cpu.py holds the emission claim to the cornell_bounce1 golden."""
    path = scenes.cornell(tmp_path, resolution=(32, 18), spp=1, integrator={"max_bounces": 1})
    flat = tg.FlattenedScene(path)
    d = flat.desc.contents
    light = [d.objects[i] for i in range(d.num_objects) if d.objects[i].emission >= 0]
    assert len(light) == 1
    emission = np.array(list(d.textures[light[0].emission].value), np.float32)
    base, e0, e1 = (np.array(list(v), np.float64) for v in (light[0].base, light[0].edge0, light[0].edge1))
    lo, hi = np.array(list(d.bounds_lo), np.float64), np.array(list(d.bounds_hi), np.float64)
    flat.close()
    assert (emission > 0).all() and abs(base[1] - 1.98) < 1e-3         # the light lies under the ceiling, facing down; the blocks end at y = 1.2
    rs = np.random.RandomState(9)
    n = 997
    origins = np.stack([rs.uniform(-0.9, 0.9, n), rs.uniform(1.3, 1.9, n), rs.uniform(-0.9, 0.9, n)], axis=1)    # above the blocks, under the light

    def aimed(targets, tmax=np.inf):
        dirs = targets - origins
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        return np.concatenate([origins, np.full((n, 1), 1e-4), dirs, np.full((n, 1), tmax)], axis=1).astype(np.float32)

    uv = rs.uniform(0.05, 0.95, (n, 2))
    at_light = aimed(base + uv[:, :1]*e0 + uv[:, 1:]*e1)
    at_floor = aimed(np.stack([rs.uniform(-0.9, 0.9, n), np.zeros(n), rs.uniform(-0.9, 0.9, n)], axis=1))
    away = rs.randn(n, 3)
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    centre, radius = 0.5*(lo + hi), 0.5*np.linalg.norm(hi - lo)
    outside = np.concatenate([centre + away*(1.05*radius + 1e-3), np.full((n, 1), 1e-4), away, np.full((n, 1), np.inf)], axis=1).astype(np.float32)
    r = tg.Renderer(path)
    try:
        for begin, end in ((0, 1), (5, 12)):
            spp = end - begin
            ssum, count = r.query_radiance(at_light, begin, end)
            want = np.zeros(3, np.float32)
            for _ in range(spp):
                want = (want + emission).astype(np.float32)
            assert (count == spp).all() and (ssum == want).all()
            for rays in (at_floor, outside):
                ssum, count = r.query_radiance(rays, begin, end)
                assert (count == spp).all() and (ssum == 0).all()
        # the end of the first segment, well clear of the light's distance on either side (the edge itself: the test below)
        hits = r.query_rays(at_light, "closest")
        assert (hits["rec"] >= 0).all()
        short, reach = at_light.copy(), at_light.copy()
        short[:, 7] = hits["t"]*np.float32(0.75)
        reach[:, 7] = hits["t"]*np.float32(1.25)
        s_short, c_short = r.query_radiance(short, 0, 3)
        s_reach, c_reach = r.query_radiance(reach, 0, 3)
        assert (c_short == 3).all() and (s_short == 0).all()
        assert (c_reach == 3).all() and (s_reach == (emission + emission + emission).astype(np.float32)).all()
        # tmin behind the light: nothing left to hit
        behind = at_light.copy()
        behind[:, 3] = np.nextafter(hits["t"], np.float32(np.inf))
        assert (r.query_radiance(behind, 0, 2)[0] == 0).all()
        # batches of 1, 997 (above) and 0 rays
        one = r.query_radiance(at_light[:1], 0, 2)
        assert one[0].shape == (1, 3) and (one[0] == emission + emission).all() and one[1][0] == 2
        none = r.query_radiance(np.zeros((0, 8), np.float32), 0, 2)
        assert none[0].shape == (0, 3) and none[1].shape == (0,)
        # nothing is written outside the n entries, and an answer is written over, not added to
        ctx = r.context()
        ssum, count = np.full((n + 16, 3), 7.5, np.float32), np.full(n + 16, 9, np.uint32)
        desc = capi.TgHipRadianceQueryDesc(0, tg.DEFAULT_SEED & 0xFFFFFFFF, 0, 2)
        for _ in range(2):
            assert tg.lib.tghip_query_radiance(ctx, C.byref(desc), at_light.ctypes.data, ssum.ctypes.data, count.ctypes.data, n) == 0
            assert (ssum[:n] == emission + emission).all() and (count[:n] == 2).all()
            assert (ssum[n:] == 7.5).all() and (count[n:] == 9).all()
        assert tg.lib.tghip_query_radiance(ctx, C.byref(desc), at_light.ctypes.data, ssum.ctypes.data, None, n) == 0      # the counts are optional
        ms = C.c_double(-1.0)
        assert tg.lib.tghip_query_radiance_kernel_time(ctx, C.byref(ms)) == 0 and ms.value > 0.0
    finally:
        r.close()


def test_the_first_segment_ends_exactly_at_tmax(tmp_path):
    """The edge of the first segment [tmin, tmax): a light-bound ray with tmax = the t tghip_query_rays reports returns 0, the same ray with
    tmax = nextafter(t, inf) the emission -- for every ray.  (The closest-hit walks are the reference's and answer within a few ulps of their far
    distance by their own arithmetic -- a quad accepts t <= far, a leaf is skipped by its box's entry distance: started with far = tmax they gave the
    emission to 480 of these 997 rays at tmax = t and nothing to 197 of them at nextafter(t) --, so a query's walk looks 2^-10 further than tmax and
    k_query_clip ends the segment exactly, behind every closest-hit launch.)"""
    path = scenes.cornell(tmp_path, resolution=(32, 18), spp=1, integrator={"max_bounces": 1})
    flat = tg.FlattenedScene(path)
    d = flat.desc.contents
    light = [d.objects[i] for i in range(d.num_objects) if d.objects[i].emission >= 0][0]
    emission = np.array(list(d.textures[light.emission].value), np.float32)
    base, e0, e1 = (np.array(list(v), np.float64) for v in (light.base, light.edge0, light.edge1))
    flat.close()
    rs = np.random.RandomState(9)
    n = 997
    origins = np.stack([rs.uniform(-0.9, 0.9, n), rs.uniform(1.3, 1.9, n), rs.uniform(-0.9, 0.9, n)], axis=1)
    uv = rs.uniform(0.05, 0.95, (n, 2))
    dirs = base + uv[:, :1]*e0 + uv[:, 1:]*e1 - origins
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    at_light = np.concatenate([origins, np.full((n, 1), 1e-4), dirs, np.full((n, 1), np.inf)], axis=1).astype(np.float32)
    r = tg.Renderer(path)
    try:
        hits = r.query_rays(at_light, "closest")
        assert (hits["rec"] >= 0).all()
        short, reach = at_light.copy(), at_light.copy()
        short[:, 7] = hits["t"]
        reach[:, 7] = np.nextafter(hits["t"], np.float32(np.inf))
        s_short, c_short = r.query_radiance(short, 0, 3)
        s_reach, c_reach = r.query_radiance(reach, 0, 3)
        print("tmax = t: %d of %d rays see the light; tmax = nextafter(t): %d" % (int((s_short != 0).any(axis=-1).sum()), n, int((s_reach != 0).any(axis=-1).sum())))
        three = (emission + emission + emission).astype(np.float32)
        assert (c_short == 3).all() and (s_short == 0).all()
        assert (c_reach == 3).all() and (s_reach == three).all()
        # the same edge where the path goes on behind it: the full integrator on the same box, the ray cut just in front of the light and just behind it
        full = tg.Renderer(scenes.cornell(tmp_path, resolution=(32, 18), spp=1, name="full.json"))
        try:
            whole = full.query_radiance(at_light, 0, 3)
            cut, kept = full.query_radiance(short, 0, 3), full.query_radiance(reach, 0, 3)
            assert (cut[1] == 3).all() and (cut[0] == 0).all()                      # nothing inside the segment, no infinite emitter: black
            assert same_bytes(kept[0], whole[0]) and same_bytes(kept[1], whole[1])   # the light inside it: the path an unbounded ray takes
        finally:
            full.close()
    finally:
        r.close()


@pytest.mark.parametrize("name", ["zoo_d", "cornell_instances", "materialtest"])
def test_the_segments_end_on_the_other_walks(name, tmp_path):
    """The same edge where the walk is not the flat list's and the path goes on: every shading class (zoo_d), the walk through the reference's instance
    tree (cornell_instances), the 8-wide walk under an environment map (materialtest).  For every camera ray that hits something at t (tghip_query_rays):
    cut at nextafter(t, inf) it returns the unbounded ray's answer bit for bit; cut at t it returns what a ray returns that hits nothing -- the same
    ray, same index and numbers, started beyond the scene's bounds: black, or the environment's radiance in its direction.  Rays that hit nothing
    are in the batch unchanged."""
    if "materialtest" in name and not scenes.have_materialtest():
        pytest.skip("materialtest assets (assets/) not present")
    mk, kw = scenes.GOLDEN_CASES[name]
    w, h = kw["resolution"]
    path = mk(tmp_path, name=name + ".json", **kw)
    flat = tg.FlattenedScene(path)
    rays = camera_rays(flat, w, h, tg.DEFAULT_SEED, 0)
    d = flat.desc.contents
    lo, hi = np.array(list(d.bounds_lo), np.float64), np.array(list(d.bounds_hi), np.float64)
    flat.close()
    r = tg.Renderer(path)
    try:
        hits = r.query_rays(rays, "closest")
        hit = hits["rec"] >= 0
        assert hit.sum() >= len(rays)//2
        # beyond the bounds along the ray, moving away from them: nothing left to hit (checked), the escaped path's answer
        beyond = rays.copy()
        reach_out = np.linalg.norm(hi - lo) + np.linalg.norm(rays[:, 0:3] - 0.5*(lo + hi), axis=1) + 1.0
        beyond[:, 0:3] = rays[:, 0:3] + rays[:, 4:7]*reach_out[:, None].astype(np.float32)
        assert (r.query_rays(beyond, "closest")["rec"] == -1).all()
        short, reach = rays.copy(), rays.copy()
        short[hit, 7] = hits["t"][hit]
        reach[hit, 7] = np.nextafter(hits["t"][hit], np.float32(np.inf))
        whole, escaped = r.query_radiance(rays, 0, 3), r.query_radiance(beyond, 0, 3)
        kept, cut = r.query_radiance(reach, 0, 3), r.query_radiance(short, 0, 3)
        print("%s: %d of %d rays hit; cut behind the hit %d differ from the unbounded ray, cut at the hit %d differ from the escaped one" % (
            name, int(hit.sum()), len(rays), int((kept[0] != whole[0]).any(axis=-1).sum()), int((cut[0][hit] != escaped[0][hit]).any(axis=-1).sum())))
        assert (whole[1] == 3).all() and not same_bytes(whole[0][hit], escaped[0][hit])
        assert same_bytes(kept[0], whole[0]) and same_bytes(kept[1], whole[1])
        assert same_bytes(cut[0][hit], escaped[0][hit]) and (cut[1] == 3).all()
        assert same_bytes(cut[0][~hit], whole[0][~hit])
    finally:
        r.close()


# ---- 6. the context's state ----

def _pass(ctx, begin, end, flags=0):
    p = capi.TgHipPassDesc(begin, end, tg.DEFAULT_SEED & 0xFFFFFFFF, 0, 1, flags)
    assert tg.lib.tghip_render_pass(ctx, C.byref(p)) == 0 and tg.lib.tghip_wait(ctx) == 0


def _state(ctx, w, h):
    ssum, count = np.empty((h, w, 3), np.float32), np.empty((h, w), np.uint32)
    rec = np.zeros(((w + 3)//4)*((h + 3)//4), oracle_lib.DEVICE_RECORD_DTYPE)
    assert tg.lib.tghip_download_framebuffer(ctx, ssum.ctypes.data, count.ctypes.data, w*h) == 0
    assert tg.lib.tghip_download_records(ctx, rec.ctypes.data, rec.size) == 0
    return ssum, count, rec


@pytest.mark.parametrize("name, flags", [("cornell", 0), ("cornell", capi.TGHIP_PASS_RECORDS), ("zoo_d", 0), ("cornell_equirectangular", 0)])
def test_passes_after_a_query_are_the_passes_without_it(name, flags, tmp_path):
    mk, kw = scenes.GOLDEN_CASES[name]
    w, h = kw["resolution"]
    path = mk(tmp_path, name=name + ".json", **kw)
    rs = np.random.RandomState(4)
    dirs = rs.randn(700, 3)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = np.concatenate([np.tile([[0.1, 1.0, 0.2, 1e-4]], (700, 1)), dirs, np.full((700, 1), np.inf)], axis=1).astype(np.float32)
    r = tg.Renderer(path)
    ctx = r.context()
    try:
        # a fresh context's [0, 8) in one pass.  (Whole groups: k_resolve adds a pass's samples up in groups of four counted from the pass's first, so
        # [0, 4) + [4, 8) and [0, 8) round alike, where [0, 2) + [2, 4) and [0, 4) would not, with or without a query between them.)
        fresh = tg.Renderer(path)
        try:
            assert tg.lib.tghip_clear_framebuffer(fresh.context()) == 0
            _pass(fresh.context(), 0, 8, flags)
            whole = _state(fresh.context(), w, h)
        finally:
            fresh.close()
        assert (whole[1] == 8).all()
        # ... and the same two passes without a query: the SampleRecords see their samples pass by pass, so theirs is the state to hold the records to
        assert tg.lib.tghip_clear_framebuffer(ctx) == 0
        _pass(ctx, 0, 4, flags)
        _pass(ctx, 4, 8, flags)
        want = _state(ctx, w, h)
        assert same_bytes(want[0], whole[0]) and same_bytes(want[1], whole[1]) and (want[2]["sample_count"] == whole[2]["sample_count"]).all()
        answers = []
        for ask in (1, 2):
            assert tg.lib.tghip_clear_framebuffer(ctx) == 0
            _pass(ctx, 0, 4, flags)
            before = _state(ctx, w, h)
            for _ in range(ask):
                answers.append(r.query_radiance(rays, 1, 4))
            after = _state(ctx, w, h)
            assert all(same_bytes(a, b) for a, b in zip(before, after))          # the query itself touches none of it
            _pass(ctx, 4, 8, flags)
            got = _state(ctx, w, h)
            assert same_bytes(got[0], whole[0]) and same_bytes(got[1], whole[1]), (name, flags, ask)      # the fresh context's [0, 8), bit for bit
            assert all(same_bytes(a, b) for a, b in zip(got, want)), (name, flags, ask)                   # the passes without the query, records included
        assert all(same_bytes(a[0], answers[0][0]) and same_bytes(a[1], answers[0][1]) for a in answers) and (answers[0][1] == 3).all()
        c0 = r.counters()
        r.query_radiance(rays, 0, 2)
        c1 = r.counters()
        print("counters: %d samples, %d iterations for 700 rays x 2 samples" % (c1.samples - c0.samples, c1.iterations - c0.iterations))
        assert c1.samples - c0.samples == 704*2 and c1.iterations > c0.iterations      # counted as by a pass: 700 rays and the 4 padding pixels of their image
    finally:
        r.close()


# ---- 7. the refusals on the device ----

def test_error_paths_leave_the_context_working(tmp_path):
    path = scenes.cornell(tmp_path, resolution=(32, 18), spp=1)
    flat = tg.FlattenedScene(path)
    rays = np.ascontiguousarray(camera_rays(flat, 32, 18, tg.DEFAULT_SEED, 0)[:256])
    flat.close()
    r = tg.Renderer(path)
    ctx = r.context()
    ssum, count = np.zeros((256, 3), np.float32), np.zeros(256, np.uint32)
    want = r.query_radiance(rays, 0, 2)

    def call(ctx_, flags=0, spp=(0, 2), reserved=(0, 0, 0), rays_=rays.ctypes.data, sum_=ssum.ctypes.data, count_=count.ctypes.data, n=256, desc=True):
        d = capi.TgHipRadianceQueryDesc(flags, tg.DEFAULT_SEED & 0xFFFFFFFF, spp[0], spp[1], 5, (C.c_uint32*3)(*reserved))
        return tg.lib.tghip_query_radiance(ctx_, C.byref(d) if desc else None, rays_, sum_, count_, n)

    try:
        assert call(ctx, n=0) == 0 and call(ctx, rays_=None, sum_=None, count_=None, n=0) == 0
        for kw, code, message in ((dict(desc=False), INVALID, "no description"), (dict(rays_=None), INVALID, "rays and rgb_sum"),
                                  (dict(sum_=None), INVALID, "rays and rgb_sum"), (dict(flags=4), INVALID, "unknown flag"),
                                  (dict(reserved=(0, 0, 1)), INVALID, "reserved"), (dict(spp=(2, 2)), INVALID, "spp_end"), (dict(spp=(3, 2)), INVALID, "spp_end"),
                                  (dict(flags=SOBOL), INVALID, "sobol_matrices"),            # this scene carries no Sobol' matrices
                                  (dict(n=2**31), INVALID, "2^31 - 1"),
                                  (dict(n=2**20, spp=(0, 2**12)), UNSUPPORTED, "2^32 samples"),
                                  # (the check looks at the pointers' values only: nothing is read through these)
                                  (dict(flags=DEVICE, rays_=rays.ctypes.data//16*16 + 8), INVALID, "16-byte aligned"),
                                  (dict(flags=DEVICE, rays_=rays.ctypes.data//16*16, sum_=ssum.ctypes.data//4*4 + 2), INVALID, "4-byte aligned"),
                                  (dict(flags=DEVICE, rays_=rays.ctypes.data//16*16, sum_=ssum.ctypes.data//4*4, count_=count.ctypes.data//4*4 + 1), INVALID,
                                   "4-byte aligned")):
            assert call(ctx, **kw) == code, kw
            assert message in tg.lib.tghip_last_error(ctx).decode(), kw
            again = r.query_radiance(rays, 0, 2)                                             # ... and the context still answers
            assert same_bytes(again[0], want[0]) and same_bytes(again[1], want[1])
        bare = tg.lib.tghip_create(0)                                                        # a context without an upload
        assert bare
        try:
            assert call(bare) == NOSCENE and call(bare, n=0) == NOSCENE
            assert call(bare, desc=False) == INVALID
        finally:
            tg.lib.tghip_destroy(bare)
        assert call(ctx) == 0 and same_bytes(ssum, want[0]) and same_bytes(count, want[1])
    finally:
        r.close()


# ---- 8. torch tensors on the device ----

def test_device_tensors(tmp_path):
    """query_radiance_into with torch tensors on the device gives the bytes of query_radiance, and a framebuffer bound to torch tensors is left alone
    by a query.  In a process of its own: torch brings its own HIP runtime and has to be imported before this package
    (tests/radiance_query_torch_worker.py)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "radiance_query_torch_worker.py")
    p = subprocess.run([sys.executable, worker, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and "RADIANCE_QUERY_TORCH_OK" in p.stdout, p.stdout[-4000:]
