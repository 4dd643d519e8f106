"""Life cycle of the C-ABI's objects on the device: contexts, scenes and pools created and destroyed many times must give their memory back.  A front end that re-opens
a renderer per frame (the reference's editor and its batch mode both do: one TraceableScene per render, renderer/TraceableScene.hpp:64-134) would otherwise run a long
session out of HBM."""
import ctypes as C

import numpy as np
import pytest

import scenes
import tungsten_amd as tg

pytestmark = pytest.mark.gpu


def _free_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_renderers_give_their_memory_back(tmp_path):
    """60 renders, each through a renderer of its own (scene upload, path pool, framebuffer, adaptive-pass buffers, auxiliary buffers in every third one):
    the device's free memory after the 60th is what it was after the 10th, and every render is the first one's image."""
    plain = scenes.cornell(tmp_path, name="a.json", resolution=(160, 90), spp=8)
    adaptive = scenes.cornell(tmp_path, name="b.json", resolution=(160, 90), spp=32, spp_step=16, renderer={"adaptive_sampling": True, "stratified_sampler": True})
    first, marks = {}, {}
    for i in range(60):
        path = adaptive if i % 3 == 2 else plain
        r = tg.Renderer(path, seed=tg.DEFAULT_SEED)
        r.render()
        mean = r.image()[0]
        r.close()
        if path in first:
            assert np.array_equal(mean, first[path]), "render %d differs from the first of its scene" % i
        else:
            first[path] = mean
        if i in (9, 59):
            marks[i] = _free_bytes()
    assert marks[9] - marks[59] < 32 << 20, "device memory shrank by %.1f MB over 50 renderers" % ((marks[9] - marks[59])/2.0**20)


def _render_once(ctx, npix, seed=tg.DEFAULT_SEED):
    """One pass of sample 0 into a cleared framebuffer; returns (sum, count) as downloaded."""
    assert tg.lib.tghip_clear_framebuffer(ctx) == 0
    p = tg.TgHipPassDesc(0, 1, seed, 0, 1, 0)
    assert tg.lib.tghip_render_pass(ctx, C.byref(p)) == 0 and tg.lib.tghip_wait(ctx) == 0
    s, c = np.empty((npix, 3), np.float32), np.empty(npix, np.uint32)
    assert tg.lib.tghip_download_framebuffer(ctx, s.ctypes.data, c.ctypes.data, npix) == 0
    return s, c


def test_a_refused_upload_leaves_the_uploaded_scene_as_it_was(tmp_path):
    """A description tghip_upload_scene refuses -- here for its camera type, one of the checks that used to come after the old scene had been released --
    leaves the context exactly as it was: the scene uploaded before renders the same pass to the same bytes, without another upload.  A valid second
    scene on the same context then renders the image a fresh context gives."""
    if not scenes.have_materialtest():
        pytest.skip("materialtest assets (assets/) not present")
    w, h = 32, 18
    box = tg.FlattenedScene(scenes.cornell(tmp_path, resolution=(w, h), spp=1))
    mt = tg.FlattenedScene(scenes.materialtest(tmp_path, resolution=(w, h), spp=1))
    ctx = tg.lib.tghip_create(0)
    assert ctx, tg.lib.tghip_last_error(None)
    assert tg.lib.tghip_upload_scene(ctx, box.desc) == 0
    s0, c0 = _render_once(ctx, w*h)
    assert c0.min() == 1 and s0.max() > 0
    bad = tg.TgHipSceneDesc.from_buffer_copy(box.desc.contents)
    bad.camera.type = 7
    assert tg.lib.tghip_upload_scene(ctx, C.byref(bad)) == -6        # TGHIP_E_UNSUPPORTED
    assert b"unknown camera type" in tg.lib.tghip_last_error(ctx)
    s1, c1 = _render_once(ctx, w*h)
    assert s1.tobytes() == s0.tobytes() and c1.tobytes() == c0.tobytes()
    assert tg.lib.tghip_upload_scene(ctx, mt.desc) == 0
    s2, c2 = _render_once(ctx, w*h)
    fresh = tg.lib.tghip_create(0)
    assert fresh, tg.lib.tghip_last_error(None)
    assert tg.lib.tghip_upload_scene(fresh, mt.desc) == 0
    s3, c3 = _render_once(fresh, w*h)
    assert s2.tobytes() == s3.tobytes() and c2.tobytes() == c3.tobytes() and s2.tobytes() != s0.tobytes()
    tg.lib.tghip_destroy(fresh)
    tg.lib.tghip_destroy(ctx)
    box.close()
    mt.close()


def test_contexts_give_their_on_demand_arrays_back(tmp_path):
    """30 contexts, each one used for everything that makes a context allocate on demand -- a TGHIP_PASS_AUX pass (pool, partial sums, aux buffers), tghip_develop
    of the frame and of an aux output into host memory (scratch images, the depth maximum), tghip_nlmeans from host pointers (four planes), tghip_query_rays in
    both modes and tghip_query_radiance with and without the Sobol' sampler on host rays (counter, rays, answers, the virtual image's framebuffer and tile seeds),
    tghip_trace_rays (per-call arrays) -- and destroyed: the device's free memory after the 30th is what it was after the 5th, and every context's develop and
    query answers are the first one's, byte for byte."""
    w, h, n = 160, 90, 1024
    flat = tg.FlattenedScene(scenes.cornell(tmp_path, resolution=(w, h), spp=1, renderer={"stratified_sampler": True}))
    assert flat.desc.contents.num_sobol_words > 0
    rnd = np.random.RandomState(7)
    d = rnd.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.empty((n, 8), np.float32)
    rays[:, 0:3] = np.array([0.0, 1.0, 0.0]) + rnd.uniform(-0.3, 0.3, size=(n, 3))
    rays[:, 3], rays[:, 4:7], rays[:, 7] = 1e-4, d, np.inf
    planes = [np.ascontiguousarray(rnd.uniform(0.0, 1.0, size=(64, 64)), np.float32) for _ in range(3)]
    planes[2] *= 0.01
    first, marks = None, {}
    for i in range(30):
        ctx = tg.lib.tghip_create(0)
        assert ctx, tg.lib.tghip_last_error(None)

        def ok(rc):
            assert rc == 0, tg.lib.tghip_last_error(ctx)
        ok(tg.lib.tghip_upload_scene(ctx, flat.desc))
        p = tg.TgHipPassDesc(0, 1, tg.DEFAULT_SEED, 0, 1, tg.capi.TGHIP_PASS_AUX)
        ok(tg.lib.tghip_render_pass(ctx, C.byref(p)))
        ok(tg.lib.tghip_wait(ctx))
        got = {}
        hdr, ldr = np.empty((w*h, 3), np.float32), np.empty((w*h, 3), np.uint8)
        dd = tg.capi.TgHipDevelopDesc(tg.capi.TGHIP_DEVELOP_FRAME, tg.capi.TGHIP_DEVELOP_MEAN, tg.capi.TGHIP_TONEMAP_GAMMA, 0)
        ok(tg.lib.tghip_develop(ctx, C.byref(dd), hdr.ctypes.data, ldr.ctypes.data, w*h))
        got["hdr"], got["ldr"] = hdr, ldr
        depth, depth8 = np.empty(w*h, np.float32), np.empty((w*h, 3), np.uint8)
        dd = tg.capi.TgHipDevelopDesc(tg.capi.TGHIP_AUX_DEPTH, tg.capi.TGHIP_DEVELOP_MEAN, 0, 0)
        ok(tg.lib.tghip_develop(ctx, C.byref(dd), depth.ctypes.data, depth8.ctypes.data, w*h))
        got["depth"], got["depth8"] = depth, depth8
        nd = tg.capi.TgHipNlMeansDesc(64, 64, 1, 1, 2, 0.45, 1.0, tg.capi.TGHIP_NLMEANS_POINTERS, 0, 0, 0)
        got["nlm"] = np.empty((64, 64), np.float32)
        ok(tg.lib.tghip_nlmeans(ctx, C.byref(nd), planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, got["nlm"].ctypes.data))
        got["closest"], got["occluded"] = np.empty((n, 4), np.float32), np.empty(n, np.uint8)
        for mode, out in ((tg.capi.TGHIP_QUERY_CLOSEST, got["closest"]), (tg.capi.TGHIP_QUERY_OCCLUDED, got["occluded"])):
            qd = tg.capi.TgHipRayQueryDesc(mode, 0)
            ok(tg.lib.tghip_query_rays(ctx, C.byref(qd), rays.ctypes.data, out.ctypes.data, n))
        for name, flags in (("radiance", 0), ("radiance_sobol", tg.capi.TGHIP_RADIANCE_SOBOL)):
            got[name], got[name + "_count"] = np.empty((n, 3), np.float32), np.empty(n, np.uint32)
            rd = tg.capi.TgHipRadianceQueryDesc(flags, tg.DEFAULT_SEED, 0, 1, 0x5EED1234)
            ok(tg.lib.tghip_query_radiance(ctx, C.byref(rd), rays.ctypes.data, got[name].ctypes.data, got[name + "_count"].ctypes.data, n))
        got["hits"] = np.empty((n, 4), np.float32)
        ok(tg.lib.tghip_trace_rays(ctx, rays.ctypes.data, got["hits"].ctypes.data, n, 1, None))
        tg.lib.tghip_destroy(ctx)
        if first is None:
            first = got
            assert got["occluded"].any() and got["radiance"].max() > 0 and got["radiance_sobol"].max() > 0 and (got["radiance_count"] == 1).all()
            assert got["hdr"].max() > 0 and got["depth"].max() > 0
            assert got["radiance"].tobytes() != got["radiance_sobol"].tobytes()
        for name in first:
            assert got[name].tobytes() == first[name].tobytes(), "context %d: %s differs from the first context's" % (i, name)
        if i in (4, 29):
            marks[i] = _free_bytes()
    flat.close()
    assert marks[4] - marks[29] < 32 << 20, "device memory shrank by %.1f MB over 25 contexts" % ((marks[4] - marks[29])/2.0**20)
