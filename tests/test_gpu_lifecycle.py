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
