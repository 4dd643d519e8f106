"""The NL-means filter on the device (tghip_nlmeans, csrc/hip/denoise.hip) against the host comparator (tgh_nlmeans_host) and the results recorded
from the reference (tests/golden/nlmeans.npz), bit for bit: every recorded case -- partial tiles at the fast path's limit and below it, a tile
one pixel wide, an image smaller than every radius, three and four channels --, host arrays and torch tensors, the context's auxiliary buffers
as source, the error cases."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_cases as dc
import scenes
import tungsten_amd as tg
from tungsten_amd import capi

pytestmark = pytest.mark.gpu

W, H = 70, 37


@pytest.fixture(scope="module")
def golden():
    return dc.load_golden()


@pytest.fixture(scope="module")
def renderer(tmp_path_factory):
    """The golden Cornell box at 70 x 37 with the auxiliary outputs, four samples per pixel."""
    tmp = tmp_path_factory.mktemp("denoise")
    r = tg.Renderer(scenes.cornell(tmp, resolution=(W, H), spp=4, edit=scenes._outputs), seed=tg.DEFAULT_SEED)
    r.render()
    assert (r.width, r.height) == (W, H)
    yield r
    r.close()


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_device_is_the_host_and_the_reference_bit_for_bit(renderer, golden, name):
    _, _, _, F, R, k, scale, _ = dc.case(name)
    image, guide, variance, want = golden[name]
    got = renderer.nlmeans(image, guide, variance, F, R, k, scale)
    assert got.shape == want.shape
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%d words differ from the reference, first at %s: %r != %r" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    assert dc.differing_words(got, dc.host_nlmeans(image, guide, variance, F, R, k, scale)) == 0
    assert dc.differing_words(renderer.nlmeans(image, guide, variance, F, R, k, scale), got) == 0     # two runs are identical
    ms = C.c_double(0.0)
    assert tg.lib.tghip_nlmeans_kernel_time(renderer.context(), C.byref(ms)) == 0 and ms.value > 0.0


@pytest.mark.parametrize("batch", [1, 2, 16])
def test_every_batch_size_gives_the_same_bits(renderer, golden, batch):
    """The offsets box-filtered at once are a matter of scheduling: the sums stay in offset order."""
    renderer.set_option("nlmeans_batch", batch)
    try:
        for name in ("prefilter_70x37", "mse_70x37_rgb", "tiny_5x4_rgb"):
            _, _, _, F, R, k, scale, _ = dc.case(name)
            image, guide, variance, want = golden[name]
            assert dc.differing_words(renderer.nlmeans(image, guide, variance, F, R, k, scale), want) == 0, name
    finally:
        renderer.set_option("nlmeans_batch", 0)


def test_limits_of_the_radii(renderer, golden):
    """F = 8 with four channels (one offset's planes above 64 KiB of LDS), R = 16, F = 0 and R = 0 against the host comparator."""
    image, guide, variance, _ = golden["packed_70x37_x4"]
    for sub, F, R in ((np.s_[:, :, :], 8, 1), (np.s_[:, :, 0], 1, 16), (np.s_[:, :, :2], 0, 2), (np.s_[:, :, 1], 2, 0)):
        args = [np.ascontiguousarray(a[sub]) for a in (image, guide, variance)]
        got = renderer.nlmeans(*args, F=F, R=R, k=0.7, variance_scale=1.5)
        assert dc.differing_words(got, dc.host_nlmeans(*args, F, R, 0.7, 1.5)) == 0, (F, R)


def test_aux_source_and_prefilter_features(renderer):
    ctx = renderer.context()
    features = renderer.prefilter_features()
    assert sorted(features) == ["albedo", "depth", "normal", "visibility"]
    changed = 0
    for output, name in enumerate(tg.AUX_OUTPUT_NAMES):
        planes = {part: renderer.develop(name, part, hdr=True) for part in ("a", "b", "variance")}
        for image_part, guide_part, slot in (("a", "b", 0), ("b", "a", 1)):
            want = dc.host_nlmeans(planes[image_part], planes[guide_part], planes["variance"], 3, 5, 0.5, 2.0)
            desc = capi.TgHipNlMeansDesc(W, H, 0, 3, 5, 0.5, 2.0, output, tg.DEVELOP_PART_NAMES.index(image_part), tg.DEVELOP_PART_NAMES.index(guide_part), 0)
            got = np.empty((H, W, capi.TGHIP_AUX_CHANNEL_COUNT[output]), np.float32)
            assert tg.lib.tghip_nlmeans(ctx, C.byref(desc), None, None, None, got.ctypes.data) == 0, tg.lib.tghip_last_error(ctx)
            assert dc.differing_words(got, want) == 0, (name, image_part)
            changed += dc.differing_words(got, planes[image_part])
            if name in features:
                assert dc.differing_words(features[name][slot], want) == 0, (name, image_part)
    assert changed > 0                                     # (the filter did something to the render's noise)


def test_device_tensors(tmp_path):
    """TGHIP_DEVELOP_DEVICE_POINTERS with torch tensors, in a process of its own: torch brings its own HIP runtime and has to be imported before
    this package (tests/denoise_torch_worker.py)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "denoise_torch_worker.py")
    p = subprocess.run([sys.executable, worker, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and "DENOISE_TORCH_OK" in p.stdout, p.stdout[-4000:]


def test_error_cases_leave_the_context_working(tmp_path, golden):
    r = tg.Renderer(scenes.cornell(tmp_path, resolution=(W, H), spp=1), seed=tg.DEFAULT_SEED)    # (no auxiliary outputs: no aux buffer)
    r.render()
    ctx = r.context()
    image, guide, variance, want = golden["final_70x37"]
    out = np.empty_like(image)
    ptr = capi.TGHIP_NLMEANS_POINTERS
    ok = dict(width=W, height=H, channels=1, F=3, R=2, k=0.5, variance_scale=1.0, source=ptr, image_part=0, guide_part=0, flags=0)

    def call(ctx_, desc, arrays=(image, guide, variance), out_=out):
        return tg.lib.tghip_nlmeans(ctx_, C.byref(desc) if desc is not None else None, *[a.ctypes.data if a is not None else None for a in arrays],
                                    out_.ctypes.data if out_ is not None else None)

    def fails(desc, **kw):
        assert call(ctx, desc, **kw) == capi.TGHIP_E_INVALID
        assert b"tghip_nlmeans" in tg.lib.tghip_last_error(ctx)

    assert call(None, capi.TgHipNlMeansDesc(**ok)) == capi.TGHIP_E_INVALID
    fails(None)
    for bad in (dict(channels=0), dict(channels=5), dict(F=9), dict(R=17), dict(k=0.0), dict(k=-0.5), dict(width=0), dict(height=0), dict(source=5)):
        fails(capi.TgHipNlMeansDesc(**dict(ok, **bad)))
    fails(capi.TgHipNlMeansDesc(**ok), arrays=(image, None, variance))                               # a pointer missing without an aux source
    fails(capi.TgHipNlMeansDesc(**ok), out_=None)
    fails(capi.TgHipNlMeansDesc(**dict(ok, source=capi.TGHIP_AUX_DEPTH)), arrays=(None, None, None))  # an aux source before an aux buffer exists
    aux = np.zeros(W*H, tg.AUX_DTYPE)
    aux["count"][:] = 2
    aux["variance"][:] = 0.5
    assert tg.lib.tghip_upload_aux(ctx, aux.ctypes.data, W*H) == 0
    fails(capi.TgHipNlMeansDesc(**dict(ok, source=capi.TGHIP_AUX_DEPTH)))                            # pointers given with an aux source
    fails(capi.TgHipNlMeansDesc(**dict(ok, source=capi.TGHIP_AUX_DEPTH, width=W - 1)), arrays=(None, None, None))   # not the frame's size
    fails(capi.TgHipNlMeansDesc(**dict(ok, source=capi.TGHIP_AUX_DEPTH, image_part=capi.TGHIP_DEVELOP_VARIANCE)), arrays=(None, None, None))
    with pytest.raises(tg.TungstenError):
        r.nlmeans(image, guide[:, :-1], variance, 3, 2, 0.5)
    # ... and the context works: a valid call with pointers, one with the aux source, and a correct render afterwards
    assert call(ctx, capi.TgHipNlMeansDesc(**ok)) == 0
    assert dc.differing_words(out, want) == 0
    flat = r.nlmeans_aux("depth", "a", "b", 3, 2, 0.5)
    assert flat.shape == (H, W, 1) and (flat == 0).all()
    mean = r.image()[0]
    r.close()
    r = tg.Renderer(scenes.cornell(tmp_path, resolution=(W, H), spp=1), seed=tg.DEFAULT_SEED)
    r.render()
    assert dc.differing_words(r.image()[0], mean) == 0
    r.close()
