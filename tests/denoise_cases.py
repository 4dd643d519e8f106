"""Shared by the NL-means tests (tests/test_denoise_cpu.py, tests/test_gpu_denoise.py) and tools/make_denoise_golden.py: the cases of
tests/golden/nlmeans.npz, their seeded inputs, the calls into the library and the bit comparison."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nlmeans.npz")
REF_NLMEANS = os.path.join(ROOT, "oracle", "_ref", "ref_nlmeans")

# name, W, H, F, R, k, variance scale, channels
CASES = [
    ("prefilter_70x37", 70, 37, 3, 5, 0.5, 2.0, 1),       # 3 x 2 tiles; the last column of tiles 6 wide = 2F (fast path at its limit), the last row 5 high < 2F (slow path)
    ("mse_70x37_rgb", 70, 37, 1, 9, 1.0, 1.0, 3),         # the MSE / selection filter's parameters; the search window wider than the partial tiles
    ("final_70x37", 70, 37, 3, 2, 0.5, 1.0, 1),           # the final-feature filter's parameters
    ("strip_33x32", 33, 32, 3, 5, 0.5, 2.0, 1),           # a tile one pixel wide
    ("tiny_5x4_rgb", 5, 4, 3, 5, 0.5, 2.0, 3),            # smaller than every radius: every rectangle takes the slow path
    ("packed_70x37_x4", 70, 37, 3, 5, 0.5, 2.0, 4),       # four packed features, as SimdNlMeans packs them
]
CASE_NAMES = [c[0] for c in CASES]


def case(name):
    return CASES[CASE_NAMES.index(name)]


def make_inputs(name):
    """(image, guide, variance), float32 [H, W] or [H, W, C]: the guide a smooth ramp plus noise, flat inside a patch of the zero band; the variance
    positive with a band of columns of exact zeros (guide[p] == guide[q] there gives 0/1e-7); the image independent noise."""
    _, w, h, _, _, _, _, ch = case(name)
    rng = np.random.RandomState(7000 + CASE_NAMES.index(name))
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    shape = (h, w, ch)
    ramp = (x/np.float32(w) + np.float32(0.5)*y/np.float32(h))[..., None]*(np.float32(1.0) + np.float32(0.25)*np.arange(ch, dtype=np.float32))
    guide = (ramp + np.float32(0.05)*rng.standard_normal(shape).astype(np.float32)).astype(np.float32)
    variance = (np.float32(0.002) + np.float32(0.004)*rng.random_sample(shape).astype(np.float32)).astype(np.float32)
    image = rng.random_sample(shape).astype(np.float32)
    b0, b1 = w//3, w//3 + max(1, w//9)
    variance[:, b0:b1] = 0.0
    guide[h//4:max(h//2, h//4 + 1), b0:b1] = np.float32(0.5)
    if ch == 1:
        image, guide, variance = image[..., 0], guide[..., 0], variance[..., 0]
    return tuple(np.ascontiguousarray(a) for a in (image, guide, variance))


def load_golden():
    """{name: (image, guide, variance, result)} as recorded from the reference's own nlMeans (tools/make_denoise_golden.py)."""
    z = np.load(GOLDEN)
    assert [str(n) for n in z["names"]] == CASE_NAMES
    for i, c in enumerate(CASES):
        assert tuple(z["params"][i]) == tuple(np.float64(v) for v in c[1:]), c[0]
    return {n: tuple(z["%s_%s" % (n, part)] for part in ("image", "guide", "variance", "result")) for n in CASE_NAMES}


def differing_words(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def desc_for(capi, image, F, R, k, scale, flags=0):
    return capi.TgHipNlMeansDesc(image.shape[1], image.shape[0], image.shape[2] if image.ndim == 3 else 1, F, R, k, scale,
                                 capi.TGHIP_NLMEANS_POINTERS, 0, 0, flags)


def host_nlmeans(image, guide, variance, F, R, k, scale):
    """tgh_nlmeans_host: the library's host comparator."""
    import tungsten_amd as tg
    from tungsten_amd import capi
    image, guide, variance = (np.ascontiguousarray(a, np.float32) for a in (image, guide, variance))
    out = np.empty_like(image)
    desc = desc_for(capi, image, F, R, k, scale)
    assert tg.lib.tgh_nlmeans_host(C.byref(desc), image.ctypes.data, guide.ctypes.data, variance.ctypes.data, out.ctypes.data) == 0
    return out


def reference_nlmeans(image, guide, variance, F, R, k, scale, tmpdir, threads=4):
    """oracle/_ref/ref_nlmeans: the reference's nlMeans<float> / nlMeans<Vec3f>; a four-channel image as four one-channel runs."""
    import subprocess
    if image.ndim == 3 and image.shape[2] not in (1, 3):
        return np.stack([reference_nlmeans(image[..., c], guide[..., c], variance[..., c], F, R, k, scale, tmpdir, threads)
                         for c in range(image.shape[2])], axis=-1)
    h, w = image.shape[:2]
    ch = image.shape[2] if image.ndim == 3 else 1
    src, dst = os.path.join(str(tmpdir), "nlm_in.raw"), os.path.join(str(tmpdir), "nlm_out.raw")
    np.concatenate([np.ascontiguousarray(a, np.float32).ravel() for a in (image, guide, variance)]).tofile(src)
    subprocess.check_call([REF_NLMEANS, str(w), str(h), str(ch), str(F), str(R), repr(float(k)), repr(float(scale)), str(threads), src, dst],
                          stdout=subprocess.DEVNULL)
    return np.fromfile(dst, np.float32).reshape(image.shape)
