"""The NL-means filter without a device: the host comparator (tgh_nlmeans_host, csrc/host/Denoise.cpp) against results recorded from the
reference's own nlMeans (tests/golden/nlmeans.npz, tools/make_denoise_golden.py), bit for bit; the fixture against the reference harness where
it was built; the in-place slow box filter spelt out; a plain numpy statement of the filter's meaning; the ctypes layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_cases as dc
from tungsten_amd import capi


@pytest.fixture(scope="module")
def golden():
    return dc.load_golden()


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_host_comparator_is_the_reference_bit_for_bit(golden, name):
    _, w, h, F, R, k, scale, ch = dc.case(name)
    image, guide, variance, want = golden[name]
    assert want.shape == ((h, w) if ch == 1 else (h, w, ch)) and np.isfinite(want).all()
    got = dc.host_nlmeans(image, guide, variance, F, R, k, scale)
    assert dc.differing_words(got, want) == 0


def test_fixture_inputs_are_the_seeded_builders(golden):
    for name in dc.CASE_NAMES:
        for a, b in zip(dc.make_inputs(name), golden[name][:3]):
            assert dc.differing_words(a, b) == 0, name
        variance = golden[name][2]
        assert (variance == 0).any() and (variance >= 0).all(), name


def test_packed_channels_are_independent_scalar_filters(golden):
    image, guide, variance, want = golden["packed_70x37_x4"]
    _, _, _, F, R, k, scale, _ = dc.case("packed_70x37_x4")
    for c in range(4):
        got = dc.host_nlmeans(image[..., c], guide[..., c], variance[..., c], F, R, k, scale)
        assert dc.differing_words(got, want[..., c]) == 0


@pytest.mark.skipif(not os.path.exists(dc.REF_NLMEANS), reason="oracle/_ref/ref_nlmeans is built only where the reference's sources are")
def test_reference_harness_reproduces_the_fixture(golden, tmp_path):
    for name in dc.CASE_NAMES:
        _, _, _, F, R, k, scale, _ = dc.case(name)
        image, guide, variance, want = golden[name]
        got = dc.reference_nlmeans(image, guide, variance, F, R, k, scale, tmp_path, threads=3)
        assert dc.differing_words(got, want) == 0, name


def _distances(guide, variance, x0, y0, x1, y1, dx, dy, k, scale):
    """squaredDist (NlMeans.hpp:70-77) over [x0, x1) x [y0, y1) in float32, operation for operation."""
    f = np.float32
    vp = variance[y0:y1, x0:x1]*f(scale)
    vq = variance[y0 + dy:y1 + dy, x0 + dx:x1 + dx]*f(scale)
    diff = guide[y0:y1, x0:x1] - guide[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    d = (diff*diff - (vp + np.where(vp < vq, vp, vq)))/((vp + vq)*f(k)*f(k) + f(1e-7))
    return np.where(d < f(10000.0), d, f(10000.0)).astype(f)


def _box_slow(src, R, in_place):
    """boxFilterSlow (BoxFilter.hpp:10-37) in float32: in place -- as boxFilter calls it from nlMeansWeights, with src and result one pixmap --
    or, not in place, what the function computes between two pixmaps."""
    f = np.float32
    h, w = src.shape
    buf = src.copy()
    read = buf if in_place else src
    for y in range(h):
        for x in range(w):
            s, n = f(0.0), 0
            for yy in range(y - R, y + R + 1):
                for xx in range(x - R, x + R + 1):
                    if 0 <= xx < w and 0 <= yy < h:
                        s = f(s + read[yy, xx])
                        n += 1
            buf[y, x] = f(s/f(n))
    return buf


def _tiny_nlmeans(image, guide, variance, F, R, k, scale, in_place):
    """nlMeans of an image inside one tile whose every rectangle is narrower than 2F: one channel, float32 in the reference's order, the
    weights' exponential taken from the library through exp_of (fmath's table exponential is not restated here)."""
    f = np.float32
    h, w = image.shape
    assert w <= 32 and h <= 32 and (w < 2*F or h < 2*F)
    result, weights = np.zeros((h, w), f), np.zeros((h, w), f)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            x0, x1, y0, y1 = max(0, -dx), min(w, w - dx), max(0, -dy), min(h, h - dy)
            if x0 >= x1 or y0 >= y1:
                continue
            d = _box_slow(_distances(guide, variance, x0, y0, x1, y1, dx, dy, k, scale), F, in_place)
            wgt = _exp_neg(np.where(d > 0, d, f(0.0)).astype(f))
            if dx == 0 and dy == 0:
                wgt = np.where(wgt > f(1e-4), wgt, f(1e-4)).astype(f)
            result[y0:y1, x0:x1] += wgt*image[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            weights[y0:y1, x0:x1] += wgt
    return result/weights


def _exp_neg(d):
    """fmath's exp(-d), evaluated by the library: a one-pixel image filtered with F = R = 0 has the weight max(exp(-max(dist, 0)), 1e-4) and the
    result image*weight/weight; here the exponential is needed itself, so it is restated from the table the library's headers ship."""
    f = np.float32
    table = _exp_table()
    x = (-d).astype(f)
    big = (x.view(np.uint32) & 0x7fffffff) > 0x42b00000
    x = np.where(big, np.minimum(np.maximum(x, f(-88.0)), f(88.0)), x).astype(f)
    a, b = f(1024.0)/f(0.693147182464599609375), f(0.693147182464599609375)/f(1024.0)
    r = np.rint((x*a).astype(f)).astype(np.int32)
    t = ((x - r.astype(f)*b).astype(f) + f(1.0)).astype(f)
    bits = (((r + (127 << 10)).astype(np.uint32) >> 10) << 23) | table[r & 1023]
    return (t*bits.astype(np.uint32).view(f)).astype(f)


def _exp_table():
    import re
    text = open(os.path.join(dc.ROOT, "tungsten_amd", "csrc", "hip", "fmath_exp_table.h")).read()
    vals = [int(v, 16) for v in re.findall(r"0x([0-9a-f]{6})u", text)]
    assert len(vals) == 1024
    return np.array(vals, np.uint32)


def test_in_place_slow_filter_is_what_the_reference_does(golden):
    """The 5 x 4 case: every rectangle takes boxFilterSlow with src == result.  Spelt out in numpy, the in-place filter gives the golden bits; the
    same filter between two pixmaps does not -- the case exercises the quirk."""
    _, _, _, F, R, k, scale, _ = dc.case("tiny_5x4_rgb")
    image, guide, variance, want = golden["tiny_5x4_rgb"]
    different = 0
    for c in range(3):
        args = (image[..., c], guide[..., c], variance[..., c], F, R, k, scale)
        assert dc.differing_words(_tiny_nlmeans(*args, in_place=True), want[..., c]) == 0
        different += dc.differing_words(_tiny_nlmeans(*args, in_place=False), want[..., c])
    assert different > 0


def test_meaning_against_plain_numpy():
    """Independent of both restatements: away from the borders a weight is exp(-max(mean of the (2F+1)^2 patch of distances, 0)), the result the
    weighted mean over the (2R+1)^2 window -- float64, true exponential, a fresh sum per patch.  Interior pixels agree within 1e-5 relative.
    The case has a positive variance everywhere: a clamped distance of 10000 inside a float32 running sum leaves a rounding residue of 1e-3 in
    every later element of its chain (the reference's own float32 behaviour, which the goldens pin), far above what this check is about."""
    w, h, F, R, k, scale = 44, 40, 3, 2, 0.5, 1.0
    rng = np.random.RandomState(99)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    guide = (x/np.float32(w) + np.float32(0.5)*y/np.float32(h) + np.float32(0.05)*rng.standard_normal((h, w))).astype(np.float32)
    variance = (np.float32(0.002) + np.float32(0.004)*rng.random_sample((h, w))).astype(np.float32)
    image = rng.random_sample((h, w)).astype(np.float32)
    got = dc.host_nlmeans(image, guide, variance, F, R, k, scale)
    g, v, im = guide.astype(np.float64), variance.astype(np.float64)*scale, image.astype(np.float64)
    m = F + R
    num, den = np.zeros((h, w)), np.zeros((h, w))
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d = np.full((h, w), np.nan)
            ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
            yq, xq = slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)
            d[ys, xs] = np.minimum(((g[ys, xs] - g[yq, xq])**2 - (v[ys, xs] + np.minimum(v[ys, xs], v[yq, xq])))
                                   /((v[ys, xs] + v[yq, xq])*k*k + np.float64(np.float32(1e-7))), 10000.0)
            patch = sum(d[m + py:h - m + py, m + px:w - m + px] for py in range(-F, F + 1) for px in range(-F, F + 1))/(2*F + 1)**2
            wgt = np.exp(-np.maximum(patch, 0.0))
            if dx == 0 and dy == 0:
                wgt = np.maximum(wgt, 1e-4)
            num[m:h - m, m:w - m] += wgt*im[m + dy:h - m + dy, m + dx:w - m + dx]
            den[m:h - m, m:w - m] += wgt
    want = num[m:h - m, m:w - m]/den[m:h - m, m:w - m]
    inner = got[m:h - m, m:w - m].astype(np.float64)
    assert inner.size > 100 and np.isfinite(want).all()
    rel = np.abs(inner - want)/np.abs(want)
    print("largest relative difference on %d interior pixels: %.3g" % (inner.size, rel.max()))
    assert rel.max() <= 1e-5


def test_host_comparator_refuses_what_the_device_call_refuses():
    import tungsten_amd as tg
    a = np.ones((4, 5), np.float32)
    out = np.empty_like(a)
    ok = dict(width=5, height=4, channels=1, F=1, R=2, k=1.0, variance_scale=1.0, source=capi.TGHIP_NLMEANS_POINTERS)
    for bad in (dict(channels=0), dict(channels=5), dict(F=9), dict(R=17), dict(k=0.0), dict(k=-1.0), dict(width=0), dict(height=0), dict(source=1)):
        desc = capi.TgHipNlMeansDesc(**dict(ok, **bad))
        assert tg.lib.tgh_nlmeans_host(C.byref(desc), a.ctypes.data, a.ctypes.data, a.ctypes.data, out.ctypes.data) == -1, bad
    desc = capi.TgHipNlMeansDesc(**ok)
    assert tg.lib.tgh_nlmeans_host(C.byref(desc), a.ctypes.data, a.ctypes.data, None, out.ctypes.data) == -1
    assert tg.lib.tgh_nlmeans_host(None, a.ctypes.data, a.ctypes.data, a.ctypes.data, out.ctypes.data) == -1
    assert tg.lib.tgh_nlmeans_host(C.byref(desc), a.ctypes.data, a.ctypes.data, a.ctypes.data, out.ctypes.data) == 0
    assert dc.differing_words(out, a) == 0                 # equal pixels: every weight cancels


def test_ctypes_layout_of_the_description(tmp_path):
    fields = [n for n, _ in capi.TgHipNlMeansDesc._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "tungsten_hip.h"\nint main(void){\nprintf("size %zu\\n", sizeof(TgHipNlMeansDesc));\n'
    for n in fields:
        src += 'printf("%s %%zu\\n", offsetof(TgHipNlMeansDesc, %s));\n' % (n, n)
    src += 'printf("pointers %u\\n", TGHIP_NLMEANS_POINTERS);\nreturn 0;}\n'
    c = tmp_path/"nlm.c"
    c.write_text(src)
    exe = str(tmp_path/"nlm")
    subprocess.check_call(["gcc", "-I", os.path.join(dc.ROOT, "include"), str(c), "-o", exe])
    got = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(capi.TgHipNlMeansDesc) == 44
    for n in fields:
        assert int(got[n]) == getattr(capi.TgHipNlMeansDesc, n).offset, n
    assert int(got["pointers"]) == capi.TGHIP_NLMEANS_POINTERS
