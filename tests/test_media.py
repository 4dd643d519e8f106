"""Participating media: analytic properties of the homogeneous medium that hold at any size, checked on
the oracle (CPU) and on the HIP path (gpu).  The per-sample parity with the reference is in test_oracle_golden.py /
test_gpu_parity.py (cases cornell_fog, cornell_smoke, cornell_fog_smoke_sobol); the per-CALL parity -- every sampleDistance, transmittance and
phase-function call of the oracle against the reference's recorded answers and of the device against the oracle, word for word -- in
tests/medium_cases.py, tests/test_medium_units_cpu.py and tests/test_gpu_medium_units.py."""
import numpy as np
import pytest

import oracle_lib
import scenes
import tungsten_amd as tg

SEED = tg.DEFAULT_SEED
SIGMA = [0.05, 0.11, 0.23]
EMISSION = [2.0, 3.0, 4.0]


def _panel(sigma_a, sigma_s=0.0):
    """An emissive, non-reflecting panel filling the view of the Cornell camera, which sits in a homogeneous medium."""
    def edit(scene):
        scene["primitives"] = [{"name": "panel", "type": "quad", "bsdf": {"type": "null"}, "emission": EMISSION,
                                "transform": {"position": [0, 1, 0], "scale": [60, 1, 60], "rotation": [90, 0, 0]}}]
        if sigma_a is not None:
            scene["media"] = [{"name": "haze", "type": "homogeneous", "sigma_a": sigma_a, "sigma_s": sigma_s}]
            scene["camera"]["medium"] = "haze"
    return edit


def _oracle_image(path, spp):
    flat = tg.FlattenedScene(path)
    osum, ocount = oracle_lib.render(flat.desc, flat.width, flat.height, 0, spp, SEED)
    flat.close()
    return osum/np.maximum(ocount, 1)[..., None]


def _gpu_image(path, spp):
    r = tg.Renderer(path, seed=SEED)
    r.render()
    mean = r.image()[0]
    r.close()
    return mean


def _beer_lambert(render, tmp_path, res):
    clear = render(scenes.cornell(tmp_path, name="clear.json", resolution=res, spp=1, edit=_panel(None)), 1)
    hazy = render(scenes.cornell(tmp_path, name="hazy.json", resolution=res, spp=1, edit=_panel(SIGMA)), 1)
    assert np.allclose(clear, np.array(EMISSION, np.float32)[None, None], rtol=1e-6), "the panel does not fill the view"
    # an absorption-only medium draws no random numbers (HomogeneousMedium.cpp:76-82): both renders take the same camera
    # sample, so per pixel hazy/clear = exp(-sigma_a t) with t the distance to the panel along that sample's ray
    t = -np.log(hazy/clear)/np.array(SIGMA)[None, None]
    assert np.allclose(t[..., 0], t[..., 1], rtol=2e-4) and np.allclose(t[..., 0], t[..., 2], rtol=2e-4)
    h, w = t.shape[:2]
    dist = 6.8                                            # camera (0, 1, 6.8) to the panel's plane z = 0
    assert t.min() >= dist*(1 - 1e-4)
    assert abs(t[h//2 - 1:h//2 + 1, w//2 - 1:w//2 + 1].mean() - dist) < 2e-3*dist
    assert t.max() > 1.05*dist                            # oblique rays travel farther


def _single_scatter_is_darker_and_not_black(render, tmp_path, res, spp):
    """With scattering the panel is seen through extinction sigma_a + sigma_s, and light scattered towards the camera adds
    radiance back: the image lies between the absorption-only images for sigma_a + sigma_s and for sigma_a alone."""
    sa, ss = [0.02, 0.02, 0.02], [0.08, 0.08, 0.08]
    img = render(scenes.cornell(tmp_path, name="scatter.json", resolution=res, spp=spp, edit=_panel(sa, ss)), spp)
    lo = render(scenes.cornell(tmp_path, name="lo.json", resolution=res, spp=1, edit=_panel([0.1, 0.1, 0.1])), 1)
    hi = render(scenes.cornell(tmp_path, name="hi.json", resolution=res, spp=1, edit=_panel(sa)), 1)
    m, l, h = img.mean(axis=(0, 1)), lo.mean(axis=(0, 1)), hi.mean(axis=(0, 1))
    assert (m > l*1.02).all() and (m < h*0.98).all(), (l, m, h)


def test_oracle_beer_lambert(tmp_path):
    _beer_lambert(_oracle_image, tmp_path, (48, 27))


def test_oracle_scattering_between_bounds(tmp_path):
    _single_scatter_is_darker_and_not_black(_oracle_image, tmp_path, (32, 18), 64)


@pytest.mark.gpu
def test_gpu_beer_lambert_full_size(tmp_path):
    _beer_lambert(_gpu_image, tmp_path, (1280, 720))


@pytest.mark.gpu
def test_gpu_scattering_between_bounds(tmp_path):
    _single_scatter_is_darker_and_not_black(_gpu_image, tmp_path, (320, 180), 64)


def _atmosphere_optical_depth(render, tmp_path, res):
    """media/AtmosphericMedium.cpp, absorption only (no random numbers drawn, :137-142): seen through a Gaussian ball of haze, density
    exp(-s^2 (|p - c|^2 - r^2)) with s = falloff_scale / radius, the panel's radiance is exp(-sigma_a * integral of the density along the ray) --
    the integral the medium evaluates in closed form through Abramowitz & Stegun's erfc (math/Erf.hpp:247-283; absolute error 1.5e-7) against
    scipy's quadrature of the density along the view axis."""
    from scipy import integrate
    centre, radius, falloff = np.array([0.0, 1.0, 3.0]), 1.5, 1.2

    def ball(scene):
        _panel(SIGMA)(scene)
        scene["media"][0].update(type="atmosphere", center=[float(v) for v in centre], radius=radius, falloff_scale=falloff)
    clear = render(scenes.cornell(tmp_path, name="clear.json", resolution=res, spp=1, edit=_panel(None)), 1)
    hazy = render(scenes.cornell(tmp_path, name="ball.json", resolution=res, spp=1, edit=ball), 1)
    depth = -np.log(hazy/clear)/np.array(SIGMA)[None, None]
    assert np.allclose(depth[..., 0], depth[..., 1], rtol=5e-4) and np.allclose(depth[..., 0], depth[..., 2], rtol=5e-4)   # one integral, three coefficients
    s = falloff/radius
    eye = np.array([0.0, 1.0, 6.8])                        # the Cornell camera looks down -z at the panel's plane z = 0
    want, _ = integrate.quad(lambda t: np.exp(-s*s*(((eye + t*np.array([0.0, 0.0, -1.0]) - centre)**2).sum() - radius*radius)), 0.0, 6.8)
    h, w = depth.shape[:2]
    got = depth[h//2 - 1:h//2 + 1, w//2 - 1:w//2 + 1, 0].mean()
    assert abs(got - want) < 5e-3*want, (got, want)
    # off the axis the ray passes the centre at a distance: the depth falls off like the Gaussian it is
    assert depth[h//2, 0, 0] < 0.8*got and depth[0, w//2, 0] < got


def test_oracle_atmosphere_optical_depth(tmp_path):
    _atmosphere_optical_depth(_oracle_image, tmp_path, (48, 27))


@pytest.mark.gpu
def test_gpu_atmosphere_optical_depth_full_size(tmp_path):
    _atmosphere_optical_depth(_gpu_image, tmp_path, (1280, 720))


def test_unsupported_media_are_rejected(tmp_path):
    def voxel(scene):
        scene["media"] = [{"name": "v", "type": "voxel", "sigma_a": 1, "sigma_s": 1}]
    with pytest.raises(Exception):
        tg.FlattenedScene(scenes.cornell(tmp_path, name="voxel.json", resolution=(16, 9), spp=1, edit=voxel)).close()

    def low_order(scene):
        _panel([0.1, 0.1, 0.1])(scene)
        scene["integrator"]["low_order_scattering"] = False
    with pytest.raises(Exception):
        tg.FlattenedScene(scenes.cornell(tmp_path, name="low.json", resolution=(16, 9), spp=1, edit=low_order)).close()


# ---- the transmittances on their own: identities the four kernels of any Transmittance satisfy (Transmittance.hpp:22-63) ----
import ctypes as _C
from tungsten_amd import capi as _capi

TRANSMITTANCES = {"exponential": (0, []), "linear": (1, [0.75]), "quadratic": (2, [0.75]), "double_exponential": (3, [1.0, 10.0]),
                  "pulse": (4, [0.0, 1.0, 4.0]), "erlang": (5, [3.0]), "davis": (6, [1.6]), "davis_weinstein": (7, [0.8, 1.2]), "interpolated": (8, [0.35])}


def _medium(kind):
    """The medium record of a transmittance; `interpolated`: followed by its two operands (include/tungsten_hip.h)."""
    arr = (_capi.TgHipMedium*3)()
    if kind == "interpolated":                       # 0.35 between linear (max_t 2) and erlang (rate 2)
        arr[0].trans_type = 8
        arr[0].trans_p[0] = 0.35
        arr[1].trans_type, arr[1].trans_p[0] = 1, 2.0
        arr[2].trans_type, arr[2].trans_p[0] = 5, 2.0
    else:
        arr[0].trans_type, p = TRANSMITTANCES[kind]
        for i, v in enumerate(p):
            arr[0].trans_p[i] = v
    _KEEP.append(arr)
    return arr[0]


_KEEP = []


def _kernel(m, k, taus):
    f = oracle_lib._lib.oracle_trans_kernel
    f.restype = _C.c_float
    f.argtypes = [_C.POINTER(_capi.TgHipMedium), _C.c_int, _C.c_float]
    return np.array([f(_C.byref(m), k, float(t)) for t in taus])


@pytest.mark.parametrize("kind", sorted(TRANSMITTANCES))
def test_transmittance_kernels_are_consistent(kind):
    """surfaceMedium = -d/dtau surfaceSurface (the collision density seen from a surface), sigmaBar = surfaceMedium(0), and for
    the transmittances without Dirac parts mediumMedium = -d/dtau mediumSurface; all kernels start at or below 1 and decay."""
    m = _medium(kind)
    f = oracle_lib._lib.oracle_trans_sigma_bar
    f.restype = _C.c_float
    f.argtypes = [_C.POINTER(_capi.TgHipMedium)]
    sigma_bar = f(_C.byref(m))
    taus = np.linspace(0.01, 1.4, 140)
    h = 1e-3
    if kind in ("linear", "quadratic"):
        taus = taus[np.abs(taus - 0.75) > 0.02]       # the kink at max_t
    if kind == "interpolated":
        taus = np.linspace(0.01, 1.9, 140)            # below its linear operand's max_t = 2
    ss = _kernel(m, 0, taus)
    assert abs(_kernel(m, 0, [0.0])[0] - 1.0) < 1e-6 and (np.diff(ss) <= 1e-6).all() and (ss >= -1e-6).all()
    if kind != "pulse":                              # (pulse: piecewise constant densities, compared through the samplers below)
        dss = -(_kernel(m, 0, taus + h) - _kernel(m, 0, taus - h))/(2*h)
        assert np.allclose(dss, _kernel(m, 1, taus), rtol=2e-2, atol=3e-3), kind
        assert abs(_kernel(m, 1, [1e-6])[0] - sigma_bar) < 1e-3*sigma_bar
    if kind not in ("linear", "pulse", "interpolated"):   # their mediumMedium is (or contains) a sum of Dirac deltas
        dms = -(_kernel(m, 2, taus + h) - _kernel(m, 2, taus - h))/(2*h)
        assert np.allclose(dms, _kernel(m, 3, taus), rtol=2e-2, atol=3e-3), kind


@pytest.mark.parametrize("start_on_surface", [1, 0])
@pytest.mark.parametrize("kind", sorted(TRANSMITTANCES))
def test_transmittance_samplers_follow_their_kernels(kind, start_on_surface):
    """sampleSurface draws tau with P(tau > x) = surfaceSurface(x), sampleMedium with P(tau > x) = mediumSurface(x)
    (HomogeneousMedium::sampleDistance relies on exactly that: surfaceProbability / mediumPdf)."""
    if kind == "interpolated" and start_on_surface:
        # its sampleSurface is the ratio-mixture of the operands' samplers while surfaceSurface weights the operands by their
        # sigmaBar (InterpolatedTransmittance.cpp:34-37, 65-68): not the same distribution unless the sigmaBars agree; the
        # sampling weight of HomogeneousMedium::sampleDistance accounts for the difference
        pytest.skip("the reference's interpolated sampleSurface is not distributed like its surfaceSurface")
    m = _medium(kind)
    n = 40000
    out = np.zeros(n, np.float32)
    f = oracle_lib._lib.oracle_trans_samples
    f.restype = None
    f.argtypes = [_C.POINTER(_capi.TgHipMedium), _C.c_int, _C.c_uint32, _C.c_int, _C.c_void_p]
    f(_C.byref(m), start_on_surface, 77, n, out.ctypes.data)
    xs = np.linspace(0.02, 1.3, 33)
    if kind in ("linear", "pulse") and not start_on_surface:
        xs = xs[np.abs((xs*8) % 1 - 0.5) > 0.1] if kind == "pulse" else xs[np.abs(xs - 0.75) > 0.02]   # away from the Dirac positions
    if kind == "interpolated" and not start_on_surface:
        xs = xs[np.abs(xs - 2.0) > 0.05]
    survival = np.array([(out > x).mean() for x in xs])
    expected = _kernel(m, 0 if start_on_surface else 2, xs)
    assert np.allclose(survival, expected, atol=4*np.sqrt(0.25/n) + 2e-3), (kind, start_on_surface, np.abs(survival - expected).max())


def test_fmath_exp_table_of_the_device_is_the_one_the_oracle_builds():
    """ExponentialTransmittance evaluates FastMath::exp = fmath's table-based exp (math/FastMath.hpp:14-27): the oracle builds the
    table of 2^(i/1024) with powf at load time exactly as fmath's constructor does, the device carries it as constants
    (tungsten_amd/csrc/hip/fmath_exp_table.h) -- the same 1024 words; and the restated function is a float exp to ~1 ulp."""
    import ctypes as C
    import math
    import os
    import re
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = oracle_lib._lib
    lib.oracle_fmath_exp_table.restype = C.POINTER(C.c_uint32)
    lib.oracle_fmath_exp.restype = C.c_float
    lib.oracle_fmath_exp.argtypes = [C.c_float]
    table = [int(lib.oracle_fmath_exp_table()[i]) for i in range(1024)]
    src = open(os.path.join(ROOT, "tungsten_amd", "csrc", "hip", "fmath_exp_table.h")).read()
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{6})u", src)]
    assert words == table
    for x in (-80.0, -10.0, -1.0, -1e-3, 0.0, 0.5, 3.25):   # (below -87.3 the result is a denormal the table method cannot form, in the reference too)
        assert abs(lib.oracle_fmath_exp(x)/math.exp(x) - 1.0) < 1e-5        # (fmath reduces the argument in float: ~1e-7 near 0, ~4e-6 at -80)
    assert lib.oracle_fmath_exp(-1000.0) == lib.oracle_fmath_exp(-88.0)      # clamped like the reference
