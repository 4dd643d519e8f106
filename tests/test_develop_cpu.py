"""The host's development of a frame (tgh_develop_host_frame / tgh_develop_host_aux, csrc/host/Develop.cpp: the loops of Integrator::writeBuffers
and OutputBuffer::save / saveLdr over plain arrays) against an independent float32 numpy restatement, on crafted values; no device.  These
functions are what the device's kernels are held to bit for bit (tests/test_gpu_develop.py)."""
import ctypes as C

import numpy as np
import pytest

import develop_cases as dc
import tungsten_amd as tg
from tungsten_amd import capi


def _same_floats(a, b):
    """Equal as float32 values, a NaN equal to a NaN (its sign and payload are the machine's, not the arithmetic's)."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)]))


@pytest.mark.parametrize("op", [capi.TGHIP_TONEMAP_LINEAR, capi.TGHIP_TONEMAP_FILMIC, capi.TGHIP_TONEMAP_GAMMA])
def test_host_frame_matches_numpy(op):
    ssum, count = dc.frame_table()
    assert count.size > 60 and (count == 0).any() and np.isnan(ssum).any() and np.isinf(ssum).any()
    hdr, ldr = dc.host_frame(ssum, count, op)
    mean, want, sure = dc.numpy_frame(ssum, count, op)
    assert _same_floats(hdr, mean)
    assert sure.mean() > 0.5                              # (gamma: numpy's float32 power may differ from powf in the last bit; the check must not be hollow)
    assert (ldr[sure] == want[sure]).all(), np.argwhere(sure & (ldr != want))[:5]


def test_conversion_is_the_x86_one():
    """What a saturating conversion would turn white is black in the reference's PNG: NaN and everything beyond int32 become INT_MIN, then 0."""
    ssum = np.array([[1e8, 3e38, np.inf], [np.nan, 8421504.0, 8421505.0], [-np.inf, -1e30, 1.0], [254.9999/255, 2147483520.0/255, 0.5]], np.float32)
    count = np.ones(4, np.uint32)
    hdr, ldr = dc.host_frame(ssum, count, capi.TGHIP_TONEMAP_LINEAR)
    assert ldr[0].tolist() == [0, 0, 0]                   # 2.55e10, inf, inf: outside int32
    assert ldr[1].tolist() == [0, 255, 0]                 # NaN; 2147483520 = the largest float below 2^31: white; the next float is 2^31 itself
    assert ldr[2].tolist() == [0, 0, 255]
    assert ldr[3].tolist() == [254, 255, 127]
    assert hdr.tobytes() == ssum.tobytes()


@pytest.mark.parametrize("k", [1, 17, 128, 254])
def test_one_ulp_around_a_byte_boundary(k):
    """k/255 and its neighbours: the 8-bit value is the truncation of the float32 product with 255, not a rounding of the quotient."""
    v = np.float32(k)/np.float32(255.0)
    trio = np.array([np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(2))], np.float32)
    hdr, ldr = dc.host_frame(np.repeat(trio[:, None], 3, axis=1), np.ones(3, np.uint32), capi.TGHIP_TONEMAP_LINEAR)
    want = [int(np.float32(t)*np.float32(255.0)) for t in trio]
    assert ldr[:, 0].tolist() == want and set(want) <= {k - 1, k}


@pytest.mark.parametrize("output", range(5))
@pytest.mark.parametrize("part", dc.PARTS)
def test_host_aux_matches_numpy(output, part):
    aux = dc.aux_table()
    hdr, ldr = dc.host_aux(aux, output, part)
    img, want = dc.numpy_aux(aux, output, part)
    assert _same_floats(hdr, img)
    assert (ldr == want).all(), np.argwhere(ldr != want)[:5]
    assert (ldr == 255).all(axis=1).any() and (ldr == 0).any()     # the table reaches the bad-pixel rule and the clamp


def test_host_aux_depth_rescale_and_bad_pixels():
    aux = np.zeros(6, tg.AUX_DTYPE)
    aux["count"][:] = 1
    aux["a"][:, 3] = [np.inf, np.nan, 2.0, 8.0, -4.0, 0.0]           # depth: +inf is skipped, a NaN never wins, the maximum is 8
    hdr, ldr = dc.host_aux(aux, capi.TGHIP_AUX_DEPTH, capi.TGHIP_DEVELOP_MEAN)
    assert hdr[:, 0].tolist()[2:] == [2.0, 8.0, -4.0, 0.0]
    assert ldr.tolist() == [[255]*3, [255]*3, [63]*3, [255]*3, [0]*3, [0]*3]   # inf / 8 and NaN are bad pixels: white; 2 / 8 * 255 = 63.75
    aux["a"][:, 3] = np.inf                                           # no finite entry: the maximum stays 0, inf / 0 is a bad pixel
    assert (dc.host_aux(aux, capi.TGHIP_AUX_DEPTH, capi.TGHIP_DEVELOP_MEAN)[1] == 255).all()
    aux["a"][:, 3] = [np.inf, np.inf, 0.5, np.inf, np.inf, np.inf]   # a single finite pixel is its own maximum
    assert dc.host_aux(aux, capi.TGHIP_AUX_DEPTH, capi.TGHIP_DEVELOP_A)[1][2].tolist() == [255]*3
    # normals outside [-1, 1] clamp; the variance part is not rescaled
    aux["a"][:, 4:7] = [[-1.0, 0.0, 1.0], [-3.0, 3.0, 0.5], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    aux["variance"][:, 4:7] = 0.5
    aux["count"][:, 2] = 3
    ldr = dc.host_aux(aux, capi.TGHIP_AUX_NORMAL, capi.TGHIP_DEVELOP_A)[1]
    assert ldr[0].tolist() == [0, 127, 255] and ldr[1].tolist() == [0, 255, 191]
    assert (dc.host_aux(aux, capi.TGHIP_AUX_NORMAL, capi.TGHIP_DEVELOP_VARIANCE)[1] == int(np.float32(0.5)/np.float32(6.0)*np.float32(255.0))).all()


def test_counts_zero_to_three():
    aux = np.zeros(4, tg.AUX_DTYPE)
    aux["count"][:, 0] = [0, 1, 2, 3]
    aux["a"][:, 0], aux["b"][:, 0], aux["variance"][:, 0] = 0.75, 0.25, 0.5
    mean = dc.host_aux(aux, capi.TGHIP_AUX_COLOR, capi.TGHIP_DEVELOP_MEAN)[0][:, 0]
    assert mean.tolist() == [0.0, 0.75, 0.5, np.float32(1.75)/np.float32(3.0)]     # (a 0 + b 0)/1, a, (a + b)/2, (2 a + b)/3
    var = dc.host_aux(aux, capi.TGHIP_AUX_COLOR, capi.TGHIP_DEVELOP_VARIANCE)[0][:, 0]
    assert np.isinf(var[0]) and var[1:].tolist() == [0.5, 0.25, np.float32(0.5)/np.float32(6.0)]   # n max(1, n - 1) = 0, 1, 2, 6


def test_bad_arguments_are_errors():
    ssum, count = dc.frame_table()
    out = np.empty((count.size, 3), np.uint8)
    assert tg.lib.tgh_develop_host_frame(ssum.ctypes.data, count.ctypes.data, count.size, 5, None, out.ctypes.data) == -1
    aux = dc.aux_table()
    assert tg.lib.tgh_develop_host_aux(aux.ctypes.data, aux.size, 5, 0, None, out.ctypes.data) == -1
    assert tg.lib.tgh_develop_host_aux(aux.ctypes.data, aux.size, 0, 4, None, out.ctypes.data) == -1
    desc = capi.TgHipDevelopDesc(capi.TGHIP_DEVELOP_FRAME, capi.TGHIP_DEVELOP_MEAN, capi.TGHIP_TONEMAP_GAMMA, 0)
    assert tg.lib.tghip_develop(None, C.byref(desc), None, out.ctypes.data, count.size) == capi.TGHIP_E_INVALID
    assert tg.lib.tghip_develop(None, None, None, None, 0) == capi.TGHIP_E_INVALID
    ms = C.c_double(0.0)
    assert tg.lib.tghip_develop_kernel_time(None, C.byref(ms)) == capi.TGHIP_E_INVALID
    assert tg.lib.tgh_renderer_develop(None, C.byref(desc), None, None, 0, None, 0) == -1 and tg.lib.tgh_renderer_tonemap(None) == -1
