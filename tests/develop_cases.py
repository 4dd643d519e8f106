"""Crafted framebuffers and auxiliary buffers for the development tests (tests/test_develop_cpu.py, tests/test_gpu_develop.py), the ctypes calls
into the host's own functions (tgh_develop_host_frame / tgh_develop_host_aux) and an independent float32 numpy restatement of what they compute."""
import ctypes as C

import numpy as np

import tungsten_amd as tg
from tungsten_amd import capi

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
INT_MIN = -2**31
FIRST = (0, 3, 4, 7, 10)
CHANNELS = capi.TGHIP_AUX_CHANNEL_COUNT
PARTS = (capi.TGHIP_DEVELOP_MEAN, capi.TGHIP_DEVELOP_A, capi.TGHIP_DEVELOP_B, capi.TGHIP_DEVELOP_VARIANCE)


def _ulp_neighbours(v):
    v = F(v)
    return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]


def frame_table():
    """(sum [n, 3] float32, count [n] uint32): one pixel per crafted value (the value in a channel, plainer ones beside it)."""
    values = [F(0.0), F(-0.0), F(-0.25), F(-1e30), F(1e-45), F(1e-40), F(1.1754942e-38), F(1.17549435e-38), F(1e-20), F(0.0031308), F(0.004),
              F(0.18), F(0.5), F(1.0), F(1.5), F(255.0), F(8421504.0), F(2147483520.0), F(2147483648.0), F(1e8), F(1e10), F(3e38), INF, -INF, NAN]
    for k in (0, 1, 2, 17, 127, 128, 200, 254, 255, 256):
        values += _ulp_neighbours(F(k)/F(255.0))
    sums, counts = [], []
    for i, v in enumerate(values):
        for cnt in (1, 0) if i % 7 == 0 else (1,):                      # some of them under a zero count as well: inf and NaN times 0
            sums.append([v, F(0.25), values[(i*5 + 3) % len(values)]]); counts.append(cnt)
    for cnt in (2, 3, 7, 255, 256, 1000003, 0xFFFFFFFF):                  # the division: 1 / count rounds, the product rounds again
        for s in (F(1.0), F(cnt % 1000)*F(0.7), F(3e38), F(1e-38)):
            sums.append([s, F(cnt % 977), F(0.1)*F(cnt % 13)]); counts.append(cnt)
    return np.array(sums, F), np.array(counts, np.uint32)


def tiled(table, n):
    """The table's rows repeated up to n rows."""
    reps = (n + len(table) - 1)//len(table)
    return np.ascontiguousarray(np.concatenate([table]*reps)[:n])


def aux_table():
    """AUX_DTYPE pixels: counts 0..3 and large ones for every output, depths with +inf / NaN / negative entries, normals outside [-1, 1],
    pixels whose channel average is NaN or infinite, values beyond int32 after the multiplication by 255."""
    vals = [F(0.0), F(-0.0), F(0.3), F(1.0), F(-1.0), F(1.5), F(-2.5), F(7.25), F(1e8), F(-1e8), F(3e38), F(1e-40), INF, -INF, NAN, F(0.49999997), F(128.0)/F(255.0)]
    rng = np.random.RandomState(7)
    rows = []
    for cnt in (0, 1, 2, 3, 4, 5, 17, 65536, 0xFFFFFFFF):
        for j in range(len(vals)):
            p = np.zeros((), tg.AUX_DTYPE)
            for name in ("a", "b", "variance"):
                p[name] = [vals[(j + 3*k + len(name)) % len(vals)] if (j + k) % 3 else F(rng.uniform(-1.2, 1.2)) for k in range(11)]
            p["count"] = [cnt, (cnt + j) % 7 if cnt < 7 else cnt, cnt, max(cnt, 1) - 1 if j % 2 else cnt, cnt]
            rows.append(p)
    return np.array(rows, tg.AUX_DTYPE)


def host_frame(ssum, count, op):
    n = count.size
    hdr, ldr = np.empty((n, 3), F), np.empty((n, 3), np.uint8)
    assert tg.lib.tgh_develop_host_frame(ssum.ctypes.data, count.ctypes.data, n, op, hdr.ctypes.data, ldr.ctypes.data) == 0
    return hdr, ldr


def host_aux(aux, output, part):
    n = aux.size
    hdr, ldr = np.empty((n, CHANNELS[output]), F), np.empty((n, 3), np.uint8)
    assert tg.lib.tgh_develop_host_aux(aux.ctypes.data, n, output, part, hdr.ctypes.data, ldr.ctypes.data) == 0
    return hdr, ldr


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the numpy restatement (float32 throughout; numpy's float32 multiply / add / divide are the IEEE operations, one rounding each) ----
def to_byte(t):
    """int(t) as x86 converts -- NaN and whatever lies outside int32 become INT_MIN -- clamped to [0, 255]."""
    with np.errstate(invalid="ignore"):
        ok = (t >= F(-2147483648.0)) & (t < F(2147483648.0))
        i = np.where(ok, np.trunc(np.where(ok, t, F(0))).astype(np.int64), INT_MIN)
    return np.clip(i, 0, 255).astype(np.uint8)


def std_max(a, b):
    """std::max(a, b) = a < b ? b : a, elementwise."""
    with np.errstate(invalid="ignore"):
        return np.where(a < b, b, a).astype(F)


def numpy_mean(ssum, count):
    with np.errstate(all="ignore"):
        inv = np.where(count != 0, F(1.0)/np.maximum(count, 1).astype(F), F(0.0)).astype(F)
        return (ssum*inv[:, None]).astype(F)


def libm_powf(x, y):
    libm = C.CDLL("libm.so.6")
    libm.powf.restype, libm.powf.argtypes = C.c_float, [C.c_float, C.c_float]
    return np.array([libm.powf(float(v), float(y)) for v in x.reshape(-1)], F).reshape(x.shape)


def numpy_tonemap(c, op):
    """(tone-mapped float32 image, mask of the entries the restatement vouches for)."""
    sure = np.ones(c.shape, bool)
    with np.errstate(all="ignore"):
        if op == capi.TGHIP_TONEMAP_LINEAR:
            return c, sure
        if op == capi.TGHIP_TONEMAP_FILMIC:
            x = std_max(np.zeros_like(c), c - F(0.004))
            return ((x*(F(6.2)*x + F(0.5)))/(x*(F(6.2)*x + F(1.7)) + F(0.06))).astype(F), sure
        assert op == capi.TGHIP_TONEMAP_GAMMA
        y = F(1.0)/F(2.2)
        a, b = np.power(c, y).astype(F), libm_powf(c, y)
        return b, (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))   # only where numpy's float32 power and powf agree to the bit


def numpy_frame(ssum, count, op):
    mean = numpy_mean(ssum, count)
    with np.errstate(all="ignore"):
        t, sure = numpy_tonemap(std_max(mean, np.zeros_like(mean)), op)
        return mean, to_byte((t*F(255.0)).astype(F)), sure


def numpy_aux(aux, output, part):
    ch0, nch = FIRST[output], CHANNELS[output]
    cnt = aux["count"][:, output].astype(np.uint32)
    a, b, var = aux["a"][:, ch0:ch0 + nch], aux["b"][:, ch0:ch0 + nch], aux["variance"][:, ch0:ch0 + nch]
    with np.errstate(all="ignore"):
        cnt_a, cnt_b = ((cnt.astype(np.uint64) + 1) % 2**32//2).astype(F), (cnt//2).astype(F)
        if part == capi.TGHIP_DEVELOP_MEAN:
            img = ((a*cnt_a[:, None]).astype(F) + (b*cnt_b[:, None]).astype(F)).astype(F)/np.maximum(cnt, 1).astype(F)[:, None]
        elif part == capi.TGHIP_DEVELOP_A:
            img = a.copy()
        elif part == capi.TGHIP_DEVELOP_B:
            img = b.copy()
        else:
            den = (cnt.astype(np.uint64)*np.maximum(1, (cnt.astype(np.uint64) + 2**32 - 1) % 2**32) % 2**32).astype(F)   # uint32 arithmetic, wrap included
            img = var/den[:, None]
        img = img.astype(F)
        rescale, lo, hi = part != capi.TGHIP_DEVELOP_VARIANCE, F(0.0), F(0.0)
        if output == capi.TGHIP_AUX_DEPTH:
            winners = img[(img > 0) & (img != INF)]           # from 0.0f by std::max: only entries above zero win, NaN never
            hi = F(winners.max()) if winners.size else F(0.0)
        elif output == capi.TGHIP_AUX_NORMAL:
            lo, hi = F(-1.0), F(1.0)
        else:
            rescale = False
        f = np.repeat(img, 3, axis=1) if nch == 1 else img
        if rescale:
            f = ((f - lo).astype(F)/F(hi - lo)).astype(F)
        avg = ((f[:, 0] + f[:, 1]).astype(F) + f[:, 2]).astype(F)/F(3.0) if nch == 3 else f[:, 0]
        bad = np.isnan(avg) | np.isinf(avg)
        ldr = np.where(bad[:, None], np.uint8(255), to_byte((f*F(255.0)).astype(F)))
    return img, ldr.astype(np.uint8)
