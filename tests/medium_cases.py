"""The cases of the per-call medium comparisons (tests/test_medium_units_cpu.py, tests/test_gpu_medium_units.py, tools/make_medium_golden.py,
tools/medium_cases_check.cpp): for every medium of scenes.medium_corners a seeded, deterministic list of cases, crafted ones first, random fill
after.  A case is a ray (origin p, unit direction d rounded to float32, max_t), MediumState::bounce before the call, a second unit direction wo for
the phase function's eval, and the two sampler streams the case draws from.  Inputs are finite float32 -- except max_t, where +inf is a legitimate
input (the segment left the scene) and occurs for every medium.

What the crafted cases are built around is read from the flattened scene (TgHipMedium), so the cases follow the medium wherever the scene file puts
its parameters.  Everything is computed in float64 and rounded once.

Crafted max_t
  every medium     +inf, 1e-6, 5e-4, 1, 1e3, 1e6
  linear, quadratic (also as an operand of `interpolated`): per channel c the max_t that puts sigma_t[c]*max_t at the transmittance's max_t ("at": the
                   float32 whose product lies closest), one float32 step either side of it ("+ulp", "-ulp"), and 9e-4 either side ("+9e-4", "-9e-4":
                   inside the 1e-3 Dirac window of `linear`; 1.1e-3 either side, "+1.1e-3" / "-1.1e-3", lies outside it)
  pulse            likewise at every cell boundary a + (b - a) i/n and every cell centre a + (b - a)(i + 1/2)/n (boundaries at tau <= 0 are left out:
                   no segment has a negative length)
  The list is ordered by priority -- the six values, "at" for every threshold and channel, the other kinds on one channel per threshold (the channel
  rotates), then the rest -- because the two pulse media have more crafted max_t than FIXTURE_CASES: their first FIXTURE_CASES hold the first three
  groups, the rest follows at once and is held to the oracle on the device, not to the reference's recording.
Crafted state_bounce   0, 1, the medium's max_bounce, max_bounce + 1
Crafted rays
  every medium     d along each axis and its negative, one of general position
  exponential      d perpendicular to the falloff direction (dx == 0 exactly where that direction is an axis), along it and against it; p 50 and 200
                   units up and down the falloff direction (expf(+-x) overflowing and underflowing); every ray meets max_t = +inf (dx < 0 among them)
  atmosphere       through the centre, tangent to the ball (h = one radius), h = 6 radii, starting inside; starting 10 and 1e3 radii away, aimed at the
                   ball and away from it (t0 of both signs); every ray meets max_t = +inf
  `h_steep`        rays through the centre starting where erf(s t0) is -1 + 2^-52 and where it is -1 exactly: the two last reachable branches of erfInv
Crafted wo         +d, -d, dot(d, wo) of +1e-7 and -1e-7, one of general position

The device's Rng replays nothing, so every case draws from its own counter-based streams -- (SEED, stream, 0) for sampleDistance, (SEED, stream, 1)
for the phase sample --, which the host reproduces with oracle_lib.rng_streams_at.  Crafted sampling numbers (xi of exactly 0, or 1 - ulp) are out of scope."""
import math
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import oracle_lib  # noqa: E402
GOLDEN = os.path.join(ROOT, "tests", "golden", "medium_corners.npz")
RESIDUAL = os.path.join(ROOT, "tests", "golden", "medium_corners_residual.json")

SEED = 0x11647002
CASES_PER_MEDIUM = 2048
FIXTURE_CASES = 128          # the first cases of every medium: what the reference's answers are recorded for
MAX_MEDIA = 64               # stream indices leave room for this many media
NXD, NXP = 4, 2              # numbers handed to the replay samplers of sampleDistance (the channel, the interpolation's boolean, two for `pulse` from a
#                              surface or `erlang` from the medium) and of the phase sample (next2D)
# the result words the oracle and the reference harness write per case; the device's TgHipMediumResult holds the first 24 the same way
WORDS = ("ok", "t", "weight.x", "weight.y", "weight.z", "exited", "bounce_after") + \
    tuple("tr_%s.%s" % (k, c) for k in ("ss", "sm", "ms", "mm") for c in "xyz") + \
    ("phase_f", "w.x", "w.y", "w.z", "phase_pdf", "consumed_dist", "consumed_phase")
INT_WORDS = [0, 5, 6, 24, 25]
DIST_WORDS = [1, 2, 3, 4, 5, 6]                 # compared where sampleDistance succeeded
(EXPONENTIAL, LINEAR, QUADRATIC, DOUBLE_EXPONENTIAL, PULSE, ERLANG, DAVIS, DAVIS_WEINSTEIN, INTERPOLATED) = range(9)      # TGHIP_TRANS_*
HOMOGENEOUS, EXP_MEDIUM, ATMOSPHERE = 0, 1, 2                                                                               # TGHIP_MEDIUM_*
ISOTROPIC, HENYEY_GREENSTEIN, RAYLEIGH = 0, 1, 2                                                                            # TGHIP_PHASE_*
BOX_LO, BOX_HI = np.array([-1.5, -0.5, -1.5]), np.array([1.5, 2.5, 1.5])     # around the Cornell box
BASE_MAX_T = (np.inf, 1e-6, 5e-4, 1.0, 1e3, 1e6)
BOUNCE_KINDS = ("zero", "one", "limit", "past")

f32 = np.float32


def _unit(v):
    v = np.asarray(v, np.float64)
    return v/np.linalg.norm(v)


def _orthonormal(n):
    n = _unit(n)
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    t = _unit(np.cross(n, a))
    return n, t, np.cross(n, t)


def medium_indices(desc):
    """The indices into desc.media of the scene's own media in scene order: the two entries behind an `interpolated` medium are its operands."""
    d = desc.contents
    out, i = [], 0
    while i < d.num_media:
        out.append(i)
        i += 3 if d.media[i].trans_type == INTERPOLATED else 1
    return out


def medium_geometry(desc, index):
    """What the crafted cases need of desc.media[index]: float64 arrays and ints."""
    m = desc.contents.media[index]
    g = {"index": int(index), "trans_type": int(m.trans_type), "medium_type": int(m.medium_type), "phase_type": int(m.phase_type), "g": float(m.phase_g),
         "max_bounce": int(m.max_bounce), "absorption_only": bool(m.absorption_only), "falloff_scale": float(m.falloff_scale)}
    for k in ("sigma_s", "sigma_t", "trans_p", "unit_point", "falloff_dir"):
        g[k] = np.array(list(getattr(m, k)), np.float64)
    leaves = [m] if m.trans_type != INTERPOLATED else [desc.contents.media[index + 1], desc.contents.media[index + 2]]
    g["leaves"] = [(int(l.trans_type), [float(x) for x in l.trans_p]) for l in leaves]
    return g


def thresholds(g):
    """[(tag, tau)] where a kernel of the medium's transmittance (or of an operand) has an edge."""
    out = []
    for ty, p in g["leaves"]:
        if ty in (LINEAR, QUADRATIC):
            out.append(("max_t", p[0]))
        if ty == PULSE:
            a, b, n = p[0], p[1], int(p[2])
            for i in range(n + 1):
                out.append(("edge%d" % i, a + (b - a)*i/n))
                if i < n:
                    out.append(("centre%d" % i, a + (b - a)*(i + 0.5)/n))
    return [(tag, tau) for tag, tau in out if tau > 0.0]


def _at(sigma, tau):
    """The float32 max_t whose float32 product with sigma lies closest to tau."""
    sigma = f32(sigma)
    t = f32(tau/float(sigma))
    cands = [t]
    for _ in range(3):
        cands = [np.nextafter(cands[0], f32(-np.inf))] + cands + [np.nextafter(cands[-1], f32(np.inf))]
    return min(cands, key=lambda c: abs(float(f32(sigma*c)) - tau))


def crafted_max_t(g):
    """[(kind, float32 max_t)] in priority order; kind: "" + the value, or "c<channel>:<threshold>:<at | +ulp | -ulp | +9e-4 | -9e-4 | +1.1e-3 | -1.1e-3>"."""
    out = [("%g" % v, f32(v)) for v in BASE_MAX_T]
    if g["medium_type"] != HOMOGENEOUS:
        return out
    th = thresholds(g)
    sig = g["sigma_t"]

    def variants(tag, tau, c):
        at = _at(sig[c], tau)
        return [("c%d:%s:+ulp" % (c, tag), np.nextafter(at, f32(np.inf))), ("c%d:%s:-ulp" % (c, tag), np.nextafter(at, f32(-np.inf))),
                ("c%d:%s:+9e-4" % (c, tag), f32((tau + 9e-4)/float(f32(sig[c])))), ("c%d:%s:-9e-4" % (c, tag), f32((tau - 9e-4)/float(f32(sig[c])))),
                ("c%d:%s:+1.1e-3" % (c, tag), f32((tau + 1.1e-3)/float(f32(sig[c])))), ("c%d:%s:-1.1e-3" % (c, tag), f32((tau - 1.1e-3)/float(f32(sig[c]))))]
    for tag, tau in th:
        for c in range(3):
            out.append(("c%d:%s:at" % (c, tag), _at(sig[c], tau)))
    for j, (tag, tau) in enumerate(th):
        out += variants(tag, tau, j % 3)[:4]
    for j, (tag, tau) in enumerate(th):
        out += variants(tag, tau, j % 3)[4:]
        for c in range(3):
            if c != j % 3:
                out += variants(tag, tau, c)
    return [(k, v) for k, v in out if v > 0]


def crafted_bounce(g):
    return [0, 1, g["max_bounce"], g["max_bounce"] + 1]


GENERAL_P = np.array([0.31, 0.87, 0.43])
GENERAL_D = _unit([0.36, -0.48, 0.8])


def _steep_start(s, want):
    """A float32 distance L at which 1 + erf(-s L), in double, is `want` (2^-52, or 0): the ray starts L before the centre and runs through it."""
    s = float(f32(s))
    L = f32(5.0/s)
    for _ in range(1 << 22):
        if 1.0 + math.erf(-s*float(L)) <= want:
            return L
        L = f32(float(L)*(1.0 + 2e-5))
    raise AssertionError("no such start")


def crafted_rays(g):
    """[(kind, float32 p, float32 d)] for one medium."""
    out = []

    def add(kind, p, d):
        out.append((kind, np.asarray(p, np.float64).astype(f32), _unit(d).astype(f32)))
    if g["medium_type"] == EXP_MEDIUM:
        u, t, b = _orthonormal(g["falloff_dir"])
        axis = np.abs(np.abs(g["falloff_dir"]).max() - 1.0) == 0.0
        across = np.roll(np.abs(g["falloff_dir"]), 1) if axis else t        # an axis across an axis: dx == 0 exactly
        add("across", GENERAL_P, across)
        add("along", GENERAL_P, u)
        add("against", GENERAL_P, -u)
        for dist in (50.0, -50.0, 200.0, -200.0):
            add("p%+g" % dist, g["unit_point"] + dist*u + 0.1*t, GENERAL_D)
            add("p%+g_across" % dist, g["unit_point"] + dist*u + 0.1*t, across)
    if g["medium_type"] == ATMOSPHERE:
        c, r = g["unit_point"], g["falloff_dir"][0]
        a, t, b = _orthonormal(GENERAL_D)
        add("through", c - 3.0*r*a, a)
        add("tangent", c + r*t - 3.0*r*a, a)
        add("h_6", c + 6.0*r*t - 2.0*r*a, a)
        add("inside", c + 0.3*r*b + 0.2*r*a, t)
        add("centre", c, b)
        for far in (10.0, 1e3):
            add("from_%g_at" % far, c - far*r*a + 0.4*r*t, a)
            add("from_%g_away" % far, c + far*r*a + 0.4*r*t, a)
        if g["falloff_scale"]*r > 6.5:
            # along the x axis: t0 = -L exactly, h = 0
            for kind, want in (("erf_-1+2^-52", 2.0**-52), ("erf_-1", 0.0)):
                L = _steep_start(g["falloff_scale"], want)
                add(kind, np.array([float(f32(c[0])) - float(L), float(f32(c[1])), float(f32(c[2]))]), [1.0, 0.0, 0.0])
    for k in range(3):
        for sgn in (1.0, -1.0):
            add("%s%s" % ("+" if sgn > 0 else "-", "xyz"[k]), GENERAL_P, sgn*np.eye(3)[k])
    add("general", GENERAL_P, GENERAL_D)
    return out


def crafted_wo(d):
    """[(kind, float32 unit vector)] for the float32 direction d."""
    n, t, b = _orthonormal(np.asarray(d, np.float64))
    side = _unit(0.8*t + 0.6*b)
    out = [("+d", np.asarray(d, f32)), ("-d", -np.asarray(d, f32))]
    for kind, z in (("dot+1e-7", 1e-7), ("dot-1e-7", -1e-7)):
        out.append((kind, (np.sqrt(1.0 - z*z)*side + z*n).astype(f32)))
    out.append(("general", _unit(0.5*n - 0.3*t + 0.7*b).astype(f32)))
    return out


def _sphere(xi0, xi1):
    z = 1.0 - 2.0*xi0
    phi = 2.0*np.pi*xi1
    r = np.sqrt(np.maximum(1.0 - z*z, 0.0))
    return np.stack([r*np.cos(phi), r*np.sin(phi), z], axis=1)


def make_cases(g, name, n=CASES_PER_MEDIUM):
    """The first n cases of one medium (g: medium_geometry; name: the medium's name, which seeds the fill): dict of p [n, 3], d [n, 3], max_t [n],
    wo [n, 3] float32, bounce [n] int32 and the kinds of the crafted values (lists of names, "" for a random one).  A prefix of a longer list is the
    shorter list."""
    rng = np.random.RandomState((zlib.crc32(name.encode()) ^ SEED) & 0xFFFFFFFF)
    R = rng.random_sample((n, 16))            # per case: p (3), d (2), wo (2), max_t (2), bounce (1), four choices, spare -- drawn whether used or not
    MT, B, RAYS = crafted_max_t(g), crafted_bounce(g), crafted_rays(g)
    nmt, nr, nw = len(MT), len(RAYS), 5
    crafted = max(FIXTURE_CASES, nmt)
    product = g["medium_type"] != HOMOGENEOUS       # every crafted ray with every crafted max_t
    assert not product or nmt*nr <= FIXTURE_CASES
    sig = float(np.mean(g["sigma_t"]))
    centre = g["unit_point"] if g["medium_type"] == ATMOSPHERE else np.array([0.0, 1.0, 0.0])
    extent = 4.0*g["falloff_dir"][0] if g["medium_type"] == ATMOSPHERE else 1.0
    box = BOX_LO + R[:, 0:3]*(BOX_HI - BOX_LO)
    if g["medium_type"] == ATMOSPHERE:
        box = centre + (R[:, 0:3]*2.0 - 1.0)*extent
    uni_d, uni_w = _sphere(R[:, 3], R[:, 4]), _sphere(R[:, 5], R[:, 6])
    pick = (R[:, 10:14]*1e6).astype(np.int64)
    p, d, wo = np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    max_t, bounce = np.zeros(n, f32), np.zeros(n, np.int32)
    tk, bk, rk, wk = [], [], [], []
    for k in range(n):
        if k < crafted:
            imt = k % nmt
            ir, iw = ((k//nmt) % nr, k % nw) if product else (k % nr, (k//nr) % nw)
            ib = (k + k//4) % 4 if product else (k + k//nmt) % 4
        else:
            imt = pick[k, 0] % nmt if R[k, 10] < 0.25 else -1
            ib = pick[k, 1] % 4 if R[k, 11] < 0.25 else -1
            ir = pick[k, 2] % nr if R[k, 12] < 0.25 else -1
            iw = pick[k, 3] % nw if R[k, 13] < 0.25 else -1
        if imt >= 0:
            kind, max_t[k] = MT[imt]
            tk.append(kind)
        else:
            tk.append("")
            max_t[k] = np.inf if R[k, 7] < 0.08 else f32(10.0**(-3.0 + 5.0*R[k, 8])/sig)       # optical depths of 1e-3 .. 1e2
        if ib >= 0:
            bounce[k] = B[ib]
            bk.append(BOUNCE_KINDS[ib])
        else:
            bounce[k] = (0, 0, 1, 2)[int(R[k, 9]*4)]
            bk.append("")
        if ir >= 0:
            kind, p[k], d[k] = RAYS[ir]
            rk.append(kind)
        else:
            rk.append("")
            p[k] = box[k].astype(f32)
            aim = centre + (uni_w[k]*0.7)*extent*0.25 - p[k].astype(np.float64)
            d[k] = (_unit(aim) if g["medium_type"] == ATMOSPHERE and R[k, 14] < 0.6 and np.linalg.norm(aim) > 0 else _unit(uni_d[k])).astype(f32)
        if iw >= 0:
            kind, wo[k] = crafted_wo(d[k])[iw]
            wk.append(kind)
        else:
            wk.append("")
            wo[k] = _unit(uni_w[k]).astype(f32)
    assert np.isfinite(p).all() and np.isfinite(d).all() and np.isfinite(wo).all() and not np.isnan(max_t).any() and (max_t > 0).all()
    for v in (d, wo):
        assert (np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0) < 1e-6).all()
    return {"p": p, "d": d, "max_t": max_t, "wo": wo, "bounce": bounce, "t_kind": tk, "b_kind": bk, "r_kind": rk, "w_kind": wk}


CASE_KEYS = ("p", "d", "max_t", "wo", "bounce")


def stream_index(position, k=0):
    """The sampler stream of case k of the medium at `position` of scenes.medium_corner_list()."""
    return position*CASES_PER_MEDIUM + k


def streams(position, n, extra=1):
    """(xi_dist [n, NXD + extra], xi_phase [n, NXP + extra]) float32: the first numbers of each case's two streams."""
    first = stream_index(position)
    return oracle_lib.rng_streams_at(SEED, first, n, 0, NXD + extra), oracle_lib.rng_streams_at(SEED, first, n, 1, NXP + extra)


def oracle_words(desc, index, cases, xi_dist, xi_phase):
    """[n, 26] result words of the oracle for the cases of the medium desc.media[index]."""
    n = cases["p"].shape[0]
    return oracle_lib.medium_cases(desc, np.full(n, index, np.int32), cases["bounce"], cases["p"], cases["d"], cases["max_t"], cases["wo"],
                                   xi_dist[:, :NXD], xi_phase[:, :NXP])


def differing(got, want):
    """Per case, does any compared word differ?  got / want: [n, 26] uint32 words.  Bit patterns; a NaN matches a NaN, +-inf and -0 only themselves.
    ok, the four transmittances, phase_f, w, phase_pdf and the phase sample's count always; t, weight, exited, bounce_after and sampleDistance's
    count where both say the call succeeded.  What lies behind a refused call is unspecified."""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    same = got == want
    nan = np.isnan(got.view(f32)) & np.isnan(want.view(f32))
    nan[:, INT_WORDS] = False
    same |= nan
    ended = (got[:, 0] == 0) & (want[:, 0] == 0)
    same[np.ix_(ended, DIST_WORDS + [24])] = True
    return ~same.all(axis=1)


def device_words(r):
    """[n, 24] words of a tungsten_amd.MEDIUM_RESULT_DTYPE array in the order of WORDS, and the two streams' next numbers [n, 2]."""
    words = np.ascontiguousarray(r).view(np.uint32).reshape(len(r), -1)
    return words[:, :24].copy(), words[:, 24:26].copy().view(f32)


def erfinv_branch(z):
    """Which of the seven branches of Erf::erfInv a double z takes (1 .. 7), as the code decides it."""
    p = -z if z < 0 else z
    q = 1.0 - p
    if p <= 0.5:
        return 1
    if q >= 0.25:
        return 2
    x = math.sqrt(-math.log(q)) if q > 0 else math.inf
    return 3 if x < 3.0 else 4 if x < 6.0 else 5 if x < 18.0 else 6 if x < 44.0 else 7


def atmosphere_inner(g, cases, xi_dist):
    """AtmosphericMedium::inverseOpticalDepth's `inner` per case, restated in float64 from the case (t0 and h as the float32 code forms them, to
    rounding): what the census reads the erfInv branch and the inner >= 1 leg from."""
    s, r = float(f32(g["falloff_scale"])), float(f32(g["falloff_dir"][0]))
    sig = g["sigma_t"].astype(f32)
    out = np.zeros(len(xi_dist))
    for k in range(len(xi_dist)):
        pc = (cases["p"][k] - g["unit_point"].astype(f32)).astype(f32)
        dk = cases["d"][k]
        t0 = f32(f32(f32(pc[0]*dk[0]) + f32(pc[1]*dk[1])) + f32(pc[2]*dk[2]))
        h = float(np.linalg.norm((pc - dk*t0).astype(f32).astype(np.float64)))
        tau = float(f32(-np.log(f32(1.0) - xi_dist[k, 1]))/sig[int(xi_dist[k, 0]*f32(3.0))])
        with np.errstate(over="ignore"):
            out[k] = math.erf(s*float(t0)) + 2.0*float(f32(1.0)/f32(1.77245385091))*float(np.exp(s*s*(h - r)*(h + r)))*s*tau
    return out


def census(words, cases, g, xi_dist):
    """What the oracle's answers [n, 26] say the cases of one medium reach: a dict of counts."""
    words = np.asarray(words, np.uint32)
    fw = words.view(f32)
    ok, exited = words[:, 0] == 1, words[:, 5] == 1
    c = {"ends": int((~ok).sum()), "infinite_t": int((ok & np.isinf(fw[:, 1])).sum()),
         "clamped": int((ok & exited & (words[:, 1] == cases["max_t"].view(np.uint32))).sum())}
    for k, kind in enumerate(BOUNCE_KINDS):
        c["bounce_" + kind] = int(sum(1 for b in cases["b_kind"] if b == kind))
    if not g["absorption_only"]:
        channel = (xi_dist[:, 0]*f32(3.0)).astype(np.int32)
        for ch in range(3):
            c["exit_%d" % ch] = int((ok & exited & (channel == ch)).sum())
            c["scatter_%d" % ch] = int((ok & ~exited & (channel == ch)).sum())
    dirac = [ty for ty, _ in g["leaves"] if ty in (LINEAR, PULSE)]
    if dirac and g["medium_type"] == HOMOGENEOUS:
        # inside a Dirac window: max_t crafted 9e-4 from the edge of `linear`, or at / 9e-4 from a cell centre of `pulse`, on the crafted channel
        for leg, name in enumerate(("ss", "sm", "ms", "mm")):
            hits = 0
            for k, kind in enumerate(cases["t_kind"]):
                parts = kind.split(":")
                if len(parts) == 3 and (parts[1] == "max_t" or parts[1].startswith("centre")) and parts[2] in ("at", "+9e-4", "-9e-4", "+ulp", "-ulp"):
                    hits += fw[k, 7 + 3*leg + int(parts[0][1])] != 0.0
            c["dirac_" + name] = int(hits)
    if g["medium_type"] == ATMOSPHERE and not g["absorption_only"]:
        inner = atmosphere_inner(g, cases, xi_dist)
        live = cases["bounce"] <= g["max_bounce"]
        c["inner_ge_1"] = int((live & (inner >= 1.0)).sum())
        for b in range(1, 8):
            c["erfinv_%d" % b] = int(sum(1 for k in np.nonzero(live & (inner < 1.0))[0] if erfinv_branch(inner[k]) == b))
    return c


def variant_masks(renderer, capi):
    """{variant: mask} of the families whose instantiation carries FEAT_MEDIA, read from tghip_debug_bsdf_info's variant_mask."""
    FEAT_MEDIA = 1 << 23                        # csrc/hip/pt_variants.h
    out = {}
    for v in range(capi.TGHIP_BSDF_VARIANT_COUNT):
        mask = renderer.debug_bsdf_info(v)[-1]
        if mask & FEAT_MEDIA:
            out[v] = mask
    return out


def write_case_file(path, per_medium, indices):
    """The cases as tools/medium_cases_check.cpp reads them: u32 media, cases per medium, NXD, NXP; per medium i32 index into the flattened media, then
    per case i32 bounce, f32 p[3], d[3], max_t, wo[3], xi_dist[NXD], xi_phase[NXP].  per_medium: [(cases, xi_dist, xi_phase)] in scene order."""
    n = per_medium[0][0]["p"].shape[0]
    with open(path, "wb") as f:
        f.write(np.array([len(per_medium), n, NXD, NXP], np.uint32).tobytes())
        for (cases, xd, xp), index in zip(per_medium, indices):
            f.write(np.array([index], np.int32).tobytes())
            rec = np.concatenate([cases["bounce"].view(f32)[:, None], cases["p"], cases["d"], cases["max_t"][:, None], cases["wo"], xd[:, :NXD],
                                  xp[:, :NXP]], axis=1).astype(f32)
            f.write(rec.tobytes())


def main(out_dir):
    """The scene and its case file (all CASES_PER_MEDIUM cases of every medium) for tools/medium_cases_check.cpp."""
    import scenes
    import tungsten_amd as tg
    os.makedirs(out_dir, exist_ok=True)
    flat = tg.FlattenedScene(scenes.medium_corners(out_dir))
    indices = medium_indices(flat.desc)
    per_medium = []
    for pos, (name, _) in enumerate(scenes.medium_corner_list()):
        xd, xp = streams(pos, CASES_PER_MEDIUM, extra=0)
        per_medium.append((make_cases(medium_geometry(flat.desc, indices[pos]), name), xd, xp))
    flat.close()
    write_case_file(os.path.join(out_dir, "medium_cases.bin"), per_medium, indices)
    print("%d media, %d cases each" % (len(per_medium), CASES_PER_MEDIUM))


if __name__ == "__main__":
    main(sys.argv[1])
