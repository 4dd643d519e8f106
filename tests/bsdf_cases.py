"""The cases of the per-call BSDF comparisons (tests/test_bsdf_units_cpu.py, tests/test_gpu_bsdf_units.py, tools/make_bsdf_golden.py): for every
named bsdf of scenes.bsdf_corners a seeded, deterministic list of (wi, wo, uv, requested) -- crafted directions first, random fill after -- and
the sampler stream each case draws from.  Vectors are unit vectors rounded to float32, as a path produces them.

Crafted (the first CRAFTED_PERIOD cases walk through every combination, the first FIXTURE_CASES hold every single direction):
  wi         the normal and its opposite; z of +-1e-3, +-1e-5, +-1e-7 and exactly +-0, each at another azimuth (one of them along an axis);
             both hemispheres at moderate and steep angles
  wo         per kind the float32 vector and its two one-ulp neighbours in z: the exact mirror (-x, -y, z), the exact reverse -wi, the refracted
             direction for the bsdf's ior computed in float32 as DielectricBsdf::sample does, the same hemisphere at grazing, and uniform
  uv         0, 1, points exactly on checker and texel boundaries, then uniform
  requested  all lobes, all but specular, each single lobe bit, and none

The numbers a sample draws cannot be chosen: the device's Rng replays nothing, so every case draws from the counter-based stream (SEED, stream
index, 0), which the host reproduces with oracle_lib.rng_stream.  Crafted sampling numbers (xi of exactly 0 or 1 - ulp) are therefore out of scope."""
import os
import zlib

import numpy as np

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bsdf_corners.npz")
RESIDUAL = os.path.join(ROOT, "tests", "golden", "bsdf_corners_residual.json")

SEED = 0x0B5DF001
CASES_PER_BSDF = 4096
FIXTURE_CASES = 96           # the first cases of every bsdf: what the reference's answers are recorded for
NXI = 16                     # numbers of the stream handed to the replay samplers of the oracle and the reference (no bsdf draws more)
ALL_LOBES, ALL_BUT_SPECULAR = 0x7F, 0xFFFFFF4F            # bsdfs/BsdfLobes.hpp:13-33
REQUESTED = (ALL_LOBES, ALL_BUT_SPECULAR, 1, 2, 4, 8, 16, 32, 64, 128, 0)
# the result words both the reference harness and oracle_lib.bsdf_cases write per case
WORDS = ("f.x", "f.y", "f.z", "pdf", "sample_ok", "s_wo.x", "s_wo.y", "s_wo.z", "s_weight.x", "s_weight.y", "s_weight.z", "s_pdf", "s_lobe", "consumed")
SAMPLE_WORDS = slice(5, 14)  # compared only where the sample succeeded

f32 = np.float32


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v/np.linalg.norm(v)).astype(f32)


def _at_height(z, azimuth):
    """Unit vector with exactly the float32 z given (z tiny: x, y carry the length)."""
    r = np.sqrt(max(1.0 - float(z)*float(z), 0.0))
    v = np.array([r*np.cos(azimuth), r*np.sin(azimuth), 0.0]).astype(f32)
    v[2] = f32(z)
    return v


def crafted_wi():
    out = [np.array([0, 0, 1], f32), np.array([0, 0, -1], f32)]
    tiny = (1e-3, -1e-3, 1e-5, -1e-5, 1e-7, -1e-7, 0.0, -0.0)
    for k, z in enumerate(tiny):
        out.append(_at_height(f32(z), 0.0 if k == 6 else 0.4 + 0.77*k))       # (+0 along the x axis: y is exactly 0 as well)
    out += [_unit([0.3, -0.2, 0.9]), _unit([-0.5, 0.4, -0.7]), _unit([0.8, 0.55, 0.15]), _unit([-0.6, -0.75, -0.1]),
            _unit([0.05, 0.02, 0.99]), _unit([0.7, -0.7, 0.02])]
    return out                                                                  # 16 directions


def refracted(wi, ior):
    """DielectricBsdf::sample's transmitted direction in float32 (DielectricBsdf.cpp:55-78, Fresnel.hpp:75-92), rows of wi [n, 3]; the mirror
    direction under total internal reflection."""
    wi = np.asarray(wi, f32)
    one = f32(1.0)
    eta = np.where(wi[:, 2] < 0, f32(ior), one/f32(ior)).astype(f32)
    cos_i = np.abs(wi[:, 2])
    sin_t_sq = (eta*eta)*(one - cos_i*cos_i)
    assert sin_t_sq.dtype == f32
    cos_t = np.sqrt(np.maximum(one - sin_t_sq, f32(0.0)))
    out = np.stack([-wi[:, 0]*eta, -wi[:, 1]*eta, -np.copysign(cos_t, wi[:, 2])], axis=1).astype(f32)
    tir = sin_t_sq > one
    out[tir] = wi[tir]*np.array([-1, -1, 1], f32)
    return out


def _sphere(xi0, xi1):
    z = 1.0 - 2.0*xi0
    phi = 2.0*np.pi*xi1
    r = np.sqrt(np.maximum(1.0 - z*z, 0.0))
    return np.stack([r*np.cos(phi), r*np.sin(phi), z], axis=1).astype(f32)


WO_KINDS = ("mirror", "reverse", "refracted", "grazing", "uniform")
CRAFTED_PERIOD = 16*len(WO_KINDS)*3      # every (wi, wo kind, ulp step) combination: 16 and 15 are coprime


def crafted_uv(tex_w, tex_h):
    return np.array([(0.0, 0.0), (1.0, 1.0), (0.5, 0.25), (0.125, 0.875), (3.0/tex_w, 1.0/tex_h), (1.0, 0.0), (0.0, 1.0 - 2.0**-24)], f32)


def bsdf_ior(bsdf):
    return float(bsdf.get("ior", 1.5))


def make_cases(bsdf, n=CASES_PER_BSDF, texture_size=(8, 4)):
    """The first n cases of one bsdf (its scene-file dictionary): dict of wi [n, 3], wo [n, 3], uv [n, 2] float32 and requested [n] uint32.  A prefix
    of a longer list is the shorter list."""
    rng = np.random.RandomState((zlib.crc32(bsdf["name"].encode()) ^ SEED) & 0xFFFFFFFF)
    R = rng.random_sample((n, 10))        # per case: wi (2), wo (2), uv (2), three choices, the grazing azimuth -- drawn whether used or not
    W = np.stack(crafted_wi())
    U = crafted_uv(*texture_size)
    REQ = np.array(REQUESTED, np.uint32)
    k = np.arange(n)
    crafted = k < CRAFTED_PERIOD
    pick = (R[:, 6:9]*1e6).astype(np.int64)
    # wi
    wi = np.where((crafted | (R[:, 6] >= 0.8))[:, None], W[np.where(crafted, k, pick[:, 0]) % len(W)], _sphere(R[:, 0], R[:, 1])).astype(f32)
    # wo: kind and one-ulp step (crafted: k mod 15 walks through the fifteen (kind, step) pairs while k mod 16 walks through wi)
    kind = np.where(crafted, (k % 15) % 5, np.where(R[:, 7] < 0.6, 4, pick[:, 1] % 4))
    step = np.where(crafted, (k % 15)//5 - 1, 0)
    sign = np.where(np.signbit(wi[:, 2]), f32(-1), f32(1)).astype(f32)
    graze = _sphere(np.full(n, 0.5), R[:, 9])
    graze[:, 2] = f32(2e-4)*sign
    wo = np.select([(kind == 0)[:, None], (kind == 1)[:, None], (kind == 2)[:, None], (kind == 3)[:, None]],
                   [wi*np.array([-1, -1, 1], f32), -wi, refracted(wi, bsdf_ior(bsdf)), graze], _sphere(R[:, 2], R[:, 3])).astype(f32)
    wo[:, 2] = np.where(step > 0, np.nextafter(wo[:, 2], f32(np.inf)), np.where(step < 0, np.nextafter(wo[:, 2], f32(-np.inf)), wo[:, 2]))
    # uv, requested
    uv = np.where((crafted & (k % 11 < 8))[:, None], U[k % len(U)], R[:, 4:6].astype(f32)).astype(f32)
    req = np.where(crafted, np.where(k % 3 == 0, REQ[0], REQ[(k//3) % len(REQ)]), np.where(R[:, 8] < 0.6, REQ[0], REQ[pick[:, 2] % len(REQ)])).astype(np.uint32)
    return {"wi": wi, "wo": wo, "uv": uv, "requested": req}


def stream_index(bsdf_position, k):
    """The sampler stream of case k of the bsdf at `bsdf_position` in scenes.bsdf_corner_list()."""
    return bsdf_position*CASES_PER_BSDF + k


def streams(bsdf_position, n, extra=1):
    """[n, NXI + extra] float32: the first numbers of each case's stream (rngStart(SEED, stream, 0))."""
    return oracle_lib.rng_streams(SEED, stream_index(bsdf_position, 0), n, NXI + extra)


def scene_index(scene_json, name):
    """Index of the named bsdf in the scene's own list (what the reference harness is given)."""
    return [b.get("name") for b in scene_json["bsdfs"]].index(name)


def oracle_words(desc, flat_index, cases, xi):
    """[n, 14] result words of the oracle for the cases of one bsdf (flat_index: its place in the flattened table)."""
    n = cases["wi"].shape[0]
    return oracle_lib.bsdf_cases(desc, np.full(n, flat_index, np.int32), cases["requested"], cases["wi"], cases["wo"], cases["uv"], xi[:, :NXI])


def differing(got, want):
    """Per case, does any compared word differ?  got / want: [n, 14] uint32 words.  Bit patterns; a NaN matches a NaN; the words of the sample are
    compared only where both say it succeeded (and sample_ok itself always)."""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    same = got == want
    nan = np.isnan(got.view(f32)) & np.isnan(want.view(f32))
    nan[:, [4, 12, 13]] = False                       # integer words
    same |= nan
    failed = (got[:, 4] == 0) & (want[:, 4] == 0)
    same[failed, SAMPLE_WORDS] = True
    return ~same.all(axis=1)
