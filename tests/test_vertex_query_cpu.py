"""The host side of tghip_query_vertex (tungsten_amd/csrc/host/VertexQuery.cpp, through tgh_query_vertex_check): every refusal of a call with its
message, the accepted corner values, the layout of TgHipVertexQueryDesc and TgHipPath against ctypes and numpy -- and the facts
tests/test_gpu_vertex_query.py builds on, checked here before a device is asked: its cases are pinhole, uniform-sampler goldens on which the oracle is
the reference, and the oracle's log of the numbers a path draws counts the booleans.  No test here needs a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import scenes
import tungsten_amd as tg
import vertex_cases as vc
from tungsten_amd import capi
from test_oracle_golden import _oracle_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, DEVICE, START = capi.TGHIP_E_INVALID, capi.TGHIP_DEVELOP_DEVICE_POINTERS, capi.TGHIP_VERTEX_START
ALIGNED, ODD = 0x10000, 0x10004        # pointer VALUES: the check reads nothing through them
OPERAND = (0, 0, 1, 1, 0)              # a scene of five media -- entry 1 interpolated, its operands behind it


def check(flags=START, seed=1, sample=0, first_index=0, first_number=2, medium=-1, turns=1, reserved=0, rays=ALIGNED, media=None, paths=ALIGNED,
          alive=None, n=16, desc=True, scene=True):
    """(return code, message) of tgh_query_vertex_check."""
    d = capi.TgHipVertexQueryDesc(flags, seed, sample, first_index, first_number, medium, turns, reserved)
    operand = (C.c_uint8*len(OPERAND))(*OPERAND)
    s = capi.TgHostVertexScene(len(OPERAND), operand)
    err = C.create_string_buffer(256)
    rc = tg.lib.tgh_query_vertex_check(C.byref(d) if desc else None, rays, media, paths, alive, n, C.byref(s) if scene else None, err, len(err))
    return rc, err.value.decode()


def test_what_a_call_may_look_like():
    for dev in (0, DEVICE):
        assert check(START | dev) == (0, "")
        assert check(START | dev, n=1) == (0, "") and check(START | dev, n=2**31 - 1) == (0, "")
        assert check(START | dev, media=ALIGNED + 4, alive=ALIGNED + 8) == (0, "")
        assert check(dev, rays=None) == (0, "") and check(dev, rays=None, alive=ALIGNED) == (0, "")     # later turns: the paths carry their rays
        assert check(START | dev, rays=None, paths=None, n=0) == (0, "")                               # an empty batch asks nothing of its arrays
        assert check(dev, rays=None, paths=None, n=0) == (0, "")
    assert check(START, rays=ODD, media=ODD + 1, paths=ODD + 1, alive=ODD + 3) == (0, "")             # host memory has no alignment requirement
    for medium in (capi.TGHIP_MEDIUM_OF_CAMERA, capi.TGHIP_MEDIUM_NONE, 0, 1, 4):
        assert check(medium=medium) == (0, "")
    assert check(first_number=1024) == (0, "") and check(first_number=0) == (0, "")
    assert check(turns=2**32 - 1) == (0, "")
    assert check(sample=2**32 - 1, first_index=2**32 - 1, seed=2**32 - 1) == (0, "")
    assert check(scene=False) == (0, "") and check(scene=False, medium=capi.TGHIP_MEDIUM_OF_CAMERA) == (0, "")


@pytest.mark.parametrize("kw, message", [
    (dict(desc=False), "no description"),
    (dict(paths=None), "paths are needed"),
    (dict(flags=0, rays=None, paths=None), "paths are needed"),
    (dict(rays=None), "TGHIP_VERTEX_START needs rays"),
    (dict(flags=0), "rays and media are TGHIP_VERTEX_START's"),
    (dict(flags=0, rays=None, media=ALIGNED), "rays and media are TGHIP_VERTEX_START's"),
    (dict(flags=DEVICE, rays=None, media=ALIGNED, n=0), "rays and media are TGHIP_VERTEX_START's"),
    (dict(flags=4), "unknown flag bits"),
    (dict(flags=START | 0x80000000), "unknown flag bits"),
    (dict(reserved=1), "reserved words must be zero"),
    (dict(turns=0), "turns must be at least 1"),
    (dict(turns=0, n=0, rays=None, paths=None), "turns must be at least 1"),
    (dict(first_number=1025), "first_number above 1024"),
    (dict(first_number=2**32 - 1), "first_number above 1024"),
    (dict(n=2**31), "more than 2^31 - 1 rays"),
    (dict(n=2**40, rays=None, paths=None), "more than 2^31 - 1 rays"),
    (dict(flags=START | DEVICE, rays=ODD), "16-byte aligned"),
    (dict(flags=START | DEVICE, paths=ODD), "16-byte aligned"),
    (dict(flags=DEVICE, rays=None, paths=ALIGNED + 8), "16-byte aligned"),
    (dict(flags=START | DEVICE, media=ALIGNED + 2), "4-byte aligned"),
    (dict(flags=START | DEVICE, alive=ALIGNED + 1), "4-byte aligned"),
    (dict(flags=DEVICE, rays=None, alive=ALIGNED + 2), "4-byte aligned"),
    (dict(medium=-3), "medium index outside"),
    (dict(medium=5), "medium index outside"),
    (dict(medium=0, scene=False), "medium index outside"),
    (dict(medium=2), "operand of an interpolated transmittance"),
    (dict(medium=3), "operand of an interpolated transmittance"),
])
def test_every_refusal_has_its_message(kw, message):
    rc, msg = check(**kw)
    assert rc == INVALID
    assert msg.startswith("tghip_query_vertex: ") and message in msg, msg


def test_every_misalignment_of_device_pointers_is_refused():
    for a in range(1, 16):
        assert check(START | DEVICE, rays=ALIGNED + a)[0] == INVALID
        assert check(START | DEVICE, paths=ALIGNED + a)[0] == INVALID
        assert (check(START | DEVICE, media=ALIGNED + a)[0] == INVALID) == (a % 4 != 0)
        assert (check(START | DEVICE, alive=ALIGNED + a)[0] == INVALID) == (a % 4 != 0)


def test_the_message_is_optional():
    d = capi.TgHipVertexQueryDesc(4, 0, 0, 0, 0, -1, 1, 0)
    assert tg.lib.tgh_query_vertex_check(C.byref(d), ALIGNED, None, ALIGNED, None, 1, None, None, 0) == INVALID
    tiny = C.create_string_buffer(4)
    assert tg.lib.tgh_query_vertex_check(C.byref(d), ALIGNED, None, ALIGNED, None, 1, None, tiny, len(tiny)) == INVALID and tiny.raw[3:] == b"\0"


def test_the_layouts():
    """sizeof(TgHipPath) = 112, a multiple of 16, and every field where include/tungsten_hip.h puts it: ctypes and PATH_DTYPE agree word for word (the
    C side pins the sizes with static_asserts in csrc/host/VertexQuery.cpp)"""
    assert C.sizeof(capi.TgHipVertexQueryDesc) == 32
    assert [f[0] for f in capi.TgHipVertexQueryDesc._fields_] == ["flags", "seed", "sample", "first_index", "first_number", "medium", "turns", "reserved"]
    assert C.sizeof(capi.TgHipPath) == 112 and C.sizeof(capi.TgHipPath) % 16 == 0 and tg.PATH_DTYPE.itemsize == 112
    want = {"o": 0, "tmin": 12, "d": 16, "tmax": 28, "throughput": 32, "emission": 44, "status": 56, "medium": 60, "medium_state_bounce": 64, "bounce": 68,
            "flags": 72, "rec": 76, "t": 80, "rng_state": 84, "key": 92, "drawn": 96, "reserved": 100}
    for name, offset in want.items():
        assert getattr(capi.TgHipPath, name).offset == offset, name
        assert tg.PATH_DTYPE.fields[name][1] == offset, name
    assert list(tg.PATH_DTYPE.names) == [f[0] for f in capi.TgHipPath._fields_]
    # the first 32 bytes are a TgHipRay
    assert C.sizeof(capi.TgHipRay) == 32
    assert [getattr(capi.TgHipPath, f[0]).offset for f in capi.TgHipRay._fields_] == [getattr(capi.TgHipRay, f[0]).offset for f in capi.TgHipRay._fields_]
    assert (capi.TGHIP_VERTEX_START, capi.TGHIP_PATH_WAS_SPECULAR) == (2, 1)
    assert (capi.TGHIP_PATH_ALIVE, capi.TGHIP_PATH_END_ESCAPED, capi.TGHIP_PATH_END_MAX_BOUNCES, capi.TGHIP_PATH_END_ABSORBED,
            capi.TGHIP_PATH_END_ZERO_THROUGHPUT, capi.TGHIP_PATH_END_ROULETTE, capi.TGHIP_PATH_END_NAN) == tuple(range(7))
    assert len(tg.PATH_END_NAMES) == 7
    header = open(os.path.join(ROOT, "include", "tungsten_hip.h")).read()
    for k, name in enumerate(("ALIVE", "END_ESCAPED", "END_MAX_BOUNCES", "END_ABSORBED", "END_ZERO_THROUGHPUT", "END_ROULETTE", "END_NAN")):
        assert "TGHIP_PATH_%s = %d" % (name, k) in header


def test_the_check_tool_runs_clean_under_the_sanitizers(tmp_path):
    """tools/vertex_query_check.cpp: tgh_query_vertex_check over generated good and malformed calls, each held to the rule restated there, built with
    -fsanitize=address,undefined as a stand-alone program and run as a subprocess on the CPU, in the environment it inherits (the sanitizers' runtimes are
    linked statically: the test puts nothing into LD_PRELOAD)."""
    exe = str(tmp_path/"vertex_query_check")
    src = [os.path.join(ROOT, p) for p in ("tools/vertex_query_check.cpp", "tungsten_amd/csrc/host/VertexQuery.cpp")]
    subprocess.check_call(["g++", "-std=c++11", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include")] + src + ["-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "vertex_query_check: " in p.stdout and " refused, " in p.stdout


# ---- what the device tests build on ----

@pytest.mark.parametrize("name", vc.CHAIN_CASES)
def test_the_chain_cases_are_pinhole_uniform_goldens_the_oracle_reproduces(name, tmp_path):
    if "materialtest" in name and not scenes.have_materialtest():
        pytest.skip("materialtest assets (assets/) not present")
    mk, kw = scenes.GOLDEN_CASES[name]
    gold = np.load(os.path.join(scenes.GOLDEN, name + "_samples.npz"))
    ref, seed = gold["samples"], int(gold["seed"])
    h, w, spp, _ = ref.shape
    assert w*h <= 2304 and np.isfinite(ref).all()
    flat = tg.FlattenedScene(mk(tmp_path, name=name + "_q.json", **kw))
    try:
        assert flat.desc.contents.camera.type == 0 and not flat.info.stratified_sampler
        assert flat.desc.contents.settings.max_bounces >= 1
    finally:
        flat.close()
    assert (_oracle_samples(mk, kw, name, tmp_path, ref, seed) == ref).all()


@pytest.mark.parametrize("name", vc.DEVICE_ONLY_CASES)
def test_the_dropped_candidates_are_goldens_the_oracle_does_not_reproduce(name, tmp_path):
    """The candidates left out of the oracle == golden cases (tests/vertex_cases.py: CHAIN_DROPPED, each with its reason): pinhole, uniform-sampler
    goldens like the others, but the oracle's samples are not the golden's.  The day the oracle learns the fibre BCSDFs this test fails, and the name
    goes back among the chain cases."""
    assert name not in vc.CHAIN_CASES and vc.CHAIN_DROPPED[name]
    mk, kw = vc.golden_case(name)
    gold = np.load(os.path.join(scenes.GOLDEN, name + "_samples.npz"))
    ref, seed = gold["samples"], int(gold["seed"])
    h, w, spp, _ = ref.shape
    assert w*h <= 2304 and np.isfinite(ref).all()
    flat = tg.FlattenedScene(mk(tmp_path, name=name + "_q.json", **kw))
    try:
        assert flat.desc.contents.camera.type == 0 and not flat.info.stratified_sampler
    finally:
        flat.close()
    ora = _oracle_samples(mk, kw, name, tmp_path, ref, seed)
    print("%s: the oracle differs from the golden in %d of %d samples" % (name, int((ora != ref).any(axis=-1).sum()), w*h*spp))
    assert (ora != ref).any()


@pytest.mark.parametrize("name", vc.STREAM_CASES)
def test_the_oracles_log_counts_every_number_booleans_included(name, tmp_path):
    """oracle_trace_sample_log returns how many numbers a path took: the logged values are the path's stream in order -- so a boolean (the transparency
    test of every surface vertex, the roulette) is logged like any other number, and the count is what TgHipPath::drawn reaches."""
    mk, kw = scenes.GOLDEN_CASES[name]
    gold = np.load(os.path.join(scenes.GOLDEN, name + "_samples.npz"))
    seed, (h, w, spp, _) = int(gold["seed"]), gold["samples"].shape
    flat = tg.FlattenedScene(mk(tmp_path, name=name + ".json", **kw))
    try:
        hits = 0
        for py in range(0, h, 5):
            for px in range(0, w, 7):
                rgb, n, log = vc.oracle_drawn(flat, seed, px, py, spp - 1, with_log=True)
                want = oracle_lib.rng_stream(seed, px + py*w, spp - 1, n)
                assert n >= 2 and (np.array(log[:n], np.float32) == np.array(want, np.float32)).all()
                assert (rgb == oracle_lib.trace_sample(flat.desc, seed, px, py, spp - 1)).all()
                hits += n >= 3            # the third number of a path that hits a surface is handleSurface's transparency boolean
        assert hits >= 4
    finally:
        flat.close()
