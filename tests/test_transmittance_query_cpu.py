"""The host side of tghip_query_transmittance (tungsten_amd/csrc/host/TransmittanceQuery.cpp, through tgh_query_transmittance_check): every refusal
of a call with its message, the layout of TgHipTransmittanceQueryDesc and TgHipTransmittance, the new symbols -- and the census of the committed
golden (tests/golden/transmittance_cases.npz, the reference's own generalizedShadowRay on the cases of tests/transmittance_cases.py): every leg the
specification names is reached by at least 16 cases.  No test here needs a device; tests/test_gpu_transmittance_query.py holds the kernels."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import scenes
import transmittance_cases as tc
import tungsten_amd as tg
from tungsten_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, DEVICE = capi.TGHIP_E_INVALID, capi.TGHIP_DEVELOP_DEVICE_POINTERS
STARTS, ENDS = capi.TGHIP_TRANSMITTANCE_STARTS_ON_SURFACE, capi.TGHIP_TRANSMITTANCE_ENDS_ON_SURFACE
ALIGNED, ODD = 0x10000, 0x10004        # pointer VALUES: the check reads nothing through them
# a scene of five media -- entry 1 interpolated, its operands behind it -- and six objects: quad, instances, sphere, infinite sphere, mesh, sun cap
OPERAND = (0, 0, 1, 1, 0)
TYPES = (capi.TGHIP_OBJ_QUAD, capi.TGHIP_OBJ_INSTANCES, capi.TGHIP_OBJ_SPHERE, capi.TGHIP_OBJ_INFINITE_SPHERE, capi.TGHIP_OBJ_MESH,
         capi.TGHIP_OBJ_INFINITE_SPHERE_CAP)


def check(flags=0, medium=-1, end_cap=-1, bounce=0, reserved=(0, 0, 0, 0), rays=ALIGNED, media=None, out=ALIGNED, n=16, desc=True, scene=True):
    """(return code, message) of tgh_query_transmittance_check."""
    d = capi.TgHipTransmittanceQueryDesc(flags, medium, end_cap, bounce, (C.c_uint32*4)(*reserved))
    operand, types = (C.c_uint8*len(OPERAND))(*OPERAND), (C.c_int32*len(TYPES))(*TYPES)
    s = capi.TgHostTransmittanceScene(len(OPERAND), operand, len(TYPES), types)
    err = C.create_string_buffer(256)
    rc = tg.lib.tgh_query_transmittance_check(C.byref(d) if desc else None, rays, media, out, n, C.byref(s) if scene else None, err, len(err))
    return rc, err.value.decode()


def test_what_a_call_may_look_like():
    for flags in (0, DEVICE, STARTS, ENDS, DEVICE | STARTS | ENDS):
        assert check(flags) == (0, "")
        assert check(flags, n=1) == (0, "") and check(flags, n=2**31 - 1) == (0, "")
        assert check(flags, rays=None, out=None, n=0) == (0, "")                      # an empty batch asks nothing of its arrays
        assert check(flags, media=ALIGNED + 4) == (0, "")
    assert check(0, rays=ODD, media=ODD + 1, out=ODD + 1) == (0, "")                  # host memory has no alignment requirement
    for medium in (capi.TGHIP_MEDIUM_OF_CAMERA, capi.TGHIP_MEDIUM_NONE, 0, 1, 4):
        assert check(medium=medium) == (0, "")
    for cap in (-1, 0, 2, 4):
        assert check(end_cap=cap) == (0, "")
    assert check(bounce=255) == (0, "")
    assert check(scene=False) == (0, "") and check(scene=False, medium=capi.TGHIP_MEDIUM_OF_CAMERA) == (0, "")


@pytest.mark.parametrize("kw, message", [
    (dict(desc=False), "no description"),
    (dict(rays=None), "rays and out are needed"),
    (dict(out=None), "rays and out are needed"),
    (dict(rays=None, out=None, n=1), "rays and out are needed"),
    (dict(flags=8), "unknown flag bits"),
    (dict(flags=DEVICE | 0x80000000), "unknown flag bits"),
    (dict(reserved=(1, 0, 0, 0)), "reserved words must be zero"),
    (dict(reserved=(0, 7, 0, 0)), "reserved words must be zero"),
    (dict(reserved=(0, 0, 1, 0)), "reserved words must be zero"),
    (dict(reserved=(0, 0, 0, 1)), "reserved words must be zero"),
    (dict(n=2**31), "more than 2^31 - 1 rays"),
    (dict(n=2**40, rays=None, out=None), "more than 2^31 - 1 rays"),
    (dict(flags=DEVICE, rays=ODD), "16-byte aligned"),
    (dict(flags=DEVICE, out=ODD), "16-byte aligned"),
    (dict(flags=DEVICE, out=ALIGNED + 8), "16-byte aligned"),
    (dict(flags=DEVICE, media=ALIGNED + 2), "4-byte aligned"),
    (dict(flags=DEVICE | ENDS, media=ALIGNED + 1), "4-byte aligned"),
    (dict(medium=-3), "medium index outside"),
    (dict(medium=5), "medium index outside"),
    (dict(medium=0, scene=False), "medium index outside"),
    (dict(medium=2), "operand of an interpolated transmittance"),
    (dict(medium=3), "operand of an interpolated transmittance"),
    (dict(end_cap=-2), "end cap outside"),
    (dict(end_cap=6), "end cap outside"),
    (dict(end_cap=0, scene=False), "end cap outside"),
    (dict(end_cap=1), "instances object"),
    (dict(end_cap=3), "infinite emitter"),
    (dict(end_cap=5), "infinite emitter"),
    (dict(bounce=256), "bounce above 255"),
    (dict(bounce=2**32 - 1, n=0, rays=None, out=None), "bounce above 255"),
])
def test_every_refusal_has_its_message(kw, message):
    rc, msg = check(**kw)
    assert rc == INVALID
    assert msg.startswith("tghip_query_transmittance: ") and message in msg, msg


def test_every_misalignment_of_device_pointers_is_refused():
    for a in range(1, 16):
        assert check(DEVICE, rays=ALIGNED + a)[0] == INVALID
        assert check(DEVICE, out=ALIGNED + a)[0] == INVALID
        assert (check(DEVICE, media=ALIGNED + a)[0] == INVALID) == (a % 4 != 0)


def test_the_message_is_optional():
    d = capi.TgHipTransmittanceQueryDesc(8, -1, -1, 0)
    assert tg.lib.tgh_query_transmittance_check(C.byref(d), ALIGNED, None, ALIGNED, 1, None, None, 0) == INVALID
    assert tg.lib.tgh_query_transmittance_check(None, None, None, None, 0, None, None, 0) == INVALID
    err = C.create_string_buffer(8)                                                   # a short buffer gets the message's beginning
    assert tg.lib.tgh_query_transmittance_check(C.byref(d), ALIGNED, None, ALIGNED, 1, None, err, len(err)) == INVALID and err.value == b"tghip_q"


def test_layout_and_symbols(tmp_path):
    dfields = [f[0] for f in capi.TgHipTransmittanceQueryDesc._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tungsten_host.h"\nint main(void){\n'
           'printf("size %zu\\ndesc_size %zu\\nrgb %zu\\ncrossed %zu\\n", sizeof(TgHipTransmittance), sizeof(TgHipTransmittanceQueryDesc), '
           'offsetof(TgHipTransmittance, rgb), offsetof(TgHipTransmittance, crossed));\n'
           + "".join('printf("%s %%zu\\n", offsetof(TgHipTransmittanceQueryDesc, %s));\n' % (f, f) for f in dfields) +
           'printf("starts %u\\nends %u\\nnone %d\\ncamera %d\\nabi %d\\n", TGHIP_TRANSMITTANCE_STARTS_ON_SURFACE, TGHIP_TRANSMITTANCE_ENDS_ON_SURFACE, '
           'TGHIP_MEDIUM_NONE, TGHIP_MEDIUM_OF_CAMERA, TGHIP_ABI_VERSION);\nreturn 0;}\n')
    c = tmp_path/"tq.c"
    c.write_text(src)
    exe = str(tmp_path/"tq")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    got = {k: int(v) for k, v in (l.split() for l in subprocess.check_output([exe]).decode().splitlines())}
    assert got["size"] == C.sizeof(capi.TgHipTransmittance) == tg.TRANSMITTANCE_DTYPE.itemsize == 16
    assert got["desc_size"] == C.sizeof(capi.TgHipTransmittanceQueryDesc) == 32
    assert (got["rgb"], got["crossed"]) == (capi.TgHipTransmittance.rgb.offset, capi.TgHipTransmittance.crossed.offset) == (0, 12)
    assert tuple(tg.TRANSMITTANCE_DTYPE.fields[f][1] for f in ("rgb", "crossed")) == (0, 12)
    assert dfields == ["flags", "medium", "end_cap", "bounce", "reserved"]
    for f in dfields:
        assert got[f] == getattr(capi.TgHipTransmittanceQueryDesc, f).offset, f
    assert [got[f] for f in dfields] == [0, 4, 8, 12, 16]
    assert (got["starts"], got["ends"], got["none"], got["camera"]) == (2, 4, -1, -2) == (
        STARTS, ENDS, capi.TGHIP_MEDIUM_NONE, capi.TGHIP_MEDIUM_OF_CAMERA)
    assert got["abi"] == 10                     # no existing struct changed
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("tghip_query_transmittance", "tghip_query_transmittance_kernel_time", "tgh_query_transmittance_check"):
        assert name in capi.PROTOTYPES and hasattr(lib, name), name


def test_error_paths_without_a_context():
    d = capi.TgHipTransmittanceQueryDesc(0, -1, -1, 0)
    ms = C.c_double(0.0)
    assert tg.lib.tghip_query_transmittance(None, C.byref(d), None, None, None, 0) == INVALID
    assert tg.lib.tghip_query_transmittance_kernel_time(None, C.byref(ms)) == INVALID


@pytest.mark.skipif(tg.device_count() > 0, reason="this is the no-GPU contract")
def test_no_device_means_loud_failure_not_a_cpu_fallback(tmp_path):
    p = scenes.cornell(tmp_path, resolution=(32, 18), spp=1)
    rays = np.array([[0, 1, 6.8, 1e-4, 0, 0, -1, np.inf]], np.float32)
    with pytest.raises(tg.TungstenError) as e:
        tg.Renderer(p).query_transmittance(rays)
    assert "no HIP device" in str(e.value)


def test_the_committed_cases_are_the_ones_this_tree_generates():
    """The golden's rays and parameters are tests/transmittance_cases.py's: a changed generator needs a regenerated fixture."""
    golden, mine = tc.load_golden(), tc.make_groups()
    assert len(golden) == len(mine)
    for g, m in zip(golden, mine):
        for k in ("scene", "leg", "medium", "end_cap", "bounce", "starts", "ends", "media"):
            assert g[k] == m[k], (g["scene"], g["leg"], k)
        assert g["rays"].tobytes() == m["rays"].tobytes(), (g["scene"], g["leg"])
        assert g["rgb"].shape == (len(m["rays"]), 3) and g["rgb"].dtype == np.uint32
    assert sum(len(g["rays"]) for g in golden) <= 4000
    assert os.path.getsize(tc.GOLDEN) < 1 << 20


def test_census_of_the_golden():
    """Every leg of generalizedShadowRay the specification names is reached by at least 16 cases of the committed golden, with a non-trivial
    answer where the leg allows one (tests/transmittance_cases.py: census says what counts for each leg)."""
    have = tc.census(tc.load_golden())
    for leg in tc.LEGS:
        print("%-44s %5d" % (leg, have.get(leg, 0)))
    short = {leg: have.get(leg, 0) for leg in tc.LEGS if have.get(leg, 0) < 16}
    assert not short, short
    # the order of the two multiplications shows somewhere: a fractional alpha crossed inside a medium whose answer is not a power of the alpha
    fog = [g for g in tc.load_golden() if g["scene"] == "tq_fog" and g["leg"] == "medium_homogeneous"]
    assert sum(int(((g["crossed"] >= 2) & (g["rgb"].view(np.float32) > 0).all(axis=1)).sum()) for g in fog) >= 16


def test_every_scene_of_the_cases_flattens_with_the_names_where_the_cases_expect_them(tmp_path):
    """names_of: a medium's and a primitive's index in the flattened description is its place in the scene file (operands of an `interpolated`
    medium behind it) -- held here to the description's own tables for every scene of the cases."""
    for name in sorted(tc.SCENES):
        path = tc.build_scene(name, tmp_path)
        media, prims = tc.names_of(path)
        flat = tg.FlattenedScene(path)
        try:
            d = flat.desc.contents
            assert d.num_objects >= len(prims)
            assert d.num_media == (max(media.values()) + (3 if name == "tq_interpolated" else 1) if media else 0), name
            if name == "tq_interpolated":
                assert d.media[media["fog"]].trans_type == tc.TRANS_INTERPOLATED
            want = {"quad": capi.TGHIP_OBJ_QUAD, "cube": capi.TGHIP_OBJ_CUBE, "sphere": capi.TGHIP_OBJ_SPHERE, "disk": capi.TGHIP_OBJ_DISK,
                    "mesh": capi.TGHIP_OBJ_MESH, "instances": capi.TGHIP_OBJ_INSTANCES}
            with open(path) as f:
                for i, p in enumerate(json.load(f)["primitives"]):
                    assert d.objects[i].type == want[p["type"]], (name, p["name"])
        finally:
            flat.close()
