"""The host side of tghip_query_direct (tungsten_amd/csrc/host/DirectQuery.cpp, through tgh_query_direct_check): every refusal of a call with its
message, the accepted corner values, the layout of TgHipDirectQueryDesc and TgHipDirect -- and the census of the committed golden
(tests/golden/direct_cases.npz, the reference's own estimateDirect / volumeEstimateDirect on the cases of tests/direct_cases.py): every leg the
specification names is reached by at least 8 (ray, sample) items, every scene of the case table is there, and the golden's inputs are what the case
table generates.  No test here needs a device; tests/test_gpu_direct_query.py holds the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import direct_cases as dc
import tungsten_amd as tg
from tungsten_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, DEVICE, VOLUME = capi.TGHIP_E_INVALID, capi.TGHIP_E_UNSUPPORTED, capi.TGHIP_DEVELOP_DEVICE_POINTERS, capi.TGHIP_DIRECT_VOLUME
ALIGNED, ODD = 0x10000, 0x10004        # pointer VALUES: the check reads nothing through them
# a scene of five media -- entry 1 interpolated, its operands behind it --, three lights, the camera in medium 4
OPERAND, NUM_LIGHTS, CAMERA_MEDIUM = (0, 0, 1, 1, 0), 3, 4


def check(flags=0, seed=1, spp=(0, 1), medium=-1, bounce=1, light=-1, skip=0, rays=ALIGNED, media=None, out=ALIGNED, n=16, desc=True, scene=True,
          camera_medium=CAMERA_MEDIUM):
    """(return code, message) of tgh_query_direct_check."""
    d = capi.TgHipDirectQueryDesc(flags, seed, spp[0], spp[1], medium, bounce, light, skip)
    operand = (C.c_uint8*len(OPERAND))(*OPERAND)
    s = capi.TgHostDirectScene(len(OPERAND), operand, NUM_LIGHTS, camera_medium)
    err = C.create_string_buffer(256)
    rc = tg.lib.tgh_query_direct_check(C.byref(d) if desc else None, rays, media, out, n, C.byref(s) if scene else None, err, len(err))
    return rc, err.value.decode()


def test_what_a_call_may_look_like():
    for flags in (0, DEVICE):
        assert check(flags) == (0, "")
        assert check(flags, n=1) == (0, "") and check(flags, n=2**31 - 1) == (0, "")
        assert check(flags, rays=None, out=None, n=0) == (0, "")                      # an empty batch asks nothing of its arrays
        assert check(flags, media=ALIGNED + 4) == (0, "")
    assert check(0, rays=ODD, media=ODD + 1, out=ODD + 1) == (0, "")                  # host memory has no alignment requirement
    for medium in (capi.TGHIP_MEDIUM_OF_CAMERA, capi.TGHIP_MEDIUM_NONE, 0, 1, 4):
        assert check(medium=medium) == (0, "")
    assert check(skip=1024) == (0, "")
    assert check(light=NUM_LIGHTS - 1) == (0, "") and check(light=0) == (0, "")
    assert check(bounce=255) == (0, "") and check(bounce=0) == (0, "")
    assert check(spp=(2**32 - 2, 2**32 - 1)) == (0, "")
    assert check(spp=(0, 2), n=2**31 - 1) == (0, "")                                  # 2^32 - 2 items
    assert check(scene=False) == (0, "") and check(scene=False, medium=capi.TGHIP_MEDIUM_OF_CAMERA) == (0, "")
    # volume mode: a medium to start in, the camera's, or one per ray
    assert check(VOLUME, medium=0) == (0, "") and check(VOLUME, medium=capi.TGHIP_MEDIUM_OF_CAMERA) == (0, "")
    assert check(VOLUME, medium=capi.TGHIP_MEDIUM_NONE, media=ALIGNED) == (0, "")
    assert check(VOLUME, medium=capi.TGHIP_MEDIUM_OF_CAMERA, media=ALIGNED, camera_medium=-1) == (0, "")


@pytest.mark.parametrize("kw, message", [
    (dict(desc=False), "no description"),
    (dict(rays=None), "rays and out are needed"),
    (dict(out=None), "rays and out are needed"),
    (dict(rays=None, out=None, n=1), "rays and out are needed"),
    (dict(flags=4), "unknown flag bits"),
    (dict(flags=DEVICE | 0x80000000), "unknown flag bits"),
    (dict(n=2**31), "more than 2^31 - 1 rays"),
    (dict(n=2**40, rays=None, out=None), "more than 2^31 - 1 rays"),
    (dict(flags=DEVICE, rays=ODD), "16-byte aligned"),
    (dict(flags=DEVICE, out=ODD), "16-byte aligned"),
    (dict(flags=DEVICE, out=ALIGNED + 8), "16-byte aligned"),
    (dict(flags=DEVICE, media=ALIGNED + 2), "4-byte aligned"),
    (dict(medium=-3), "medium index outside"),
    (dict(medium=5), "medium index outside"),
    (dict(medium=0, scene=False), "medium index outside"),
    (dict(medium=2), "operand of an interpolated transmittance"),
    (dict(medium=3), "operand of an interpolated transmittance"),
    (dict(spp=(1, 1)), "spp_end must be above spp_begin"),
    (dict(spp=(5, 2)), "spp_end must be above spp_begin"),
    (dict(spp=(0, 0), n=0, rays=None, out=None), "spp_end must be above spp_begin"),
    (dict(skip=1025), "skip above 1024"),
    (dict(skip=2**32 - 1), "skip above 1024"),
    (dict(light=-2), "light outside"),
    (dict(light=NUM_LIGHTS), "light outside"),
    (dict(light=0, scene=False), "light outside"),
    (dict(bounce=256), "bounce above 255"),
    (dict(bounce=2**32 - 1, n=0, rays=None, out=None), "bounce above 255"),
    (dict(flags=VOLUME, medium=capi.TGHIP_MEDIUM_NONE), "volume mode needs a medium"),
    (dict(flags=VOLUME, medium=capi.TGHIP_MEDIUM_OF_CAMERA, camera_medium=-1), "volume mode needs a medium"),
    (dict(flags=VOLUME | DEVICE, medium=capi.TGHIP_MEDIUM_OF_CAMERA, scene=False), "volume mode needs a medium"),
])
def test_every_refusal_has_its_message(kw, message):
    rc, msg = check(**kw)
    assert rc == INVALID
    assert msg.startswith("tghip_query_direct: ") and message in msg, msg


@pytest.mark.parametrize("kw", [dict(spp=(0, 2), n=2**31), dict(spp=(0, 2**32 - 1), n=2), dict(spp=(0, 2**31), n=2), dict(spp=(7, 2**16 + 7), n=2**16)])
def test_too_many_items_are_unsupported(kw):
    if kw["n"] > 2**31 - 1:
        assert check(**kw)[0] == INVALID            # (the ray count is refused first)
        return
    rc, msg = check(**kw)
    assert rc == UNSUPPORTED and "2^32 or more" in msg, msg


def test_every_misalignment_of_device_pointers_is_refused():
    for a in range(1, 16):
        assert check(DEVICE, rays=ALIGNED + a)[0] == INVALID
        assert check(DEVICE, out=ALIGNED + a)[0] == INVALID
        assert (check(DEVICE, media=ALIGNED + a)[0] == INVALID) == (a % 4 != 0)


def test_the_message_is_optional():
    d = capi.TgHipDirectQueryDesc(4, 1, 0, 1, -1, 1, -1, 0)
    assert tg.lib.tgh_query_direct_check(C.byref(d), ALIGNED, None, ALIGNED, 1, None, None, 0) == INVALID
    assert tg.lib.tgh_query_direct_check(None, None, None, None, 0, None, None, 0) == INVALID
    err = C.create_string_buffer(8)                                                   # a short buffer gets the message's beginning
    assert tg.lib.tgh_query_direct_check(C.byref(d), ALIGNED, None, ALIGNED, 1, None, err, len(err)) == INVALID and err.value == b"tghip_q"


def test_the_structs_are_laid_out_as_the_header_says(tmp_path):
    dfields = [f[0] for f in capi.TgHipDirectQueryDesc._fields_]
    ofields = [f[0] for f in capi.TgHipDirect._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tungsten_hip.h"\nint main(void) {\n'
           'printf("size %zu\\ndesc_size %zu\\n", sizeof(TgHipDirect), sizeof(TgHipDirectQueryDesc));\n'
           + "".join('printf("d_%s %%zu\\n", offsetof(TgHipDirectQueryDesc, %s));\n' % (f, f) for f in dfields)
           + "".join('printf("o_%s %%zu\\n", offsetof(TgHipDirect, %s));\n' % (f, f) for f in ofields) + "return 0; }\n")
    c = tmp_path/"layout.c"
    c.write_text(src)
    exe = str(tmp_path/"layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(c), "-o", exe])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe]).decode().splitlines())}
    assert got["size"] == C.sizeof(capi.TgHipDirect) == dc_dtype_size() == 32
    assert got["desc_size"] == C.sizeof(capi.TgHipDirectQueryDesc) == 32
    for f in dfields:
        assert got["d_" + f] == getattr(capi.TgHipDirectQueryDesc, f).offset, f
    for f in ofields:
        assert got["o_" + f] == getattr(capi.TgHipDirect, f).offset == tg.DIRECT_DTYPE.fields[f][1], f


def dc_dtype_size():
    return tg.DIRECT_DTYPE.itemsize


def test_the_symbols_are_there():
    for name in ("tghip_query_direct", "tghip_query_direct_kernel_time", "tgh_query_direct_check"):
        assert hasattr(tg.lib, name), name
    assert hasattr(tg.Renderer, "query_direct") and hasattr(tg.Renderer, "query_direct_into")


# ---- the committed golden ----

@pytest.fixture(scope="module")
def golden():
    return dc.load_golden()


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dq_scenes")
    return {name: dc.build_scene(name, tmp) for name in dc.SCENES}


def test_the_golden_holds_what_the_case_table_generates(golden):
    groups = dc.make_groups()
    assert len(groups) == len(golden)
    for mine, theirs in zip(groups, golden):
        for key in ("scene", "leg", "spp", "seed", "medium", "media", "bounce", "light_name", "skip", "volume"):
            assert mine[key] == theirs[key], (mine["leg"], key)
        assert mine["rays"].tobytes() == theirs["rays"].tobytes(), mine["leg"]
        n, spp = len(mine["rays"]), mine["spp"][1] - mine["spp"][0]
        assert 64 <= n <= 512 and 1 <= spp <= 5
        assert theirs["rgb"].shape == (n, spp, 3) and theirs["rgb"].dtype == np.uint32
        for part in ("transmittance", "recorded", "taken", "legs", "light", "hit"):
            assert theirs[part].shape == (n, spp), part


def test_every_scene_of_the_case_table_is_in_the_golden(golden):
    assert {g["scene"] for g in golden} == set(dc.SCENES)


def test_the_census_reaches_every_leg(golden, scene_files):
    have = dc.census(golden, {name: dc.primitives_of(path) for name, path in scene_files.items()})
    short = {leg: have.get(leg, 0) for leg in dc.LEGS if have.get(leg, 0) < 8}
    assert not short, short


def test_the_golden_is_sane(golden):
    for g in golden:
        rgb = g["rgb"].view(np.float32)
        assert np.isfinite(rgb).all() and (rgb >= 0).all(), g["leg"]
        taken = g["taken"] != 0
        assert (rgb[~taken] == 0).all() and not g["recorded"][~taken].any()
        assert (taken == taken[:, :1]).all()                       # a ray hits, or starts in a medium, whatever the sample
        if g["volume"]:
            assert not g["recorded"].any()                         # the reference passes no `transmittance` there
        t = g["transmittance"].view(np.float32)[g["recorded"] != 0]
        assert ((t >= 0) & (t <= 1)).all()
    # a fixed light in a one-light scene is the same call as chooseLight
    by_leg = {g["leg"]: g for g in golden}
    assert by_leg["box"]["rgb"].tobytes() == by_leg["box_light_0"]["rgb"].tobytes()
    assert by_leg["two_lights"]["rgb"].tobytes() != by_leg["fixed_light"]["rgb"].tobytes()
