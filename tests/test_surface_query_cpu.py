"""The host side of tghip_query_surface (tungsten_amd/csrc/host/SurfaceQuery.cpp, through tgh_query_surface_check): every refusal of a call with its
message, the layout of TgHipSurface and TgHipSurfaceQueryDesc, the new symbols -- and, on the oracle alone, the premise of the GPU test that holds
the answers to the auxiliary output buffers: in a one-sample TGHIP_PASS_AUX pass every *eligible* pixel (tests/surface_cases.py) records depth,
normal and albedo at its camera ray's FIRST hit.  No test here needs a device; tests/test_gpu_surface_query.py holds the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scenes
import surface_cases
import tungsten_amd as tg
from tungsten_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, DEVICE = capi.TGHIP_E_INVALID, capi.TGHIP_DEVELOP_DEVICE_POINTERS
ALIGNED, ODD = 0x10000, 0x10004        # pointer VALUES: the check reads nothing through them
DEPTH, ALBEDO = capi.TGHIP_AUX_DEPTH, capi.TGHIP_AUX_ALBEDO


def check(flags=0, reserved=(0, 0, 0), rays=ALIGNED, out=ALIGNED, n=16, desc=True):
    """(return code, message) of tgh_query_surface_check."""
    d = capi.TgHipSurfaceQueryDesc(flags, (C.c_uint32*3)(*reserved))
    err = C.create_string_buffer(256)
    rc = tg.lib.tgh_query_surface_check(C.byref(d) if desc else None, rays, out, n, err, len(err))
    return rc, err.value.decode()


def test_what_a_call_may_look_like():
    for flags in (0, DEVICE):
        assert check(flags) == (0, "")
        assert check(flags, n=1) == (0, "") and check(flags, n=2**31 - 1) == (0, "")
        assert check(flags, rays=None, out=None, n=0) == (0, "")                      # an empty batch asks nothing of its arrays
    assert check(0, rays=ODD, out=ODD + 1) == (0, "")                                 # host memory has no alignment requirement


@pytest.mark.parametrize("kw, message", [
    (dict(desc=False), "no description"),
    (dict(rays=None), "rays and out are needed"),
    (dict(out=None), "rays and out are needed"),
    (dict(rays=None, out=None, n=1), "rays and out are needed"),
    (dict(flags=2), "unknown flag bits"),
    (dict(flags=DEVICE | 0x80000000), "unknown flag bits"),
    (dict(reserved=(1, 0, 0)), "reserved words must be zero"),
    (dict(reserved=(0, 7, 0)), "reserved words must be zero"),
    (dict(reserved=(0, 0, 1)), "reserved words must be zero"),
    (dict(n=2**31), "more than 2^31 - 1 rays"),
    (dict(n=2**40, rays=None, out=None), "more than 2^31 - 1 rays"),
    (dict(flags=DEVICE, rays=ODD), "16-byte aligned"),
    (dict(flags=DEVICE, out=ODD), "16-byte aligned"),
    (dict(flags=DEVICE, out=ALIGNED + 8), "16-byte aligned"),
])
def test_every_refusal_has_its_message(kw, message):
    rc, msg = check(**kw)
    assert rc == INVALID
    assert msg.startswith("tghip_query_surface: ") and message in msg, msg


def test_every_misalignment_of_device_pointers_is_refused():
    for a in range(1, 16):
        assert check(DEVICE, rays=ALIGNED + a)[0] == INVALID
        assert check(DEVICE, out=ALIGNED + a)[0] == INVALID


def test_the_message_is_optional():
    d = capi.TgHipSurfaceQueryDesc(4)
    assert tg.lib.tgh_query_surface_check(C.byref(d), ALIGNED, ALIGNED, 1, None, 0) == INVALID
    assert tg.lib.tgh_query_surface_check(None, None, None, 0, None, 0) == INVALID
    err = C.create_string_buffer(8)                                                   # a short buffer gets the message's beginning
    assert tg.lib.tgh_query_surface_check(C.byref(d), ALIGNED, ALIGNED, 1, err, len(err)) == INVALID and err.value == b"tghip_q"


def test_layout_and_symbols(tmp_path):
    fields = [f[0] for f in capi.TgHipSurface._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tungsten_host.h"\nint main(void){\n'
           'printf("size %zu\\ndesc_size %zu\\ndesc_flags %zu\\ndesc_reserved %zu\\n", sizeof(TgHipSurface), sizeof(TgHipSurfaceQueryDesc), '
           'offsetof(TgHipSurfaceQueryDesc, flags), offsetof(TgHipSurfaceQueryDesc, reserved));\n'
           + "".join('printf("%s %%zu\\n", offsetof(TgHipSurface, %s));\n' % (f, f) for f in fields) +
           'printf("hit %u\\nback %u\\nemissive %u\\ninfinite %u\\nabi %d\\n", TGHIP_SURFACE_HIT, TGHIP_SURFACE_BACK_SIDE, TGHIP_SURFACE_EMISSIVE, '
           'TGHIP_SURFACE_INFINITE, TGHIP_ABI_VERSION);\nreturn 0;}\n')
    c = tmp_path/"sq.c"
    c.write_text(src)
    exe = str(tmp_path/"sq")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    got = {k: int(v) for k, v in (l.split() for l in subprocess.check_output([exe]).decode().splitlines())}
    assert got["size"] == C.sizeof(capi.TgHipSurface) == tg.SURFACE_DTYPE.itemsize == 96
    assert got["desc_size"] == C.sizeof(capi.TgHipSurfaceQueryDesc) == 16
    assert (got["desc_flags"], got["desc_reserved"]) == (capi.TgHipSurfaceQueryDesc.flags.offset, capi.TgHipSurfaceQueryDesc.reserved.offset) == (0, 4)
    assert fields == list(tg.SURFACE_DTYPE.names)
    for f in fields:
        assert got[f] == getattr(capi.TgHipSurface, f).offset == tg.SURFACE_DTYPE.fields[f][1], f
    assert [got[f] for f in ("t", "rec", "instance", "object", "bsdf", "flags", "reserved")] == [12, 28, 44, 56, 60, 76, 92]
    assert (got["hit"], got["back"], got["emissive"], got["infinite"]) == (1, 2, 4, 8) == (
        capi.TGHIP_SURFACE_HIT, capi.TGHIP_SURFACE_BACK_SIDE, capi.TGHIP_SURFACE_EMISSIVE, capi.TGHIP_SURFACE_INFINITE)
    assert got["abi"] == 10                     # no existing struct changed
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("tghip_query_surface", "tghip_query_surface_kernel_time", "tgh_query_surface_check"):
        assert name in capi.PROTOTYPES and hasattr(lib, name), name


def test_error_paths_without_a_context():
    d = capi.TgHipSurfaceQueryDesc(0)
    ms = C.c_double(0.0)
    assert tg.lib.tghip_query_surface(None, C.byref(d), None, None, 0) == INVALID
    assert tg.lib.tghip_query_surface_kernel_time(None, C.byref(ms)) == INVALID


@pytest.mark.skipif(tg.device_count() > 0, reason="this is the no-GPU contract")
def test_no_device_means_loud_failure_not_a_cpu_fallback(tmp_path):
    p = scenes.cornell(tmp_path, resolution=(32, 18), spp=1)
    rays = np.array([[0, 1, 6.8, 1e-4, 0, 0, -1, np.inf]], np.float32)
    with pytest.raises(tg.TungstenError) as e:
        tg.Renderer(p).query_surface(rays)
    assert "no HIP device" in str(e.value)


@pytest.mark.parametrize("name", sorted(surface_cases.AUX_SCENES))
def test_an_eligible_pixel_records_its_first_hit(name, tmp_path):
    """The premise of tests/test_gpu_surface_query.py::test_the_cameras_own_rays_against_the_aux_pass, on the oracle: in a one-sample aux pass an
    eligible pixel has ONE depth sample and it is the camera ray's t, bit for bit -- so the normal and albedo recorded with it are the first hit's."""
    if name == "materialtest" and not scenes.have_materialtest():
        pytest.skip("materialtest assets (assets/) not present")
    case = surface_cases.AuxCase(name, tmp_path)
    try:
        n = case.w*case.h
        for s in (0, 1):
            rays, hits, aux, eligible = case.sample(s)
            hit = hits["rec"] >= 0
            share = eligible.sum()/float(n)
            print("%s sample %d: %d pixels, %d hits, %d eligible (%.3f)" % (name, s, n, int(hit.sum()), int(eligible.sum()), share))
            assert (aux["count"][eligible, DEPTH] == 1).all()
            assert aux["a"][eligible, 3].tobytes() == hits["t"][eligible].tobytes()
            assert share >= 0.35
            if surface_cases.AUX_SCENES[name]:
                assert (eligible == hit).all()
            if name in surface_cases.ELIGIBLE:
                assert int(eligible.sum()) == surface_cases.ELIGIBLE[name][s]
            if name in surface_cases.SKY_SCENES:
                assert (aux["count"][~hit, ALBEDO] == 1).all() and (~hit).sum() > 0
            if name == "cornell":
                assert (aux["count"][~hit, ALBEDO] == 0).all() and (~hit).sum() > 0
    finally:
        case.close()
