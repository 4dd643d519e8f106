"""The host side of tghip_query_rays (tungsten_amd/csrc/host/RayQuery.cpp, through tgh_query_rays_check): every refusal of a call with its message,
the layout of TgHipRayQueryDesc, the three new symbols, and -- on a machine without a GPU -- a loud failure instead of a CPU path.  No test here
needs a device; tests/test_gpu_ray_queries.py holds the kernels to the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tungsten_amd as tg
from tungsten_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = capi.TGHIP_E_INVALID
CLOSEST, OCCLUDED, DEVICE = capi.TGHIP_QUERY_CLOSEST, capi.TGHIP_QUERY_OCCLUDED, capi.TGHIP_DEVELOP_DEVICE_POINTERS
ALIGNED, ODD = 0x10000, 0x10004        # pointer VALUES: the check reads nothing through them


def check(mode=CLOSEST, flags=0, reserved=(0, 0), rays=ALIGNED, out=ALIGNED, n=16, desc=True):
    """(return code, message) of tgh_query_rays_check."""
    d = capi.TgHipRayQueryDesc(mode, flags, (C.c_uint32*2)(*reserved))
    err = C.create_string_buffer(256)
    rc = tg.lib.tgh_query_rays_check(C.byref(d) if desc else None, rays, out, n, err, len(err))
    return rc, err.value.decode()


def test_what_a_call_may_look_like():
    for mode in (CLOSEST, OCCLUDED):
        for flags in (0, DEVICE):
            assert check(mode, flags) == (0, "")
            assert check(mode, flags, n=1) == (0, "") and check(mode, flags, n=2**31 - 1) == (0, "")
            assert check(mode, flags, rays=None, out=None, n=0) == (0, "")            # an empty batch asks nothing of its arrays
    assert check(CLOSEST, 0, rays=ODD, out=ODD + 1) == (0, "")                        # host memory has no alignment requirement
    for a in range(16):                                                               # occlusion bytes on the device: any address
        assert check(OCCLUDED, DEVICE, out=ALIGNED + a) == (0, "")


@pytest.mark.parametrize("kw, message", [
    (dict(desc=False), "no description"),
    (dict(rays=None), "rays and out are needed"),
    (dict(out=None), "rays and out are needed"),
    (dict(rays=None, out=None, n=1), "rays and out are needed"),
    (dict(mode=2), "unknown mode"),
    (dict(mode=0xFFFFFFFF), "unknown mode"),
    (dict(flags=2), "unknown flag bits"),
    (dict(flags=DEVICE | 0x80000000), "unknown flag bits"),
    (dict(reserved=(1, 0)), "reserved words must be zero"),
    (dict(reserved=(0, 7)), "reserved words must be zero"),
    (dict(n=2**31), "more than 2^31 - 1 rays"),
    (dict(n=2**40, rays=None, out=None), "more than 2^31 - 1 rays"),
    (dict(flags=DEVICE, rays=ODD), "16-byte aligned"),
    (dict(flags=DEVICE, out=ODD), "16-byte aligned"),
    (dict(mode=OCCLUDED, flags=DEVICE, rays=ALIGNED + 8), "16-byte aligned"),
])
def test_every_refusal_has_its_message(kw, message):
    rc, msg = check(**kw)
    assert rc == INVALID
    assert msg.startswith("tghip_query_rays: ") and message in msg, msg


def test_every_misalignment_of_device_pointers_is_refused():
    for a in range(1, 16):
        assert check(CLOSEST, DEVICE, rays=ALIGNED + a)[0] == INVALID
        assert check(CLOSEST, DEVICE, out=ALIGNED + a)[0] == INVALID
        assert check(OCCLUDED, DEVICE, rays=ALIGNED + a)[0] == INVALID


def test_the_message_is_optional():
    d = capi.TgHipRayQueryDesc(5, 0)
    assert tg.lib.tgh_query_rays_check(C.byref(d), ALIGNED, ALIGNED, 1, None, 0) == INVALID
    assert tg.lib.tgh_query_rays_check(None, None, None, 0, None, 0) == INVALID
    err = C.create_string_buffer(8)                                                   # a short buffer gets the message's beginning
    assert tg.lib.tgh_query_rays_check(C.byref(d), ALIGNED, ALIGNED, 1, err, len(err)) == INVALID and err.value == b"tghip_q"


def test_layout_and_symbols(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tungsten_host.h"\nint main(void){\n'
           'printf("size %zu\\nmode %zu\\nflags %zu\\nreserved %zu\\n", sizeof(TgHipRayQueryDesc), offsetof(TgHipRayQueryDesc, mode), '
           'offsetof(TgHipRayQueryDesc, flags), offsetof(TgHipRayQueryDesc, reserved));\n'
           'printf("closest %d\\noccluded %d\\ndevice %u\\nabi %d\\n", (int)TGHIP_QUERY_CLOSEST, (int)TGHIP_QUERY_OCCLUDED, '
           'TGHIP_DEVELOP_DEVICE_POINTERS, TGHIP_ABI_VERSION);\nreturn 0;}\n')
    c = tmp_path/"rq.c"
    c.write_text(src)
    exe = str(tmp_path/"rq")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    got = {k: int(v) for k, v in (l.split() for l in subprocess.check_output([exe]).decode().splitlines())}
    ct = capi.TgHipRayQueryDesc
    assert got["size"] == C.sizeof(ct) == 16
    assert [f[0] for f in ct._fields_] == ["mode", "flags", "reserved"]
    assert (got["mode"], got["flags"], got["reserved"]) == (ct.mode.offset, ct.flags.offset, ct.reserved.offset) == (0, 4, 8)
    assert (got["closest"], got["occluded"], got["device"]) == (CLOSEST, OCCLUDED, DEVICE) == (0, 1, 1)
    assert got["abi"] == 10                     # no existing struct changed
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("tghip_query_rays", "tghip_query_rays_kernel_time", "tgh_query_rays_check"):
        assert name in capi.PROTOTYPES and hasattr(lib, name), name
    assert tg.QUERY_MODE_NAMES == ("closest", "occluded")


def test_error_paths_without_a_context():
    d = capi.TgHipRayQueryDesc(CLOSEST, 0)
    ms = C.c_double(0.0)
    assert tg.lib.tghip_query_rays(None, C.byref(d), None, None, 0) == INVALID
    assert tg.lib.tghip_query_rays_kernel_time(None, C.byref(ms)) == INVALID


@pytest.mark.skipif(tg.device_count() > 0, reason="this is the no-GPU contract")
def test_no_device_means_loud_failure_not_a_cpu_fallback(tmp_path):
    import scenes
    p = scenes.cornell(tmp_path, resolution=(32, 18), spp=1)
    rays = np.array([[0, 1, 6.8, 1e-4, 0, 0, -1, np.inf]], np.float32)
    with pytest.raises(tg.TungstenError) as e:
        tg.Renderer(p).query_rays(rays)
    assert "no HIP device" in str(e.value)
    with pytest.raises(tg.TungstenError):
        tg.Renderer(p).query_rays(rays, mode="occluded")
