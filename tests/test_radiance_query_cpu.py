"""The host side of tghip_query_radiance (tungsten_amd/csrc/host/RadianceQuery.cpp through tgh_query_radiance_check, the ray-paths flag of
tungsten_amd/csrc/host/LaunchChoice.cpp through tgh_launch_choice, tools/radiance_query_check.cpp under the sanitizers): every refusal of a call with
its message on both sides of its edge, the launch shape of a query's pass on every scene of the launched-kernel inventory, the layout of
TgHipRadianceQueryDesc and the new symbols, and the two facts about the oracle and the goldens that tests/test_gpu_radiance_query.py builds on.  No
test here needs a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import launch_cases
import oracle_lib
import scenes
import tungsten_amd as tg
from tungsten_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = capi.TGHIP_E_INVALID, capi.TGHIP_E_UNSUPPORTED
DEVICE, SOBOL, RAY_PATHS = capi.TGHIP_DEVELOP_DEVICE_POINTERS, capi.TGHIP_RADIANCE_SOBOL, capi.TGH_CHOICE_RAY_PATHS
ALIGNED = 0x10000                      # a pointer VALUE: the check reads nothing through it


def check(flags=0, spp=(0, 1), reserved=(0, 0, 0), rays=ALIGNED, rgb_sum=ALIGNED, count=ALIGNED, n=16, has_sobol=True, desc=True):
    """(return code, message) of tgh_query_radiance_check."""
    d = capi.TgHipRadianceQueryDesc(flags, 7, spp[0], spp[1], 11, (C.c_uint32*3)(*reserved))
    err = C.create_string_buffer(256)
    rc = tg.lib.tgh_query_radiance_check(C.byref(d) if desc else None, rays, rgb_sum, count, n, int(has_sobol), err, len(err))
    return rc, err.value.decode()


def test_what_a_call_may_look_like():
    for flags in (0, DEVICE, SOBOL, DEVICE | SOBOL):
        assert check(flags) == (0, "")
        assert check(flags, n=1) == (0, "") and check(flags, n=2**31 - 1) == (0, "")
        assert check(flags, count=None) == (0, "")                                     # the counts are optional
        assert check(flags, rays=None, rgb_sum=None, count=None, n=0) == (0, "")       # an empty batch asks nothing of its arrays
        assert check(flags, spp=(5, 6)) == (0, "") and check(flags, spp=(0, 2**32 - 1), n=1) == (0, "")
    assert check(0, has_sobol=False) == (0, "") and check(DEVICE, has_sobol=False) == (0, "")
    assert check(0, rays=ALIGNED + 4, rgb_sum=ALIGNED + 1, count=ALIGNED + 3) == (0, "")   # host memory has no alignment requirement
    assert check(DEVICE, rgb_sum=ALIGNED + 4, count=ALIGNED + 12) == (0, "")           # the outputs on the device: any word
    assert check(0, spp=(0, 2), n=2**31 - 1) == (0, "")                                # 2^32 - 2 samples: the largest call


@pytest.mark.parametrize("kw, message", [
    (dict(desc=False), "no description"),
    (dict(rays=None), "rays and rgb_sum are needed"),
    (dict(rgb_sum=None), "rays and rgb_sum are needed"),
    (dict(rays=None, rgb_sum=None, n=1), "rays and rgb_sum are needed"),
    (dict(flags=4), "unknown flag bits"),
    (dict(flags=DEVICE | SOBOL | 0x80000000), "unknown flag bits"),
    (dict(flags=RAY_PATHS), "unknown flag bits"),
    (dict(reserved=(1, 0, 0)), "reserved words must be zero"),
    (dict(reserved=(0, 1, 0)), "reserved words must be zero"),
    (dict(reserved=(0, 0, 9)), "reserved words must be zero"),
    (dict(spp=(0, 0)), "spp_end must be above spp_begin"),
    (dict(spp=(4, 4)), "spp_end must be above spp_begin"),
    (dict(spp=(5, 4)), "spp_end must be above spp_begin"),
    (dict(flags=SOBOL, has_sobol=False), "needs sobol_matrices"),
    (dict(flags=SOBOL | DEVICE, has_sobol=False), "needs sobol_matrices"),
    (dict(n=2**31), "more than 2^31 - 1 rays"),
    (dict(n=2**40, rays=None, rgb_sum=None), "more than 2^31 - 1 rays"),
    (dict(flags=DEVICE, rays=ALIGNED + 8), "rays must be 16-byte aligned"),
    (dict(flags=DEVICE, rgb_sum=ALIGNED + 2), "4-byte aligned"),
    (dict(flags=DEVICE, count=ALIGNED + 1), "4-byte aligned"),
])
def test_every_refusal_has_its_message(kw, message):
    rc, msg = check(**kw)
    assert rc == INVALID
    assert msg.startswith("tghip_query_radiance: ") and message in msg, msg


def test_every_misalignment_of_every_device_pointer_is_refused():
    for a in range(1, 16):
        assert check(DEVICE, rays=ALIGNED + a)[0] == INVALID, a
        assert check(0, rays=ALIGNED + a)[0] == 0
    for a in range(16):
        want = INVALID if a % 4 else 0
        assert check(DEVICE, rgb_sum=ALIGNED + a)[0] == want, a
        assert check(DEVICE, count=ALIGNED + a)[0] == want, a


def test_calls_of_2_to_32_samples_are_unsupported():
    """Both sides of the edge: 2^32 - 1 samples are a call, 2^32 are the refusal the pass plan makes of a record pass of that size."""
    assert check(n=1, spp=(0, 2**32 - 1)) == (0, "")
    assert check(n=2**16, spp=(0, 2**16 - 1)) == (0, "")
    for kw in (dict(n=2**16, spp=(0, 2**16)), dict(n=2**16, spp=(9, 9 + 2**16)), dict(n=2**31 - 1, spp=(0, 3)), dict(n=2, spp=(0, 2**31))):
        rc, msg = check(**kw)
        assert rc == UNSUPPORTED and msg.startswith("tghip_query_radiance: ") and "2^32 samples or more" in msg, (kw, msg)
    assert check(n=0, rays=None, rgb_sum=None, spp=(0, 2**32 - 1)) == (0, "")           # nothing times anything


def test_the_message_is_optional():
    d = capi.TgHipRadianceQueryDesc(4, 0, 0, 1)
    assert tg.lib.tgh_query_radiance_check(C.byref(d), ALIGNED, ALIGNED, ALIGNED, 1, 1, None, 0) == INVALID
    assert tg.lib.tgh_query_radiance_check(None, None, None, None, 0, 0, None, 0) == INVALID
    err = C.create_string_buffer(8)                                                    # a short buffer gets the message's beginning
    assert tg.lib.tgh_query_radiance_check(C.byref(d), ALIGNED, ALIGNED, ALIGNED, 1, 1, err, len(err)) == INVALID and err.value == b"tghip_q"


def test_layout_and_symbols(tmp_path):
    names = ["flags", "seed", "spp_begin", "spp_end", "sobol_seed", "reserved"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "tungsten_host.h"\nint main(void){\nprintf("size %zu\\n", sizeof(TgHipRadianceQueryDesc));\n'
    for n in names:
        src += 'printf("%s %%zu\\n", offsetof(TgHipRadianceQueryDesc, %s));\n' % (n, n)
    src += ('printf("sobol %u\\ndevice %u\\nchoice %u\\nabi %d\\npass_flags %u\\n", TGHIP_RADIANCE_SOBOL, TGHIP_DEVELOP_DEVICE_POINTERS, TGH_CHOICE_RAY_PATHS, '
            'TGHIP_ABI_VERSION, TGHIP_PASS_SOBOL | TGHIP_PASS_RECORDS | TGHIP_PASS_AUX | TGHIP_PASS_SAMPLES);\nreturn 0;}\n')
    c = tmp_path/"rq.c"
    c.write_text(src)
    exe = str(tmp_path/"rq")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    got = {k: int(v) for k, v in (l.split() for l in subprocess.check_output([exe]).decode().splitlines())}
    ct = capi.TgHipRadianceQueryDesc
    assert got["size"] == C.sizeof(ct) == 32
    assert [f[0] for f in ct._fields_] == names
    assert [got[n] for n in names] == [getattr(ct, n).offset for n in names] == [0, 4, 8, 12, 16, 20]
    assert (got["sobol"], got["device"], got["choice"]) == (SOBOL, DEVICE, RAY_PATHS) == (2, 1, 0x40000000)
    assert got["choice"] & got["pass_flags"] == 0 and got["choice"] not in (1 << 16, 1 << 31)   # no pass flag, and not the two bits pinned as unknown
    assert got["abi"] == 10                     # no existing struct changed
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("tghip_query_radiance", "tghip_query_radiance_kernel_time", "tgh_query_radiance_check"):
        assert name in capi.PROTOTYPES and hasattr(lib, name), name


def test_error_paths_without_a_context():
    d = capi.TgHipRadianceQueryDesc(0, 0, 0, 1)
    ms = C.c_double(0.0)
    assert tg.lib.tghip_query_radiance(None, C.byref(d), None, None, None, 0) == INVALID
    assert tg.lib.tghip_query_radiance_kernel_time(None, C.byref(ms)) == INVALID


@pytest.mark.skipif(tg.device_count() > 0, reason="this is the no-GPU contract")
def test_no_device_means_loud_failure_not_a_cpu_fallback(tmp_path):
    p = scenes.cornell(tmp_path, resolution=(32, 18), spp=1)
    rays = np.array([[0, 1, 6.8, 1e-4, 0, 0, -1, np.inf]], np.float32)
    with pytest.raises(tg.TungstenError) as e:
        tg.Renderer(p).query_radiance(rays)
    assert "no HIP device" in str(e.value)


# ---- the launch shape of a query's pass ----

@pytest.fixture(scope="module")
def descs(tmp_path_factory):
    """scene name -> FlattenedScene of every scene of tests/golden/launch_inventory.json that can be built here"""
    out = {}
    for scene in launch_cases.SCENES:
        if launch_cases.have(scene):
            out[scene] = tg.FlattenedScene(launch_cases.build(scene, tmp_path_factory.mktemp(scene)))
    yield out
    for flat in out.values():
        flat.close()


def test_a_query_pass_has_the_launch_shape_of_a_camera_fix_on_every_inventory_scene(descs):
    """With the ray-paths flag: never nextPath and the walk in one kernel (fused_flat, one_launch), never k_finish inside the walk (fold_finish), no
    k_tail; k_query_paths in front of the closest-hit launch.  The walks and the shading launches are those of the same scene's pass without the flag
    wherever that pass already had none of the four -- the flag chooses nothing else."""
    assert len(descs) >= 15
    untouched = 0
    for scene, flat in descs.items():
        for sobol in (0, 1):                                  # TGHIP_PASS_SOBOL, as TGHIP_RADIANCE_SOBOL asks for it
            for short in (0, 1):
                plain = capi.launch_choice(tg.lib, flat.desc, {}, sobol, short)
                query = capi.launch_choice(tg.lib, flat.desc, {}, sobol | RAY_PATHS, short)
                case = (scene, sobol, short)
                assert (query.fused_flat, query.one_launch, query.fold_finish, query.tail_eligible) == (0, 0, 0, 0), case
                assert query.camera_rays == 1 and query.camera_rays_name == b"k_query_paths", case
                assert query.tail == b"" and query.closest.name != b"" and query.shadow.name != b"", case
                assert b"k_finish_trace_closest_wide" not in query.closest.name, case
                assert "k_query_paths" in query.kernel_names() and "k_camera_rays" not in query.kernel_names(), case
                if plain.camera_rays:
                    assert plain.camera_rays_name == b"k_camera_rays", case
                if not (plain.fused_flat or plain.one_launch or plain.fold_finish or plain.tail_eligible):
                    untouched += 1
                    assert (query.closest.name, query.shadow.name) == (plain.closest.name, plain.shadow.name), case
                    assert [(l.name, l.cls) for l in query.shade[:query.num_shade]] == [(l.name, l.cls) for l in plain.shade[:plain.num_shade]], case
                    assert (query.parts, query.blocks_per_cu, query.slot_cap, query.walk_arrays) == (plain.parts, plain.blocks_per_cu, plain.slot_cap,
                                                                                                    plain.walk_arrays), case
    assert untouched >= 8


def test_without_the_flag_the_camera_fix_scenes_keep_their_own_launch(descs):
    c = capi.launch_choice(tg.lib, descs["cornell_cubemap_cross"].desc, {}, 0, 0)
    assert c.camera_rays == 1 and c.camera_rays_name == b"k_camera_rays"
    c = capi.launch_choice(tg.lib, descs["cornell"].desc, {}, 0, 0)
    assert c.camera_rays == 0 and c.camera_rays_name == b"" and c.fused_flat == 1


# ---- tools/radiance_query_check.cpp ----

def test_the_check_tool_runs_clean_under_the_sanitizers(tmp_path):
    """checkRadianceQuery, the virtual image and the plan for n in {0, 1, 15, 16, 17, 255, 256, 257, 997, 65 537, 2^31 - 1} and several sample ranges,
    built with -fsanitize=address,undefined as a stand-alone program and run as a subprocess on the CPU, in the environment it inherits: the test puts nothing into LD_PRELOAD, and the
    sanitizers' runtimes are linked statically, so the program asks nothing of what a machine may preload."""
    exe = str(tmp_path/"radiance_query_check")
    src = [os.path.join(ROOT, p) for p in ("tools/radiance_query_check.cpp", "tungsten_amd/csrc/host/RadianceQuery.cpp", "tungsten_amd/csrc/host/PassPlan.cpp")]
    subprocess.check_call(["g++", "-std=c++11", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"] + src + ["-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "radiance_query_check: " in p.stdout and " planned, " in p.stdout


# ---- what the device tests build on: checked here, on the CPU, before a device is asked ----

_oracle_lib = oracle_lib._lib
_oracle_lib.oracle_trace_sample_log.argtypes = [oracle_lib.DESC_P, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]
_oracle_lib.oracle_trace_sample_log.restype = C.c_int


@pytest.mark.parametrize("name", ["cornell", "cornell_box_filter", "cornell_fog"])
def test_the_rebuilt_camera_ray_is_the_ray_the_oracle_traces(name, tmp_path):
    """trace_sample(pixel, s) draws rng_stream(seed, pixel, s, 2) first -- its two numbers for the pixel filter -- and nothing before them: so
    camera_ray of those two numbers is the ray it traces, and the path's own numbers start at the stream's third."""
    mk, kw = scenes.GOLDEN_CASES[name]
    gold = np.load(os.path.join(scenes.GOLDEN, name + "_samples.npz"))
    seed, (h, w, spp, _) = int(gold["seed"]), gold["samples"].shape
    flat = tg.FlattenedScene(mk(tmp_path, name=name + ".json", **kw))
    assert flat.desc.contents.camera.type == 0                 # TGHIP_CAMERA_PINHOLE
    rgb, log = (C.c_float*3)(), (C.c_float*64)()
    for py in range(0, h, 5):
        for px in range(0, w, 7):
            for s in (0, spp - 1):
                n = _oracle_lib.oracle_trace_sample_log(flat.desc, seed, 0, 0, px, py, s, rgb, log, 64)
                want = oracle_lib.rng_stream(seed, px + py*w, s, 3)
                assert n >= 2 and log[0] == want[0] and log[1] == want[1]
                if n >= 3:
                    assert log[2] == want[2]
                assert (np.array(rgb[:], np.float32) == oracle_lib.trace_sample(flat.desc, seed, px, py, s)).all()
    flat.close()


def test_direct_hits_of_the_light_in_the_bounce1_golden_are_its_emission(tmp_path):
    """max_bounces 1: a camera ray that hits the Cornell box's light returns the light's emission and nothing else (the path ends there); the emission
    is the scene file's.  tests/test_gpu_radiance_query.py relies on that for its closed-form rays."""
    mk, kw = scenes.GOLDEN_CASES["cornell_bounce1"]
    gold = np.load(os.path.join(scenes.GOLDEN, "cornell_bounce1_samples.npz"))
    ref, seed = gold["samples"], int(gold["seed"])
    h, w, spp, _ = ref.shape
    flat = tg.FlattenedScene(mk(tmp_path, name="b1.json", **kw))
    d = flat.desc.contents
    light = [i for i in range(d.num_objects) if d.objects[i].emission >= 0]
    assert len(light) == 1
    emission = np.array(list(d.textures[d.objects[light[0]].emission].value), np.float32)
    assert (emission > 0).all()
    rays = np.zeros((h, w, spp, 8), np.float32)
    for py in range(h):
        for px in range(w):
            for k in range(spp):
                xi = oracle_lib.rng_stream(seed, px + py*w, k, 2)
                o, dr = oracle_lib.camera_ray(flat.desc, px, py, xi[0], xi[1])
                rays[py, px, k] = [o[0], o[1], o[2], 1e-4, dr[0], dr[1], dr[2], np.inf]
    hits = oracle_lib.trace_rays(flat.desc, rays.reshape(-1, 8))[0]
    on_light = np.array([r >= 0 and (d.recs[r].meta & 0x1FFFFFFF) == light[0] for r in hits["rec"]]).reshape(h, w, spp)
    flat.close()
    assert on_light.sum() >= 4
    assert (ref[on_light] == emission).all()
    assert not (ref[~on_light] == emission).all(axis=-1).any()
