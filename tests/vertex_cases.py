"""What tests/test_vertex_query_cpu.py and tests/test_gpu_vertex_query.py share: the cases of the chain test and the oracle's count of the numbers a
path draws."""
import ctypes as C

import numpy as np

import fibre_cases
import oracle_lib
import scenes

# "The chain is the sample": every case of test_gpu_radiance_query.CAMERA_CASES (restated: importing that module would mark nothing, but it is a GPU
# test file) and the further uniform-sampler pinhole goldens on which the oracle is the reference (tests/test_vertex_query_cpu.py checks all three facts
# for every name here, on the CPU)
CAMERA_CASES = ("cornell", "cornell_nee_off", "cornell_minb2", "cornell_box_filter", "cornell_mesh_light", "zoo_d", "cornell_instances", "cornell_fog",
                "materialtest")
FURTHER_CASES = ("cornell_bounce2", "cornell_smoke", "cornell_expfog", "cornell_atmosphere", "cornell_two_lights", "cornell_point_lights",
                 "cornell_skydome", "cornell_bump", "materialtest_transparency", "fibre_wire_mesh")
# Candidates the oracle cannot vouch for, by name, with the reason: the issue's rule drops them from the oracle == golden cases.  The device chain
# needs no oracle -- it is held to the reference's golden and to tghip_query_radiance --, so they stay as device-only cases of the GPU test.
CHAIN_DROPPED = {"fibre_wire_mesh": "a pinhole, uniform-sampler golden (tests/fibre_cases.py) of the rough_wire BCSDF, which the CPU oracle does not implement "
                                    "(it knows neither rough_wire nor lambertian_fiber): its samples are not the golden's"}
DEVICE_ONLY_CASES = tuple(CHAIN_DROPPED)
CHAIN_CASES = CAMERA_CASES + tuple(n for n in FURTHER_CASES if n not in CHAIN_DROPPED)
# the cases whose every path is held to the oracle's count of drawn numbers
STREAM_CASES = ("cornell", "cornell_fog", "zoo_d")


def golden_case(name):
    """(builder, kwargs) of a golden case: scenes.GOLDEN_CASES, or the fibre goldens' table of the same layout"""
    return scenes.GOLDEN_CASES[name] if name in scenes.GOLDEN_CASES else fibre_cases.CASES[name]


_lib = oracle_lib._lib
_lib.oracle_trace_sample_log.argtypes = [oracle_lib.DESC_P, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]
_lib.oracle_trace_sample_log.restype = C.c_int
LOG_CAP = 1 << 16


def oracle_drawn(flat, seed, px, py, s, with_log=False):
    """(rgb, how many numbers the oracle's path of pixel (px, py), sample s drew with the uniform sampler, the two filter numbers included[, the log])"""
    rgb, log = (C.c_float*3)(), (C.c_float*LOG_CAP)()
    n = _lib.oracle_trace_sample_log(flat.desc, seed, 0, 0, px, py, s, rgb, log, LOG_CAP)
    assert n < LOG_CAP                     # (the log stops counting where it is full)
    out = (np.array(rgb[:], np.float32), n)
    return out + (log,) if with_log else out
