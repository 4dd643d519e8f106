"""Builds the reference harness of the NL-means filter (tools/ref_nlmeans.cpp, against the reference's headers and oracle/_ref/libcore.a, with
the core flags of oracle/Makefile.ref: -O3 -march=nehalem, no FMA) into the git-ignored oracle/_ref/, and records what the reference's own
nlMeans computes for the cases of tests/denoise_cases.py into tests/golden/nlmeans.npz: inputs, parameters and results -- data only.

    python tools/make_denoise_golden.py            # build the harness, write the fixture
    python tools/make_denoise_golden.py --build    # build the harness only
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"
OUT = os.path.join(ROOT, "oracle", "_ref")


def build_harness(reference=REFERENCE):
    """g++ with oracle/Makefile.ref's CORE_FLAGS; returns the program's path."""
    src = os.path.join(reference, "src")
    exe = os.path.join(OUT, "ref_nlmeans")
    cmd = ["g++", "-std=c++11", "-O3", "-DNDEBUG", "-march=nehalem", "-fstrict-aliasing", "-fvisibility-inlines-hidden", "-w",
           "-DCONSTEXPR=constexpr", "-DEMBREE_STATIC_LIB=1", '-DINSTALL_PREFIX="/usr/local"', "-DLODEPNG_NO_COMPILE_DISK=1",
           "-DRAPIDJSON_HAS_STDSTRING=1", "-DSTBI_NO_STDIO=1",
           "-I" + os.path.join(src, "core"), "-I" + os.path.join(src, "thirdparty"), "-I" + os.path.join(src, "thirdparty", "embree", "include"),
           "-I" + src, os.path.join(ROOT, "tools", "ref_nlmeans.cpp"), "-o", exe,
           os.path.join(OUT, "libcore.a"), os.path.join(OUT, "libthirdparty.a"), os.path.join(OUT, "libembree.a"),
           os.path.join(OUT, "libembree_sse42.a"), os.path.join(OUT, "libembree.a"), "-ldl", "-lpthread"]
    subprocess.check_call(cmd, cwd=ROOT)
    return exe


def main():
    build_harness()
    if "--build" in sys.argv[1:]:
        return
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import denoise_cases as dc
    arrays = {"names": np.array(dc.CASE_NAMES), "params": np.array([c[1:] for c in dc.CASES], np.float64)}
    with tempfile.TemporaryDirectory() as tmp:
        for name, w, h, F, R, k, scale, ch in dc.CASES:
            image, guide, variance = dc.make_inputs(name)
            result = dc.reference_nlmeans(image, guide, variance, F, R, k, scale, tmp)
            assert np.isfinite(result).all(), name
            for part, a in (("image", image), ("guide", guide), ("variance", variance), ("result", result)):
                arrays["%s_%s" % (name, part)] = a
            print("%-18s %dx%dx%d F %d R %d: mean %.6f" % (name, w, h, ch, F, R, float(result.mean())))
    np.savez_compressed(dc.GOLDEN, **arrays)
    print("%s: %d bytes" % (os.path.relpath(dc.GOLDEN, ROOT), os.path.getsize(dc.GOLDEN)))


if __name__ == "__main__":
    main()
