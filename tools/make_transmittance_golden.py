"""Builds the reference harness of generalizedShadowRay (tools/ref_transmittance.cpp, against the reference's headers and oracle/_ref/libcore.a,
with the core flags of oracle/Makefile.ref: the recipe of tools/make_denoise_golden.py) into the git-ignored oracle/_ref/, and records what the
reference's own TraceBase::generalizedShadowRay answers for the cases of tests/transmittance_cases.py into tests/golden/transmittance_cases.npz:
rays, per-ray start media, per-call parameters and results -- data only.

    python tools/make_transmittance_golden.py            # build the harness, write the fixture
    python tools/make_transmittance_golden.py --build    # build the harness only
"""
import json
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
    exe = os.path.join(OUT, "ref_transmittance")
    cmd = ["g++", "-std=c++11", "-O3", "-DNDEBUG", "-march=nehalem", "-fstrict-aliasing", "-fvisibility-inlines-hidden", "-w",
           "-DCONSTEXPR=constexpr", "-DEMBREE_STATIC_LIB=1", '-DINSTALL_PREFIX="/usr/local"', "-DLODEPNG_NO_COMPILE_DISK=1",
           "-DRAPIDJSON_HAS_STDSTRING=1", "-DSTBI_NO_STDIO=1",
           "-I" + os.path.join(src, "core"), "-I" + os.path.join(src, "thirdparty"), "-I" + os.path.join(src, "thirdparty", "embree", "include"),
           "-I" + src, os.path.join(ROOT, "tools", "ref_transmittance.cpp"), "-o", exe,
           os.path.join(OUT, "libcore.a"), os.path.join(OUT, "libthirdparty.a"), os.path.join(OUT, "libembree.a"),
           os.path.join(OUT, "libembree_sse42.a"), os.path.join(OUT, "libembree.a"), "-ldl", "-lpthread"]
    subprocess.check_call(cmd, cwd=ROOT)
    return exe


def _hex(row):
    return " ".join("%08x" % w for w in np.asarray(row, np.float32).view(np.uint32))


def reference_answers(exe, path, groups, tmp):
    """The harness on the groups of one scene: per group (rgb bits [n, 3] uint32, crossed [n] int32, end [n] int32)"""
    cases, out = os.path.join(tmp, "cases.txt"), os.path.join(tmp, "out.txt")
    with open(cases, "w") as f:
        for g in groups:
            f.write("group %d %s %s %d %d %d %d\n" % (len(g["rays"]), g["medium"] or "-", g["end_cap"] or "-", g["bounce"], g["starts"], g["ends"],
                                                      g["media"] is not None))
            for i, ray in enumerate(g["rays"]):
                f.write(_hex(ray) + (" " + g["media"][i] if g["media"] is not None else "") + "\n")
    subprocess.check_call([exe, path, cases, out], cwd=tmp)
    words = np.array([[int(w, 16) for w in line.split()[:3]] + [int(w) for w in line.split()[3:]] for line in open(out)], np.int64)
    assert len(words) == sum(len(g["rays"]) for g in groups)
    answers, at = [], 0
    for g in groups:
        w = words[at:at + len(g["rays"])]
        at += len(g["rays"])
        answers.append((w[:, 0:3].astype(np.uint32), w[:, 3].astype(np.int32), w[:, 4].astype(np.int32)))
    return answers


def main():
    exe = build_harness()
    if "--build" in sys.argv[1:]:
        return
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import transmittance_cases as tc
    groups = tc.make_groups()
    arrays, table = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for scene in sorted({g["scene"] for g in groups}, key=[g["scene"] for g in groups].index):
            path = tc.build_scene(scene, tmp)
            mine = [(k, g) for k, g in enumerate(groups) if g["scene"] == scene]
            for (k, g), (rgb, crossed, end) in zip(mine, reference_answers(exe, path, [g for _, g in mine], tmp)):
                assert np.isfinite(rgb.view(np.float32)).all(), (scene, g["leg"])
                arrays["g%03d_rays" % k], arrays["g%03d_rgb" % k] = g["rays"], rgb
                arrays["g%03d_crossed" % k], arrays["g%03d_end" % k] = crossed, end
                print("%-20s %-28s %4d rays: %4d lit, crossed up to %d" % (scene, g["leg"], len(rgb), int((rgb.view(np.float32) != 0).any(axis=1).sum()),
                                                                           int(crossed.max())))
    for g in groups:
        table.append({k: g[k] for k in ("scene", "leg", "medium", "end_cap", "bounce", "starts", "ends", "media")})
    arrays["groups"] = np.array(json.dumps(table))
    np.savez_compressed(tc.GOLDEN, **arrays)
    print("%s: %d bytes, %d cases" % (os.path.relpath(tc.GOLDEN, ROOT), os.path.getsize(tc.GOLDEN), sum(len(g["rays"]) for g in groups)))
    have = tc.census(tc.load_golden())
    for leg in tc.LEGS:
        print("%-44s %5d%s" % (leg, have.get(leg, 0), "" if have.get(leg, 0) >= 16 else "   <-- fewer than 16"))


if __name__ == "__main__":
    main()
