"""Builds the reference harness of estimateDirect (tools/ref_direct.cpp, against the reference's headers and oracle/_ref/libcore.a, with the core
flags of oracle/Makefile.ref: the recipe of tools/make_transmittance_golden.py) into the git-ignored oracle/_ref/, and records what the reference's
own TraceBase::estimateDirect / volumeEstimateDirect answers for the cases of tests/direct_cases.py into tests/golden/direct_cases.npz: rays,
per-ray start media, per-call parameters and per-sample results -- data only.

    python tools/make_direct_golden.py            # build the harness, write the fixture, print the census
    python tools/make_direct_golden.py --build    # build the harness only
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
    exe = os.path.join(OUT, "ref_direct")
    cmd = ["g++", "-std=c++11", "-O3", "-DNDEBUG", "-march=nehalem", "-fstrict-aliasing", "-fvisibility-inlines-hidden", "-w",
           "-DCONSTEXPR=constexpr", "-DEMBREE_STATIC_LIB=1", '-DINSTALL_PREFIX="/usr/local"', "-DLODEPNG_NO_COMPILE_DISK=1",
           "-DRAPIDJSON_HAS_STDSTRING=1", "-DSTBI_NO_STDIO=1",
           "-I" + os.path.join(src, "core"), "-I" + os.path.join(src, "thirdparty"), "-I" + os.path.join(src, "thirdparty", "embree", "include"),
           "-I" + src, os.path.join(ROOT, "tools", "ref_direct.cpp"), "-o", exe,
           os.path.join(OUT, "libcore.a"), os.path.join(OUT, "libthirdparty.a"), os.path.join(OUT, "libembree.a"),
           os.path.join(OUT, "libembree_sse42.a"), os.path.join(OUT, "libembree.a"), "-ldl", "-lpthread"]
    subprocess.check_call(cmd, cwd=ROOT)
    return exe


def _hex(row):
    return " ".join("%08x" % w for w in np.asarray(row, np.float32).view(np.uint32))


def reference_answers(exe, path, groups, slots, tmp):
    """The harness on the groups of one scene: per group a dict of [n, spp, ...] arrays (direct_cases.PARTS without the rays)"""
    cases, out = os.path.join(tmp, "cases.txt"), os.path.join(tmp, "out.txt")
    with open(cases, "w") as f:
        for g in groups:
            f.write("group %d %d %d %d %s %d %d %d %d %d\n" % (len(g["rays"]), g["spp"][0], g["spp"][1], g["seed"], g["medium"] or "-", g["bounce"],
                                                             -1 if g["light_name"] is None else slots[g["light_name"]], g["skip"], g["volume"],
                                                             g["media"] is not None))
            for i, ray in enumerate(g["rays"]):
                f.write(_hex(ray) + (" " + g["media"][i] if g["media"] is not None else "") + "\n")
    subprocess.check_call([exe, path, cases, out], cwd=tmp)
    words = np.array([[int(w, 16) for w in line.split()[:4]] + [int(w) for w in line.split()[4:]] for line in open(out)], np.int64)
    assert len(words) == sum(len(g["rays"])*(g["spp"][1] - g["spp"][0]) for g in groups)
    answers, at = [], 0
    for g in groups:
        n, spp = len(g["rays"]), g["spp"][1] - g["spp"][0]
        w = words[at:at + n*spp].reshape(n, spp, -1)
        at += n*spp
        answers.append(dict(rgb=w[:, :, 0:3].astype(np.uint32), transmittance=w[:, :, 3].astype(np.uint32), recorded=w[:, :, 4].astype(np.uint8),
                            taken=w[:, :, 5].astype(np.uint8), legs=w[:, :, 6].astype(np.int32), light=w[:, :, 7].astype(np.int32),
                            hit=w[:, :, 8].astype(np.int32)))
    return answers


def main():
    exe = build_harness()
    if "--build" in sys.argv[1:]:
        return
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import direct_cases as dc
    groups = dc.make_groups()
    arrays, table, primitives = {}, [], {}
    with tempfile.TemporaryDirectory() as tmp:
        for scene in sorted({g["scene"] for g in groups}, key=[g["scene"] for g in groups].index):
            path = dc.build_scene(scene, tmp)
            primitives[scene] = dc.primitives_of(path)
            mine = [(k, g) for k, g in enumerate(groups) if g["scene"] == scene]
            for (k, g), a in zip(mine, reference_answers(exe, path, [g for _, g in mine], dc.light_slots(path), tmp)):
                assert np.isfinite(a["rgb"].view(np.float32)).all(), (scene, g["leg"])
                arrays["g%03d_rays" % k] = g["rays"]
                for part, value in a.items():
                    arrays["g%03d_%s" % (k, part)] = value
                print("%-18s %-26s %4d rays x %d: %4d taken, %4d lit" % (scene, g["leg"], len(g["rays"]), a["taken"].shape[1], int(a["taken"].sum()),
                                                                         int((a["rgb"].view(np.float32) != 0).any(axis=2).sum())))
    for g in groups:
        table.append({k: g[k] for k in ("scene", "leg", "spp", "seed", "medium", "media", "bounce", "light_name", "skip", "volume")})
    arrays["groups"] = np.array(json.dumps(table))
    np.savez_compressed(dc.GOLDEN, **arrays)
    print("%s: %d bytes, %d items" % (os.path.relpath(dc.GOLDEN, ROOT), os.path.getsize(dc.GOLDEN),
                                      sum(len(g["rays"])*(g["spp"][1] - g["spp"][0]) for g in groups)))
    have = dc.census(dc.load_golden(), primitives)
    for leg in dc.LEGS:
        print("%-32s %5d%s" % (leg, have.get(leg, 0), "" if have.get(leg, 0) >= 8 else "   <-- fewer than 8"))


if __name__ == "__main__":
    main()
