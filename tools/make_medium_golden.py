"""Records what the reference's own Medium::sampleDistance, Medium::transmittance, PhaseFunction::eval and PhaseFunction::sample answer for the first
FIXTURE_CASES cases (tests/medium_cases.py) of every medium of scenes.medium_corners into tests/golden/medium_corners.npz: the case inputs, the
reference's result words and the media's names -- data only (the numbers the samplers replayed are the first NXD / NXP of the case's two streams:
medium_cases.streams).  The answers come from `oracle/_ref/ref_harness medium-cases` (oracle/ref_harness.cpp, built by oracle/Makefile.ref).

The oracle is run on the same cases: every case in which one of its words is not the reference's is listed, and more than MAX_RESIDUAL of the
fixture's cases is refused.  `--residual` writes the differing cases, each with the word and both values, to
tests/golden/medium_corners_residual.json (to be explained, not to be hidden).

    python tools/make_medium_golden.py [--residual]
    python tools/make_medium_golden.py --cases N      # the comparison alone on the first N cases of every medium (N = 2048: the device test's list); writes nothing
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
MAX_RESIDUAL = 0.001          # of the fixture's cases


def reference_words(scene_path, names, which, cases, xi_dist, xi_phase, tmp):
    """The harness on n cases: [n, 26] uint32 words.  which: [n] indices into names."""
    import medium_cases as mc
    n = len(which)
    rec = np.zeros((n, 12 + mc.NXD + mc.NXP), np.float32)
    rec[:, 0] = np.asarray(which, np.int32).view(np.float32)
    rec[:, 1] = np.asarray(cases["bounce"], np.int32).view(np.float32)
    rec[:, 2:5], rec[:, 5:8], rec[:, 8], rec[:, 9:12] = cases["p"], cases["d"], cases["max_t"], cases["wo"]
    rec[:, 12:12 + mc.NXD], rec[:, 12 + mc.NXD:] = xi_dist[:, :mc.NXD], xi_phase[:, :mc.NXP]
    cf, of = os.path.join(tmp, "medium_cases.bin"), os.path.join(tmp, "medium_out.bin")
    with open(cf, "wb") as f:
        f.write(np.array([n, mc.NXD, mc.NXP, len(names)], np.uint32).tobytes())
        for name in names:
            f.write(name.encode().ljust(64, b"\0")[:64])
        f.write(rec.tobytes())
    subprocess.check_call([HARNESS, "medium-cases", scene_path, cf, of])
    return np.fromfile(of, np.uint32).reshape(n, 26)


def scene_cases(desc, n):
    """(names, which [N], media indices [N], cases dict of [N, ...], xi_dist [N, NXD], xi_phase [N, NXP]): medium after medium, n cases each."""
    import medium_cases as mc
    import scenes
    names = [name for name, _ in scenes.medium_corner_list()]
    indices = mc.medium_indices(desc)
    parts, xds, xps, which = [], [], [], []
    for pos, name in enumerate(names):
        parts.append(mc.make_cases(mc.medium_geometry(desc, indices[pos]), name, n))
        xd, xp = mc.streams(pos, n, extra=0)
        xds.append(xd)
        xps.append(xp)
        which += [pos]*n
    cases = {k: np.concatenate([p[k] for p in parts]) for k in mc.CASE_KEYS}
    which = np.array(which, np.int32)
    return names, which, np.array(indices, np.int32)[which], cases, np.concatenate(xds), np.concatenate(xps)


def main():
    import medium_cases as mc
    import oracle_lib
    import scenes
    import tungsten_amd as tg
    args = sys.argv[1:]
    n_cases = int(args[args.index("--cases") + 1]) if "--cases" in args else mc.FIXTURE_CASES
    residual = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = scenes.medium_corners(tmp)
        flat = tg.FlattenedScene(path)
        names, which, index, cases, xd, xp = scene_cases(flat.desc, n_cases)
        ref = reference_words(path, names, which, cases, xd, xp, tmp)
        assert int(ref[:, 24].max()) <= mc.NXD and int(ref[:, 25].max()) <= mc.NXP, "a call consumed more numbers than the replay samplers were given"
        got = oracle_lib.medium_cases(flat.desc, index, cases["bounce"], cases["p"], cases["d"], cases["max_t"], cases["wo"], xd, xp)
        flat.close()
    bad = mc.differing(got, ref)
    for i in np.nonzero(bad)[0]:
        words = [[mc.WORDS[k], hex(got[i, k]), hex(ref[i, k])] for k in np.nonzero(got[i] != ref[i])[0]]
        residual.setdefault(names[which[i]], []).append({"case": int(i % n_cases), "words": words})
        print("  %s case %d: %s" % (names[which[i]], i % n_cases, words))
    for pos, name in enumerate(names):
        m = which == pos
        print("%-24s ok %4d  exited %4d  infinite t %3d  of %d" % (name, int((ref[m, 0] == 1).sum()), int((ref[m, 5] == 1).sum()),
                                                                 int(np.isinf(ref[m, 1].view(np.float32)).sum()), int(m.sum())))
    total, differ = len(which), int(bad.sum())
    print("%d cases; the oracle differs from the reference in %d cases (%d media)" % (total, differ, len(residual)))
    if "--cases" in args:
        return 0 if differ <= MAX_RESIDUAL*total else 1
    if differ > MAX_RESIDUAL*total:
        print("REFUSED: more than %.1f %% of the fixture's cases differ; fix the oracle (or the device code it restates) first" % (100*MAX_RESIDUAL))
        return 1
    out = {k: cases[k] for k in mc.CASE_KEYS}
    np.savez_compressed(mc.GOLDEN, cases_per_medium=np.uint32(mc.FIXTURE_CASES), seed=np.uint32(mc.SEED), nxd=np.uint32(mc.NXD), nxp=np.uint32(mc.NXP),
                        names=np.array(names), ref=ref, **out)
    print("%s: %d bytes" % (os.path.relpath(mc.GOLDEN, ROOT), os.path.getsize(mc.GOLDEN)))
    if "--residual" in args:
        with open(mc.RESIDUAL, "w") as f:
            json.dump(residual, f, sort_keys=True, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
