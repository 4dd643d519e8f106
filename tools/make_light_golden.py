"""Records what the reference's own TraceBase::chooseLight and Primitive::sampleDirect / approximateRadiance / intersect + intersectionInfo / evalDirect /
directPdf answer for the first FIXTURE_CASES cases (tests/light_cases.py) of every sampled light of the six scenes.light_corners scenes into
tests/golden/light_corners.npz: the case inputs, the reference's result words and the lights' names -- data only (the numbers the samplers replayed are
the first NXC / NXS of the case's two streams: light_cases.streams).  The answers come from `oracle/_ref/ref_harness light-cases` (oracle/ref_harness.cpp,
built by oracle/Makefile.ref).

The oracle is run on the same cases: every case in which one of its words is not the reference's is listed, and more than MAX_RESIDUAL of the
fixture's cases is refused.  `--residual` writes the differing cases to tests/golden/light_corners_residual.json (to be explained, not to be hidden).

    python tools/make_light_golden.py [--residual]
    python tools/make_light_golden.py --cases N      # the comparison alone on the first N cases of every light (N = 4096: the device test's list); writes nothing
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


def reference_words(scene_path, slots, cases, xi_choose, xi_sample, tmp):
    """The harness on n cases: [n, 20] uint32 words.  slots: [n] indices in TraceableScene::lights()."""
    import light_cases as lc
    n = len(slots)
    rec = np.zeros((n, 7 + lc.NXC + lc.NXS), np.float32)
    rec[:, 0] = np.asarray(slots, np.int32).view(np.float32)
    rec[:, 1:4], rec[:, 4:7], rec[:, 7:7 + lc.NXC], rec[:, 7 + lc.NXC:] = cases["p"], cases["w"], xi_choose[:, :lc.NXC], xi_sample[:, :lc.NXS]
    cf, of = os.path.join(tmp, "light_cases.bin"), os.path.join(tmp, "light_out.bin")
    with open(cf, "wb") as f:
        f.write(np.array([n, lc.NXC, lc.NXS], np.uint32).tobytes())
        f.write(rec.tobytes())
    subprocess.check_call([HARNESS, "light-cases", scene_path, cf, of])
    return np.fromfile(of, np.uint32).reshape(n, 20)


def scene_cases(desc, which, n):
    """(names, slots [N], cases dict of [N, ...], xi_choose [N, NXC], xi_sample [N, NXS]) of one scene's lights, light after light, n cases each."""
    import light_cases as lc
    import scenes
    pos = scenes.LIGHT_CORNER_SCENES.index(which)
    names = [name for name, _, _ in scenes.light_corner_list(which)]
    parts, xcs, xss, slots = [], [], [], []
    for slot, name in enumerate(names):
        parts.append(lc.make_cases(lc.light_geometry(desc, slot), name, n))
        xc, xs = lc.streams(pos, slot, n, extra=0)
        xcs.append(xc)
        xss.append(xs)
        slots += [slot]*n
    cases = {k: np.concatenate([p[k] for p in parts]) for k in ("p", "w")}
    return names, np.array(slots, np.int32), cases, np.concatenate(xcs), np.concatenate(xss)


def main():
    import light_cases as lc
    import oracle_lib
    import scenes
    import tungsten_amd as tg
    args = sys.argv[1:]
    n_cases = int(args[args.index("--cases") + 1]) if "--cases" in args else lc.FIXTURE_CASES
    out, residual, total, differ = {}, {}, 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        for which in scenes.LIGHT_CORNER_SCENES:
            path = scenes.light_corners(tmp, which)
            flat = tg.FlattenedScene(path)
            names, slots, cases, xc, xs = scene_cases(flat.desc, which, n_cases)
            ref = reference_words(path, slots, cases, xc, xs, tmp)
            assert int(ref[:, 18].max()) <= lc.NXC and int(ref[:, 19].max()) <= lc.NXS, "a call consumed more numbers than the replay samplers were given"
            got = oracle_lib.light_cases(flat.desc, slots, cases["p"], cases["w"], xc, xs)
            want = lc.chosen_as_objects(ref, flat.desc)
            d = flat.desc.contents
            dirac = np.array([d.objects[d.lights[s]].type == lc.POINT for s in slots])
            bad = lc.differing(got, want) | (dirac & lc.differing(got, want, dirac=True))
            flat.close()
            for i in np.nonzero(bad)[0]:
                residual.setdefault("%s/%s" % (which, names[slots[i]]), []).append(int(i % n_cases))
                words = [(lc.WORDS[k], hex(got[i, k]), hex(want[i, k])) for k in np.nonzero(got[i] != want[i])[0]]
                print("  %s/%s case %d: %s" % (which, names[slots[i]], i % n_cases, words))
            total += len(slots)
            differ += int(bad.sum())
            out[which + "_names"] = np.array(names)
            out[which + "_p"], out[which + "_w"], out[which + "_ref"] = cases["p"], cases["w"], ref
            ok = ref[:, 2] == 1
            hit = ref[:, 9] == 1
            for slot, name in enumerate(names):
                m = slots == slot
                print("%-6s %-12s chosen %3d/%d  sampled %3d  hit %3d  of %d" % (which, name, int((ref[m, 0].view(np.int32) >= 0).sum()), int(m.sum()),
                                                                                 int(ok[m].sum()), int(hit[m].sum()), int(m.sum())))
    print("%d cases; the oracle differs from the reference in %d cases (%d lights)" % (total, differ, len(residual)))
    if "--cases" in args:
        return 0 if differ <= MAX_RESIDUAL*total else 1
    if differ > MAX_RESIDUAL*total:
        print("REFUSED: more than %.1f %% of the fixture's cases differ; fix the oracle (or the device code it restates) first" % (100*MAX_RESIDUAL))
        return 1
    np.savez_compressed(lc.GOLDEN, cases_per_light=np.uint32(lc.FIXTURE_CASES), seed=np.uint32(lc.SEED), nxc=np.uint32(lc.NXC), nxs=np.uint32(lc.NXS), **out)
    print("%s: %d bytes" % (os.path.relpath(lc.GOLDEN, ROOT), os.path.getsize(lc.GOLDEN)))
    if "--residual" in sys.argv[1:]:
        with open(lc.RESIDUAL, "w") as f:
            json.dump(residual, f, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
