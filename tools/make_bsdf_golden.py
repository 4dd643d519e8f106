"""Records what the reference's own Bsdf::eval / pdf / sample answer for the first FIXTURE_CASES cases (tests/bsdf_cases.py) of every named bsdf of
scenes.bsdf_corners into tests/golden/bsdf_corners.npz: the case inputs, the reference's result words and the bsdfs' names -- data only (the numbers
the samplers replayed are the first NXI of the stream (seed, stream index of the case, 0): bsdf_cases.streams).  The answers come from `oracle/_ref/ref_harness bsdf-cases` (oracle/ref_harness.cpp, built by oracle/Makefile.ref).

The oracle is run on the same cases: every case in which one of its words is not the reference's is listed, and more than MAX_RESIDUAL of the
fixture's cases is refused.  `--residual` writes the differing cases to tests/golden/bsdf_corners_residual.json (to be explained, not to be hidden).

    python tools/make_bsdf_golden.py [--residual]
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


def reference_words(scene_path, bsdf_index, cases, xi, tmp):
    """The harness on n cases: [n, 14] uint32 words.  bsdf_index: [n] indices in the scene's own list."""
    import bsdf_cases as bc
    n = len(bsdf_index)
    rec = np.zeros((n, 10 + bc.NXI), np.float32)
    rec[:, 0] = np.asarray(bsdf_index, np.int32).view(np.float32)
    rec[:, 1] = np.asarray(cases["requested"], np.uint32).view(np.float32)
    rec[:, 2:5], rec[:, 5:8], rec[:, 8:10], rec[:, 10:] = cases["wi"], cases["wo"], cases["uv"], xi[:, :bc.NXI]
    cf, of = os.path.join(tmp, "bsdf_cases.bin"), os.path.join(tmp, "bsdf_out.bin")
    with open(cf, "wb") as f:
        f.write(np.array([n, bc.NXI], np.uint32).tobytes())
        f.write(rec.tobytes())
    subprocess.check_call([HARNESS, "bsdf-cases", scene_path, cf, of])
    return np.fromfile(of, np.uint32).reshape(n, 14)


def fixture_cases(scene_json):
    """(names, bsdf index in the scene's list [N], cases dict of [N, ...], xi [N, NXI]) of the whole fixture, bsdf after bsdf."""
    import bsdf_cases as bc
    import scenes
    names = [b["name"] for b in scenes.bsdf_corner_list()]
    parts, xis, index = [], [], []
    for pos, b in enumerate(scenes.bsdf_corner_list()):
        parts.append(bc.make_cases(b, bc.FIXTURE_CASES, scenes.CORNER_TEXTURE_SIZE))
        xis.append(bc.streams(pos, bc.FIXTURE_CASES, extra=0))
        index += [bc.scene_index(scene_json, b["name"])]*bc.FIXTURE_CASES
    cases = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    return names, np.array(index, np.int32), cases, np.concatenate(xis)


def main():
    import bsdf_cases as bc
    import oracle_lib
    import scenes
    import tungsten_amd as tg
    from test_oracle_golden import flat_bsdf_index
    with tempfile.TemporaryDirectory() as tmp:
        path = scenes.bsdf_corners(tmp)
        with open(path) as f:
            sj = json.load(f)
        names, index, cases, xi = fixture_cases(sj)
        ref = reference_words(path, index, cases, xi, tmp)
        assert int(ref[:, 13].max()) <= bc.NXI, "a sample consumed more numbers than the replay samplers were given"
        flat = tg.FlattenedScene(path)
        flat_index = np.array([flat_bsdf_index(sj, int(i)) for i in index], np.int32)
        got = oracle_lib.bsdf_cases(flat.desc, flat_index, cases["requested"], cases["wi"], cases["wo"], cases["uv"], xi)
        flat.close()
    bad = bc.differing(got, ref)
    residual = {}
    for i in np.nonzero(bad)[0]:
        residual.setdefault(names[i//bc.FIXTURE_CASES], []).append(int(i % bc.FIXTURE_CASES))
    print("%d bsdfs, %d cases; the oracle differs from the reference in %d cases (%d bsdfs)" % (len(names), len(index), int(bad.sum()), len(residual)))
    for name, ks in sorted(residual.items()):
        print("  %-28s %3d: %s" % (name, len(ks), ks[:12]))
    if bad.sum() > MAX_RESIDUAL*len(index):
        print("REFUSED: more than %.1f %% of the fixture's cases differ; fix the oracle (or the device code it restates) first" % (100*MAX_RESIDUAL))
        return 1
    np.savez_compressed(bc.GOLDEN, names=np.array(names), cases_per_bsdf=np.uint32(bc.FIXTURE_CASES), seed=np.uint32(bc.SEED),
                        nxi=np.uint32(bc.NXI), wi=cases["wi"], wo=cases["wo"], uv=cases["uv"], requested=cases["requested"], ref=ref)
    print("%s: %d bytes" % (os.path.relpath(bc.GOLDEN, ROOT), os.path.getsize(bc.GOLDEN)))
    if "--residual" in sys.argv[1:]:
        with open(bc.RESIDUAL, "w") as f:
            json.dump(residual, f, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
