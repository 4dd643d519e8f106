"""Records tests/golden/walk_refill_counts.json: the ray, slot and visit counters of the passes tests/test_gpu_walk_refill.py renders, under
count_traversal=1 with every other option at its default.  Run on a GPU with the library of the commit BEFORE a change of the decoupled walks
(TUNGSTEN_AMD_LIB names it), so that the test holds the changed walks to what the earlier ones visited.

    TUNGSTEN_AMD_LIB=tungsten_amd/lib/libtungsten_hip_<parent>.so python tools/make_walk_refill_golden.py [--out tests/golden/walk_refill_counts.json]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "walk_refill_counts.json"))
    a = ap.parse_args()
    import scenes
    import test_gpu_walk_refill as t
    out = {}
    with tempfile.TemporaryDirectory(prefix="walk_refill_") as tmp:
        for scene in sorted(t.SCENES):
            if "materialtest" in scene and not scenes.have_materialtest():
                sys.exit("materialtest assets (assets/) not present")
            for w, h, spp in sorted({s[:3] for s in t.SHAPES}):
                path = t.scene_path(scene, w, h, spp, tmp)
                _, _, c = t.render(path, True, t.SCENES[scene][1])
                out[t.golden_key(scene, w, h, spp)] = c
                print(t.golden_key(scene, w, h, spp), c)
    with open(a.out, "w") as f:
        json.dump({"recorded_with": "count_traversal=1, default options, seed %d" % t.SEED, "counters": out}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
