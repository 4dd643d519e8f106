"""Generates tests/golden/stex_*_samples.npz -- the per-sample radiance of the sampled-texture cases (tests/sampled_texture_cases.py: checker
environments, constant / checker / `ies` apertures, pivoted caps) -- by running the REFERENCE ITSELF: oracle/_ref/ref_harness samples, through
tools/make_golden.py's samples() (same seed convention, same array layout as every other per-sample golden).  TEST INFRASTRUCTURE; needs oracle/_ref
(built by __graft_entry__.build() where the reference is mounted):

    python tools/make_sampled_texture_golden.py [case ...]
"""
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden  # noqa: E402  (puts the repository and tests/ on sys.path)
import scenes  # noqa: E402
import sampled_texture_cases  # noqa: E402


def main():
    if not os.path.exists(make_golden.HARNESS):
        raise SystemExit("oracle/_ref/ref_harness missing: run `python -c 'import __graft_entry__ as g; g.build()'` where the reference exists")
    names = sys.argv[1:] or sorted(sampled_texture_cases.CASES)
    tmp = tempfile.mkdtemp(prefix="tg_stex_golden_")
    try:
        for name in names:
            mk, kw = sampled_texture_cases.CASES[name]
            path = mk(tmp, name=name + ".json", **kw)
            with open(path) as f:
                sc = json.load(f)
            w, h = sc["camera"]["resolution"]
            make_golden.samples(path, w, h, sc["renderer"]["spp"], os.path.join(scenes.GOLDEN, name + "_samples.npz"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
