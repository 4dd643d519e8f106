"""Generates the goldens of the fibre BCSDFs (tests/fibre_cases.py) by running the REFERENCE ITSELF -- the CPU oracle does not know the two types:

  tests/golden/fibre_*_samples.npz   the per-sample radiance of every case (oracle/_ref/ref_harness samples, through tools/make_golden.py's samples():
                                     same seed convention and array layout as every other per-sample golden), plus `lambert_twin_differing`: in how
                                     many samples the same scene with `lambert` in the fibres' place differs, rendered the same way
  tests/golden/fibre_bsdf_cases.npz  eval / pdf / sample of every BSDF of fibre_cases.bsdf_list() on fibre_cases.bsdf_fixture_cases()
                                     (ref_harness bsdf-cases, the binary format of tools/make_bsdf_golden.py): inputs and the 14 result words per case,
                                     NaN and infinities as the words they are

Before anything is written the goldens are checked to say something (check_samples / check_bsdf_words; tests/test_fibres_cpu.py repeats the checks on
the committed files).  TEST INFRASTRUCTURE; needs oracle/_ref (built by __graft_entry__.build() where the reference is mounted):

    python tools/make_fibre_golden.py [case ... | bsdf]
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden  # noqa: E402  (puts the repository and tests/ on sys.path)
import make_bsdf_golden  # noqa: E402
import bsdf_cases as bc  # noqa: E402
import fibre_cases  # noqa: E402
import oracle_lib  # noqa: E402
import scenes  # noqa: E402


def render(mk, kw, name, tmp, out):
    path = mk(tmp, name=name + ".json", **kw)
    with open(path) as f:
        sc = json.load(f)
    w, h = sc["camera"]["resolution"]
    make_golden.samples(path, w, h, sc["renderer"]["spp"], out)
    return out


def check_samples(name, samples, twin):
    """A golden that says something: finite, not black, and not what the scene gives with Lambert surfaces."""
    assert samples.shape == (27, 48, 8, 3) and samples.dtype == np.float32, (name, samples.shape)
    assert np.isfinite(samples).all(), "%s: the reference's samples are not finite" % name
    assert samples.max() > 0, "%s: black" % name
    differing = int((samples.view(np.uint32) != twin.view(np.uint32)).any(axis=-1).sum())
    assert differing > 0, "%s: the same samples as with lambert" % name
    return differing


def check_bsdf_words(names, ref, per):
    """The recorded words are finite where the reference guards (a refused lobe set: black, zero pdf, failed sample) and not all black."""
    for pos, name in enumerate(names):
        block = ref[pos*per:(pos + 1)*per]
        f = block[:, :4].view(np.float32)
        assert (f[np.isfinite(f)] != 0).any(), "%s: every recorded eval and pdf is zero" % name
        assert block[:, 4].any(), "%s: no sample succeeded" % name


def make_bsdf(tmp):
    names, position, cases, stream, per = fibre_cases.bsdf_fixture_cases()
    path = fibre_cases.bsdf_scene(tmp)
    with open(path) as f:
        sj = json.load(f)
    index = np.array([bc.scene_index(sj, names[p]) for p in position], np.int32)
    xi = np.concatenate([oracle_lib.rng_streams(bc.SEED, int(stream[pos*per]), per, bc.NXI) for pos in range(len(names))])
    ref = make_bsdf_golden.reference_words(path, index, cases, xi, tmp)
    assert int(ref[:, 13].max()) <= bc.NXI
    check_bsdf_words(names, ref, per)
    np.savez_compressed(fibre_cases.BSDF_GOLDEN, names=np.array(names), cases_per_bsdf=per, seed=np.uint32(bc.SEED), stream=stream,
                        wi=cases["wi"], wo=cases["wo"], uv=cases["uv"], requested=cases["requested"], ref=ref)
    nan = int(np.isnan(ref[:, [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11]].view(np.float32)).any(axis=1).sum())
    print("%-40s %d bytes: %d bsdfs x %d cases, %d samples succeeded, %d cases with a NaN word" % (
        os.path.basename(fibre_cases.BSDF_GOLDEN), os.path.getsize(fibre_cases.BSDF_GOLDEN), len(names), per, int(ref[:, 4].sum()), nan))


def main():
    if not os.path.exists(make_golden.HARNESS):
        raise SystemExit("oracle/_ref/ref_harness missing: run `python -c 'import __graft_entry__ as g; g.build()'` where the reference exists")
    names = sys.argv[1:] or sorted(fibre_cases.CASES) + ["bsdf"]
    tmp = tempfile.mkdtemp(prefix="tg_fibre_golden_")
    try:
        for name in names:
            if name == "bsdf":
                make_bsdf(tmp)
                continue
            out = os.path.join(scenes.GOLDEN, name + "_samples.npz")
            render(*fibre_cases.CASES[name], name, tmp, out)
            twin_out = os.path.join(tmp, name + "_twin.npz")
            render(*fibre_cases.lambert_twin(name), name + "_twin", tmp, twin_out)
            gold = dict(np.load(out))
            differing = check_samples(name, gold["samples"], np.load(twin_out)["samples"])
            np.savez_compressed(out, lambert_twin_differing=np.int64(differing), **gold)
            print("%-40s differs from its Lambert twin in %d of %d samples" % (name, differing, gold["samples"].shape[0]*gold["samples"].shape[1]*gold["samples"].shape[2]))
        wires = [np.load(os.path.join(scenes.GOLDEN, n + "_samples.npz"))["samples"] for n in fibre_cases.ROUGHNESS_CASES]
        for i in range(len(wires)):
            for j in range(i):
                assert (wires[i].view(np.uint32) != wires[j].view(np.uint32)).any(), "two roughness goldens are the same"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
