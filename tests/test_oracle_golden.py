"""Pins oracle/oracle.c (the CPU restatement, TEST INFRASTRUCTURE) against outputs of the reference
itself committed under tests/golden/ (tools/make_golden.py: oracle/ref_harness.cpp links the reference's
libcore.a and drives its PathTracer::traceSample with the shared counter-based random stream).

Tolerances: integers / RNG exact; closest-hit distances exact (Embree's rcp + Newton restated,
triangle_intersector_moeller.h:45-48); other deterministic floats rel 1e-5; per-sample radiance BIT-IDENTICAL in every case
(67 cases, 601 344 samples, since the reference's top-level Embree tree was restated at the end of round 4; DIVERGING below is empty)."""
import json
import os

import numpy as np
import pytest

import light_cases as lc
import oracle_lib
import scenes
import tungsten_amd as tg

G = scenes.GOLDEN
ALL_BUT_SPECULAR = 0x4F   # BsdfLobes.hpp:13-33


def close(a, b, rel, floor=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= rel*max(np.abs(b).max(), floor) + 1e-7


def flat_bsdf_index(scene_json, scene_index):
    """Index of scene bsdf #i in the flattened table (nested inline bsdfs are appended depth-first,
    TraceableScene.cpp addBsdf)."""
    bsdfs = scene_json["bsdfs"]
    names = {b.get("name"): i for i, b in enumerate(bsdfs)}
    order = {}
    counter = [0]

    def add(b, key):
        if isinstance(b, str):
            b, key = bsdfs[names[b]], ("top", names[b])
        if key in order:
            return
        order[key] = counter[0]
        counter[0] += 1
        for k in ("substrate", "bsdf0", "bsdf1", "base"):
            if k in b:
                add(b[k], (key, k))
    for i, b in enumerate(bsdfs):
        add(b, ("top", i))
    return order[("top", scene_index)]


def _needs_materialtest(name):
    if name == "water_caustic" and not scenes.have_water_caustic():
        pytest.skip("water-caustic assets (assets/) not present")
    if ("materialtest" in name or name == "mesh1m") and not scenes.have_materialtest():   # mesh1m is lit by materialtest's HDRI
        pytest.skip("materialtest assets (assets/) not present")


# Samples in which the oracle leaves the reference's path (every channel within 1e-3 is "the same path"), per case.  EMPTY since the end of round 4:
# the one cause that was left -- coincident faces: the Cornell box's blocks stand ON the floor quad, so the bottom face of a see-through block
# (smoke, glass, cut-out, the zoo's transmissive materials) and the floor under it are hit at the same distance, and the traversal order decides
# which one a ray sees (99 samples in 12 cases: cornell_fog 1, cornell_fog_davis 2, cornell_fog_rayleigh 1, cornell_fog_smoke_sobol 9,
# cornell_png_scalar 11, cornell_smoke 17, zoo_a 7, zoo_b 8, zoo_b_sobol 7, zoo_e 20, zoo_f 6, cornell_expfog_smoke_sobol 10) -- went when the
# oracle (and the device) began to visit a flat list of analytic primitives the way Embree's user-geometry BVH visits its one-primitive
# leaves: slab test of the primitive's own bounds(), nearest box entry first (equal entries: the later record first), a leaf entered behind the
# hit so far skipped (oracle.c: embree_ordered_flat).  The `*_lifted` twins below, with every solid a millimetre off the
# floor, were exact before and still are.
# (cornell_instances left this list earlier in round 4: Instance::intersect gives every instance a ray with farT = infinity, Instance.cpp:296, and
# keeps the LAST hit in the visiting order of its own BVH -- the oracle walks that very tree, restated node for node, in that order.)
# A case listed here would be held to 1.5 x its measured count + 5 samples.
DIVERGING = {}
# Cases whose residual against the reference is pinned EXACTLY: tests/golden/order_residual.json holds the (y, x, sample) index of every sample
# in which the oracle's radiance is not the reference's bit for bit; the device must reproduce the ORACLE in every sample (tests/test_gpu_samples.py),
# so the same set is the device's.  cornell_instance_ties (round 6): glass boxes -- instances of a mesh -- standing on the floor quad and against a
# wall; where a box's face and the quad behind it are hit at the same distance, the reference's top-level Embree tree over ALL finite primitives
# (the instance set being one item, TraceableScene.hpp:112-134) decides which one the path sees, and this library walks a BVH2 of its own over the
# scene-level records there: 18 of 10 368 samples take the other surface.  A different set -- one more, one fewer, another 18 -- fails.
PINNED = json.load(open(os.path.join(G, "order_residual.json"))) if os.path.exists(os.path.join(G, "order_residual.json")) else {}


def diverge_bound(name, samples):
    """Largest number of divergent samples the tests accept for a case (also the device's bound, tests/test_gpu_samples.py)."""
    return int(1.5*DIVERGING.get(name, 0)) + 5 if name in DIVERGING else 0


# Cases in which the oracle's radiance is the reference's BIT FOR BIT in every sample (float32 ==, all three channels) -- every golden case, 67 of
# 67 with 601 344 samples, since the end of round 4: the whole path -- camera,
# filter, intersections, frames, BSDFs, light selection and sampling, MIS, Russian roulette, media, textures -- restated operation by operation.
# Since round 4 that includes every case with a triangle mesh (materialtest with all its hero materials, the 998 000-triangle mesh, the water
# caustic, mesh emitters, the bump-mapped mesh): Embree's triangle test is restated down to its right-associated dot product and its
# RCPPS-plus-Newton reciprocal (oracle.c: edot / intel_rcpps / embree_rcp), which was what kept 0.1 - 1.4 % of their samples on other paths.
BIT_IDENTICAL = set(scenes.GOLDEN_CASES) - set(DIVERGING) - set(PINNED)


def _oracle_samples(mk, kw, name, tmp_path, ref, seed):
    h, w, spp, _ = ref.shape
    flat = tg.FlattenedScene(mk(tmp_path, name=name + ".json", **kw))
    assert (flat.width, flat.height) == (w, h)
    # "stratified_sampler": true scenes draw from the SobolPathSampler of the pixel's 16x16 tile
    tile_seeds = oracle_lib.dice_tiles(w, h, seed)[0] if flat.info.stratified_sampler else None
    got = np.empty_like(ref)
    for y in range(h):
        for x in range(w):
            ts = None if tile_seeds is None else tile_seeds[(y//16)*((w + 15)//16) + x//16]
            for s in range(spp):
                got[y, x, s] = oracle_lib.trace_sample(flat.desc, seed, x, y, s, tile_seed=ts)
    flat.close()
    return got


@pytest.mark.parametrize("name", sorted(scenes.LIFTED_CASES))
def test_oracle_is_the_reference_bit_for_bit_without_coincident_faces(name, tmp_path):
    """The smoke / fog / glass-box / cutout / BSDF-zoo cases with every solid lifted a millimetre off the floor (tests/scenes.py:
    LIFTED_CASES): no tie between a box's bottom face and the floor quad left for the traversal order to decide -- and not one of the
    10 368 samples of a case in which the oracle's radiance is not the reference's, bit for bit."""
    mk, kw = scenes.LIFTED_CASES[name]
    gold = np.load(os.path.join(G, name + "_samples.npz"))
    ref = gold["samples"]
    got = _oracle_samples(mk, kw, name, tmp_path, ref, int(gold["seed"]))
    assert (got.view(np.uint32) == ref.view(np.uint32)).all() or (got == ref).all()


@pytest.mark.parametrize("name", sorted(scenes.GOLDEN_CASES))
def test_oracle_matches_reference_per_sample(name, tmp_path):
    _needs_materialtest(name)
    mk, kw = scenes.GOLDEN_CASES[name]
    gold = np.load(os.path.join(G, name + "_samples.npz"))
    ref = gold["samples"]
    seed = int(gold["seed"])
    got = _oracle_samples(mk, kw, name, tmp_path, ref, seed)
    if name in BIT_IDENTICAL:
        assert (got == ref).all(), "%s: %d samples are not the reference's bit for bit" % (name, int((got != ref).any(axis=-1).sum()))
    if name in PINNED:
        where = [[int(v) for v in c] for c in np.argwhere((got.view(np.uint32) != ref.view(np.uint32)).any(axis=-1))]
        assert where == PINNED[name], "%s: the samples that are not the reference's are not the pinned ones: %s against %s" % (name, where[:6], PINNED[name][:6])
        return
    err = np.abs(got - ref).max(axis=-1)
    bad = err > 1e-3*(np.abs(ref).max(axis=-1) + 1e-3)
    assert int(bad.sum()) <= diverge_bound(name, bad.size), "%s: %d of %d samples differ from the reference (measured: %d)" % (
        name, int(bad.sum()), bad.size, DIVERGING.get(name, 0))
    # the mean image is insensitive to the few divergent paths
    assert np.allclose(got.mean(axis=(0, 1, 2)), ref.mean(axis=(0, 1, 2)), rtol=0.03)


@pytest.mark.parametrize("scene", ["cornell", "materialtest", "zoo_a", "zoo_b", "zoo_c", "zoo_d", "zoo_e", "zoo_f"])
def test_oracle_units(scene, tmp_path):
    _needs_materialtest(scene)
    with open(os.path.join(G, scene + "_units.json")) as f:
        u = json.load(f)
    if scene == "cornell":
        path = scenes.cornell(tmp_path, resolution=(96, 54), spp=1)
    elif scene == "materialtest":
        path = scenes.materialtest(tmp_path, resolution=(96, 54), spp=1)
    else:
        path = scenes.cornell_zoo(tmp_path, scene, resolution=(96, 54), spp=1)
    with open(path) as f:
        sj = json.load(f)
    flat = tg.FlattenedScene(path)
    d = flat.desc

    # RNG: PCG-XSH-RR + hash32 keyed by (seed, pixel, sample) -- integer work, exact
    for r in u["rng"]:
        got = oracle_lib.rng_stream(r["seed"], r["pixel"], r["sample"], 16)
        assert (got == np.array(r["values"], np.float32)).all()

    # camera rays + closest hits
    rays, want = [], []
    for r in u["rays"]:
        if "px" in r:
            o, dd = oracle_lib.camera_ray(d, r["px"], r["py"], r["xi"][0], r["xi"][1])
            assert close(o, r["o"], 1e-6) and close(dd, r["d"], 2e-6), r
        rays.append(r["o"] + [r["tmin"]] + r["d"] + [np.inf])
        want.append(r)
    hits, nodes, prims = oracle_lib.trace_rays(d, np.array(rays, np.float32))
    assert prims > 0 and (nodes > 0 or flat.desc.contents.num_recs <= 16)   # flat-list rule (TGHIP_FLAT_MAX_RECS)
    # (exact since round 4: Embree's triangle test is restated down to its reciprocal, and Quad / Cube / Sphere::intersect always were)
    mism = 0
    for hgot, r in zip(hits, want):
        if bool(r["hit"]) != (hgot["rec"] >= 0) or (r["hit"] and np.float32(r["t"]) != hgot["t"]):
            mism += 1
    assert mism == 0, "%d of %d closest hits differ" % (mism, len(want))

    # BSDF eval / pdf / sample
    for b in u["bsdfs"]:
        bi = flat_bsdf_index(sj, b["index"])
        assert d.contents.bsdfs[bi].lobes == b["lobes"], b["name"]
        for c in b["cases"]:
            f, pdf = oracle_lib.bsdf_eval(d, bi, c["wi"], c["wo"], c["uv"], c["requested"])
            assert close(f, c["f"], 2e-4), (b["name"], c, f)
            assert close(pdf, c["pdf"], 2e-4), (b["name"], c, pdf)
            ok, wo, weight, spdf, lobe, consumed = oracle_lib.bsdf_sample(d, bi, c["wi"], c["uv"], c["requested"], c["xi"])
            assert ok == bool(c["sample_ok"]), (b["name"], c)
            assert consumed == c["consumed"], (b["name"], c)
            if ok:
                assert close(wo, c["s_wo"], 2e-4) and close(weight, c["s_weight"], 1e-3), (b["name"], c, wo, weight)
                assert close(spdf, c["s_pdf"], 1e-3) and lobe == c["s_lobe"], (b["name"], c, spdf, lobe)

    # lights: sampleDirect
    for L in u["lights"]:
        for c in L["cases"]:
            ok, dd, dist, pdf = oracle_lib.light_sample(d, L["index"], c["p"], c["xi"][0], c["xi"][1])
            assert ok == bool(c["ok"]), c
            if ok:
                assert close(dd, c["d"], 1e-5), c
                assert close(pdf, c["pdf"], 2e-4), (c, pdf)
                if c["dist"] < 1e29:
                    assert close(dist, c["dist"], 1e-5), c

    # lights: approximateRadiance at every recorded point and -- along the recorded sampled direction, the ray of the BSDF-sampling leg -- directPdf and
    # evalDirect, through the batched entry of the per-call light comparisons.  "%.9g" round-trips a float32, so these are float32 equalities; a case
    # that differs would be pinned by scene, light and case in tests/golden/units_light_residual.json (there is none).
    pinned = json.load(open(lc.UNITS_RESIDUAL)).get(scene, {}) if os.path.exists(lc.UNITS_RESIDUAL) else {}
    differing, total = {}, 0
    for L in u["lights"]:
        cs = L["cases"]
        n = len(cs)
        total += n
        p = np.array([c["p"] for c in cs], np.float32)
        w = np.array([c.get("d", [0.0, 1.0, 0.0]) for c in cs], np.float32)
        xs = np.full((n, lc.NXS), 0.5, np.float32)
        xs[:, :2] = [c["xi"] for c in cs]
        words = oracle_lib.light_cases(d, np.full(n, L["index"], np.int32), p, w, np.full((n, lc.NXC), 0.5, np.float32), xs)
        fl = words.view(np.float32)
        for k, c in enumerate(cs):
            same = fl[k, 8] == np.float32(c["approx"]) and bool(words[k, 2]) == bool(c["ok"])
            if "direct_pdf" in c:
                same = same and words[k, 9] == 1 and fl[k, 17] == np.float32(c["direct_pdf"]) and (fl[k, 14:17] == np.array(c["emission"], np.float32)).all()
            elif c["ok"]:
                same = same and words[k, 9] == 0             # the reference's ray along the sampled direction missed the light
            if not same:
                differing.setdefault(L["name"], []).append(k)
    assert differing == pinned, "%s: light cases that are not the reference's: %s" % (scene, differing)
    assert sum(len(v) for v in pinned.values()) <= 0.001*total
    flat.close()


@pytest.mark.parametrize("scene,spp", [("cornell", 2048), ("materialtest", 512)])
def test_oracle_converges_to_the_unmodified_reference_binary(scene, spp, tmp_path):
    """Statistical anchor: the oracle with the counter-based stream against `tungsten -s seed`
    with its own per-tile sampler at high spp.  8x8-box-downsampled means within 5 sigma of the oracle's own
    standard error + 1% of the value; whole-image mean within 1.2%."""
    _needs_materialtest(scene)
    gold = np.load(os.path.join(G, scene + "_converged.npz"))
    ref = gold["mean"]
    mk = scenes.cornell if scene == "cornell" else scenes.materialtest
    flat = tg.FlattenedScene(mk(tmp_path, resolution=(64, 36), spp=spp))
    h, w = flat.height, flat.width
    halves = []
    for k in range(2):
        s, c = oracle_lib.render(flat.desc, w, h, k*spp//2, (k + 1)*spp//2, tg.DEFAULT_SEED)
        halves.append(s/np.maximum(c, 1)[..., None])
    flat.close()
    got = 0.5*(halves[0] + halves[1])

    def pool(a):
        return a[:32, :64].reshape(4, 8, 8, 8, 3).mean(axis=(1, 3))
    sigma = np.abs(pool(halves[0]) - pool(halves[1]))/2.0          # standard error estimate of the full render
    err = np.abs(pool(got) - pool(ref))
    assert (err <= 5*sigma + 0.01*pool(ref) + 2e-3).all(), float((err/(5*sigma + 0.01*pool(ref) + 2e-3)).max())
    assert np.allclose(got.mean(axis=(0, 1)), ref.mean(axis=(0, 1)), rtol=0.012)


def test_oracle_shards_partition_the_image(tmp_path):
    """Tile sharding (16x16 tiles round-robin, PathTraceIntegrator.cpp:27-42): shards are disjoint and their sum is
    the unsharded render, bit-exactly."""
    flat = tg.FlattenedScene(scenes.cornell(tmp_path, resolution=(80, 45), spp=2))
    whole, wc = oracle_lib.render(flat.desc, 80, 45, 0, 2, 7)
    acc, cnt = np.zeros_like(whole), np.zeros_like(wc)
    for i in range(3):
        s, c = oracle_lib.render(flat.desc, 80, 45, 0, 2, 7, shard_index=i, shard_count=3)
        assert ((c > 0) & (cnt > 0)).sum() == 0
        acc += s
        cnt += c
    flat.close()
    assert (acc == whole).all() and (cnt == wc).all() and (wc == 2).all()
