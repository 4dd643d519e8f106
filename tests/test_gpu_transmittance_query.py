"""tghip_query_transmittance on the device (csrc/hip/transmittance_query.hip): every case of the committed golden -- the reference's own
TraceBase::generalizedShadowRay, tests/transmittance_cases.py -- bit for bit; on rays outside the golden the walk restated on the host from merged
units (tghip_query_rays, tghip_query_surface, tghip_debug_medium), the occlusion query, single medium segments; batch shapes and scheduling
options; torch tensors on the device; a query between two passes; the refusals on a live context."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import medium_cases
import scenes
import surface_cases
import transmittance_cases as tc
import tungsten_amd as tg
from tungsten_amd import capi

pytestmark = pytest.mark.gpu

INVALID, NOSCENE, DEVICE = capi.TGHIP_E_INVALID, capi.TGHIP_E_NOSCENE, capi.TGHIP_DEVELOP_DEVICE_POINTERS
LOBE_FORWARD = 128
GOLDEN = tc.load_golden()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Scene(object):
    """One scene of the cases on the device, with the name tables of its file"""

    def __init__(self, name, tmp):
        self.path = tc.build_scene(name, tmp)
        self.media, self.prims = tc.names_of(self.path)
        self.renderer = tg.Renderer(self.path)

    def ask(self, g):
        """The device's answer to group g of the cases"""
        media = None
        if g["media"] is not None:
            media = np.array([-1 if m == "-" else self.media[m] for m in g["media"]], np.int32)
        return self.renderer.query_transmittance(g["rays"], media=media, medium=None if g["medium"] is None else self.media[g["medium"]],
                                                 end_cap=-1 if g["end_cap"] is None else self.prims[g["end_cap"]], bounce=g["bounce"],
                                                 starts_on_surface=g["starts"], ends_on_surface=g["ends"])

    def close(self):
        self.renderer.close()


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    tmp, made = tmp_path_factory.mktemp("transmittance"), {}

    def get(name):
        if name not in made:
            made[name] = Scene(name, tmp)
        return made[name]
    yield get
    for s in made.values():
        s.close()


# ---- 1. the device equals the reference ----

@pytest.mark.parametrize("name", sorted({g["scene"] for g in GOLDEN}))
def test_device_equals_reference(name, scene):
    s = scene(name)
    cases = 0
    for g in GOLDEN:
        if g["scene"] != name:
            continue
        got = s.ask(g)
        rgb = np.ascontiguousarray(got["rgb"]).view(np.uint32)
        off = np.nonzero((rgb != g["rgb"]).any(axis=1))[0]
        print("%s %s medium %s cap %s bounce %d flags %d%d: %d rays, %d differ, crossed %s" % (
            name, g["leg"], g["medium"], g["end_cap"], g["bounce"], g["starts"], g["ends"], len(rgb), len(off),
            "equal" if (got["crossed"] == g["crossed"]).all() else "differs"))
        for i in off[:8]:
            print("   ray %d: device %s reference %s (crossed %d, end %d)" % (i, got["rgb"][i], g["rgb"][i].view(np.float32), g["crossed"][i], g["end"][i]))
        assert len(off) == 0, (name, g["leg"])
        assert (got["crossed"] == g["crossed"].astype(np.uint32)).all(), (name, g["leg"])
        cases += len(rgb)
    assert cases > 0


# ---- 2. stepping check against merged units ----

def medium_tr(r, variant, medium, o, d, max_t, starts, ends):
    """tghip_debug_medium's `tr` word per ray for its own flag pair: [n, 3] float32"""
    cases = np.zeros(len(o), tg.MEDIUM_CASE_DTYPE)
    cases["medium"], cases["variant"], cases["p"], cases["d"], cases["max_t"], cases["wo"] = medium, variant, o, d, max_t, d
    tr = r.debug_medium(cases)["tr"]
    k = np.where(starts, 0, 2) + np.where(ends, 0, 1)          # (1,1), (1,0), (0,1), (0,0)
    return tr[np.arange(len(o)), k]


def host_walk(s, rays, medium, bounce, starts, ends, max_bounces, min_bounces):
    """generalizedShadowRay on the host for a scene whose see-through surfaces have a transparency of exactly one: the closest hit of every segment
    from tghip_query_rays, the surface from tghip_query_surface, each segment's medium factor from tghip_debug_medium, multiplied in order"""
    r = s.renderer
    flat = tg.FlattenedScene(s.path)
    T = surface_cases.Tables(flat)
    flat.close()
    variant = sorted(medium_cases.variant_masks(r, capi))[0]
    n = len(rays)
    o, tmin, d, tmax = rays[:, 0:3].copy(), rays[:, 3].copy(), rays[:, 4:7].copy(), rays[:, 7].copy()
    thr, med = np.ones((n, 3), np.float32), np.full(n, medium, np.int32)
    bnc, crossed, on_surface = np.full(n, bounce, np.int64), np.zeros(n, np.uint32), np.full(n, starts, bool)
    out = np.zeros(n, tg.TRANSMITTANCE_DTYPE)
    live = np.ones(n, bool)
    rounds = 0
    while live.any():
        rounds += 1
        i = np.nonzero(live)[0]
        seg = np.ascontiguousarray(np.column_stack([o[i], tmin[i], d[i], tmax[i]]).astype(np.float32))
        hits, surf = r.query_rays(seg, "closest"), r.query_surface(seg)
        hit = hits["rec"] >= 0
        assert (surf["rec"] == hits["rec"]).all()
        lobes = np.where(hit, T.lobes[np.maximum(surf["bsdf"], 0)], 0)
        dark = hit & ((lobes & LOBE_FORWARD) == 0)
        passing = hit & ~dark
        bnc[i[passing]] += 1
        crossed[i[passing]] += 1
        dark |= passing & (bnc[i] >= max_bounces)
        in_medium = ~dark & (med[i] >= 0)
        if in_medium.any():
            j = i[in_medium]
            far = np.where(hit[in_medium], hits["t"][in_medium], tmax[j]).astype(np.float32)
            thr[j] = thr[j]*medium_tr(r, variant, med[j], o[j], d[j], far, on_surface[j], np.full(len(j), ends, bool))
        done = dark | ~hit
        final = np.where((dark | (bnc[i] < min_bounces))[:, None], np.float32(0), thr[i])
        out["rgb"][i[done]] = final[done]
        out["crossed"][i[done]] = crossed[i[done]]
        go = i[~done]
        obj = surf["object"][~done]
        back = (surf["flags"][~done] & capi.TGHIP_SURFACE_BACK_SIDE) != 0
        inner = np.array([T.objects[k].int_medium for k in obj], np.int32)
        outer = np.array([T.objects[k].ext_medium for k in obj], np.int32)
        med[go] = np.where((inner >= 0) | (outer >= 0), np.where(back, outer, inner), med[go])
        t = hits["t"][~done]
        o[go] = o[go] + d[go]*t[:, None]                     # float32, a multiplication and an addition
        tmax[go] = tmax[go] - t
        tmin[go] = np.float32(5e-4)
        on_surface[go] = True
        live[i[done]] = False
    return out, rounds


def test_stepping_against_merged_units(scene):
    s = scene("tq_fog_smoke")
    rs = np.random.RandomState(77)
    a, b = rs.uniform((-0.95, 0.05, -0.95), (0.95, 1.9, 0.95), (384, 3)), rs.uniform((-0.95, 0.05, -0.95), (0.95, 1.9, 0.95), (384, 3))
    rays = tc._segments(a, b)
    rays[::3, 7] = np.inf
    fog = s.media["fog"]
    for starts, ends in tc.FLAG_PAIRS:
        want, rounds = host_walk(s, rays, fog, 0, starts, ends, 12, 0)
        got = s.renderer.query_transmittance(rays, medium="camera", starts_on_surface=starts, ends_on_surface=ends)
        lit = (want["rgb"] != 0).any(axis=1)
        print("flags %d%d: %d rays, %d rounds on the host, %d lit, crossed up to %d" % (starts, ends, len(rays), rounds, int(lit.sum()), int(want["crossed"].max())))
        assert same_bytes(got, want)
        assert lit.sum() >= 64 and want["crossed"].max() >= 2 and (~lit).sum() >= 64


# ---- 3. occlusion agreement ----

def rounds_of(r):
    n = C.c_uint32(0xFFFFFFFF)
    assert tg.lib.tghip_query_transmittance_rounds(r.context(), C.byref(n)) == 0
    return n.value


def test_occlusion_agreement(tmp_path):
    compared = []
    for mk, name in ((scenes.cornell, "cornell"), (scenes.cornell_instances, "instances")) + (((scenes.materialtest, "materialtest"),) if scenes.have_materialtest() else ()):
        path = mk(tmp_path, resolution=(48, 27), spp=1, name=name + "_occ.json", integrator={"min_bounces": 0})
        flat = tg.FlattenedScene(path)
        d = flat.desc.contents
        lo, hi = np.array(list(d.bounds_lo)), np.array(list(d.bounds_hi))
        plain = d.num_media == 0 and not any(d.bsdfs[i].lobes & LOBE_FORWARD for i in range(d.num_bsdfs))
        flat.close()
        if not plain:
            continue
        compared.append(name)
        rs = np.random.RandomState(5)
        o = lo + (hi - lo)*rs.rand(3000, 3)*1.2 - 0.1*(hi - lo)
        dirs = rs.randn(3000, 3)
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        rays = np.concatenate([o, np.full((3000, 1), 1e-4), dirs, np.full((3000, 1), np.inf)], axis=1).astype(np.float32)
        rays[::5, 7] = 0.3*np.linalg.norm(hi - lo)
        r = tg.Renderer(path)
        try:
            occluded = r.query_rays(rays, "occluded")
            got = r.query_transmittance(rays, medium=None)
            print("%s: %d of %d rays occluded" % (name, int(occluded.sum()), len(rays)))
            assert 300 < occluded.sum() < 2700
            assert (got["rgb"] == (1 - occluded.astype(np.float32))[:, None]).all()
            assert (got["crossed"] == 0).all()
            assert rounds_of(r) == 1
        finally:
            r.close()
    print("compared: %s" % compared)
    assert "cornell" in compared and "instances" in compared


def test_rounds_of_the_last_call(scene):
    """tghip_query_transmittance_rounds: 1 + the most crossings behind which a ray of the batch went on -- one round where every ray ends at once"""
    s = scene("tq_stack")
    for g in GOLDEN:
        if g["scene"] == "tq_stack":
            got = s.ask(g)
            assert rounds_of(s.renderer) == 1 + int(got["crossed"].max()), g["leg"]           # (max_bounces = 64 ends no ray here)
    assert {int(g["crossed"].max()) for g in GOLDEN if g["scene"] == "tq_stack"} >= {0, 1, 4}
    s = scene("tq_stack_mb3")
    g = next(g for g in GOLDEN if g["scene"] == "tq_stack_mb3" and g["bounce"] == 0)
    assert s.ask(g)["crossed"].max() == 3 and rounds_of(s.renderer) == 3                       # (the third crossing ends at max_bounces = 3)
    assert tg.lib.tghip_query_transmittance_rounds(s.renderer.context(), None) == INVALID
    assert tg.lib.tghip_query_transmittance_rounds(None, C.byref(C.c_uint32(0))) == INVALID


# ---- 4. pure medium segments ----

@pytest.mark.parametrize("name", ["tq_fog", "tq_expfog", "tq_atmosphere", "tq_davis_weinstein", "tq_interpolated", "tq_gas_linear", "tq_gas_pulse"])
def test_pure_medium_segments(name, scene):
    s = scene(name)
    rs = np.random.RandomState(21)
    if name.startswith("tq_gas"):
        medium = s.media["gas1" if name == "tq_gas_linear" else "gas4"]
        a, b = tc._box(rs, 128, (-2.0, 0.45, 0.2), (-0.2, 0.8, 0.9)), tc._box(rs, 128, (-2.0, 0.45, 0.2), (-0.2, 0.8, 0.9))
        rays = tc._segments(a, b)
    else:
        medium = s.media["fog"]
        rays = tc.miss_rays(rs, 128)
        rays[::2, 7] = rs.uniform(0.05, 3.0, 64)
    variant = sorted(medium_cases.variant_masks(s.renderer, capi))[0]
    assert (s.renderer.query_rays(rays, "closest")["rec"] < 0).all()
    for starts, ends in tc.FLAG_PAIRS:
        want = medium_tr(s.renderer, variant, medium, rays[:, 0:3], rays[:, 4:7], rays[:, 7], np.full(128, starts, bool), np.full(128, ends, bool))
        got = s.renderer.query_transmittance(rays, medium=medium, starts_on_surface=starts, ends_on_surface=ends)
        assert same_bytes(np.ascontiguousarray(got["rgb"]), np.ascontiguousarray(want)), (name, starts, ends)
        assert (got["crossed"] == 0).all()
        per_ray = s.renderer.query_transmittance(rays, media=np.full(128, medium, np.int32), medium=None, starts_on_surface=starts, ends_on_surface=ends)
        assert same_bytes(per_ray, got)


# ---- 5. batch shapes and scheduling ----

def test_batch_shapes(scene):
    s = scene("tq_stack_mb3")
    r = s.renderer
    rs = np.random.RandomState(9)
    rays = np.concatenate([tc.stack_rays(rs, 400), tc.stack_rays(rs, 100, infinite=True), tc.cutout_rays(rs, 100), tc.blocked_rays(rs, 50)])
    rays = rays[rs.permutation(len(rays))]
    full = r.query_transmittance(rays, medium=None)
    assert full["crossed"].max() == 3 and ((full["rgb"] != 0).any(axis=1) & (full["crossed"] == 2)).sum() >= 16
    for n in (0, 1, 63, 64, 65, 257, len(rays)):
        got = r.query_transmittance(rays[:n], medium=None)
        assert same_bytes(got, full[:n]), n
    # every ray ends in round 0
    first = np.nonzero(full["crossed"] == 0)[0]
    assert len(first) >= 64
    assert same_bytes(r.query_transmittance(rays[first], medium=None), full[first])
    # exactly one ray reaches the last round max_bounces = 3 allows: its third closest-hit walk
    last = np.nonzero((full["crossed"] >= 2) & (full["rgb"] != 0).any(axis=1))[0][:1]
    for at in (0, len(first)//2, len(first)):
        pick = np.concatenate([first[:at], last, first[at:]])
        assert same_bytes(r.query_transmittance(rays[pick], medium=None), full[pick]), at
    # the walk's options at their extremes
    try:
        for blocks in (1, 0, 4096):
            r.set_option("query_blocks", blocks)
            for refill in (1, 64, 0):
                r.set_option("query_refill_at", refill)
                assert same_bytes(r.query_transmittance(rays, medium=None), full), (blocks, refill)
    finally:
        r.set_option("query_blocks", 0)
        r.set_option("query_refill_at", 0)
    perm = rs.permutation(len(rays))
    assert same_bytes(r.query_transmittance(rays[perm], medium=None), full[perm])


def test_options_and_batch_sizes_on_instances(scene):
    for s, rays in [(scene("tq_instances"), next(g for g in GOLDEN if g["scene"] == "tq_instances")["rays"])]:
        r = s.renderer
        full = r.query_transmittance(rays, medium=None)
        try:
            for blocks, refill in ((1, 1), (1, 64), (0, 1), (0, 64)):
                r.set_option("query_blocks", blocks)
                r.set_option("query_refill_at", refill)
                assert same_bytes(r.query_transmittance(rays, medium=None), full), (blocks, refill)
        finally:
            r.set_option("query_blocks", 0)
            r.set_option("query_refill_at", 0)
        for n in (1, 65, 257):
            assert same_bytes(r.query_transmittance(rays[:n], medium=None), full[:n])


@pytest.mark.skipif(not scenes.have_materialtest(), reason="materialtest assets (assets/) not present")
def test_the_wide_walk_against_the_host_walk(tmp_path):
    """materialtest walks the 8-wide BVH: the device against the host walk of test 2 on a variant with a forward boundary across the scene at half its height"""
    def edit(scene):
        scene["bsdfs"].append({"name": "gate", "type": "forward", "albedo": 1})
        scene["primitives"].append({"name": "gate", "type": "quad", "bsdf": "gate", "transform": {"position": [0, 0.6, 0], "scale": [10, 1, 10]}})
    path = scenes.materialtest(tmp_path, resolution=(48, 27), spp=1, name="materialtest_gate.json", edit=edit)
    flat = tg.FlattenedScene(path)
    d = flat.desc.contents
    lo, hi = np.array(list(d.bounds_lo)), np.array(list(d.bounds_hi))
    wide, max_bounces, min_bounces = d.num_wide_nodes > 0, d.settings.max_bounces, d.settings.min_bounces
    flat.close()
    rs = np.random.RandomState(3)
    rays = tc._segments(rs.uniform(lo, hi, (600, 3)), rs.uniform(lo, hi, (600, 3)))
    rays[::4, 7] = np.inf

    class S(object):
        pass
    s = S()
    s.path, s.renderer = path, tg.Renderer(path)
    try:
        print("materialtest: wide nodes %s" % wide)
        want, rounds = host_walk(s, rays, -1, 0, False, False, max_bounces, min_bounces)
        got = s.renderer.query_transmittance(rays, medium=None)
        print("%d rounds, %d lit, crossed up to %d" % (rounds, int((want["rgb"] != 0).any(axis=1).sum()), int(want["crossed"].max())))
        assert same_bytes(got, want)
        assert want["crossed"].max() >= 1
    finally:
        s.renderer.close()


# ---- 6. device pointers ----

def test_device_tensors(tmp_path):
    """query_transmittance_into with torch tensors on the device gives the bytes of query_transmittance and writes nothing outside the n entries.
    In a process of its own: torch brings its own HIP runtime and has to be imported before this package."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "transmittance_query_torch_worker.py")
    p = subprocess.run([sys.executable, worker, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and "TRANSMITTANCE_QUERY_TORCH_OK" in p.stdout, p.stdout[-4000:]


# ---- 7. a query between two passes ----

def test_a_query_between_two_passes_leaves_the_context_alone(tmp_path):
    """Samples [0, 8) of a fresh context as the passes [0, 4) and [4, 8), with and without a query between them: image, counts, auxiliary buffers and
    records byte for byte."""
    path = tc.build_scene("tq_fog", tmp_path)
    g = next(g for g in GOLDEN if g["scene"] == "tq_fog")
    w, h = tc.SMALL["resolution"]
    state = {}
    for ask in (False, True):
        r = tg.Renderer(path, seed=tg.DEFAULT_SEED)
        ctx, n = r.context(), w*h
        records = np.zeros(((w + 3)//4)*((h + 3)//4), surface_cases.oracle_lib.DEVICE_RECORD_DTYPE)
        records["sample_count"] = np.arange(records.size)              # (these passes keep no records: a pattern the query must leave as it is)
        records["mean"] = 0.25*np.arange(records.size)
        assert tg.lib.tghip_upload_records(ctx, records.ctypes.data, records.size) == 0
        for k, (lo, hi) in enumerate(((0, 4), (4, 8))):
            p = tg.TgHipPassDesc(lo, hi, tg.DEFAULT_SEED, 0, 1, capi.TGHIP_PASS_AUX)
            assert tg.lib.tghip_render_pass(ctx, C.byref(p)) == 0 and tg.lib.tghip_wait(ctx) == 0, tg.lib.tghip_last_error(ctx)
            if ask and k == 0:
                got = r.query_transmittance(g["rays"], medium="camera", starts_on_surface=g["starts"], ends_on_surface=g["ends"])
                assert same_bytes(np.ascontiguousarray(got["rgb"]).view(np.uint32), g["rgb"])
        ssum, count = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
        aux = np.zeros(n, tg.AUX_DTYPE)
        rec = np.zeros_like(records)
        assert tg.lib.tghip_download_framebuffer(ctx, ssum.ctypes.data, count.ctypes.data, n) == 0
        assert tg.lib.tghip_download_aux(ctx, aux.ctypes.data, n) == 0
        assert tg.lib.tghip_download_records(ctx, rec.ctypes.data, rec.size) == 0
        r.close()
        assert (count == 8).all() and same_bytes(rec, records)
        state[ask] = (ssum, count, aux, rec)
    for x, y in zip(state[False], state[True]):
        assert same_bytes(x, y)


# ---- 8. refusals on a live context ----

def test_refusals_leave_the_context_working(scene):
    s = scene("tq_interpolated")
    r = s.renderer
    ctx = r.context()
    g = next(g for g in GOLDEN if g["scene"] == "tq_interpolated")
    rays = np.ascontiguousarray(g["rays"])
    n = len(rays)
    fog = s.media["fog"]
    out = np.zeros(n, tg.TRANSMITTANCE_DTYPE)
    flags = (2 if g["starts"] else 0) | (4 if g["ends"] else 0)

    def call(ctx_, flags_=flags, medium=fog, end_cap=-1, bounce=0, reserved=(0, 0, 0, 0), rays_=rays.ctypes.data, media=None, out_=out.ctypes.data, n_=n, desc=True):
        d = capi.TgHipTransmittanceQueryDesc(flags_, medium, end_cap, bounce, (C.c_uint32*4)(*reserved))
        return tg.lib.tghip_query_transmittance(ctx_, C.byref(d) if desc else None, rays_, media, out_, n_)

    def answers():
        got = s.ask(g)
        return same_bytes(np.ascontiguousarray(got["rgb"]).view(np.uint32), g["rgb"])

    assert call(ctx, n_=0) == 0 and call(ctx, rays_=None, out_=None, n_=0) == 0
    assert len(r.query_transmittance(np.zeros((0, 8), np.float32))) == 0
    num_objects = len(s.prims)
    for kw, message in ((dict(desc=False), "no description"), (dict(rays_=None), "rays and out"), (dict(out_=None), "rays and out"),
                        (dict(flags_=8), "unknown flag"), (dict(reserved=(0, 0, 0, 1)), "reserved"), (dict(n_=2**31), "2^31 - 1"),
                        (dict(medium=-3), "medium index"), (dict(medium=fog + 3), "medium index"),
                        (dict(medium=fog + 1), "operand"), (dict(medium=fog + 2), "operand"),
                        (dict(end_cap=-2), "end cap"), (dict(end_cap=num_objects), "end cap"), (dict(bounce=256), "bounce"),
                        # (the check looks at the pointers' values only: nothing is read through these)
                        (dict(flags_=DEVICE, rays_=rays.ctypes.data//16*16 + 4, out_=out.ctypes.data//16*16), "16-byte aligned"),
                        (dict(flags_=DEVICE, rays_=rays.ctypes.data//16*16, out_=out.ctypes.data//16*16 + 8), "16-byte aligned"),
                        (dict(flags_=DEVICE, rays_=rays.ctypes.data//16*16, out_=out.ctypes.data//16*16, media=rays.ctypes.data//16*16 + 2), "4-byte aligned")):
        assert call(ctx, **kw) == INVALID, kw
        assert message in tg.lib.tghip_last_error(ctx).decode(), kw
        assert answers()                                                    # ... and the context still answers
    inst = scene("tq_instances")
    d = capi.TgHipTransmittanceQueryDesc(0, -1, inst.prims["swarm"], 0)
    assert tg.lib.tghip_query_transmittance(inst.renderer.context(), C.byref(d), rays.ctypes.data, None, out.ctypes.data, n) == INVALID
    assert "instances" in tg.lib.tghip_last_error(inst.renderer.context()).decode()
    bare = tg.lib.tghip_create(0)                                           # a context without an upload
    assert bare
    try:
        assert call(bare, medium=-1) == NOSCENE
        assert call(bare, desc=False) == INVALID
    finally:
        tg.lib.tghip_destroy(bare)
    # per-ray start media out of range: an unspecified answer for those rays, the others as they are, and the call returns
    media = np.full(n, fog, np.int32)
    media[::2] = 1000
    media[1] = -1000
    got = r.query_transmittance(rays, media=media, medium=fog, starts_on_surface=g["starts"], ends_on_surface=g["ends"])
    keep = np.arange(n) % 2 == 1
    keep[1] = False
    assert same_bytes(np.ascontiguousarray(got["rgb"]).view(np.uint32)[keep], g["rgb"][keep])
    # rays that are not finite, or have no direction
    bad = rays.copy()
    bad[0, 0], bad[1, 4:7], bad[2, 5], bad[3, 7] = np.nan, 0.0, np.inf, np.nan
    r.query_transmittance(bad, medium=fog)
    assert answers()
    assert call(ctx) == 0 and same_bytes(np.ascontiguousarray(out["rgb"]).view(np.uint32), g["rgb"])
    ms = C.c_double(-1.0)
    assert tg.lib.tghip_query_transmittance_kernel_time(ctx, C.byref(ms)) == 0 and ms.value > 0.0
