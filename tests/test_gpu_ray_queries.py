"""tghip_query_rays on the device (csrc/hip/ray_query.hip) against the CPU oracle and against tghip_trace_rays: closest hits with identical records
and identical t / u / v, occlusion bytes equal to "the oracle's closest hit exists" for EVERY ray -- no tolerance anywhere: the kernels run the
per-ray machines of tghip_trace_rays, whose operations are the oracle's in the oracle's order --, in the four kinds of scene the walks differ in;
answers that do not depend on how the rays are scheduled; the refusals; a query between two passes; torch tensors on the device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import scenes
import tungsten_amd as tg
from tungsten_amd import capi

pytestmark = pytest.mark.gpu

SCENES = ("cornell", "materialtest", "instances", "terraces")
EXTRA = 2500            # rays of each added group
INVALID, NOSCENE = capi.TGHIP_E_INVALID, capi.TGHIP_E_NOSCENE
CLOSEST, OCCLUDED, DEVICE = capi.TGHIP_QUERY_CLOSEST, capi.TGHIP_QUERY_OCCLUDED, capi.TGHIP_DEVELOP_DEVICE_POINTERS


def make_rays(flat, scene):
    """The batch of a scene and the oracle's answers to it: the rays of test_gpu_parity.py::test_trace_rays_matches_oracle_exactly (seed 5, n = 20000,
    a finite tmax on every 7th ray, three axis-parallel directions; tile_terraces: scenes.terrace_rays) + EXTRA rays that start outside the scene's
    bounds and point away from their centre (misses by geometry) + the first EXTRA oracle hits shot again with tmax = the hit's t and with
    tmax = nextafter(t, inf) (the edge of the interval, where closest and occluded must agree)."""
    d = flat.desc.contents
    lo, hi = np.array(list(d.bounds_lo)), np.array(list(d.bounds_hi))
    wide = d.num_wide_nodes > 0 and d.num_instances == 0
    rs = np.random.RandomState(5)
    if scene == "terraces":
        base = scenes.terrace_rays()
    else:
        n = 20000
        o = lo + (hi - lo)*rs.rand(n, 3)*1.2 - 0.1*(hi - lo)
        dirs = rs.randn(n, 3)
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        base = np.concatenate([o, np.full((n, 1), 1e-4), dirs, np.full((n, 1), np.inf)], axis=1).astype(np.float32)
        base[::7, 7] = 0.5*np.linalg.norm(hi - lo)      # finite tmax
        base[0:3, 4:7] = [[1, 0, 0], [0, -1, 0], [0, 0, 1]]   # axis-parallel directions (inf in 1/d)
    bhits = oracle_lib.trace_rays(flat.desc, base, wide=wide)[0]
    away = rs.randn(EXTRA, 3)
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    centre, radius = 0.5*(lo + hi), 0.5*np.linalg.norm(hi - lo)
    outside = np.concatenate([centre + away*(1.05*radius + 1e-3), np.full((EXTRA, 1), 1e-4), away, np.full((EXTRA, 1), np.inf)], axis=1).astype(np.float32)
    again = base[bhits["rec"] >= 0][:EXTRA]
    t = bhits["t"][bhits["rec"] >= 0][:EXTRA]
    assert len(again) == EXTRA
    at, past = again.copy(), again.copy()
    at[:, 7] = t
    past[:, 7] = np.nextafter(t, np.float32(np.inf))
    extra = np.concatenate([outside, at, past])
    ehits = oracle_lib.trace_rays(flat.desc, extra, wide=wide)[0]
    return np.concatenate([base, extra]), np.concatenate([bhits, ehits])


class Case(object):
    def __init__(self, scene, tmp):
        mk = {"cornell": scenes.cornell, "materialtest": scenes.materialtest, "instances": scenes.cornell_instances, "terraces": scenes.tile_terraces}[scene]
        self.path = mk(tmp, resolution=(64, 36), spp=1)
        flat = tg.FlattenedScene(self.path)
        self.rays, self.ohits = make_rays(flat, scene)
        flat.close()
        self.hit = self.ohits["rec"] >= 0
        self.renderer = None

    def r(self):
        if self.renderer is None:
            self.renderer = tg.Renderer(self.path)
        return self.renderer


_cases = {}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """One batch, one oracle run and one context per scene, shared by the tests of this file (none of them changes the batch)."""
    def get(scene):
        if scene == "materialtest" and not scenes.have_materialtest():
            pytest.skip("materialtest assets (assets/) not present")
        if scene not in _cases:
            _cases[scene] = Case(scene, tmp_path_factory.mktemp(scene))
        return _cases[scene]
    yield get
    for c in _cases.values():
        if c.renderer is not None:
            c.renderer.close()
    _cases.clear()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("scene", SCENES)
def test_queries_match_the_oracle_and_trace_rays(scene, case):
    c = case(scene)
    n = len(c.rays)
    # a condition on the inputs, checked on the oracle's answers before the device is asked: both answers are well represented
    assert c.hit.sum() >= n//8 and (~c.hit).sum() >= n//8, (int(c.hit.sum()), n)
    r = c.r()
    closest = r.query_rays(c.rays, "closest")
    occluded = r.query_rays(c.rays, "occluded")
    traced = r.trace_rays(c.rays)[0]
    print("%s: %d rays, %d oracle hits; closest differs from the oracle on %d records, from trace_rays on %d; occluded differs on %d"
          % (scene, n, int(c.hit.sum()), int((closest["rec"] != c.ohits["rec"]).sum()), int((closest["rec"] != traced["rec"]).sum()),
             int((occluded != c.hit).sum())))
    assert closest.dtype == traced.dtype and occluded.dtype == np.uint8 and occluded.shape == (n,)
    assert (closest["rec"] == c.ohits["rec"]).all()
    assert (closest["rec"] == traced["rec"]).all()
    for k in ("t", "u", "v"):
        assert same_bytes(closest[k][c.hit], c.ohits[k][c.hit]), k
        assert same_bytes(closest[k][c.hit], traced[k][c.hit]), k
    assert set(np.unique(occluded)) <= {0, 1}
    assert (occluded == c.hit.astype(np.uint8)).all()


@pytest.mark.parametrize("scene", SCENES)
def test_scheduling_never_changes_an_answer(scene, case):
    """Workgroups, claim threshold, batch size and ray order change which lane walks which ray when -- never a byte of the answers."""
    c = case(scene)
    r = c.r()
    want = {m: r.query_rays(c.rays, m) for m in ("closest", "occluded")}
    assert (want["closest"]["rec"] == c.ohits["rec"]).all()
    try:
        for blocks in (1, 0):                    # one workgroup: every lane refills about a hundred times
            r.set_option("query_blocks", blocks)
            for refill in (1, 32, 64):
                r.set_option("query_refill_at", refill)
                for m in want:
                    assert same_bytes(r.query_rays(c.rays, m), want[m]), (blocks, refill, m)
        r.set_option("query_refill_at", 0)
        for blocks in (1, 0):
            r.set_option("query_blocks", blocks)
            for n in (1, 63, 64, 65, 255, 257, 25000):
                for m in want:
                    assert same_bytes(r.query_rays(c.rays[:n], m), want[m][:n]), (blocks, n, m)
    finally:
        r.set_option("query_blocks", 0)
        r.set_option("query_refill_at", 0)
    perm = np.random.RandomState(11).permutation(len(c.rays))
    for m in want:
        assert same_bytes(r.query_rays(c.rays[perm], m), want[m][perm]), m


def test_error_paths_leave_the_context_working(case, tmp_path):
    c = case("cornell")
    r = c.r()
    ctx = r.context()
    rays = np.ascontiguousarray(c.rays[:256])
    hits, occ = np.zeros(256, r.query_rays(rays[:1]).dtype), np.zeros(256, np.uint8)

    def call(ctx_, mode=CLOSEST, flags=0, reserved=(0, 0), rays_=rays.ctypes.data, out=hits.ctypes.data, n=256, desc=True):
        d = capi.TgHipRayQueryDesc(mode, flags, (C.c_uint32*2)(*reserved))
        return tg.lib.tghip_query_rays(ctx_, C.byref(d) if desc else None, rays_, out, n)

    assert call(ctx, n=0) == 0 and call(ctx, rays_=None, out=None, n=0) == 0
    assert len(r.query_rays(np.zeros((0, 8), np.float32))) == 0 and len(r.query_rays(np.zeros((0, 8), np.float32), "occluded")) == 0
    for kw, message in ((dict(desc=False), "no description"), (dict(rays_=None), "rays and out"), (dict(out=None), "rays and out"),
                        (dict(mode=2), "unknown mode"), (dict(flags=2), "unknown flag"), (dict(reserved=(0, 1)), "reserved"),
                        (dict(n=2**31), "2^31 - 1"),
                        # (the check looks at the pointers' values only: nothing is read through these)
                        (dict(flags=DEVICE, rays_=rays.ctypes.data + 4), "16-byte aligned"),
                        (dict(flags=DEVICE, rays_=rays.ctypes.data//16*16, out=hits.ctypes.data//16*16 + 8), "16-byte aligned")):
        assert call(ctx, **kw) == INVALID, kw
        assert message in tg.lib.tghip_last_error(ctx).decode(), kw
        assert same_bytes(r.query_rays(rays), r.trace_rays(rays)[0])             # ... and the context still answers
    with pytest.raises(tg.TungstenError):
        r.query_rays(rays, mode="nearest")
    bare = tg.lib.tghip_create(0)                                                 # a context without an upload
    assert bare
    try:
        assert call(bare) == NOSCENE and call(bare, mode=OCCLUDED, out=occ.ctypes.data) == NOSCENE
        assert call(bare, mode=9) == INVALID
    finally:
        tg.lib.tghip_destroy(bare)
    got = r.query_rays(rays)
    assert (got["rec"] == c.ohits["rec"][:256]).all() and (r.query_rays(rays, "occluded") == c.hit[:256]).all()
    ms = C.c_double(-1.0)
    assert tg.lib.tghip_query_rays_kernel_time(ctx, C.byref(ms)) == 0 and ms.value > 0.0
    # the three rays of test_gpu_parity.py::test_empty_and_degenerate_ray_batches
    small = tg.Renderer(scenes.cornell(tmp_path, resolution=(16, 9), spp=1))
    three = np.array([[0, 1, 6.8, 1e-4, 0, 0, -1, 1e-3],      # tmax before anything
                      [0, 1, 6.8, 1e-4, 0, 0, 1, np.inf],     # pointing away
                      [0, 1, 6.8, 1e-4, 0, 0, -1, np.inf]], np.float32)
    h, o = small.query_rays(three), small.query_rays(three, "occluded")
    small.close()
    assert h["rec"][0] == -1 and h["rec"][1] == -1 and h["rec"][2] >= 0
    assert list(o) == [0, 0, 1]


def test_a_query_between_two_passes_leaves_the_image_alone(case, tmp_path):
    c = case("cornell")
    images = []
    for ask in (False, True):
        r = tg.Renderer(scenes.cornell(tmp_path, resolution=(64, 36), spp=2, spp_step=1, name="two_%d.json" % ask), seed=tg.DEFAULT_SEED)
        assert not r.step()
        if ask:
            assert (r.query_rays(c.rays, "closest")["rec"] == c.ohits["rec"]).all()
            assert (r.query_rays(c.rays, "occluded") == c.hit).all()
        assert r.step()
        mean, ssum, count = r.image()
        r.close()
        assert (count == 2).all()
        images.append(ssum)
    assert same_bytes(images[0], images[1])


def test_device_tensors(tmp_path):
    """query_rays_into with torch tensors on the device gives the bytes of query_rays.  In a process of its own: torch brings its own HIP runtime and
    has to be imported before this package (tests/ray_query_torch_worker.py)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ray_query_torch_worker.py")
    p = subprocess.run([sys.executable, worker, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and "RAY_QUERY_TORCH_OK" in p.stdout, p.stdout[-4000:]
