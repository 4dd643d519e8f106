"""tghip_query_direct on the device (csrc/hip/direct_query.hip): every group of the committed golden -- the reference's own TraceBase::estimateDirect
and volumeEstimateDirect, tests/direct_cases.py -- bit for bit; against the device's own render loop on the camera's rays of two-bounce scenes; the
hit against tghip_query_surface; a fixed light in a one-light scene; batch shapes and scheduling options; a query between two passes; torch tensors
on the device; the refusals on a live context."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import direct_cases as dc
import oracle_lib
import scenes
import tungsten_amd as tg
from tungsten_amd import capi
from test_gpu_radiance_query import camera_rays

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, NOSCENE, DEVICE, VOLUME = (capi.TGHIP_E_INVALID, capi.TGHIP_E_UNSUPPORTED, capi.TGHIP_E_NOSCENE, capi.TGHIP_DEVELOP_DEVICE_POINTERS,
                                                 capi.TGHIP_DIRECT_VOLUME)
LOBE_SPECULAR, LOBE_FORWARD = 16 | 32, 128
GOLDEN = dc.load_golden()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Scene(object):
    """One scene of the cases on the device, with the name tables of its file"""

    def __init__(self, name, tmp):
        self.path = dc.build_scene(name, tmp)
        self.media, self.prims = dc.names_of(self.path)
        self.lights = dc.light_slots(self.path)
        self.renderer = tg.Renderer(self.path)

    def params(self, g):
        media = None
        if g["media"] is not None:
            media = np.array([-1 if m == "-" else self.media[m] for m in g["media"]], np.int32)
        return dict(spp=tuple(g["spp"]), seed=g["seed"], media=media, medium=None if g["medium"] is None else self.media[g["medium"]], bounce=g["bounce"],
                    light=-1 if g["light_name"] is None else self.lights[g["light_name"]], skip=g["skip"], volume=g["volume"])

    def ask(self, g, n=None):
        """The device's answer to group g of the cases (its first n rays)"""
        kw = self.params(g)
        if n is not None and kw["media"] is not None:
            kw["media"] = kw["media"][:n]
        return self.renderer.query_direct(g["rays"] if n is None else g["rays"][:n], **kw)

    def close(self):
        self.renderer.close()


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    tmp, made = tmp_path_factory.mktemp("direct"), {}

    def get(name):
        if name not in made:
            made[name] = Scene(name, tmp)
        return made[name]
    yield get
    for s in made.values():
        s.close()


def group(leg):
    return next(g for g in GOLDEN if g["leg"] == leg)


# ---- 1. the device equals the reference, 3. the hit is tghip_query_surface's ----

@pytest.mark.parametrize("name", sorted({g["scene"] for g in GOLDEN}))
def test_device_equals_reference(name, scene):
    """Every word of rgb, visibility, count and visibility_count: the reference's per-sample values summed in float32 in sample order, from zero.
    rec is tghip_query_surface's for every ray; a miss is all zero."""
    s = scene(name)
    items = 0
    for g in GOLDEN:
        if g["scene"] != name:
            continue
        got = s.ask(g)
        rgb, vis, count, vcount = dc.expected(g)
        off = np.nonzero((np.ascontiguousarray(got["rgb"]).view(np.uint32) != rgb.view(np.uint32)).any(axis=1))[0]
        voff = np.nonzero(got["visibility"].view(np.uint32) != vis.view(np.uint32))[0]
        print("%s %s: %d rays x %d, rgb differs on %d, visibility on %d, counts %s" % (
            name, g["leg"], len(rgb), g["taken"].shape[1], len(off), len(voff),
            "equal" if (got["count"] == count).all() and (got["visibility_count"] == vcount).all() else "differ"))
        for i in off[:8]:
            print("   ray %d: device %s reference %s (legs %s, light %s)" % (i, got["rgb"][i], rgb[i], g["legs"][i], g["light"][i]))
        for i in voff[:8]:
            print("   ray %d: device visibility %r / %d reference %r / %d" % (i, got["visibility"][i], got["visibility_count"][i], vis[i], vcount[i]))
        assert len(off) == 0 and len(voff) == 0, (name, g["leg"])
        assert (got["count"] == count).all() and (got["visibility_count"] == vcount).all(), (name, g["leg"])
        assert (got["reserved"] == 0).all()
        if g["volume"]:
            assert (got["rec"] == -1).all()
        else:
            surf = s.renderer.query_surface(g["rays"])
            assert (got["rec"] == surf["rec"]).all(), (name, g["leg"])
            miss = surf["rec"] < 0
            assert (got["rec"][miss] == -1).all()
            zero = np.zeros(int(miss.sum()), tg.DIRECT_DTYPE)
            zero["rec"] = -1
            assert same_bytes(np.ascontiguousarray(got[miss]), zero)
        items += g["taken"].size
    assert items > 0


# ---- 2. the device's own render loop ----

@pytest.mark.parametrize("name, edit", [("cornell", None), ("two_lights", scenes._two_lights), ("area_lights", scenes._area_lights)])
def test_two_bounce_radiance_is_the_direct_light(name, edit, tmp_path):
    """With max_bounces = 2 a camera path adds nothing but the camera vertex' estimateDirect to a pixel whose first hit neither emits nor has a specular
    or forward lobe: tghip_query_radiance on the camera's own rays is tghip_query_direct behind the three numbers the path draws first -- the two filter
    numbers and handleSurface's transparency boolean (TraceBase.cpp:529)."""
    def two_bounces(scene):
        if edit:
            edit(scene)
        scene["integrator"]["max_bounces"] = 2
        assert "medium" not in scene["camera"]
    w, h = 16, 9
    path = scenes.cornell(tmp_path, name=name + "_mb2.json", resolution=(w, h), spp=4, edit=two_bounces)
    flat = tg.FlattenedScene(path)
    rays = camera_rays(flat, w, h, tg.DEFAULT_SEED, 0)
    d = flat.desc.contents
    lobes = np.array([d.bsdfs[i].lobes for i in range(d.num_bsdfs)], np.uint32)
    assert d.settings.max_bounces == 2
    flat.close()
    r = tg.Renderer(path, seed=tg.DEFAULT_SEED)
    try:
        surf = r.query_surface(rays)
        hit = (surf["flags"] & capi.TGHIP_SURFACE_HIT) != 0
        ok = hit & ((surf["flags"] & capi.TGHIP_SURFACE_EMISSIVE) == 0)
        ok[hit] &= (lobes[surf["bsdf"][hit]] & (LOBE_SPECULAR | LOBE_FORWARD)) == 0
        assert ok.sum()*2 >= len(rays), (name, int(ok.sum()))
        ssum, count = r.query_radiance(rays, 0, 4, seed=tg.DEFAULT_SEED)
        got = r.query_direct(rays, spp=(0, 4), seed=tg.DEFAULT_SEED, medium=None, bounce=1, skip=3)
        print("%s: %d of %d rays qualify, %d of them lit" % (name, int(ok.sum()), len(rays), int((ssum[ok] != 0).any(axis=1).sum())))
        assert (got["rgb"][ok] == ssum[ok]).all()
        assert (got["count"][ok] == count[ok]).all() and (count[ok] == 4).all()
        assert (ssum[ok] != 0).any()
    finally:
        r.close()


# ---- 4. a fixed light in a one-light scene ----

def test_slot_0_of_a_one_light_scene_is_chooselight(scene):
    s, g = scene("dq_box"), group("box")
    assert len(s.lights) == 1
    assert same_bytes(s.renderer.query_direct(g["rays"], spp=(0, 3), seed=g["seed"], medium=None, light=0),
                      s.renderer.query_direct(g["rays"], spp=(0, 3), seed=g["seed"], medium=None, light=-1))


# ---- 5. batch shapes and memory, 6. options ----

def test_batch_shapes(scene):
    s, g = scene("dq_panes"), group("under_panes")
    rs = np.random.RandomState(5)
    rays = np.ascontiguousarray(np.concatenate([g["rays"], group("at_panes")["rays"], dc.into_box(rs, 4097 - 256)]))
    assert len(rays) == 4097
    r = s.renderer
    full = r.query_direct(rays, spp=(1, 3), seed=9, medium=None)
    assert (full["rgb"] != 0).any(axis=1).sum() > 500 and (full["count"] == 2).sum() > 4000
    for n in (0, 1, 63, 64, 65):
        assert same_bytes(r.query_direct(rays[:n], spp=(1, 3), seed=9, medium=None), full[:n]), n
    assert same_bytes(r.query_direct(rays, spp=(1, 3), seed=9, medium=None), full)                     # two identical calls
    # the samples of a call are the samples of its halves, added in order
    a, b = r.query_direct(rays[:65], spp=(1, 2), seed=9, medium=None), r.query_direct(rays[:65], spp=(2, 3), seed=9, medium=None)
    assert same_bytes((a["rgb"] + b["rgb"]).astype(np.float32), full["rgb"][:65]) and (a["count"] + b["count"] == full["count"][:65]).all()


@pytest.mark.parametrize("name, leg", [("dq_panes", "under_panes"), ("dq_instances", "instances"), ("dq_caps", "volume_caps")])
def test_options_change_no_byte(name, leg, scene):
    s, g = scene(name), group(leg)
    r = s.renderer
    full = s.ask(g)
    try:
        for blocks in (1, 0):
            r.set_option("query_blocks", blocks)
            for refill in (1, 64):
                r.set_option("query_refill_at", refill)
                assert same_bytes(s.ask(g), full), (blocks, refill)
    finally:
        r.set_option("query_blocks", 0)
        r.set_option("query_refill_at", 0)
    assert same_bytes(s.ask(g), full)
    assert same_bytes(s.ask(g, 65), full[:65])


def test_queries_that_share_scratch_leave_nothing_stale(scene):
    """tghip_query_transmittance and tghip_query_direct stage a caller's host arrays in the same device scratch, the answers and the per-ray start
    media: a transmittance query of 129 rays, a direct query of 65 with other media, the transmittance query again, on one context -- each answer is
    the bytes of the same call on a context that has answered nothing else."""
    s, g = scene("dq_fog_smoke"), group("media_per_ray")
    kw = s.params(g)
    at = np.arange(129) % len(g["rays"])
    rays, media = np.ascontiguousarray(g["rays"][at]), np.ascontiguousarray(kw["media"][at])
    short = rays.copy()
    short[:, 7] = 0.25                               # (segments that mostly end in the medium they start in, not on a wall)

    def transmittance(r):
        return r.query_transmittance(short, media=media)

    def direct(r):
        return r.query_direct(rays[:65], **dict(kw, media=np.ascontiguousarray(media[::-1][:65])))

    got = [transmittance(s.renderer), direct(s.renderer), transmittance(s.renderer)]
    want = []
    for call in (transmittance, direct):
        fresh = tg.Renderer(s.path)
        try:
            want.append(call(fresh))
        finally:
            fresh.close()
    print("transmittance: %d of 129 rays let light through, %d different answers; direct: %d of 65 rays lit"
          % ((got[0]["rgb"] > 0).any(axis=1).sum(), len(np.unique(got[0]["rgb"], axis=0)), (got[1]["rgb"] != 0).any(axis=1).sum()))
    assert same_bytes(got[0], want[0]) and same_bytes(got[1], want[1]) and same_bytes(got[2], want[0])
    assert (got[0]["rgb"] > 0).any() and (got[1]["count"] > 0).any()


@pytest.mark.skipif(not scenes.have_materialtest(), reason="materialtest assets (assets/) not present")
def test_the_wide_walk(tmp_path):
    """materialtest walks the 8-wide BVH: prefixes, repeated calls and the walk's options give the same bytes there too"""
    path = scenes.materialtest(tmp_path, resolution=(16, 9), spp=1, name="materialtest_dq.json")
    flat = tg.FlattenedScene(path)
    base = camera_rays(flat, 16, 9, tg.DEFAULT_SEED, 0)
    flat.close()
    r = tg.Renderer(path)
    try:
        full = r.query_direct(base, spp=(0, 5), seed=3, medium=None)
        assert (full["rgb"] != 0).any(axis=1).sum() > len(base)//4
        assert same_bytes(r.query_direct(base[:65], spp=(0, 5), seed=3, medium=None), full[:65])
        r.set_option("query_blocks", 1)
        r.set_option("query_refill_at", 1)
        assert same_bytes(r.query_direct(base, spp=(0, 5), seed=3, medium=None), full)
    finally:
        r.close()


def test_a_large_call_runs_in_parts(scene):
    """More (ray, sample) items than are under way at once (2^20): the call runs in parts, whole rays where a ray's samples fit, runs of a ray's
    samples where they do not, and no part changes a bit: a ray's answer is that of a small call, a long run of samples goes on from the sum of
    its beginning one sample at a time."""
    s, g = scene("dq_box"), group("box")
    r = s.renderer
    # 8192 rays x 150 samples: ray 0 of the large call is ray 0 of a call of one ray (the other rays have other indices, so other numbers)
    many = np.ascontiguousarray(np.tile(g["rays"][:1], (8192, 1)))
    big = r.query_direct(many, spp=(0, 150), seed=3, medium=None)
    one = r.query_direct(g["rays"][:1], spp=(0, 150), seed=3, medium=None)
    assert one["count"][0] == 150 and (one["rgb"] != 0).any()
    assert same_bytes(big[:1], one) and (big["count"] == 150).all()
    last = r.query_direct(many[-3:], spp=(0, 150), seed=3, medium=None)       # (the last rays of the second part, as rays 0..2 of a small call: other streams)
    assert (last["count"] == 150).all()
    # one ray, 2^20 + 5 samples: the first 2^20 in one part, the rest in a second that goes on from its sums
    N = 1 << 20
    whole = r.query_direct(g["rays"][:1], spp=(0, N + 5), seed=3, medium=None)
    head = r.query_direct(g["rays"][:1], spp=(0, N), seed=3, medium=None)
    rgb, vis, vcount = head["rgb"][0].copy(), head["visibility"][0].copy(), int(head["visibility_count"][0])
    for k in range(N, N + 5):
        x = r.query_direct(g["rays"][:1], spp=(k, k + 1), seed=3, medium=None)
        rgb = (rgb + x["rgb"][0]).astype(np.float32)
        if x["visibility_count"][0]:
            vis, vcount = np.float32(vis + x["visibility"][0]), vcount + 1
    assert whole["count"][0] == N + 5 and whole["visibility_count"][0] == vcount
    assert whole["rgb"][0].tobytes() == rgb.tobytes() and np.float32(whole["visibility"][0]).tobytes() == np.float32(vis).tobytes()


# ---- 7. a query between two passes ----

def test_a_query_between_two_passes_leaves_the_context_alone(tmp_path):
    """Samples [0, 8) of a fresh context as the passes [0, 4) and [4, 8), with and without a query between them: image, counts, auxiliary buffers and
    records byte for byte."""
    path = dc.build_scene("dq_caps", tmp_path)
    g = group("caps")
    w, h = dc.SMALL["resolution"]
    media, _ = dc.names_of(path)
    state = {}
    for ask in (False, True):
        r = tg.Renderer(path, seed=tg.DEFAULT_SEED)
        ctx, n = r.context(), w*h
        records = np.zeros(((w + 3)//4)*((h + 3)//4), oracle_lib.DEVICE_RECORD_DTYPE)
        records["sample_count"] = np.arange(records.size)              # (these passes keep no records: a pattern the query must leave as it is)
        records["mean"] = 0.25*np.arange(records.size)
        assert tg.lib.tghip_upload_records(ctx, records.ctypes.data, records.size) == 0
        for k, (lo, hi) in enumerate(((0, 4), (4, 8))):
            p = tg.TgHipPassDesc(lo, hi, tg.DEFAULT_SEED, 0, 1, capi.TGHIP_PASS_AUX)
            assert tg.lib.tghip_render_pass(ctx, C.byref(p)) == 0 and tg.lib.tghip_wait(ctx) == 0, tg.lib.tghip_last_error(ctx)
            if ask and k == 0:
                got = r.query_direct(g["rays"], spp=tuple(g["spp"]), seed=g["seed"], medium=media["fog"])
                assert same_bytes(np.ascontiguousarray(got["rgb"]), dc.expected(g)[0])
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


# ---- 8. device pointers ----

def test_device_tensors(tmp_path):
    """query_direct_into with torch tensors on the device gives the bytes of query_direct and writes nothing outside the n entries.  In a process of
    its own: torch brings its own HIP runtime and has to be imported before this package."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "direct_query_torch_worker.py")
    p = subprocess.run([sys.executable, worker, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and "DIRECT_QUERY_TORCH_OK" in p.stdout, p.stdout[-4000:]


# ---- 9. refusals on a live context ----

def test_refusals_leave_the_context_working(scene):
    s, g = scene("dq_caps"), group("caps")
    r = s.renderer
    ctx = r.context()
    rays = np.ascontiguousarray(g["rays"])
    n = len(rays)
    fog, lights = s.media["fog"], len(s.lights)
    out = np.zeros(n, tg.DIRECT_DTYPE)
    want = dc.expected(g)[0]

    def call(ctx_, flags=0, seed=g["seed"], spp=tuple(g["spp"]), medium=fog, bounce=1, light=-1, skip=0, rays_=rays.ctypes.data, media=None,
             out_=out.ctypes.data, n_=n, desc=True):
        d = capi.TgHipDirectQueryDesc(flags, seed, spp[0], spp[1], medium, bounce, light, skip)
        return tg.lib.tghip_query_direct(ctx_, C.byref(d) if desc else None, rays_, media, out_, n_)

    def answers():
        return same_bytes(np.ascontiguousarray(s.ask(g)["rgb"]), want)

    assert call(ctx, n_=0) == 0 and call(ctx, rays_=None, out_=None, n_=0) == 0
    assert len(r.query_direct(np.zeros((0, 8), np.float32), medium=fog)) == 0
    assert call(ctx, skip=1024) == 0 and call(ctx, light=lights - 1) == 0
    for kw, message in ((dict(desc=False), "no description"), (dict(rays_=None), "rays and out"), (dict(out_=None), "rays and out"),
                        (dict(flags=4), "unknown flag"), (dict(n_=2**31), "2^31 - 1"), (dict(medium=-3), "medium index"), (dict(medium=fog + 1), "medium index"),
                        (dict(spp=(3, 3)), "spp_end"), (dict(spp=(4, 1)), "spp_end"), (dict(skip=1025), "skip"), (dict(light=-2), "light outside"),
                        (dict(light=lights), "light outside"), (dict(bounce=256), "bounce"),
                        (dict(flags=VOLUME, medium=capi.TGHIP_MEDIUM_NONE), "volume mode needs a medium"),
                        # (the check looks at the pointers' values only: nothing is read through these)
                        (dict(flags=DEVICE, rays_=rays.ctypes.data//16*16 + 4, out_=out.ctypes.data//16*16), "16-byte aligned"),
                        (dict(flags=DEVICE, rays_=rays.ctypes.data//16*16, out_=out.ctypes.data//16*16 + 8), "16-byte aligned"),
                        (dict(flags=DEVICE, rays_=rays.ctypes.data//16*16, out_=out.ctypes.data//16*16, media=rays.ctypes.data//16*16 + 2), "4-byte aligned")):
        assert call(ctx, **kw) == INVALID, kw
        assert message in tg.lib.tghip_last_error(ctx).decode(), kw
        assert answers()                                                    # ... and the context still answers
    assert call(ctx, spp=(0, 2**31), n_=2) == UNSUPPORTED and "2^32" in tg.lib.tghip_last_error(ctx).decode()
    assert answers()
    box = scene("dq_box")                                                   # the camera of this scene is in no medium
    d = capi.TgHipDirectQueryDesc(VOLUME, 1, 0, 1, capi.TGHIP_MEDIUM_OF_CAMERA, 1, -1, 0)
    assert tg.lib.tghip_query_direct(box.renderer.context(), C.byref(d), rays.ctypes.data, None, out.ctypes.data, n) == INVALID
    bare = tg.lib.tghip_create(0)                                           # a context without an upload
    assert bare
    try:
        assert call(bare, medium=-1) == NOSCENE
        assert call(bare, desc=False) == INVALID
    finally:
        tg.lib.tghip_destroy(bare)
    assert call(ctx) == 0 and same_bytes(np.ascontiguousarray(out["rgb"]), want)
    ms = C.c_double(-1.0)
    assert tg.lib.tghip_query_direct_kernel_time(ctx, C.byref(ms)) == 0 and ms.value > 0.0
