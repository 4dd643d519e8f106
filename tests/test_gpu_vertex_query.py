"""tghip_query_vertex on the device (csrc/hip/vertex_query.hip): caller-held paths advanced turn by turn until none is alive return the reference's own
per-sample goldens and tghip_query_radiance's answer, float32 == in every channel of every ray, no tolerance and no ray left out; every path has then
drawn as many numbers as the oracle's; the first turn is tghip_query_rays' hit and tghip_query_direct's estimate; a TgHipPath is the whole state
(reordered, thinned and split batches give the same bytes); scheduling options, parts of a large call, other queries on the same context and passes
around the call change nothing; the refusals; torch tensors on the device.  tests/test_vertex_query_cpu.py checks, without a device, the facts about
the goldens and the oracle used here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import scenes
import tungsten_amd as tg
import vertex_cases as vc
from tungsten_amd import capi
from test_gpu_radiance_query import CAMERA_CASES, camera_rays

pytestmark = pytest.mark.gpu

INVALID, NOSCENE = capi.TGHIP_E_INVALID, capi.TGHIP_E_NOSCENE
DEVICE, START = capi.TGHIP_DEVELOP_DEVICE_POINTERS, capi.TGHIP_VERTEX_START
ESCAPED, MAX_BOUNCES, ABSORBED, ZERO_THROUGHPUT, ROULETTE, NAN = range(1, 7)
LOBE_SPECULAR, LOBE_FORWARD = 16 | 32, 128


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def chain(r, rays, **kw):
    """start_paths with one turn, then query_vertex turn by turn until no path is alive -> (paths, turns)"""
    paths, alive = r.start_paths(rays, turns=1, **kw)
    turns = 1
    while alive:
        assert alive == int((paths["status"] == 0).sum())
        paths, alive = r.query_vertex(paths)
        turns += 1
    assert (paths["status"] != 0).all()
    return paths, turns


class Case(object):
    """One golden case: its rays, sample by sample, and what the chain of turns made of them on the device -- computed once for the tests that share it"""

    def __init__(self, name, tmp):
        mk, kw = vc.golden_case(name)
        gold = np.load(os.path.join(scenes.GOLDEN, name + "_samples.npz"))
        self.name, self.ref, self.seed = name, gold["samples"], int(gold["seed"])
        self.h, self.w, self.spp, _ = self.ref.shape
        assert self.w*self.h <= 2304
        self.path = mk(tmp, name=name + "_v.json", **kw)
        self.flat = tg.FlattenedScene(self.path)
        assert self.flat.desc.contents.camera.type == 0 and not self.flat.info.stratified_sampler
        self.max_bounces = int(self.flat.desc.contents.settings.max_bounces)
        self.rays = [camera_rays(self.flat, self.w, self.h, self.seed, s) for s in range(self.spp)]
        self.renderer = tg.Renderer(self.path, seed=self.seed)
        self.ends, self.turns = [], []
        for s in range(self.spp):
            paths, turns = chain(self.renderer, self.rays[s], sample=s, seed=self.seed)
            self.ends.append(paths)
            self.turns.append(turns)

    def close(self):
        self.renderer.close()
        self.flat.close()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    made = {}

    def get(name):
        if "materialtest" in name and not scenes.have_materialtest():
            pytest.skip("materialtest assets (assets/) not present")
        if name not in made:
            made[name] = Case(name, tmp_path_factory.mktemp(name))
        return made[name]
    yield get
    for c in made.values():
        c.close()


# ---- 1. the chain is the sample ----

# The end reasons a case must show.  ESCAPED on `cornell`, whose paths leave through the open front, and MAX_BOUNCES on `cornell_bounce2`; ROULETTE and
# ABSORBED as the run's own census shows them: the roulette ends paths in every case but cornell_bounce2 (it needs bounce > 2), a failed BSDF sample
# -- the emitters' black BSDF, a consistency check -- in every case but materialtest_transparency.  No case reaches ZERO_THROUGHPUT or NAN.
REACHES = {name: (ESCAPED,) + ((ROULETTE,) if name != "cornell_bounce2" else (MAX_BOUNCES,)) + ((ABSORBED,) if name != "materialtest_transparency" else ())
           for name in vc.CHAIN_CASES if name != "cornell_fog"}
REACHES["cornell_fog"] = (MAX_BOUNCES, ABSORBED, ROULETTE)         # (a closed box of fog: no path escapes)


def test_the_case_list_is_the_radiance_querys_and_the_further_goldens():
    assert vc.CAMERA_CASES == CAMERA_CASES and set(vc.CHAIN_CASES) == set(CAMERA_CASES) | (set(vc.FURTHER_CASES) - set(vc.CHAIN_DROPPED))


@pytest.mark.parametrize("name", vc.CHAIN_CASES + vc.DEVICE_ONLY_CASES)
def test_the_chain_is_the_sample(name, case):
    """start_paths(first_number=2) with one turn, then query_vertex turn by turn until alive == 0, for every sample index of the golden on the camera's
    own rays: emission is tests/golden/<case>_samples.npz and tghip_query_radiance's answer; the turns never exceed max_bounces; one call with
    turns = max_bounces returns the same bytes.  The census of end reasons is printed; see REACHES for what is asserted of it.  (The cases of
    vc.DEVICE_ONLY_CASES are goldens the CPU oracle cannot reproduce: the device is held to the reference's golden and to tghip_query_radiance all the
    same, which ask nothing of the oracle.)"""
    c = case(name)
    r = c.renderer
    census = np.zeros(7, np.int64)
    for s in range(c.spp):
        got, turns = c.ends[s], c.turns[s]
        want = c.ref[:, :, s].reshape(-1, 3)
        ssum, count = r.query_radiance(c.rays[s], s, s + 1, seed=c.seed)
        print("%s sample %d: %d turns; %d of %d paths differ from the golden, %d from tghip_query_radiance" % (
            name, s, turns, int((got["emission"] != want).any(axis=-1).sum()), c.w*c.h, int((got["emission"] != ssum).any(axis=-1).sum())))
        assert (got["emission"] == want).all() and (got["emission"] == ssum).all() and (count == 1).all()
        assert turns <= c.max_bounces
        once, alive = r.start_paths(c.rays[s], sample=s, seed=c.seed, turns=c.max_bounces)
        assert alive == 0 and same_bytes(once, got)
        assert (got["status"] >= 1).all() and (got["status"] <= 6).all() and (got["bounce"] <= c.max_bounces).all()
        census += np.bincount(got["status"], minlength=7)[:7]
    print("%s: end reasons %s" % (name, ", ".join("%s %d" % (tg.PATH_END_NAMES[k], census[k]) for k in range(1, 7))))
    for reason in REACHES.get(name, ()):
        assert census[reason] > 0, (name, tg.PATH_END_NAMES[reason])


# ---- 2. the stream ----

@pytest.mark.parametrize("name", vc.STREAM_CASES)
def test_every_path_has_drawn_what_the_oracles_path_draws(name, case):
    """`drawn` at the end of each path of the chain is the count oracle_trace_sample_log returns for that pixel and sample with the uniform sampler (it
    counts the booleans: tests/test_vertex_query_cpu.py), the two numbers of the pixel filter -- first_number -- included."""
    c = case(name)
    for s in range(c.spp):
        want = np.array([vc.oracle_drawn(c.flat, c.seed, pixel % c.w, pixel//c.w, s)[1] for pixel in range(c.w*c.h)], np.uint32)
        got = c.ends[s]["drawn"]
        print("%s sample %d: %d of %d paths drew another count; between %d and %d numbers a path" % (name, s, int((got != want).sum()), got.size, want.min(), want.max()))
        assert (got == want).all()
        assert (c.ends[s]["key"] == np.arange(c.w*c.h)).all()


# ---- 3. the pieces ----

@pytest.mark.parametrize("name, edit", [("cornell", None), ("two_lights", scenes._two_lights), ("area_lights", scenes._area_lights),
                                        ("dq_checker_light", scenes._checker_light)])
def test_the_first_turn_is_the_ray_querys_hit_and_the_direct_querys_estimate(name, edit, tmp_path):
    """The scenes of test_gpu_direct_query.test_two_bounce_radiance_is_the_direct_light: after the first turn from START rec and t are
    tghip_query_rays' for every ray, and emission is tghip_query_direct(skip=3, bounce=1)'s rgb for the rays that test qualifies.  On
    dq_checker_light (tests/direct_cases.py) half of the light samples end on a black square of the emitter: the direct query queues their
    shadow segment for its visibility output, the vertex query does not, and both add the same zero."""
    def two_bounces(scene):
        if edit:
            edit(scene)
        scene["integrator"]["max_bounces"] = 2
    w, h = 16, 9
    path = scenes.cornell(tmp_path, name=name + "_mb2.json", resolution=(w, h), spp=4, edit=two_bounces)
    flat = tg.FlattenedScene(path)
    rays = camera_rays(flat, w, h, tg.DEFAULT_SEED, 0)
    d = flat.desc.contents
    lobes = np.array([d.bsdfs[i].lobes for i in range(d.num_bsdfs)], np.uint32)
    flat.close()
    r = tg.Renderer(path, seed=tg.DEFAULT_SEED)
    try:
        surf = r.query_surface(rays)
        hit = (surf["flags"] & capi.TGHIP_SURFACE_HIT) != 0
        ok = hit & ((surf["flags"] & capi.TGHIP_SURFACE_EMISSIVE) == 0)
        ok[hit] &= (lobes[surf["bsdf"][hit]] & (LOBE_SPECULAR | LOBE_FORWARD)) == 0
        assert ok.sum()*2 >= len(rays), (name, int(ok.sum()))
        hits = r.query_rays(rays, "closest")
        for s in range(4):
            paths, alive = r.start_paths(rays, sample=s, turns=1)
            assert (paths["rec"] == hits["rec"]).all()
            assert (paths["t"][hits["rec"] >= 0] == hits["t"][hits["rec"] >= 0]).all() and (paths["t"][hits["rec"] < 0] == 0).all()
            direct = r.query_direct(rays, spp=(s, s + 1), seed=tg.DEFAULT_SEED, medium=None, bounce=1, skip=3)
            assert (paths["emission"][ok] == direct["rgb"][ok]).all()
            assert (paths["emission"][ok] != 0).any()
            assert alive == int((paths["status"] == 0).sum()) and (paths["bounce"][paths["status"] == 0] == 1).all()
    finally:
        r.close()


def test_a_hit_of_the_first_segment_counts_when_t_is_below_tmax(tmp_path):
    """test_gpu_radiance_query.test_the_first_segment_ends_exactly_at_tmax's construction: a light-bound ray with tmax = the t tghip_query_rays reports
    hits nothing -- rec -1, t 0, no emission, ESCAPED --, with tmax = nextafter(t, inf) the light: tghip_query_rays' rec and t, the light's emission."""
    path = scenes.cornell(tmp_path, resolution=(32, 18), spp=1, integrator={"max_bounces": 1})
    flat = tg.FlattenedScene(path)
    d = flat.desc.contents
    light = [d.objects[i] for i in range(d.num_objects) if d.objects[i].emission >= 0][0]
    emission = np.array(list(d.textures[light.emission].value), np.float32)
    base, e0, e1 = (np.array(list(v), np.float64) for v in (light.base, light.edge0, light.edge1))
    flat.close()
    rs = np.random.RandomState(9)
    n = 997
    origins = np.stack([rs.uniform(-0.9, 0.9, n), rs.uniform(1.3, 1.9, n), rs.uniform(-0.9, 0.9, n)], axis=1)
    uv = rs.uniform(0.05, 0.95, (n, 2))
    dirs = base + uv[:, :1]*e0 + uv[:, 1:]*e1 - origins
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    at_light = np.concatenate([origins, np.full((n, 1), 1e-4), dirs, np.full((n, 1), np.inf)], axis=1).astype(np.float32)
    r = tg.Renderer(path)
    try:
        hits = r.query_rays(at_light, "closest")
        assert (hits["rec"] >= 0).all()
        short, reach = at_light.copy(), at_light.copy()
        short[:, 7] = hits["t"]
        reach[:, 7] = np.nextafter(hits["t"], np.float32(np.inf))
        cut, alive = r.start_paths(short, turns=1)
        assert alive == 0 and (cut["rec"] == -1).all() and (cut["t"] == 0).all() and (cut["emission"] == 0).all() and (cut["status"] == ESCAPED).all()
        kept, alive = r.start_paths(reach, turns=1)
        assert alive == 0 and (kept["rec"] == hits["rec"]).all() and (kept["t"] == hits["t"]).all()
        # (the emitter's BSDF samples no direction, PathTracer.cpp:98-99: the path returns its emission there, before the bounce limit is looked at)
        assert (kept["emission"] == emission).all() and (kept["status"] == ABSORBED).all()
    finally:
        r.close()


# ---- 4. the state is the whole state ----

@pytest.mark.parametrize("name", ["zoo_d", "cornell_fog"])
def test_the_state_is_the_whole_state(name, case):
    c = case(name)
    r, rays, seed = c.renderer, c.rays[1], c.seed
    first, alive = r.start_paths(rays, sample=1, seed=seed, turns=1)
    live = first["status"] == 0
    assert 0 < alive == int(live.sum()) <= len(first)               # (zoo_d: some paths end in their first turn; in the fog every path goes on)
    assert (name == "zoo_d") == bool((~live).any())
    whole, _ = r.query_vertex(first)
    assert same_bytes(whole[~live], first[~live])                   # ended paths come back byte for byte
    assert not same_bytes(whole[live], first[live])
    # reversed, the ended ones dropped
    thin, thin_alive = r.query_vertex(np.ascontiguousarray(first[live][::-1]))
    assert same_bytes(np.ascontiguousarray(thin[::-1]), np.ascontiguousarray(whole[live]))
    assert thin_alive == int((whole["status"] == 0).sum())
    # ... to the end: the same paths whatever the batch they travel in (the thinned batch loses its ended paths again every other turn)
    a, b, index = whole, thin, np.flatnonzero(live)[::-1]
    turn, mixed = 0, 0
    while (a["status"] == 0).any():
        if turn % 2:
            keep = b["status"] == 0
            b, index = np.ascontiguousarray(b[keep]), index[keep]
        ended = a["status"] != 0
        mixed += bool(ended.any())
        before = a
        a, b = r.query_vertex(a)[0], r.query_vertex(b)[0]
        assert same_bytes(np.ascontiguousarray(a[index]), b), turn
        assert same_bytes(a[ended], before[ended]), turn            # ended paths among live ones: byte for byte
        turn += 1
    assert mixed >= 2 and same_bytes(a, c.ends[1])
    # batches cut from the larger one with first_index set: the wave edges of the ballots and the append lists
    full, _ = r.start_paths(rays, sample=1, seed=seed, turns=3)
    for n, at in ((1, 0), (1, 200), (63, 64), (64, 1), (65, 127), (257, 300)):
        part, part_alive = r.start_paths(rays[at:at + n], sample=1, seed=seed, first_index=at, turns=3)
        assert same_bytes(part, full[at:at + n]), (n, at)
        assert part_alive == int((part["status"] == 0).sum())
        later = r.query_vertex(part, turns=2)[0]
        assert same_bytes(later, r.query_vertex(full, turns=2)[0][at:at + n]), (n, at)


# ---- 5. the family's list ----

@pytest.mark.parametrize("name", ["zoo_d", "cornell_instances", "cornell_fog", "materialtest"])
def test_options_change_no_byte(name, case):
    """query_blocks, query_refill_at and max_slots; instanced scenes and the 8-wide walk among the cases"""
    c = case(name)
    r = c.renderer
    want = c.ends[0]
    try:
        for option, values in (("query_blocks", (1, 3)), ("query_refill_at", (1, 64)), ("max_slots", (256,))):
            for v in values:
                r.set_option(option, v)
                got, alive = r.start_paths(c.rays[0], sample=0, seed=c.seed, turns=c.max_bounces)
                assert alive == 0 and same_bytes(got, want), (option, v)
                assert same_bytes(chain(r, c.rays[0], sample=0, seed=c.seed)[0], want), (option, v)
            r.set_option(option, {"query_blocks": 0, "query_refill_at": 0, "max_slots": 1 << 23}[option])
    finally:
        r.set_option("query_blocks", 0)
        r.set_option("query_refill_at", 0)
        r.set_option("max_slots", 1 << 23)
    assert same_bytes(r.start_paths(c.rays[0], sample=0, seed=c.seed, turns=c.max_bounces)[0], want)


def test_a_large_call_runs_in_parts(case):
    """More paths than are under way at once (2^20): the call runs in parts, each through all its turns, and no part changes a bit -- the head and the
    tail of the large call, which lie in different parts, are small calls with first_index set"""
    c = case("cornell")
    r = c.renderer
    N, k = (1 << 20) + 257, 257
    rays = np.ascontiguousarray(np.tile(c.rays[0], ((N + len(c.rays[0]) - 1)//len(c.rays[0]), 1))[:N])
    big, alive = r.start_paths(rays, sample=2, seed=5, turns=3)
    assert alive == int((big["status"] == 0).sum()) and 0 < alive < N
    head, _ = r.start_paths(rays[:k], sample=2, seed=5, turns=3)
    tail, _ = r.start_paths(rays[N - k:], sample=2, seed=5, first_index=N - k, turns=3)
    assert same_bytes(big[:k], head) and same_bytes(big[N - k:], tail)
    assert (big["key"] == np.arange(N, dtype=np.uint32)).all()
    more, more_alive = r.query_vertex(big, turns=2)
    assert same_bytes(more[N - k:], r.query_vertex(tail, turns=2)[0]) and same_bytes(more[:k], r.query_vertex(head, turns=2)[0])
    assert more_alive == int((more["status"] == 0).sum())


def test_a_call_between_two_passes_leaves_the_context_alone(case, tmp_path):
    """Samples [0, 8) of a fresh context as the passes [0, 4) and [4, 8), with and without a chain of calls between them: image, counts, auxiliary
    buffers and records byte for byte."""
    c = case("zoo_d")
    w, h = c.w, c.h
    state = {}
    for ask in (False, True):
        r = tg.Renderer(c.path, seed=tg.DEFAULT_SEED)
        ctx, n = r.context(), w*h
        records = np.zeros(((w + 3)//4)*((h + 3)//4), oracle_lib.DEVICE_RECORD_DTYPE)
        records["sample_count"] = np.arange(records.size)              # (these passes keep no records: a pattern the call must leave as it is)
        records["mean"] = 0.25*np.arange(records.size)
        assert tg.lib.tghip_upload_records(ctx, records.ctypes.data, records.size) == 0
        for k, (lo, hi) in enumerate(((0, 4), (4, 8))):
            p = tg.TgHipPassDesc(lo, hi, tg.DEFAULT_SEED, 0, 1, capi.TGHIP_PASS_AUX)
            assert tg.lib.tghip_render_pass(ctx, C.byref(p)) == 0
            if ask and k == 0:                                          # (the pass is still under way: the call waits for it)
                assert same_bytes(chain(r, c.rays[0], sample=0, seed=c.seed)[0], c.ends[0])
            assert tg.lib.tghip_wait(ctx) == 0, tg.lib.tghip_last_error(ctx)
            if ask and k == 0:
                assert same_bytes(r.start_paths(c.rays[0], sample=0, seed=c.seed, turns=c.max_bounces)[0], c.ends[0])
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


def test_calls_on_one_context_equal_calls_on_fresh_contexts(case):
    """The call shares its staging arrays with the other queries and its shadow segments' scratch with tghip_query_direct: a transmittance query, a
    chain, a direct query of another size, the chain again, on one context -- each answer is the bytes of the same call on a context that has answered
    nothing else."""
    c = case("cornell_fog")
    rays = c.rays[0]

    def transmittance(r):
        short = rays[:129].copy()
        short[:, 7] = 0.75
        return r.query_transmittance(short)

    def vertex(r):
        return chain(r, rays, sample=0, seed=c.seed)[0]

    def direct(r):
        return r.query_direct(rays[:65], spp=(0, 3), seed=4, skip=3)

    def start_then_more(r):
        p, _ = r.start_paths(rays[:300], sample=3, seed=9, first_index=11, turns=2, media=np.where(np.arange(300) % 3 == 0, -1, -2).astype(np.int32))
        return r.query_vertex(p[::2], turns=4)[0]

    calls = (transmittance, vertex, direct, start_then_more, vertex, transmittance, direct)
    got = [call(c.renderer) for call in calls]
    want = {}
    for call in set(calls):
        fresh = tg.Renderer(c.path, seed=c.seed)
        try:
            want[call] = call(fresh)
        finally:
            fresh.close()
    for call, answer in zip(calls, got):
        assert same_bytes(answer, want[call]), call.__name__
    assert same_bytes(got[1], c.ends[0])


def test_device_tensors(tmp_path):
    """query_vertex_into with torch tensors on the device gives the bytes of start_paths / query_vertex and writes nothing outside the n states.  In a
    process of its own: torch brings its own HIP runtime and has to be imported before this package."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vertex_query_torch_worker.py")
    p = subprocess.run([sys.executable, worker, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and "VERTEX_QUERY_TORCH_OK" in p.stdout, p.stdout[-4000:]


def test_refusals_leave_the_context_working(case):
    c = case("cornell_fog")
    r = c.renderer
    ctx = r.context()
    rays = np.ascontiguousarray(c.rays[0])
    n = len(rays)
    paths = np.zeros(n + 2, tg.PATH_DTYPE)
    num_media = int(c.flat.desc.contents.num_media)
    alive = C.c_uint32(77)

    def call(ctx_, flags=START, medium=capi.TGHIP_MEDIUM_OF_CAMERA, turns=1, first_number=2, reserved=0, rays_=rays.ctypes.data, media=None,
             paths_=paths.ctypes.data, n_=n, alive_=C.addressof(alive), desc=True):
        d = capi.TgHipVertexQueryDesc(flags, c.seed, 0, 0, first_number, medium, turns, reserved)
        return tg.lib.tghip_query_vertex(ctx_, C.byref(d) if desc else None, rays_, media, paths_, n_, alive_)

    def answers():
        return same_bytes(r.start_paths(rays, sample=0, seed=c.seed, turns=c.max_bounces)[0], c.ends[0])

    assert call(ctx, n_=0) == 0 and alive.value == 0
    assert call(ctx, rays_=None, paths_=None, n_=0, alive_=None) == 0 and call(ctx, flags=0, rays_=None, paths_=None, n_=0) == 0
    empty = r.start_paths(np.zeros((0, 8), np.float32))
    assert len(empty[0]) == 0 and empty[1] == 0 and r.query_vertex(empty[0]) [1] == 0
    assert call(ctx, first_number=1024) == 0 and call(ctx, medium=num_media - 1, alive_=None) == 0
    base16 = paths.ctypes.data//16*16
    for kw, message in ((dict(desc=False), "no description"), (dict(paths_=None), "paths are needed"), (dict(rays_=None), "needs rays"),
                        (dict(flags=0), "TGHIP_VERTEX_START's"), (dict(flags=0, rays_=None, media=rays.ctypes.data), "TGHIP_VERTEX_START's"),
                        (dict(flags=4), "unknown flag"), (dict(reserved=1), "reserved"), (dict(turns=0), "turns"), (dict(first_number=1025), "first_number"),
                        (dict(n_=2**31), "2^31 - 1"), (dict(medium=-3), "medium index"), (dict(medium=num_media), "medium index"),
                        # (the check looks at the pointers' values only: nothing is read through these)
                        (dict(flags=START | DEVICE, rays_=base16 + 4, paths_=base16), "16-byte aligned"),
                        (dict(flags=START | DEVICE, rays_=base16, paths_=base16 + 8), "16-byte aligned"),
                        (dict(flags=START | DEVICE, rays_=base16, paths_=base16, media=base16 + 2), "4-byte aligned"),
                        (dict(flags=START | DEVICE, rays_=base16, paths_=base16, alive_=base16 + 1), "4-byte aligned")):
        assert call(ctx, **kw) == INVALID, kw
        assert message in tg.lib.tghip_last_error(ctx).decode(), kw
        assert answers()                                                    # ... and the context still answers
    bare = tg.lib.tghip_create(0)                                           # a context without an upload
    assert bare
    try:
        assert call(bare, medium=-1) == NOSCENE
        assert call(bare, desc=False) == INVALID
    finally:
        tg.lib.tghip_destroy(bare)
    # nothing outside the n states is written, and a state is written over
    paths[:] = np.frombuffer(b"\x5a"*tg.PATH_DTYPE.itemsize, tg.PATH_DTYPE)[0]
    guard = paths[n:].tobytes()
    assert call(ctx, turns=c.max_bounces) == 0 and alive.value == 0
    assert same_bytes(np.ascontiguousarray(paths[:n]), c.ends[0]) and paths[n:].tobytes() == guard
    # a state whose medium is out of range or whose ray is not finite: an unspecified answer, the call returns
    odd = r.start_paths(rays[:130], sample=0, seed=c.seed, turns=1)[0]
    odd["medium"][::2] = 1 << 20
    odd["medium"][1::4] = -7
    odd["d"][::5] = 0.0
    odd["o"][3::7, 1] = np.nan
    odd["tmax"][4::9] = np.nan
    r.query_vertex(odd, turns=3)
    assert answers()
    ms = C.c_double(-1.0)
    assert tg.lib.tghip_query_vertex_kernel_time(ctx, C.byref(ms)) == 0 and ms.value > 0.0
