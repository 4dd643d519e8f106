"""tghip_query_surface on the device (csrc/hip/surface_query.hip): the camera's own rays against the auxiliary output buffers of a one-sample pass --
the oracle's, which tests/test_outputs_cpu.py holds to the reference's, and the device's own -- with float32 == on every eligible pixel
(tests/surface_cases.py; tests/test_surface_query_cpu.py checks the premise on the oracle); the hit against tghip_query_rays bit for bit in every
walk; the fields that follow from the flattened description; closed-form rays on the Cornell box, independent of the oracle; answers that do not
depend on scheduling; the refusals; a query between two passes; torch tensors on the device.

A miss answers with t = 0 (every word of a miss but the four integer fields is zero), whatever tghip_query_rays leaves in a miss's t: t is compared
on the rays that hit, rec on every ray."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
import surface_cases
import tungsten_amd as tg
from tungsten_amd import capi
from surface_cases import REC_TRIANGLE, REC_QUAD, REC_INSTANCE, OBJF_SMOOTH
from test_gpu_ray_queries import make_rays

pytestmark = pytest.mark.gpu

INVALID, NOSCENE, DEVICE = capi.TGHIP_E_INVALID, capi.TGHIP_E_NOSCENE, capi.TGHIP_DEVELOP_DEVICE_POINTERS
HIT, BACK_SIDE, EMISSIVE, INFINITE = capi.TGHIP_SURFACE_HIT, capi.TGHIP_SURFACE_BACK_SIDE, capi.TGHIP_SURFACE_EMISSIVE, capi.TGHIP_SURFACE_INFINITE
INT_FIELDS = ("rec", "instance", "object", "bsdf")
BATCH_SCENES = ("cornell", "materialtest", "instances", "terraces")


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def is_plain_miss(out):
    """per answer: the four integer fields -1, every other word zero"""
    words = np.ascontiguousarray(out).view(np.uint32).reshape(-1, 24).copy()
    ok = np.ones(len(words), bool)
    for f in INT_FIELDS:
        at = tg.SURFACE_DTYPE.fields[f][1]//4
        ok &= words[:, at] == 0xFFFFFFFF
        words[:, at] = 0
    return ok & (words == 0).all(axis=1)


# ---- 1. the camera's own rays against the aux pass ----

def device_aux(r, s):
    """The device's own TGHIP_PASS_AUX pass over sample [s, s + 1) from zeroed buffers"""
    ctx, n = r.context(), r.width*r.height
    aux = np.zeros(n, tg.AUX_DTYPE)
    assert tg.lib.tghip_upload_aux(ctx, aux.ctypes.data, n) == 0
    p = tg.TgHipPassDesc(s, s + 1, tg.DEFAULT_SEED, 0, 1, capi.TGHIP_PASS_AUX)
    for rc in (tg.lib.tghip_clear_framebuffer(ctx), tg.lib.tghip_render_pass(ctx, C.byref(p)), tg.lib.tghip_wait(ctx),
               tg.lib.tghip_download_aux(ctx, aux.ctypes.data, n)):
        assert rc == 0, tg.lib.tghip_last_error(ctx)
    return aux


@pytest.mark.parametrize("name", sorted(surface_cases.AUX_SCENES))
def test_the_cameras_own_rays_against_the_aux_pass(name, tmp_path):
    if name == "materialtest" and not scenes.have_materialtest():
        pytest.skip("materialtest assets (assets/) not present")
    case = surface_cases.AuxCase(name, tmp_path)
    r = tg.Renderer(case.path, seed=tg.DEFAULT_SEED)
    try:
        for s in (0, 1):
            rays, ohits, oaux, eligible = case.sample(s)
            got = r.query_surface(rays)
            daux = device_aux(r, s)
            hit = got["rec"] >= 0
            assert (got["rec"] == ohits["rec"]).all()
            assert same_bytes(got["t"][hit], ohits["t"][hit])
            assert ((got["flags"] & HIT) != 0).tolist() == hit.tolist()
            emissive = (got["flags"] & EMISSIVE) != 0
            shown = np.where(emissive[:, None], (got["albedo"] + got["emission"]).astype(np.float32), got["albedo"])
            print("%s sample %d: %d eligible of %d pixels, %d of them emissive, %d misses" % (
                name, s, int(eligible.sum()), len(rays), int((eligible & emissive).sum()), int((~hit).sum())))
            assert eligible.sum() >= 0.35*len(rays)
            for label, aux in (("oracle", oaux), ("device", daux)):
                a = aux["a"][eligible]
                assert (aux["count"][eligible, capi.TGHIP_AUX_DEPTH] == 1).all(), label
                assert (got["t"][eligible] == a[:, 3]).all(), label
                assert (got["ns"][eligible] == a[:, 4:7]).all(), label
                assert (shown[eligible] == a[:, 7:10]).all(), label
                if name in surface_cases.SKY_SCENES:
                    assert (~hit).sum() > 0 and (got["flags"][~hit] == INFINITE).all(), label
                    assert (got["emission"][~hit] == aux["a"][~hit][:, 7:10]).all(), label
            if name in surface_cases.SKY_SCENES:
                assert (got["object"][~hit] >= 0).all() and (got["rec"][~hit] == -1).all() and (got["bsdf"][~hit] == -1).all()
            if name == "cornell":
                assert (~hit).sum() > 0 and is_plain_miss(got[~hit]).all()
    finally:
        r.close()
        case.close()


# ---- 2 / 3. the batches of tests/test_gpu_ray_queries.py ----

class Batch(object):
    def __init__(self, scene, tmp):
        mk = {"cornell": scenes.cornell, "materialtest": scenes.materialtest, "instances": scenes.cornell_instances, "terraces": scenes.tile_terraces,
              "cornell_png_textures": scenes.cornell_png}[scene]
        self.path = mk(tmp, resolution=(64, 36), spp=1)
        self.flat = tg.FlattenedScene(self.path)
        self.rays, self.ohits = make_rays(self.flat, "cornell" if scene == "cornell_png_textures" else scene)
        self.table = surface_cases.Tables(self.flat)
        self.renderer = tg.Renderer(self.path)
        self.closest = self.renderer.query_rays(self.rays, "closest")
        self.surface = self.renderer.query_surface(self.rays)

    def close(self):
        self.renderer.close()
        self.flat.close()


_batches = {}


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """One batch, one context and one answer per scene, shared by the tests of this file (none of them changes them)."""
    def get(scene):
        if scene == "materialtest" and not scenes.have_materialtest():
            pytest.skip("materialtest assets (assets/) not present")
        if scene not in _batches:
            _batches[scene] = Batch(scene, tmp_path_factory.mktemp("surface_" + scene))
        return _batches[scene]
    yield get
    for b in _batches.values():
        b.close()
    _batches.clear()


def ray_walk(r):
    plan = capi.TgHipLaunchPlan()
    p = tg.TgHipPassDesc(0, 1, tg.DEFAULT_SEED, 0, 1, 0)
    assert tg.lib.tghip_debug_launch_plan(r.context(), C.byref(p), C.byref(plan)) == 0
    return int(plan.choice.ray_walk)


@pytest.mark.parametrize("scene", BATCH_SCENES)
def test_the_hit_is_query_rays_hit(scene, batch):
    b = batch(scene)
    got, closest, n = b.surface, b.closest, len(b.rays)
    hit = closest["rec"] >= 0
    assert hit.sum() >= n//8 and (~hit).sum() >= n//8, (int(hit.sum()), n)
    assert (got["rec"] == closest["rec"]).all() and (got["rec"] == b.ohits["rec"]).all()
    assert same_bytes(got["t"][hit], closest["t"][hit])
    assert (((got["flags"] & HIT) != 0) == hit).all()
    assert ((got["flags"][~hit] & (HIT | BACK_SIDE | EMISSIVE)) == 0).all() and (got["t"][~hit].view(np.uint32) == 0).all()
    o, d, t = b.rays[:, 0:3], b.rays[:, 4:7], got["t"]
    p = (o[hit] + (d[hit]*t[hit, None]).astype(np.float32)).astype(np.float32)       # float32 multiply, then float32 add: unfused
    assert same_bytes(np.ascontiguousarray(got["p"][hit]), p)
    assert (got["reserved"] == 0).all()
    print("%s: %d rays, %d hits, ray walk %d" % (scene, n, int(hit.sum()), ray_walk(b.renderer)))


def test_the_batches_cover_the_walks(batch):
    walks = {}
    for scene in BATCH_SCENES:
        if scene == "materialtest" and not scenes.have_materialtest():
            continue
        walks[scene] = ray_walk(batch(scene).renderer)
    print("ray walks: %s%s" % (walks, "" if 1 in walks.values() else " (none of them takes walk 1, the BVH2)"))
    need = {0, 2, 3} if scenes.have_materialtest() else {0, 2}
    assert need <= set(walks.values()), walks


@pytest.mark.parametrize("scene, options, walk", [("cornell", {}, 0), ("terraces", {"wide_bvh": 0}, 1), ("terraces", {}, 3)])
def test_the_walks_without_instances_are_query_rays_walks(scene, options, walk, batch):
    """On the flat list, the BVH2 and the 8-wide BVH the surface query walks with tghip_query_rays' own closest-hit kernels: record and t are that
    query's, at one ray, one wave plus one and more than one workgroup."""
    b = batch(scene)
    r = b.renderer
    try:
        for k, v in options.items():
            r.set_option(k, v)
        assert ray_walk(r) == walk
        for n in (1, 65, 257):
            got, closest = r.query_surface(b.rays[:n]), r.query_rays(b.rays[:n], "closest")
            hit = closest["rec"] >= 0
            assert (got["rec"] == closest["rec"]).all(), (scene, walk, n)
            assert same_bytes(got["t"][hit], closest["t"][hit]) and (got["t"][~hit].view(np.uint32) == 0).all(), (scene, walk, n)
        assert hit.any()
    finally:
        for k in options:
            r.set_option(k, 1)


def quat_rotate(q, v):
    """Quaternions [n, 4] (w, x, y, z) times vectors [n, 3], float64 (math/Quaternion.hpp:78-88)"""
    w, qv = q[:, 0:1], q[:, 1:4]
    tt = 2.0*np.cross(qv, v)
    return v + w*tt + np.cross(qv, tt)


def master_records(table, nodes, root):
    """the records under BVH2 node `root`"""
    out, stack = [], [int(root)]
    while stack:
        ref = stack.pop()
        if ref & 0x80000000:
            first, count = ref & 0x07FFFFFF, (ref >> 27) & 15
            out.extend(range(first, first + count))
        else:
            stack.extend([int(nodes[ref].child0) & 0xFFFFFFFF, int(nodes[ref].child1) & 0xFFFFFFFF])
    return set(out)


@pytest.mark.parametrize("scene", BATCH_SCENES + ("cornell_png_textures",))
def test_fields_derived_from_the_description(scene, batch):
    b = batch(scene)
    T, got, d = b.table, b.surface, b.flat.desc
    hit = got["rec"] >= 0
    idx = np.nonzero(hit)[0]
    rec = got["rec"][idx].astype(np.int64)
    kind = T.kind[rec]
    tri = kind == REC_TRIANGLE
    inst = got["instance"][idx].astype(np.int64)
    assert len(idx) > 1000
    # object, bsdf, emissive, instance
    if T.num_instances == 0:
        assert (inst == -1).all()
        assert (got["object"][idx] == T.rec_object[rec]).all()
    else:
        through = inst >= 0
        assert through.sum() > 500 and (~through).sum() > 500
        assert (T.kind[inst[through]] == REC_INSTANCE).all()
        assert (got["object"][idx][~through] == T.rec_object[rec[~through]]).all()
        assert (got["object"][idx][through] == T.rec_object[inst[through]]).all()         # the `instances` object
        assert all(T.objects[o].type == 5 for o in np.unique(got["object"][idx][through]))   # TGHIP_OBJ_INSTANCES
        nodes, masters = d.contents.nodes, {}
        for i in np.unique(inst[through]):
            root = int(T.recs[i, 8])
            if root not in masters:
                masters[root] = master_records(T, nodes, root)
            assert set(rec[inst == i].tolist()) <= masters[root], int(i)
    assert (got["bsdf"][idx] == T.bsdf_of(rec)).all()
    assert (((got["flags"][idx] & EMISSIVE) != 0) == (T.obj_emission[got["object"][idx]] >= 0)).all()
    # quads: the object's normal, the raw hit's (u, v)
    quad = kind == REC_QUAD
    if quad.any():
        normal = T.obj_normal[T.rec_object[rec[quad]]]
        assert same_bytes(np.ascontiguousarray(got["ng"][idx][quad]), normal) and same_bytes(np.ascontiguousarray(got["ns"][idx][quad]), normal)
        assert same_bytes(got["uv"][idx][quad][:, 0].copy(), b.closest["u"][idx][quad]) and same_bytes(got["uv"][idx][quad][:, 1].copy(), b.closest["v"][idx][quad])
    # albedo is the material's albedo texture at uv (a transparency material's base's)
    albedo_tex = {int(m): T.albedo_texture(int(m)) for m in np.unique(got["bsdf"][idx])}
    for i in idx:
        want = surface_cases.texture_eval(d, albedo_tex[int(got["bsdf"][i])], got["uv"][i][0], got["uv"][i][1])
        assert same_bytes(np.ascontiguousarray(got["albedo"][i]), want), (int(i), got[i])
    # triangles: the geometric normal, the back-side flag, flat shading
    if tri.any():
        ti, tr, tinst = idx[tri], rec[tri], inst[tri]
        cross = np.cross(T.recf[tr, 4:7].astype(np.float64), T.recf[tr, 8:11].astype(np.float64))
        length = np.linalg.norm(cross, axis=1)
        ng = cross/length[:, None]
        dl = b.rays[ti, 4:7].astype(np.float64)
        through = tinst >= 0
        if through.any():
            # the instance record's quaternion: p0 = w, b = (x, y, z); its conjugate takes the ray into the master's space
            q = T.recf[tinst[through]][:, [7, 4, 5, 6]].astype(np.float64)
            ng[through] = quat_rotate(q, ng[through])
            dl[through] = quat_rotate(q*np.array([1.0, -1.0, -1.0, -1.0]), dl[through])
        worst = float(np.abs(got["ng"][ti] - ng).max())
        facing = (cross*dl).sum(axis=1)
        sure = np.abs(facing) > 1e-4*length
        assert (((got["flags"][ti][sure] & BACK_SIDE) != 0) == (facing[sure] > 0.0)).all()
        flat_shaded = (T.obj_flags[T.rec_object[tr]] & OBJF_SMOOTH) == 0
        assert same_bytes(np.ascontiguousarray(got["ns"][ti][flat_shaded]), np.ascontiguousarray(got["ng"][ti][flat_shaded]))
        print("%s: %d triangle hits (%d through an instance, %d flat-shaded), largest |ng - float64 normal| %.3g, back side checked on %d" % (
            scene, int(tri.sum()), int(through.sum()), int(flat_shaded.sum()), worst, int(sure.sum())))
        assert worst <= 1e-5 and sure.sum() > tri.sum()//2


# ---- 4. closed form on the Cornell box, independent of the oracle ----

def test_closed_form_rays_on_the_cornell_box(tmp_path):
    """Four hand-placed, axis-parallel rays in the box of tungsten_amd/workloads.py: cornell -- floor y = 0, back wall z = -1, the light a quad at
    y = 1.98 under the ceiling at y = 2, the two boxes below y = 1.21 and away from x = -0.6, z = 0.85 -- with the planes read from the description's
    quads, not from the oracle.  Quad::evalDirect (primitives/Quad.cpp) gives the emission only to a ray that arrives AGAINST the quad's normal
    (dot(d, n) < 0, Quad::intersectionInfo's backSide false); the light's normal points down into the box, so it shines seen from below and is
    black, with BACK_SIDE set, seen from above."""
    path = scenes.cornell(tmp_path, resolution=(32, 18), spp=1)
    flat = tg.FlattenedScene(path)
    T = surface_cases.Tables(flat)
    quads = [i for i, o in enumerate(T.objects) if o.type == 1]               # TGHIP_OBJ_QUAD
    light, = [i for i in quads if T.objects[i].emission >= 0]
    floor, = [i for i in quads if T.objects[i].emission < 0 and T.objects[i].normal[1] > 0.9]
    back, = [i for i in quads if T.objects[i].emission < 0 and abs(T.objects[i].normal[2]) > 0.9]
    assert T.objects[light].normal[1] < -0.9 and abs(T.objects[light].base[1] - 1.98) < 1e-6
    radiance = surface_cases.texture_eval(flat.desc, T.objects[light].emission, 0.5, 0.5)
    assert (radiance > 0).all()
    flat.close()
    cases = [((-0.6, 1.0, 0.85), (0, -1, 0), floor), ((0.1, 1.5, 0.5), (0, 0, -1), back),
             ((0.0, 1.5, 0.0), (0, 1, 0), light), ((0.0, 1.99, 0.0), (0, -1, 0), light)]       # ... the light from below, the light from above
    rays = np.array([list(o) + [1e-4] + list(d) + [np.inf] for o, d, _ in cases], np.float32)
    r = tg.Renderer(path)
    try:
        got = r.query_surface(rays)
    finally:
        r.close()
    for k, (_, _, obj) in enumerate(cases):
        ob = T.objects[obj]
        nrm = np.array(list(ob.normal), np.float64)
        o64, d64 = rays[k, 0:3].astype(np.float64), rays[k, 4:7].astype(np.float64)
        t64 = np.dot(nrm, np.array(list(ob.base), np.float64) - o64)/np.dot(nrm, d64)
        print("ray %d: object %d, t %.9g (float64 %.12g), flags %d" % (k, got["object"][k], got["t"][k], t64, got["flags"][k]))
        assert got["flags"][k] & HIT and got["object"][k] == obj and got["bsdf"][k] == ob.bsdf and got["instance"][k] == -1, (k, got[k])
        assert same_bytes(np.ascontiguousarray(got["ng"][k]), np.array(list(ob.normal), np.float32))
        assert abs(float(got["t"][k]) - t64) <= 2*float(np.spacing(np.float32(t64))), (k, got["t"][k], t64)
        assert bool(got["flags"][k] & BACK_SIDE) == (np.dot(d64, nrm) >= 0.0)
        tex = T.textures[T.albedo_texture(int(ob.bsdf))]
        assert tex.type == capi.TGHIP_TEX_CONSTANT
        assert same_bytes(np.ascontiguousarray(got["albedo"][k]), np.array(list(tex.value), np.float32))
        assert bool(got["flags"][k] & EMISSIVE) == (obj == light)
    assert (got["emission"][0] == 0).all() and (got["emission"][1] == 0).all()
    assert not got["flags"][2] & BACK_SIDE and same_bytes(np.ascontiguousarray(got["emission"][2]), radiance)
    assert got["flags"][3] & BACK_SIDE and (got["emission"][3] == 0).all()


# ---- 5. scheduling never changes an answer ----

@pytest.mark.parametrize("scene", BATCH_SCENES)
def test_scheduling_never_changes_an_answer(scene, batch):
    b = batch(scene)
    r, want = b.renderer, b.surface
    assert same_bytes(r.query_surface(b.rays), want)                        # the same batch twice
    try:
        for blocks in (1, 0):
            r.set_option("query_blocks", blocks)
            for refill in (1, 32, 64):
                r.set_option("query_refill_at", refill)
                assert same_bytes(r.query_surface(b.rays), want), (blocks, refill)
        r.set_option("query_refill_at", 0)
        for blocks in (1, 0):
            r.set_option("query_blocks", blocks)
            for n in (1, 63, 257, 997):
                assert same_bytes(r.query_surface(b.rays[:n]), want[:n]), (blocks, n)
    finally:
        r.set_option("query_blocks", 0)
        r.set_option("query_refill_at", 0)
    perm = np.random.RandomState(11).permutation(len(b.rays))
    assert same_bytes(r.query_surface(b.rays[perm]), want[perm])


# ---- 6. refusals ----

def test_refusals_leave_the_context_working(batch):
    b = batch("cornell")
    r = b.renderer
    ctx = r.context()
    rays = np.ascontiguousarray(b.rays[:256])
    want = b.surface[:256]
    out = np.zeros(256, tg.SURFACE_DTYPE)

    def call(ctx_, flags=0, reserved=(0, 0, 0), rays_=rays.ctypes.data, out_=out.ctypes.data, n=256, desc=True):
        d = capi.TgHipSurfaceQueryDesc(flags, (C.c_uint32*3)(*reserved))
        return tg.lib.tghip_query_surface(ctx_, C.byref(d) if desc else None, rays_, out_, n)

    assert call(ctx, n=0) == 0 and call(ctx, rays_=None, out_=None, n=0) == 0
    assert len(r.query_surface(np.zeros((0, 8), np.float32))) == 0
    for kw, message in ((dict(desc=False), "no description"), (dict(rays_=None), "rays and out"), (dict(out_=None), "rays and out"),
                        (dict(flags=2), "unknown flag"), (dict(reserved=(0, 0, 1)), "reserved"), (dict(n=2**31), "2^31 - 1"),
                        # (the check looks at the pointers' values only: nothing is read through these)
                        (dict(flags=DEVICE, rays_=rays.ctypes.data//16*16 + 4, out_=out.ctypes.data//16*16), "16-byte aligned"),
                        (dict(flags=DEVICE, rays_=rays.ctypes.data//16*16, out_=out.ctypes.data//16*16 + 8), "16-byte aligned")):
        assert call(ctx, **kw) == INVALID, kw
        assert message in tg.lib.tghip_last_error(ctx).decode(), kw
        assert same_bytes(r.query_surface(rays), want)                      # ... and the context still answers, with a fresh context's bytes
    fresh = tg.Renderer(b.path)
    try:
        assert same_bytes(fresh.query_surface(rays), want)
    finally:
        fresh.close()
    bare = tg.lib.tghip_create(0)                                           # a context without an upload
    assert bare
    try:
        assert call(bare) == NOSCENE
        assert call(bare, flags=4) == INVALID
    finally:
        tg.lib.tghip_destroy(bare)
    assert call(ctx) == 0 and same_bytes(out, want)
    ms = C.c_double(-1.0)
    assert tg.lib.tghip_query_surface_kernel_time(ctx, C.byref(ms)) == 0 and ms.value > 0.0


# ---- 7. a query between two passes ----

def test_a_query_between_two_passes_leaves_the_context_alone(batch, tmp_path):
    """Samples [0, 8) of a fresh context as the passes [0, 4) and [4, 8), with and without a query between them: image, counts, auxiliary buffers and
    records byte for byte.  (The ONE pass [0, 8) of a third context is rendered too and only reported: a pass of eight samples sums its work items
    in other groups than two passes of four, query or no query -- csrc/host/PassPlan.cpp.)"""
    b = batch("cornell")
    path = scenes.cornell(tmp_path, resolution=(64, 36), spp=8)
    state = {}
    for label, passes, ask in (("two passes", ((0, 4), (4, 8)), False), ("two passes and a query", ((0, 4), (4, 8)), True), ("one pass", ((0, 8),), False)):
        r = tg.Renderer(path, seed=tg.DEFAULT_SEED)
        ctx, n = r.context(), 64*36
        records = np.zeros(((64 + 3)//4)*((36 + 3)//4), surface_cases.oracle_lib.DEVICE_RECORD_DTYPE)
        records["sample_count"] = np.arange(records.size)              # (these passes keep no records: a pattern the query must leave as it is)
        records["mean"] = 0.25*np.arange(records.size)
        assert tg.lib.tghip_upload_records(ctx, records.ctypes.data, records.size) == 0
        for k, (lo, hi) in enumerate(passes):
            p = tg.TgHipPassDesc(lo, hi, tg.DEFAULT_SEED, 0, 1, capi.TGHIP_PASS_AUX)
            assert tg.lib.tghip_render_pass(ctx, C.byref(p)) == 0 and tg.lib.tghip_wait(ctx) == 0, tg.lib.tghip_last_error(ctx)
            if ask and k == 0:
                assert same_bytes(r.query_surface(b.rays), b.surface)
        ssum, count = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
        aux = np.zeros(n, tg.AUX_DTYPE)
        rec = np.zeros_like(records)
        assert tg.lib.tghip_download_framebuffer(ctx, ssum.ctypes.data, count.ctypes.data, n) == 0
        assert tg.lib.tghip_download_aux(ctx, aux.ctypes.data, n) == 0
        assert tg.lib.tghip_download_records(ctx, rec.ctypes.data, rec.size) == 0
        r.close()
        assert (count == 8).all() and same_bytes(rec, records)
        state[label] = (ssum, count, aux, rec)
    print("one pass [0, 8) against two passes without a query: image %s, aux %s" % tuple(
        "equal" if same_bytes(state["one pass"][k], state["two passes"][k]) else "differs" for k in (0, 2)))
    for x, y in zip(state["two passes"], state["two passes and a query"]):
        assert same_bytes(x, y)


# ---- 8. torch tensors ----

def test_device_tensors(tmp_path):
    """query_surface_into with torch tensors on the device gives the bytes of query_surface.  In a process of its own: torch brings its own HIP
    runtime and has to be imported before this package (tests/surface_query_torch_worker.py)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "surface_query_torch_worker.py")
    p = subprocess.run([sys.executable, worker, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and "SURFACE_QUERY_TORCH_OK" in p.stdout, p.stdout[-4000:]
