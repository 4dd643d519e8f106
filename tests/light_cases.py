"""The cases of the per-call light comparisons (tests/test_light_units_cpu.py, tests/test_gpu_light_units.py, tools/make_light_golden.py,
tools/light_cases_check.cpp): for every sampled light of the six scenes.light_corners scenes a seeded, deterministic list of (p, w) -- a shading
point and a unit direction, crafted ones first, random fill after -- and the two sampler streams each case draws from.  Every input is one a path can
produce: positions are finite float32, directions unit vectors rounded to float32; no NaN and no infinity goes in (a NaN in a RESULT -- 0/0 at a point
light's own position -- is compared as a NaN).

The geometry the crafted cases are built around is read from the flattened scene (TgHipObject), so the cases follow the emitter wherever the scene
file puts it.  Everything is computed in float64 in the emitter's own frame and rounded once.

Crafted p (per emitter kind)
  quad, disk     in the emitter's plane, and one ulp either side of it; in the plane beside the emitter; behind; 1e-4 above the surface; for the disk a
                 point on its emission cone's boundary
  sphere, point  the centre; on the sphere's surface and one ulp inside / outside it (the point light: one ulp next to its position)
  cube           the centre, inside, on a face, on an edge, on a corner
  cylinder       the centre, on the axis, on the wall, on a cap's rim
  mesh           a vertex, the large triangle's centroid, 1e-4 above it, behind it
  quad           20 .. 3500 units away in twelve directions: where a millimetre-sized emitter's solid angle is rounding noise of either sign
  every kind     1e4 and 1e6 units along the normal and along a tangent (the weights that go to "unknown" or to 0), a point of general position,
                 uniform points of a box around the scene, and some of those a hundred times as far from the emitter
Crafted w
  towards the emitter's centre, straight away from it; along the emitter's normal and its opposite
  dot(n, w) of +1e-7, -1e-7 and 0
  quad           through each corner and each edge midpoint exactly, and one ulp outside
  infinite       the two poles of the light's local frame; the u seam and one ulp either side of it; directions on the bitmap's (and the checker's)
                 texel boundaries; for the cap its rim and one ulp either side
  uniform

The device's Rng replays nothing, so every case draws from its own counter-based streams -- (SEED, stream, 0) for chooseLight, (SEED, stream, 1) for
sampleDirect --, which the host reproduces with oracle_lib.rng_streams_at.  Crafted sampling numbers (xi of exactly 0, or 1 - ulp) are out of scope."""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import oracle_lib  # noqa: E402
GOLDEN = os.path.join(ROOT, "tests", "golden", "light_corners.npz")
RESIDUAL = os.path.join(ROOT, "tests", "golden", "light_corners_residual.json")
UNITS_RESIDUAL = os.path.join(ROOT, "tests", "golden", "units_light_residual.json")

SEED = 0x11647001
CASES_PER_LIGHT = 4096
FIXTURE_CASES = 160          # the first cases of every light: what the reference's answers are recorded for (every crafted p and w occurs among them)
MAX_LIGHTS = 16              # stream indices leave room for the most lights a scene may hold
NXC, NXS = 2, 6              # numbers handed to the replay samplers of chooseLight (draws one) and sampleDirect (a capped cylinder draws four)
# the result words the oracle and the reference harness write per case; the device's TgHipLightResult holds the first 18 the same way
WORDS = ("chosen", "choose_weight", "sample_ok", "d.x", "d.y", "d.z", "dist", "pdf", "approx", "hit", "t", "u", "v", "back_side",
         "emission.x", "emission.y", "emission.z", "direct_pdf", "consumed_choose", "consumed_sample")
INT_WORDS = [0, 2, 9, 13, 18, 19]
# emitter types (include/tungsten_hip.h: TGHIP_OBJ_*) and flags
MESH, QUAD, CUBE, SPHERE, INFINITE_SPHERE, DISK, CAP, POINT, CYLINDER = 0, 1, 2, 3, 4, 6, 7, 8, 9
KIND_OF = {"mesh": MESH, "quad": QUAD, "cube": CUBE, "sphere": SPHERE, "infinite_sphere": INFINITE_SPHERE, "skydome": INFINITE_SPHERE, "disk": DISK,
           "infinite_sphere_cap": CAP, "point": POINT, "cylinder": CYLINDER}
OBJF_SKYDOME = 4
BOX_LO, BOX_HI = np.array([-1.5, -0.5, -1.5]), np.array([1.5, 2.5, 1.5])     # around the Cornell box

f32 = np.float32


def _unit(v):
    v = np.asarray(v, np.float64)
    n = np.linalg.norm(v)
    return v/n if n > 0 else np.array([0.0, 1.0, 0.0])


def _ulp_step(v, axis_of, steps):
    """float32 vector v with the component along the largest |axis_of| component moved `steps` ulps (sign: along axis_of)."""
    v = np.asarray(v, f32).copy()
    k = int(np.argmax(np.abs(axis_of)))
    up = (steps > 0) == (axis_of[k] > 0)
    for _ in range(abs(steps)):
        v[k] = np.nextafter(v[k], f32(np.inf) if up else f32(-np.inf))
    return v


def _orthonormal(n):
    n = _unit(n)
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    t = _unit(np.cross(n, a))
    return n, t, np.cross(n, t)


def light_geometry(desc, slot):
    """What the crafted cases need of the light in `slot` of desc.lights, read from the flattened object: float64 arrays."""
    d = desc.contents
    o = d.objects[d.lights[slot]]
    g = {"type": int(o.type), "flags": int(o.flags), "object": int(d.lights[slot])}
    for k in ("base", "edge0", "edge1", "normal", "pos", "scale"):
        g[k] = np.array(list(getattr(o, k)), np.float64)
    g["rot"] = np.array(list(o.rot), np.float64).reshape(3, 3)
    if o.type == MESH:
        n = int(o.num_light_tris)
        block = np.ctypeslib.as_array(d.light_tris, shape=(int(d.num_light_tri_floats),))[o.first_light_tri:o.first_light_tri + 10*n + 1]
        g["tris"] = np.array(block[n + 1:], np.float64).reshape(n, 3, 3)
    if o.type == INFINITE_SPHERE and o.emission >= 0:
        t = d.textures[o.emission]
        g["tex_res"] = (int(t.w), int(t.h)) if t.type == 2 else (int(t.res_u), int(t.res_v)) if t.type == 1 else (8, 4)
    return g


def _frame(g):
    """(centre, normal, tangent, half-size) of the emitter: where `towards the light` points and what `along the normal` means."""
    ty = g["type"]
    if ty == QUAD:
        return g["base"] + 0.5*g["edge0"] + 0.5*g["edge1"], _unit(g["normal"]), _unit(g["edge0"]), 0.5*np.linalg.norm(g["edge0"])
    if ty == DISK:
        return g["pos"], _unit(g["normal"]), _unit(g["edge0"]), g["scale"][0]
    if ty == SPHERE:
        return g["pos"], g["rot"] @ np.array([0.0, 0.0, 1.0]), g["rot"] @ np.array([1.0, 0.0, 0.0]), g["scale"][0]
    if ty == POINT:
        return g["pos"], np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]), 0.0
    if ty == CUBE:
        return g["pos"], g["rot"] @ np.array([0.0, 1.0, 0.0]), g["rot"] @ np.array([1.0, 0.0, 0.0]), float(np.max(g["scale"]))
    if ty == CYLINDER:
        return g["pos"], g["rot"] @ np.array([1.0, 0.0, 0.0]), g["rot"] @ np.array([0.0, 1.0, 0.0]), float(g["scale"][1])
    if ty == MESH:
        tri = g["tris"][0]
        n = _unit(np.cross(tri[1] - tri[0], tri[2] - tri[0]))
        return tri.mean(axis=0), n, _unit(tri[1] - tri[0]), 0.2
    if ty == CAP:
        n, t, _ = _orthonormal(g["normal"])
        return np.array([0.0, 1.0, 0.0]), n, t, 1.0
    return np.array([0.0, 1.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]), 1.0       # infinite sphere: any point will do


def crafted_p(g):
    """[(kind, float32 point)] for one emitter."""
    c, n, t, half = _frame(g)
    b = np.cross(n, t)
    ty = g["type"]
    out = []

    def add(kind, p):
        out.append((kind, np.asarray(p, np.float64).astype(f32)))
    if ty in (QUAD, DISK):
        inplane = c + 0.3*half*t + 0.2*half*b
        add("plane", inplane)
        out.append(("plane+ulp", _ulp_step(inplane.astype(f32), n, 1)))
        out.append(("plane-ulp", _ulp_step(inplane.astype(f32), n, -1)))
        add("plane_beside", c + 3.0*half*t)
        add("behind", c - 0.5*n + 0.1*half*t)
        add("above_1e-4", c + 1e-4*n + 0.25*half*b)
        if ty == DISK:
            cos_apex = g["scale"][1]
            add("cone_boundary", g["base"] + 0.7*(cos_apex*n + np.sqrt(max(1.0 - cos_apex*cos_apex, 0.0))*t))
    elif ty == SPHERE:
        r = g["scale"][0]
        dirn = _unit(0.5*n + 0.6*t + 0.3*b)
        add("centre", c)
        surf = (c + r*dirn).astype(f32)
        out.append(("surface", surf))
        out.append(("surface+ulp", _ulp_step(surf, dirn, 1)))
        out.append(("surface-ulp", _ulp_step(surf, dirn, -1)))
        add("inside", c + 0.5*r*dirn)
    elif ty == POINT:
        add("centre", c)
        out.append(("centre+ulp", _ulp_step(c.astype(f32), n, 1)))
        add("near_1e-4", c + 1e-4*t)
    elif ty == CUBE:
        s, R = g["scale"], g["rot"]
        for kind, l in (("centre", (0, 0, 0)), ("inside", (0.3, -0.2, 0.5)), ("face", (1, 0.2, -0.4)), ("edge", (1, 1, 0.1)), ("corner", (1, 1, 1)),
                        ("face_1e-4", (0.1, 1 + 1e-4/s[1], 0.3))):
            add(kind, c + R @ (np.array(l)*s))
    elif ty == CYLINDER:
        r, h, R = g["scale"][0], g["scale"][1], g["rot"]
        for kind, l in (("centre", (0, 0, 0)), ("axis", (0, 0.3*h, 0)), ("wall", (r, 0.2*h, 0)), ("rim", (0, h, r)), ("beyond_cap", (0.3*r, 1.5*h, 0)),
                        ("wall_1e-4", ((r + 1e-4)*np.cos(0.7), -0.4*h, (r + 1e-4)*np.sin(0.7)))):
            add(kind, c + R @ np.array(l))
    elif ty == MESH:
        tri = g["tris"][0]
        add("vertex", tri[0])
        add("centroid", c)
        add("above_1e-4", c + 1e-4*n)
        add("behind", c - 0.3*n)
        add("front", c + 0.3*n + 0.05*t)
    if ty == QUAD:
        # distances at which a millimetre-sized emitter's solid angle is below the last bit of the 2 pi it is subtracted from: rounding noise of either sign
        for i in range(12):
            dist = 20.0*1.6**i
            add("far_%d" % int(dist), c + dist*_unit(n + (0.15 + 0.1*i)*t - (0.4 - 0.13*i)*b))
    for dist in (1e4, 1e6):
        add("normal_%g" % dist, c + dist*n)
        add("tangent_%g" % dist, c + dist*t + 1e-3*dist*n)
    add("general", np.array([0.31, 0.87, 0.43]))
    return out


def _inf_direction(g, u, v):
    """InfiniteSphere::uvToDirection in float64: the world direction of (u, v) of the light's map."""
    phi, theta = (u - 0.5)*2.0*np.pi, v*np.pi
    local = np.array([np.cos(phi)*np.sin(theta), -np.cos(theta), np.sin(phi)*np.sin(theta)])
    return local if g["flags"] & OBJF_SKYDOME else g["rot"] @ local


def crafted_w(g, p):
    """[(kind, float32 unit vector)] for one emitter seen from the float32 point p."""
    c, n, t, half = _frame(g)
    b = np.cross(n, t)
    ty = g["type"]
    p = np.asarray(p, np.float64)
    infinite = ty in (INFINITE_SPHERE, CAP)
    to_c = n if infinite or np.linalg.norm(c - p) == 0 else _unit(c - p)
    out = []

    def add(kind, w):
        out.append((kind, _unit(w).astype(f32)))
    add("towards", to_c)
    add("away", -to_c)
    add("normal", n)
    add("-normal", -n)
    for kind, z in (("grazing+1e-7", 1e-7), ("grazing-1e-7", -1e-7), ("grazing_0", 0.0)):
        add(kind, np.sqrt(1.0 - z*z)*_unit(0.8*t + 0.6*b) + z*n)
    if ty == QUAD:
        base, e0, e1 = g["base"], g["edge0"], g["edge1"]
        for i, (a, bb) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1), (0.5, 0), (1, 0.5), (0.5, 1), (0, 0.5))):
            target = base + a*e0 + bb*e1
            if np.linalg.norm(target - p) == 0:
                continue
            w = _unit(target - p).astype(f32)
            out.append(("rim%d" % i, w))
            outward = (target - c) - np.dot(target - c, w.astype(np.float64))*w.astype(np.float64)
            if np.linalg.norm(outward) > 0:
                out.append(("rim%d+ulp" % i, _ulp_step(w, outward, 1)))
    if ty == INFINITE_SPHERE:
        W, H = g.get("tex_res", (8, 4))
        add("pole+", _inf_direction(g, 0.3, 1.0))
        add("pole-", _inf_direction(g, 0.3, 0.0))
        seam = _inf_direction(g, 0.0, 0.5)
        out.append(("seam", _unit(seam).astype(f32)))
        zl = (np.eye(3) if g["flags"] & OBJF_SKYDOME else g["rot"]) @ np.array([0.0, 0.0, 1.0])      # local +z: across the seam
        out.append(("seam+ulp", _ulp_step(_unit(seam).astype(f32), zl, 1)))
        out.append(("seam-ulp", _ulp_step(_unit(seam).astype(f32), zl, -1)))
        # exactly on the seam with z of +0 and of -0 in the light's frame: atan2f(-0, -1) is -pi, atan2f(+0, -1) is +pi -- u of 0 or of 1.  (Exact
        # for the skydome and for an unrotated sphere, whose world directions are the local ones; a rotation leaves just two more seam directions.)
        unrotated = bool(g["flags"] & OBJF_SKYDOME) or (g["rot"] == np.eye(3)).all()
        for kind, z in (("seam+0", 0.0), ("seam-0", -0.0)):
            local = np.array([-1.0, 0.0, z])
            out.append((kind, (local if unrotated else g["rot"] @ local).astype(f32)))
        for k, (u, v) in enumerate(((1.0/W, 0.5/H), (3.0/W, 1.0/H), (0.5, 0.5), (float(W - 1)/W, float(H - 1)/H), (2.5/W, 2.0/H), (0.25, 0.75))):
            add("texel%d" % k, _inf_direction(g, u, v))
    if ty == CAP:
        cos_cap = g["scale"][0]
        rim = _unit(cos_cap*n + np.sqrt(max(1.0 - cos_cap*cos_cap, 0.0))*t).astype(f32)
        out.append(("cap_rim", rim))
        out.append(("cap_rim+ulp", _ulp_step(rim, n, 1)))
        out.append(("cap_rim-ulp", _ulp_step(rim, n, -1)))
        add("cap_inside", n + 0.01*b)
    return out


def _sphere(xi0, xi1):
    z = 1.0 - 2.0*xi0
    phi = 2.0*np.pi*xi1
    r = np.sqrt(np.maximum(1.0 - z*z, 0.0))
    return np.stack([r*np.cos(phi), r*np.sin(phi), z], axis=1)


def _emitter_points(g, R):
    """One point on or next to the emitter per row of R [n, 3] in [0, 1): what the random directions aim at, so that small emitters get hit."""
    c, n, t, half = _frame(g)
    b = np.cross(n, t)
    ty = g["type"]
    a = R*1.2 - 0.1                                               # a little beyond the edges as well
    if ty == QUAD:
        return g["base"] + a[:, :1]*g["edge0"] + a[:, 1:2]*g["edge1"]
    if ty == MESH:
        tri = g["tris"][(R[:, 2]*len(g["tris"])).astype(int) % len(g["tris"])]
        return tri[:, 0] + a[:, :1]*(tri[:, 1] - tri[:, 0]) + (a[:, 1:2]*(1.0 - a[:, :1]))*(tri[:, 2] - tri[:, 0])
    if ty == CUBE:
        return c + ((a*2.0 - 1.0)*g["scale"]) @ g["rot"].T
    if ty == CYLINDER:
        r, h = g["scale"][0], g["scale"][1]
        ang = 2.0*np.pi*R[:, 0]
        local = np.stack([r*1.05*np.sqrt(R[:, 2])*np.cos(ang), (a[:, 1]*2.0 - 1.0)*h, r*1.05*np.sqrt(R[:, 2])*np.sin(ang)], axis=1)
        return c + local @ g["rot"].T
    rad = max(half, 1e-3)*1.1
    return c + rad*(np.sqrt(R[:, :1])*np.cos(2.0*np.pi*R[:, 1:2])*t + np.sqrt(R[:, :1])*np.sin(2.0*np.pi*R[:, 1:2])*b) + \
        (rad*(R[:, 2:3]*2.0 - 1.0)*n if ty in (SPHERE, POINT) else 0.0)


def make_cases(g, name, n=CASES_PER_LIGHT):
    """The first n cases of one light (g: light_geometry; name: the light's name, which seeds the fill): dict of p [n, 3], w [n, 3] float32 and the
    kinds of the crafted ones (lists of names, "" for a random one).  A prefix of a longer list is the shorter list."""
    rng = np.random.RandomState((zlib.crc32(name.encode()) ^ SEED) & 0xFFFFFFFF)
    R = rng.random_sample((n, 12))            # per case: p (3), w (2), the aim point (3), three choices, spare -- drawn whether used or not
    P = crafted_p(g)
    nw = len(crafted_w(g, P[0][1]))
    crafted = len(P)*nw                        # every crafted p with every crafted w kind
    period = len(P)*nw//int(np.gcd(len(P), nw))
    c, nrm, t, half = _frame(g)
    infinite = g["type"] in (INFINITE_SPHERE, CAP)
    box = BOX_LO + R[:, 0:3]*(BOX_HI - BOX_LO)
    far = R[:, 11] < 0.15                      # some of the box's points pushed out a hundredfold, away from the emitter
    box = np.where(far[:, None], c + (box - c)*100.0, box).astype(f32)
    aim = _emitter_points(g, R[:, 5:8])
    uni = _sphere(R[:, 3], R[:, 4])
    pick = (R[:, 8:11]*1e6).astype(np.int64)
    p = np.zeros((n, 3), f32)
    w = np.zeros((n, 3), f32)
    pk, wk = [], []
    for k in range(n):
        if k < crafted:
            # both indices walk on together -- every p and every w within the first max(len(P), nw) cases --, and w moves on by one more after every
            # lcm(len(P), nw) cases, which brings the pairs the two periods alone never form
            ip, iw = k % len(P), (k + k//period) % nw
        else:
            ip = pick[k, 0] % len(P) if R[k, 8] < 0.25 else -1
            iw = pick[k, 1] % nw if R[k, 9] < 0.25 else -1
        pk.append(P[ip][0] if ip >= 0 else "")
        p[k] = P[ip][1] if ip >= 0 else box[k]
        if iw >= 0:
            W = crafted_w(g, p[k])
            kind, w[k] = W[iw % len(W)]
            wk.append(kind)
        else:
            wk.append("")
            to_aim = aim[k] - p[k].astype(np.float64)
            if infinite or R[k, 10] < 0.4 or np.linalg.norm(to_aim) == 0:
                w[k] = _unit(uni[k]).astype(f32)
            else:
                w[k] = _unit(to_aim).astype(f32)
    assert np.isfinite(p).all() and np.isfinite(w).all() and (np.abs(np.linalg.norm(w.astype(np.float64), axis=1) - 1.0) < 1e-6).all()
    return {"p": p, "w": w, "p_kind": pk, "w_kind": wk}


def stream_index(scene_position, slot, k=0):
    """The sampler stream of case k of the light in `slot` of scene number scene_position of scenes.LIGHT_CORNER_SCENES."""
    return (scene_position*MAX_LIGHTS + slot)*CASES_PER_LIGHT + k


def streams(scene_position, slot, n, extra=1):
    """(xi_choose [n, NXC + extra], xi_sample [n, NXS + extra]) float32: the first numbers of each case's two streams."""
    first = stream_index(scene_position, slot)
    return oracle_lib.rng_streams_at(SEED, first, n, 0, NXC + extra), oracle_lib.rng_streams_at(SEED, first, n, 1, NXS + extra)


def oracle_words(desc, slot, cases, xi_choose, xi_sample):
    """[n, 20] result words of the oracle for the cases of one light."""
    n = cases["p"].shape[0]
    return oracle_lib.light_cases(desc, np.full(n, slot, np.int32), cases["p"], cases["w"], xi_choose[:, :NXC], xi_sample[:, :NXS])


def chosen_as_objects(ref, desc):
    """The reference harness names the chosen light by its slot in TraceableScene::lights(); the oracle and the device by its object index."""
    d = desc.contents
    table = np.array([d.lights[i] for i in range(d.num_lights)] + [-1], np.int64)
    out = np.array(ref, np.uint32, copy=True)
    out[:, 0] = table[out[:, 0].view(np.int32)].astype(np.int32).view(np.uint32)
    return out


def differing(got, want, dirac=False):
    """Per case, does any compared word differ?  got / want: [n, 20] uint32 words.  Bit patterns; a NaN matches a NaN.  chosen, sample_ok, approx and
    hit always; the weight and the count chooseLight consumed where both chose a light; d, dist, pdf and sampleDirect's count where both say the
    sample succeeded; t, u, v, back_side, emission and direct_pdf where both say the ray hit -- and direct_pdf always for a Dirac light, which is
    never hit.  What lies behind a failed call is unspecified."""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    same = got == want
    nan = np.isnan(got.view(f32)) & np.isnan(want.view(f32))
    nan[:, INT_WORDS] = False
    same |= nan
    none = (got[:, 0].view(np.int32) < 0) & (want[:, 0].view(np.int32) < 0)
    same[np.ix_(none, [1, 18])] = True
    failed = (got[:, 2] == 0) & (want[:, 2] == 0)
    same[np.ix_(failed, [3, 4, 5, 6, 7, 19])] = True
    miss = (got[:, 9] == 0) & (want[:, 9] == 0)
    same[np.ix_(miss, [10, 11, 12, 13, 14, 15, 16] + ([] if dirac else [17]))] = True
    return ~same.all(axis=1)


def device_words(r):
    """[n, 18] words of a tungsten_amd.LIGHT_RESULT_DTYPE array in the order of WORDS, and the two streams' next numbers [n, 2]."""
    words = np.ascontiguousarray(r).view(np.uint32).reshape(len(r), -1)
    return words[:, :18].copy(), words[:, 18:20].copy().view(f32)


(LEAN, SIMPLE, COAT, GLASS, PLASTIC, MEDIA, TAIL, FULL, ALL) = range(9)        # capi.TGHIP_BSDF_VARIANT_*


def families_for(t):
    """The shading families the launch code may pick for a scene with the traits t (capi.TgHostSceneTraits), in the order it decides
    (csrc/host/LaunchChoice.cpp: the class families, the fused flat launches, k_tail): the all-features family for a scene with cylinders, bump maps,
    procedural textures or fibres, for a media scene the lean media family covers not, and for every auxiliary-output pass; the media family; the full
    family for mesh emitters and, next to the class families, for instances; else LEAN or SIMPLE for class 0 and COAT / GLASS / PLASTIC / TAIL
    (a superset of the launches of any one scene: which of them run depends on the materials, which no light cares about).  The `_INST` twins of
    SIMPLE / COAT / GLASS / PLASTIC that instanced scenes launch differ from them in FEAT_INSTANCES alone, a bit no light needs: SIMPLE ... stand for them.
    A restatement, and a superset on purpose: tests/test_launch_choice_cpu.py holds the families the launch choice names (csrc/host/LaunchChoice.cpp) to it."""
    fams = {ALL}
    if t.all_features_shading:
        return fams
    if t.have_media:
        return fams | ({MEDIA} if t.media_simple and not t.have_mesh_light else set())
    if t.have_mesh_light:
        return fams | {FULL}
    if t.have_instances:
        return fams | {SIMPLE, COAT, GLASS, PLASTIC, FULL}
    return fams | {LEAN if t.lean_scene else SIMPLE, COAT, GLASS, PLASTIC, TAIL, FULL}


def write_case_file(path, scene_lights):
    """The cases as tools/light_cases_check.cpp reads them: u32 lights, cases per light, NXC, NXS; per light and case f32 p[3], w[3], xi_choose[NXC],
    xi_sample[NXS].  scene_lights: [(cases, xi_choose, xi_sample)] in slot order."""
    n = scene_lights[0][0]["p"].shape[0]
    with open(path, "wb") as f:
        f.write(np.array([len(scene_lights), n, NXC, NXS], np.uint32).tobytes())
        for cases, xc, xs in scene_lights:
            f.write(np.concatenate([cases["p"], cases["w"], xc[:, :NXC], xs[:, :NXS]], axis=1).astype(f32).tobytes())


def main(out_dir):
    """The scenes and their case files (all CASES_PER_LIGHT cases of every light) for tools/light_cases_check.cpp."""
    import scenes
    import tungsten_amd as tg
    os.makedirs(out_dir, exist_ok=True)
    for pos, which in enumerate(scenes.LIGHT_CORNER_SCENES):
        flat = tg.FlattenedScene(scenes.light_corners(out_dir, which))
        per_light = []
        for slot, (name, _, _) in enumerate(scenes.light_corner_list(which)):
            xc, xs = streams(pos, slot, CASES_PER_LIGHT, extra=0)
            per_light.append((make_cases(light_geometry(flat.desc, slot), name), xc, xs))
        flat.close()
        write_case_file(os.path.join(out_dir, "light_cases_%s.bin" % which), per_light)
        print("%s: %d lights, %d cases each" % (which, len(per_light), CASES_PER_LIGHT))


if __name__ == "__main__":
    main(sys.argv[1])
