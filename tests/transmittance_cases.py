"""Case table of tghip_query_transmittance: the scenes, the seeded rays and the per-call parameters whose answers the reference's own
TraceBase::generalizedShadowRay gives (tools/ref_transmittance.cpp, recorded by tools/make_transmittance_golden.py into
tests/golden/transmittance_cases.npz), and the census of the legs those cases reach.  tests/test_transmittance_query_cpu.py takes the census from the
committed golden; tests/test_gpu_transmittance_query.py holds the device to every case, bit for bit.

A group is one call: a scene, a start medium and an end cap by their JSON names, a start bounce, the two surface flags, its rays and -- some groups --
a start medium per ray.  Scenes are variants of the Cornell box with both blocks a millimetre off the floor (no coincident faces) and of the
reference's non-exponential example scene."""
import json
import os

import numpy as np

import scenes
from scenes import (_atmosphere, _davis_weinstein_fog, _expfog, _fog, _fog_and_smoke, _interpolated_fog)
from texture_cases import _lift

GOLDEN = os.path.join(scenes.GOLDEN, "transmittance_cases.npz")
SEED = 0x7A115ED
INF = np.float32(np.inf)
END_MISS, END_CAP, END_OPAQUE, END_ZERO_ALPHA, END_MAX_BOUNCES, END_CULLED = range(6)
FLAG_PAIRS = ((False, False), (False, True), (True, False), (True, True))     # (starts_on_surface, ends_on_surface)
TRANS_INTERPOLATED = 8


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------

PANE_Y = (1.35, 1.45, 1.55, 1.65)
PANE_ALPHA = (None, 0.6, None, 0.25)          # None: a `forward` boundary; else a `transparency` of that constant alpha


def _panes(scene):
    """A stack of four parallel see-through quads above the blocks -- forward, alpha 0.6, forward, alpha 0.25 -- and three upright cut-outs in front
    of the short block whose alpha is exactly 0 or 1: a checker, a disk and a blade (tq_stack adds a .png: _png_cut)."""
    _lift(scene)
    base = {"type": "lambert", "albedo": [0.3, 0.5, 0.7]}
    for i, (y, alpha) in enumerate(zip(PANE_Y, PANE_ALPHA)):
        bsdf = {"name": "pane%d" % i, "type": "forward", "albedo": 1} if alpha is None else \
               {"name": "pane%d" % i, "type": "transparency", "albedo": 1, "alpha": alpha, "base": base}
        scene["bsdfs"].append(bsdf)
        scene["primitives"].append({"name": "pane%d" % i, "type": "quad", "bsdf": "pane%d" % i,
                                    "transform": {"position": [0.3, y, 0.2], "scale": [1.0, 1.0, 1.0]}})
    cuts = (("checker", {"type": "checker", "on_color": 1.0, "off_color": 0.0, "res_u": 4, "res_v": 4}, -0.6),
            ("disk", {"type": "disk", "value": 1.0}, 0.0), ("blade", {"type": "blade", "blades": 5, "angle": 0.6, "value": 1.0}, 0.6))
    for name, alpha, x in cuts:
        scene["bsdfs"].append({"name": "cut_" + name, "type": "transparency", "albedo": 1, "alpha": alpha, "base": base})
        scene["primitives"].append({"name": "cut_" + name, "type": "quad", "bsdf": "cut_" + name,
                                    "transform": {"position": [x, 0.5, 0.9], "scale": [0.5, 1.0, 0.5], "rotation": [90, 0, 0]}})


def _png_cut(scene):
    """A fourth upright cut-out above the three, its alpha the alpha channel of tq_alpha.png: squares of 255 (nothing gets through), of 0, and of a
    dotted 128 that the texture's interpolation spreads into fractions"""
    scene["bsdfs"].append({"name": "cut_png", "type": "transparency", "albedo": 1, "alpha": "tq_alpha.png", "base": {"type": "lambert", "albedo": [0.7, 0.6, 0.2]}})
    scene["primitives"].append({"name": "cut_png", "type": "quad", "bsdf": "cut_png",
                                "transform": {"position": [0.0, 1.02, 0.9], "scale": [0.5, 1.0, 0.5], "rotation": [90, 0, 0]}})


def _stack_with_png(tmpdir, name):
    y, x = np.mgrid[0:32, 0:32]
    alpha = np.where(((x//4 + y//4) % 2) == 0, 255, np.where((x + y) % 3 == 0, 128, 0))
    scenes.write_png(os.path.join(tmpdir, "tq_alpha.png"), np.stack([x*8 % 256, y*8 % 256, (x*y) % 256, alpha], axis=-1), 6, filters=(1, 3), level=6)
    return scenes.cornell(tmpdir, name=name, edit=_with(_panes, _png_cut), **SMALL)


def _with(*edits, **integrator):
    def edit(scene):
        for e in edits:
            e(scene)
        scene["integrator"].update(integrator)
    return edit


def _caps(scene):
    """The quad light and a sphere, a cube and a disk emitter in the fog, away from the blocks"""
    _lift(scene)
    _fog(scene)
    scene["primitives"] += [
        {"name": "bulb", "type": "sphere", "bsdf": "light", "emission": [6, 3, 1], "transform": {"position": [-0.55, 1.5, 0.1], "scale": 0.12, "rotation": [0, 25, 15]}},
        {"name": "brick", "type": "cube", "bsdf": "light", "emission": [2, 5, 3],
         "transform": {"position": [0.7, 1.5, -0.6], "scale": [0.2, 0.12, 0.16], "rotation": [0, 30, 0]}},
        {"name": "sidelight", "type": "disk", "bsdf": "light", "emission": [2, 6, 9],
         "transform": {"position": [-0.97, 1.6, 0.3], "scale": 0.15, "rotation": [0, 0, -90]}}]


def _veil(scene):
    """cornell_instances with the second master's first material see-through"""
    scene["bsdfs"].append({"name": "veil", "type": "transparency", "albedo": 1, "alpha": 0.5, "base": {"type": "lambert", "albedo": [0.6, 0.3, 0.2]}})
    swarm = next(p for p in scene["primitives"] if p["name"] == "swarm")
    swarm["masters"][1]["bsdf"] = ["veil", "rightWall"]


GASES = (("linear", "gas1"), ("quadratic", "gas2"), ("double_exponential", "gas3"), ("pulse", "gas4"),
         ("erlang", {"type": "erlang", "rate": 3.0}), ("davis", {"type": "davis", "alpha": 1.6}))

SMALL = dict(resolution=(48, 27), spp=1)
SCENES = {
    "tq_stack": _stack_with_png,
    "tq_stack_mb3": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_with(_panes, max_bounces=3)),
    "tq_stack_min2": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_with(_panes, min_bounces=2)),
    "tq_fog": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_with(_panes, _fog)),
    "tq_expfog": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_with(_panes, _expfog)),
    "tq_atmosphere": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_with(_panes, _atmosphere)),
    "tq_davis_weinstein": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_with(_panes, _davis_weinstein_fog)),
    "tq_interpolated": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_with(_panes, _interpolated_fog)),
    "tq_fog_smoke": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_with(_lift, _fog_and_smoke)),
    "tq_caps": lambda t, n: scenes.cornell(t, name=n, **SMALL, edit=_caps),
    "tq_mesh": lambda t, n: scenes.cornell_mesh_light(t, name=n, **SMALL, edit=_with(_lift, _fog)),
    "tq_instances": lambda t, n: scenes.cornell_instances(t, name=n, **SMALL, edit=_veil),
}
for _tag, _gas in GASES:
    SCENES["tq_gas_" + _tag] = (lambda g: lambda t, n: scenes.non_exponential(t, g, name=n, **SMALL))(_gas)


def build_scene(name, tmpdir):
    return SCENES[name](str(tmpdir), name + ".json")


def names_of(path):
    """(media, primitives) of a scene file: name -> index in TgHipSceneDesc::media (an `interpolated` medium's two operands ride behind it) and in
    ::objects (the scene's primitives in file order)"""
    with open(path) as f:
        scene = json.load(f)
    media, index = {}, 0
    for m in scene.get("media", []):
        media[m["name"]] = index
        t = m.get("transmittance")
        index += 3 if isinstance(t, dict) and t.get("type") == "interpolated" else 1
    return media, {p["name"]: i for i, p in enumerate(scene["primitives"])}


# ---- rays ---------------------------------------------------------------------------------------------------------------------------------------

def _segments(a, b, infinite=False, tmin=1e-4):
    """rays [n, 8] from the points a towards the points b, ending there -- or never"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = b - a
    length = np.linalg.norm(d, axis=1)
    rays = np.empty((len(a), 8), np.float32)
    rays[:, 0:3] = a
    rays[:, 3] = tmin
    rays[:, 4:7] = d/length[:, None]
    rays[:, 7] = INF if infinite else length
    return rays


def _box(rs, n, lo, hi):
    return rs.uniform(lo, hi, size=(n, 3))


def stack_rays(rs, n, infinite=False):
    """From just below the stack to a level under it, between its panes or above it: 0 to 4 crossings, the end in free space"""
    a = _box(rs, n, (-0.1, 1.27, -0.2), (0.7, 1.33, 0.6))
    levels = np.array([1.31, 1.40, 1.50, 1.60, 1.75])
    b = _box(rs, n, (-0.1, 0.0, -0.2), (0.7, 0.0, 0.6))
    b[:, 1] = levels[np.arange(n) % 5] + rs.uniform(-0.01, 0.01, n)
    b[n//2:, 0] += rs.uniform(-0.6, 0.6, n - n//2)       # some leave the stack sideways
    return _segments(a, b, infinite)


def cutout_rays(rs, n):
    a = _box(rs, n, (-0.9, 0.2, 1.1), (0.9, 1.3, 1.4))
    b = _box(rs, n, (-0.9, 0.2, 0.82), (0.9, 1.3, 0.88))
    upper = b[:, 1] > 0.78                                # (up there is the .png cut-out alone, a third as wide as the row below)
    a[upper, 0] /= 3.0
    b[upper, 0] /= 3.0
    return _segments(a, b)


def blocked_rays(rs, n):
    """Downwards from under the stack: the blocks and the floor"""
    a = _box(rs, n, (-0.8, 1.22, -0.8), (0.8, 1.3, 0.8))
    b = _box(rs, n, (-0.8, -0.5, -0.8), (0.8, -0.4, 0.8))
    return _segments(a, b, True)


def miss_rays(rs, n):
    """Out of the open front: nothing is hit, tmax = inf"""
    a = _box(rs, n, (-0.8, 0.2, 1.0), (0.8, 1.8, 1.5))
    return _segments(a, a + np.column_stack([rs.uniform(-0.3, 0.3, n), rs.uniform(-0.3, 0.3, n), np.ones(n)]), True)


def aimed_rays(rs, n, centre, spread):
    """From the free space above the blocks at points within `spread` of `centre`, never ending: about half reach the primitive there"""
    a = _box(rs, n, (-0.8, 1.25, -0.8), (0.8, 1.9, 0.9))
    return _segments(a, np.asarray(centre) + rs.uniform(-1.0, 1.0, (n, 3))*np.asarray(spread), True)


def edge_on_rays(rs, n):
    """At the quad light (y = 1.98, x in [-0.24, 0.23], z in [-0.22, 0.16]) almost in its plane: the slope is 1e-2 ... 1e-6 of the direction"""
    target = np.column_stack([rs.uniform(-0.2, 0.19, n), np.full(n, 1.98), rs.uniform(-0.18, 0.12, n)])
    phi = rs.uniform(0, 2*np.pi, n)
    slope = 10.0**rs.uniform(-6, -2, n)*np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    d = np.column_stack([np.cos(phi), slope, np.sin(phi)])
    a = target - d*rs.uniform(0.3, 0.7, n)[:, None]
    return _segments(a, target, True)


LIGHT_LO, LIGHT_HI = np.array([-0.24, 1.98, -0.22]), np.array([0.23, 1.98, 0.16])       # the Cornell box's quad light


def light_rays_through_stack(rs, n):
    """From under the pane stack at points of the quad light, ending ON it as a light sample's shadow ray does: tmax is the distance, for every fourth ray one
    ulp more.  The light is reached in the fifth segment, where the distance that remains and the quad's t are an ulp apart either way."""
    a = _box(rs, n, (0.15, 1.0, 0.15), (0.7, 1.3, 0.6))
    b = _box(rs, n, LIGHT_LO + [0.04, 0, 0.04], LIGHT_HI - [0.04, 0, 0.04])
    rays = _segments(a, b)
    rays[3::4, 7] = np.nextafter(rays[3::4, 7], INF)
    return rays


def light_edge_rays(rs, n):
    """At points ON the four edges of the quad light, from the free space under the ceiling: the direction's rounding puts the hit a few 1e-8 inside
    or outside, where Quad::intersect's test and the slab test of the quad's flat box need not agree.  Even rays never end, odd ones end at twice
    the distance."""
    a = _box(rs, n, (-0.8, 1.25, -0.8), (0.8, 1.9, 0.9))
    u = rs.uniform(0.05, 0.95, n)
    edge = np.arange(n) % 4
    b = np.empty((n, 3))
    b[:, 1] = 1.98
    b[:, 0] = np.where(edge == 0, LIGHT_LO[0], np.where(edge == 1, LIGHT_HI[0], LIGHT_LO[0] + u*(LIGHT_HI[0] - LIGHT_LO[0])))
    b[:, 2] = np.where(edge == 2, LIGHT_LO[2], np.where(edge == 3, LIGHT_HI[2], LIGHT_LO[2] + u*(LIGHT_HI[2] - LIGHT_LO[2])))
    rays = _segments(a, b, True)
    rays[1::2, 7] = (2.0*np.linalg.norm(b - a, axis=1)).astype(np.float32)[1::2]
    return rays


def through_tall_box(rs, n):
    """Across the tall block (a forward container of smoke in the fog): (rays, per-ray start medium) -- even rays start in the fog left of it, odd
    ones inside it in the smoke"""
    a = _box(rs, n, (-0.95, 0.2, -0.5), (-0.85, 1.0, -0.15))
    inside = np.arange(n) % 2 == 1
    a[inside] = np.array([-0.335, 0.6, -0.29]) + rs.uniform(-0.1, 0.1, (int(inside.sum()), 3))*[1, 4, 1]
    b = _box(rs, n, (0.15, 0.7, -0.5), (0.3, 1.1, -0.15))
    return _segments(a, b), ["smoke" if i else "fog" for i in inside]


def gas_rays(rs, n):
    """The first box of the non-exponential scene (x -2.1..-0.1, y -1.1..0.9, z -1..1, its front wall a forward boundary of the gas at z = 1):
    inside to inside, from the front into the gas, from the gas out of the front; (rays, per-ray start medium with None for the gas)"""
    inside = lambda k: _box(rs, k, (-2.0, 0.45, 0.2), (-0.2, 0.8, 0.9))          # (above the blocks)
    front = lambda k: _box(rs, k, (-2.0, 0.3, 1.2), (-0.2, 0.8, 1.8))
    k = n//3
    rays = np.concatenate([_segments(inside(k), inside(k)), _segments(front(k), inside(k)), _segments(inside(n - 2*k), front(n - 2*k))])
    return rays, [None]*k + ["-"]*k + [None]*(n - 2*k)


# ---- groups -------------------------------------------------------------------------------------------------------------------------------------

def _group(scene, leg, rays, medium=None, end_cap=None, bounce=0, starts=False, ends=False, media=None):
    return dict(scene=scene, leg=leg, rays=np.ascontiguousarray(rays, np.float32), medium=medium, end_cap=end_cap, bounce=int(bounce),
                starts=bool(starts), ends=bool(ends), media=media)


NSTACK, NEDGE = 256, 64


def make_groups():
    # (a group that keeps the first rays of a larger draw: the draws are as they were when the groups behind it were tuned)
    rs = np.random.RandomState(SEED)
    g = []
    # no medium: crossings, blocked, cut-outs, a miss with tmax = inf
    g.append(_group("tq_stack", "stack", stack_rays(rs, 160)))
    g.append(_group("tq_stack", "stack_blocked", stack_rays(rs, 80, infinite=True)))
    g.append(_group("tq_stack", "blocked", blocked_rays(rs, 48)))
    g.append(_group("tq_stack", "cutouts", cutout_rays(rs, 288)))
    g.append(_group("tq_stack", "miss", miss_rays(rs, 32)))
    # the bounce limits on the stack
    for bounce in (0, 1):
        g.append(_group("tq_stack_mb3", "max_bounces", stack_rays(rs, 120)[:96], bounce=bounce))
    for bounce in (0, 1, 2):
        g.append(_group("tq_stack_min2", "min_bounces", stack_rays(rs, 80)[:72], bounce=bounce))
    # the camera's medium around the stack: fractional alpha inside a medium, every flag pair
    for scene, tag in (("tq_fog", "homogeneous"), ("tq_expfog", "exponential"), ("tq_atmosphere", "atmosphere"),
                       ("tq_davis_weinstein", "davis_weinstein"), ("tq_interpolated", "interpolated")):
        for starts, ends in FLAG_PAIRS:
            g.append(_group(scene, "medium_" + tag, stack_rays(rs, 40)[:32], medium="fog", starts=starts, ends=ends))
    g.append(_group("tq_fog", "miss_in_fog", miss_rays(rs, 16), medium="fog"))
    # the non-exponential gases behind their forward front wall, the start medium per ray
    for tag, gas in GASES:
        name = gas if isinstance(gas, str) else "gas1"
        for starts, ends in FLAG_PAIRS:
            rays, media = gas_rays(rs, 36)
            g.append(_group("tq_gas_" + tag, "medium_" + tag, rays, medium=name, starts=starts, ends=ends, media=[m or name for m in media]))
    # into the smoke and out again through forward boundaries
    for starts, ends in FLAG_PAIRS:
        rays, media = through_tall_box(rs, 32)
        g.append(_group("tq_fog_smoke", "enter_leave", rays, medium="fog", starts=starts, ends=ends, media=media))
    # end caps in the fog
    for cap, centre, spread in (("light", (-0.005, 1.98, -0.03), (0.4, 0.0, 0.35)), ("bulb", (-0.55, 1.5, 0.1), (0.2, 0.2, 0.2)),
                                ("brick", (0.7, 1.5, -0.6), (0.2, 0.12, 0.16)), ("sidelight", (-0.97, 1.6, 0.3), (0.0, 0.2, 0.2))):
        g.append(_group("tq_caps", "cap_" + cap, aimed_rays(rs, 64, centre, spread), medium="fog", end_cap=cap, ends=True))
    g.append(_group("tq_caps", "cap_edge_on", edge_on_rays(rs, 96)[:48], medium="fog", end_cap="light", ends=True))
    g.append(_group("tq_mesh", "cap_mesh", aimed_rays(rs, 64, (0.1, 1.55, 0.0), (0.35, 0.3, 0.35)), medium="fog", end_cap="lamp", ends=True))
    # through instances
    a, b = _box(rs, 640, (-0.9, 0.1, -0.9), (0.9, 1.7, 0.9)), _box(rs, 640, (-0.9, 0.1, -0.9), (0.9, 1.7, 0.9))
    g.append(_group("tq_instances", "instances", _segments(a, b)))
    # the quad light behind the pane stack and at its edges (a stream of their own: the groups above stay as they are)
    rs = np.random.RandomState(SEED + 1)
    g.append(_group("tq_fog", "cap_light_behind_stack", light_rays_through_stack(rs, NSTACK), medium="fog", end_cap="light", ends=True))
    g.append(_group("tq_caps", "cap_light_edges", light_edge_rays(rs, NEDGE), medium="fog", end_cap="light", ends=True))
    return g


# ---- the golden ---------------------------------------------------------------------------------------------------------------------------------

def load_golden():
    """The groups with the reference's answers: every group gains rgb [n, 3] uint32 (the floats' bits), crossed [n] and end [n] (END_*)"""
    z = np.load(GOLDEN, allow_pickle=False)
    table = json.loads(str(z["groups"]))
    groups = []
    for k, t in enumerate(table):
        g = dict(t)
        for part in ("rays", "rgb", "crossed", "end"):
            g[part] = z["g%03d_%s" % (k, part)]
        groups.append(g)
    return groups


def census(groups):
    """leg -> number of cases that reach it with the answer the leg is about"""
    c = {}

    def add(leg, mask):
        c[leg] = c.get(leg, 0) + int(np.count_nonzero(mask))

    for g in groups:
        rgb = g["rgb"].view(np.float32)
        lit = (rgb != 0).any(axis=1)
        fractional = lit & (rgb != 1).any(axis=1)
        crossed, end, leg = g["crossed"], g["end"], g["leg"]
        through = (end == END_MISS) | (end == END_CAP)
        if g["medium"] is None and g["end_cap"] is None and "bounces" not in leg:
            for k in range(3):
                add("crossed_%d" % k, through & lit & (crossed == k))
            add("crossed_3_or_more", through & lit & (crossed >= 3))
        add("blocked_first_segment", (end == END_OPAQUE) & (crossed == 0) & ~lit)
        add("blocked_behind_a_crossing", (end == END_OPAQUE) & (crossed >= 1) & ~lit)
        add("transparency_zero", (end == END_ZERO_ALPHA) & ~lit)
        if leg == "cutouts":
            # which cut-out the ray meets: where it crosses their plane z = 0.9
            r = g["rays"].astype(np.float64)
            at = r[:, 0:3] + r[:, 4:7]*((0.9 - r[:, 2])/r[:, 6])[:, None]
            for name, (x0, x1, y0, y1) in CUTOUTS.items():
                inside = (at[:, 0] > x0) & (at[:, 0] < x1) & (at[:, 1] > y0) & (at[:, 1] < y1)
                add("transparency_zero_" + name, inside & (end == END_ZERO_ALPHA) & ~lit)
        if leg.startswith("medium_"):
            # (between two points inside the medium the linear and the pulse transmittance are a delta's value, 0 almost everywhere: the one answer)
            by_model = (leg[len("medium_"):], bool(g["starts"]), bool(g["ends"])) in ZERO_BY_MODEL
            add("%s_%d%d" % (leg, g["starts"], g["ends"]), through if by_model else through & lit)
            if g["scene"] == "tq_fog":
                add("fractional_alpha_in_medium", through & fractional & (crossed >= 2))   # (two panes up: the alpha 0.6 one is crossed)
        if leg == "enter_leave":
            add("enter_and_leave", through & fractional & (crossed >= 2))
        if g["media"] is not None:
            add("start_medium_per_ray", through & fractional)
        if leg == "max_bounces":
            add("bounce_ends_at_max_minus_1", through & lit & (g["bounce"] + crossed == 2))
            add("bounce_ends_at_max", (end == END_MAX_BOUNCES) & ~lit & (g["bounce"] + crossed == 3))
        if leg == "min_bounces":
            add("min_bounces_above_count", through & ~lit & (g["bounce"] + crossed < 2))
            add("min_bounces_below_count", through & lit & (g["bounce"] + crossed >= 2))
        if leg == "cap_light_behind_stack":
            # the quad the ray is aimed at, behind four crossings with the distance that remains an ulp from the quad's t: found -- or not found by
            # the scene's tree although Quad::intersect finds it (Embree's slab test of its flat box), or out of reach for Quad::intersect too
            add("cap_quad_reached_behind_crossings", (end == END_CAP) & fractional & (crossed >= 1))
            add("cap_quad_culled_by_the_box", (end == END_CULLED) & fractional & (crossed >= 1))
            add("cap_quad_behind_tmax", (end == END_MISS) & fractional & (crossed >= 1))
        elif leg == "cap_light_edges":
            add("cap_quad_edge_reached", (end == END_CAP) & fractional)
            add("cap_quad_edge_missed", end == END_OPAQUE)
        elif leg.startswith("cap_"):
            add(leg + "_reached", (end == END_CAP) & fractional)
            if leg != "cap_edge_on":
                add(leg + "_missed", end != END_CAP)
        if leg == "instances":
            add("through_instances", through & fractional & (crossed >= 1))
            add("blocked_by_instances", (end == END_OPAQUE))
        if leg in ("miss", "miss_in_fog"):
            add("nothing_hit_tmax_inf", (end == END_MISS) & np.isinf(g["rays"][:, 7]) & (crossed == 0))
    return c


CUTOUTS = {"checker": (-0.85, -0.35, 0.25, 0.75), "disk": (-0.25, 0.25, 0.25, 0.75), "blade": (0.35, 0.85, 0.25, 0.75), "png": (-0.25, 0.25, 0.77, 1.27)}
ZERO_BY_MODEL = {("linear", False, False), ("pulse", False, False)}
MEDIUM_TAGS = ("homogeneous", "exponential", "atmosphere", "davis_weinstein", "interpolated") + tuple(t for t, _ in GASES)
LEGS = ["crossed_0", "crossed_1", "crossed_2", "crossed_3_or_more", "blocked_first_segment", "blocked_behind_a_crossing", "transparency_zero",
        "fractional_alpha_in_medium", "enter_and_leave", "start_medium_per_ray", "bounce_ends_at_max_minus_1", "bounce_ends_at_max",
        "min_bounces_above_count", "min_bounces_below_count", "cap_edge_on_reached", "through_instances", "blocked_by_instances",
        "nothing_hit_tmax_inf", "cap_quad_reached_behind_crossings", "cap_quad_culled_by_the_box", "cap_quad_behind_tmax", "cap_quad_edge_reached",
        "cap_quad_edge_missed"] + \
       ["transparency_zero_" + c for c in ("checker", "disk", "blade", "png")] + \
       ["medium_%s_%d%d" % (t, s, e) for t in MEDIUM_TAGS for s, e in FLAG_PAIRS] + \
       ["cap_%s_%s" % (c, w) for c in ("light", "bulb", "brick", "sidelight", "mesh") for w in ("reached", "missed")]
