"""The `disk`, `blade` and `ies` textures on the host (no GPU): every case of tests/texture_cases.py loads and flattens, each new texture arrives
with the type, the parameters and the average the reference computes -- in float32, in its order of operations --, and the IES bake is held to
the reference itself: the unchanged CPU oracle renders the flattened IES scenes (an `ies` texture is an ordinary scalar bitmap there) and must
return the reference's per-sample radiance (tests/golden/tex_ies_*_samples.npz) bit for bit, which pins the parser and the bake."""
import ctypes as C
import ctypes.util
import json
import os
import subprocess

import numpy as np
import pytest

import scenes
import texture_cases
import tungsten_amd as tg
from test_oracle_golden import _oracle_samples
from tungsten_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PI = F(3.1415926536)                      # math/Angle.hpp:8
TWO_PI = PI*F(2.0)
INV_TWO_PI = F(0.5)*(F(1.0)/PI)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float]


def sinf(x):
    return F(_libm.sinf(float(x)))


def cosf(x):
    return F(_libm.cosf(float(x)))


def _vec(v):
    return np.array([v, v, v] if not isinstance(v, (list, tuple)) else v, F)


def blade_init(blades, angle):
    """BladeTexture::init (textures/BladeTexture.cpp:22-31) in float32 with the host's sinf / cosf."""
    n = F(blades)
    blade_angle = TWO_PI/n
    sin_a, cos_a = sinf(blade_angle*F(0.5)), cosf(blade_angle*F(0.5))
    area = F(0.25)*F(0.5)*n*sinf(blade_angle)
    k = sinf(PI/n)
    return dict(blade_angle=blade_angle, area=area, edge=(-sin_a*F(2.0)*k, cos_a*F(2.0)*k), normal=(cos_a, sin_a), angle=F(angle))


def _flatten(name, tmp_path):
    mk, kw = texture_cases.CASES[name]
    path = mk(tmp_path, name=name + ".json", **kw)
    with open(path) as f:
        scene = json.load(f)
    return tg.FlattenedScene(path), scene


def _textures(d):
    return [d.textures[i] for i in range(d.num_textures)]


def _same(a, b):
    return (np.asarray(list(a) if hasattr(a, "__len__") else [a], F).view(np.uint32) == np.asarray(list(b) if hasattr(b, "__len__") else [b], F).view(np.uint32)).all()


def _texels(d, t):
    n = t.w*t.h
    return np.ctypeslib.as_array(d.texels, shape=(d.num_texel_floats,))[t.texel_offset:t.texel_offset + n].copy()


@pytest.mark.parametrize("name", sorted(texture_cases.CASES))
def test_case_flattens_with_the_reference_parameters(name, tmp_path):
    flat, scene = _flatten(name, tmp_path)
    d = flat.desc.contents
    tex = _textures(d)
    declared = texture_cases.declared_textures(scene)
    assert declared, "a texture case without a new texture"
    for key, js in declared:
        power = key == "power"
        if js["type"] == "disk":
            value = _vec(js.get("value", 1.0))
            found = [t for t in tex if t.type == capi.TGHIP_TEX_DISK and (power or _same(t.value, value))]
            assert found, "%s: no flattened disk texture with value %s" % (name, value)
            for t in found:
                v = np.array(list(t.value), F)
                assert _same(t.avg, PI*F(0.25)*v)                     # DiskTexture::average
                assert t.texel_offset == -1 and t.dist_offset == -1 and t.w == 0 and t.h == 0
        elif js["type"] == "blade":
            value = _vec(js.get("value", 1.0))
            blades = js.get("blades", 6)
            b = blade_init(blades, js["angle"] if "angle" in js else F(0.5)*PI/F(6))
            found = [t for t in tex if t.type == capi.TGHIP_TEX_BLADE and t.res_u == blades and _same(t.scale, b["angle"]) and (power or _same(t.value, value))]
            assert found, "%s: no flattened blade texture with %d blades, angle %s, value %s" % (name, blades, b["angle"], value)
            for t in found:
                v = np.array(list(t.value), F)
                if power:
                    # Primitive::prepareForRender: the clone's value scaled by ONE factor (the quad's powerToRadianceFactor)
                    ratio = v/value
                    assert np.allclose(ratio, ratio[0], rtol=3e-7) and ratio[0] > 0
                assert _same(t.on_color, [b["blade_angle"], b["area"], F(1.0)/b["area"]])
                assert _same(t.off_color, [b["normal"][0], b["normal"][1], b["edge"][0]]) and _same(t.pad, b["edge"][1])
                assert _same(t.avg, b["area"]*v)                      # BladeTexture::average
                assert t.texel_offset == -1 and t.dist_offset == -1
        else:
            res = js.get("resolution", 256)
            found = [t for t in tex if t.type == capi.TGHIP_TEX_BITMAP and (t.w, t.h) == (2*res, res) and not (t.flags & capi.TGHIP_TEXF_RGB)]
            assert found, "%s: no flattened %d x %d scalar bitmap" % (name, 2*res, res)
            for t in found:
                # BitmapTexture() leaves _valid false and IesTexture never sets it: interpolate on, clamp off, but looked up as an invalid bitmap
                assert t.flags & capi.TGHIP_TEXF_LINEAR and not (t.flags & (capi.TGHIP_TEXF_CLAMP | capi.TGHIP_TEXF_VALID))
                texels = _texels(d, t)
                assert texels.max() == F(1.0) and texels.min() >= 0.0   # divided by the maximum
                avg = np.cumsum(texels/F(t.w*t.h), dtype=F)[-1]         # BitmapTexture::init accumulates texel/(w h) in order
                assert _same(t.avg, [F(t.scale)*avg]*3)
                assert (t.scale == 1.0) != power                        # scaleValues of a `power` bitmap scales _scale (BitmapTexture.cpp:457-460)
    # the environment of a sampled infinite sphere gets its Distribution2D only where the emission is a bitmap
    for i in range(d.num_infinite_lights):
        env = d.textures[d.objects[d.infinite_lights[i]].emission]
        assert (env.dist_offset >= 0) == (env.type == capi.TGHIP_TEX_BITMAP)
    flat.close()


def test_texture_struct_keeps_its_layout():
    """sizeof(TgHipTexture) and the offsets of its fields are the parent's: oracle/oracle.c and oracle/ref_binding compile against the same header."""
    assert C.sizeof(capi.TgHipTexture) == 96
    offsets = {n: getattr(capi.TgHipTexture, n).offset for n, _ in capi.TgHipTexture._fields_}
    assert offsets == {"type": 0, "flags": 4, "w": 8, "h": 12, "value": 16, "scale": 28, "on_color": 32, "res_u": 44, "off_color": 48, "res_v": 60,
                       "avg": 64, "pad": 76, "texel_offset": 80, "dist_offset": 88}
    assert (capi.TGHIP_TEX_CONSTANT, capi.TGHIP_TEX_CHECKER, capi.TGHIP_TEX_BITMAP, capi.TGHIP_TEX_DISK, capi.TGHIP_TEX_BLADE) == (0, 1, 2, 3, 4)
    # (the header still compiles as C with the two new enumerators; tests/test_abi.py compares the sizes with the C compiler's)
    src = '#include "tungsten_hip.h"\nint a[TGHIP_TEX_DISK == 3 && TGHIP_TEX_BLADE == 4 && sizeof(TgHipTexture) == 96 ? 1 : -1];\n'
    assert subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src.encode()).returncode == 0


def test_an_unknown_texture_type_is_still_refused(tmp_path):
    def edit(scene):
        scene["bsdfs"][0]["albedo"] = {"type": "marble", "value": 0.5}
    with pytest.raises(tg.TungstenError) as e:
        tg.FlattenedScene(scenes.cornell(tmp_path, resolution=(16, 9), spp=1, edit=edit, name="marble.json"))
    assert "Texture type 'marble' is outside the path_tracer_hip hot-path scope" in str(e.value)


@pytest.mark.parametrize("name", texture_cases.IES_CASES)
def test_oracle_renders_the_ies_bake_like_the_reference(name, tmp_path):
    """The unchanged oracle on the flattened scene against the reference's own samples: float32 == in all three channels of all 10 368 samples."""
    mk, kw = texture_cases.CASES[name]
    gold = np.load(os.path.join(scenes.GOLDEN, name + "_samples.npz"))
    ref = gold["samples"]
    got = _oracle_samples(mk, kw, name, tmp_path, ref, int(gold["seed"]))
    assert (got == ref).all(), "%s: %d samples are not the reference's" % (name, int((got != ref).any(axis=-1).sum()))
    assert ref.max() > 0


def test_the_card_case_visits_every_texel(tmp_path):
    """tex_ies_card: one nearest lookup of the 32 x 16 bake per sample -- and no texel value of the bake that no sample returned."""
    flat, _ = _flatten("tex_ies_card", tmp_path)
    d = flat.desc.contents
    t = [t for t in _textures(d) if t.type == capi.TGHIP_TEX_BITMAP][0]
    assert (t.w, t.h) == (32, 16)
    texels = _texels(d, t)
    flat.close()
    ref = np.load(os.path.join(scenes.GOLDEN, "tex_ies_card_samples.npz"))["samples"]
    assert (ref[..., 0] == ref[..., 1]).all() and (ref[..., 0] == ref[..., 2]).all()
    assert (ref == ref[:, :, :1]).all()                     # dirac filter: the samples of a pixel are one ray
    seen = set(ref[..., 0].ravel().view(np.uint32).tolist())
    assert set(texels.view(np.uint32).tolist()) <= seen


def test_a_missing_ies_file_gives_inv_two_pi(tmp_path):
    path = texture_cases.build(tmp_path, name="missing.json", edit=texture_cases.missing_ies, **texture_cases.SIZE)
    assert not os.path.exists(os.path.join(str(tmp_path), texture_cases.MISSING_IES))
    flat = tg.FlattenedScene(path)
    d = flat.desc.contents
    found = [t for t in _textures(d) if t.type == capi.TGHIP_TEX_BITMAP]
    assert len(found) == 1 and (found[0].w, found[0].h) == (16, 8)
    texels = _texels(d, found[0])
    assert texels.size == 128 and (texels.view(np.uint32) == INV_TWO_PI.view(np.uint32)).all()
    flat.close()
