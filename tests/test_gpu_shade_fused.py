"""k_shade_fused -- class 0, the escaped paths and the scene's one further shading class in ONE launch per iteration ("shade_fused", default 1)
-- against the per-class launches it replaces ("shade_fused" = 0), through the C ABI.

The fused launch runs the same per-slot code on the same slots and ORs the same bits into the same queue bitmaps, so nothing is compared
against a tolerance: framebuffer sums and sample counts are equal bit for bit, for the uniform sampler and for Sobol' + adaptive passes
(the FEAT_QMC twins).  Every image is rendered once per setting, in this process; there are no reference files.

The images are small (64x48), so the whole pass is below the shim's tail threshold and k_tail -- which the option does not touch -- would
take every iteration: the renders switch it off ("tail_kernel" = 0), which leaves the wavefront loop the option is about.  "time_kernels"
makes the shim count its shading launches (TgHipCounters::launches_shade); each case asserts that there were some."""
import pytest

import tungsten_amd as tg
from tungsten_amd import workloads

pytestmark = pytest.mark.gpu

W, H = 64, 48
_DIELECTRIC = {"type": "dielectric", "ior": 1.5, "albedo": 1}
_SOBOL_ADAPTIVE = {"adaptive_sampling": True, "stratified_sampler": True}


def _three_classes(scene):
    """Lambert floor (class 0), a conductor stand (class 1), dielectric "Material" (class 2)."""
    workloads._mt_material(_DIELECTRIC)(scene)
    for i, b in enumerate(scene["bsdfs"]):
        if b["name"] == "Stand":
            scene["bsdfs"][i] = {"name": "Stand", "albedo": 1, "type": "rough_conductor", "material": "Cu", "distribution": "beckmann", "roughness": 0.1}


CASES = {
    # name: (variant keywords, classes besides class 0)
    "coat_uniform": (dict(spp=8), 1),
    "coat_sobol_adaptive": (dict(spp=8, spp_step=4, renderer=_SOBOL_ADAPTIVE), 1),      # two passes of 4 spp
    "glass_uniform": (dict(spp=8, edit=workloads._mt_material(_DIELECTRIC)), 1),
    "three_classes": (dict(spp=8, edit=_three_classes), 2),
}

_rendered = {}


def _render(name, fused, tmp_path_factory):
    key = (name, fused)
    if key not in _rendered:
        kw, _ = CASES[name]
        tmp = tmp_path_factory.mktemp("%s_%d" % (name, fused))
        path = workloads.materialtest(tmp, resolution=(W, H), name=name + ".json", **kw)
        r = tg.Renderer(path, seed=tg.DEFAULT_SEED)
        try:
            r.set_option("shade_fused", fused)
            r.set_option("tail_kernel", 0)
            r.set_option("time_kernels", 1)
            passes = 0
            done = False
            while not done:
                done = r.step()
                passes += 1
            _, ssum, count = r.image()
            c = r.counters()
            _rendered[key] = (ssum.copy(), count.copy(), int(c.launches_shade), int(c.samples), passes)
        finally:
            r.close()
    return _rendered[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_and_per_class_launches_render_the_same_bits(name, tmp_path_factory):
    ssum1, count1, launches1, samples1, passes1 = _render(name, 1, tmp_path_factory)
    ssum0, count0, launches0, samples0, passes0 = _render(name, 0, tmp_path_factory)
    print("%s: launches_shade fused %d, per class %d; %d samples in %d passes" % (name, launches1, launches0, samples1, passes1))
    assert passes1 == passes0 == (2 if "adaptive" in name else 1)
    assert samples1 == samples0 and samples1 > 0
    if "adaptive" not in name:
        assert (count1 == 8).all()
    assert count1.tobytes() == count0.tobytes()
    assert ssum1.tobytes() == ssum0.tobytes()
    assert launches1 > 0 and launches0 > 0               # the wavefront loop ran (not k_tail alone)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_launch_is_taken_for_one_further_class_only(name, tmp_path_factory):
    further = CASES[name][1]
    launches1 = _render(name, 1, tmp_path_factory)[2]
    launches0 = _render(name, 0, tmp_path_factory)[2]
    if further == 1:
        assert launches1 < launches0                      # one launch instead of two per iteration and part
        assert 2*launches1 == launches0
    else:
        assert launches1 == launches0                     # three classes: the per-class launches, whatever the option says

