"""How a batch of the wavefront loop is launched part by part (tungsten_hip.hip: runBatch): what whole renders with "time_kernels" on count --
(launches_trace_closest, launches_trace_shadow, launches_shade, tail_launches, iterations) -- stated as literals, and every render's image held to the
one-part, no-tail image of its scene bit for bit.  The tuples were recorded on the commit before the batch's parts had one description and one launch
loop, by running these renders there twice (both runs gave the same tuples); with "time_kernels" on every part's launches are bracketed and
counted, so a part that is launched twice, not at all, or outside its bracket moves a tuple.

The renders: materialtest 192 x 108 at 8 spp without the tail kernel on 1, 2, 4 and 8 streams, checked every iteration and every third one (the
split loop, every part's launches counted); the same scene at 16 x 9 and 4 spp in four-sample items on 8 streams and on 1 -- work items are counted
over whole 16 x 16 tiles (PassPlan.cpp: tiles * 256 * samples / samples per item), so the image's one tile is 256 items: fewer than the
2 * 8 * 64 = 1024 a split into eight asks for, so the 8 parts wanted fall back to ONE part, and the render launches what the one-stream render
launches.  ("chunk_samples" = 4 is set for that: in the one-sample items a pass this short gets by default the tile is 1024 items, enough for eight
parts, and the commit before launched (64, 64, 64, 0, 8) for it.)  materialtest 192 x 108 on 2 streams with the tail kernel from 30000 live paths
on: each part ends in a launch of k_tail behind the tail's fork, joined after it -- the render must count a tail launch.  cornell_instances
160 x 90 with the same options: a split loop over an instanced scene, which is never eligible for the tail kernel (LaunchChoice.cpp) and counts none."""
import math

import pytest

import scenes
import tungsten_amd as tg

pytestmark = pytest.mark.gpu

SEED = tg.DEFAULT_SEED

SHAPES = {
    "materialtest": lambda tmp: scenes.materialtest(tmp, resolution=(192, 108), spp=8),
    "materialtest_tiny": lambda tmp: scenes.materialtest(tmp, resolution=(16, 9), spp=4),
    "cornell_instances": lambda tmp: scenes.cornell_instances(tmp, **dict(scenes.GOLDEN_CASES["cornell_instances"][1], resolution=(160, 90), spp=8)),
}

# name -> (shape, options)
RENDERS = {}
for _streams in (1, 2, 4, 8):
    for _check in (1, 3):
        RENDERS["materialtest streams=%d check_interval=%d" % (_streams, _check)] = ("materialtest", dict(tail_kernel=0, streams=_streams, check_interval=_check))
RENDERS["tiny streams=8"] = ("materialtest_tiny", dict(tail_kernel=0, chunk_samples=4, streams=8))
RENDERS["tiny streams=1"] = ("materialtest_tiny", dict(tail_kernel=0, chunk_samples=4, streams=1))
RENDERS["materialtest tail on 2 streams"] = ("materialtest", dict(tail_kernel=1, tail_threshold=30000, streams=2))
RENDERS["cornell_instances tail on 2 streams"] = ("cornell_instances", dict(tail_kernel=1, tail_threshold=30000, streams=2))

# (launches_trace_closest, launches_trace_shadow, launches_shade, tail_launches, iterations), recorded on the parent commit (see above)
LAUNCHES_BEFORE = {
    "materialtest streams=1 check_interval=1": (10, 10, 10, 0, 10),
    "materialtest streams=1 check_interval=3": (12, 12, 12, 0, 12),
    "materialtest streams=2 check_interval=1": (20, 20, 20, 0, 10),
    "materialtest streams=2 check_interval=3": (24, 24, 24, 0, 12),
    "materialtest streams=4 check_interval=1": (40, 40, 40, 0, 10),
    "materialtest streams=4 check_interval=3": (48, 48, 48, 0, 12),
    "materialtest streams=8 check_interval=1": (80, 80, 80, 0, 10),
    "materialtest streams=8 check_interval=3": (96, 96, 96, 0, 12),
    "tiny streams=8": (16, 16, 16, 0, 16),
    "tiny streams=1": (16, 16, 16, 0, 16),
    "materialtest tail on 2 streams": (16, 16, 16, 1, 8),
    "cornell_instances tail on 2 streams": (64, 64, 128, 0, 32),
}

_paths, _base = {}, {}


def render(shape, tmp_path_factory, **opts):
    if shape not in _paths:
        _paths[shape] = SHAPES[shape](tmp_path_factory.mktemp(shape))
    r = tg.Renderer(_paths[shape], seed=SEED)
    try:
        for k, v in opts.items():
            r.set_option(k, v)
        r.render()
        _, ssum, count = r.image()
        return ssum, count, r.counters()
    finally:
        r.close()


def base_image(shape, tmp_path_factory):
    """The image of the shape's scene on one stream without the tail kernel (and without the timing events), rendered once"""
    if shape not in _base:
        _base[shape] = render(shape, tmp_path_factory, streams=1, tail_kernel=0)[:2]
    return _base[shape]


def launches(c):
    return (int(c.launches_trace_closest), int(c.launches_trace_shadow), int(c.launches_shade), int(c.tail_launches), int(c.iterations))


@pytest.mark.parametrize("name", sorted(RENDERS))
def test_a_render_launches_what_it_did_and_renders_the_one_part_image(name, tmp_path_factory):
    shape, opts = RENDERS[name]
    if shape.startswith("materialtest") and not scenes.have_materialtest():
        pytest.skip("materialtest assets (assets/) not present")
    base, base_count = base_image(shape, tmp_path_factory)
    ssum, count, c = render(shape, tmp_path_factory, time_kernels=1, **opts)
    got = launches(c)
    print("%s: launches (closest, shadow, shade, tail, iterations) %s, ms (closest, shade, shadow) %r" % (name, got, (c.ms_trace_closest, c.ms_shade, c.ms_trace_shadow)))
    assert (count == base_count).all() and (count > 0).all()
    assert ssum.tobytes() == base.tobytes(), "image changed with %r" % (opts,)
    for ms in (c.ms_trace_closest, c.ms_shade, c.ms_trace_shadow):
        assert math.isfinite(ms) and ms >= 0.0
    assert got == LAUNCHES_BEFORE[name]
    if name == "materialtest tail on 2 streams":
        assert got[3] > 0                # (k_tail ran: its fork and join were issued)
    if name == "tiny streams=8":         # (the fallback: eight parts wanted, one part's launches counted)
        assert got == LAUNCHES_BEFORE["tiny streams=1"]

