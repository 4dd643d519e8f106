"""tghip_query_transmittance on device memory: kernel milliseconds, rays per second and rounds on four batches, and on a scene without a forward
lobe and without a medium its ratio to tghip_query_rays (occluded) on the same rays (profiles/transmittance_query/bench.txt).

    python tools/transmittance_query_bench.py [--width 1280 --height 720 --rounds 9] > profiles/transmittance_query/bench.txt

  shadow   materialtest with its "Material" a `transparency` of alpha 0.5: from the first hit of every pixel's camera ray one ray towards a fixed
           point high above the scene (a light's place), starting on the surface -- shadow rays through and around the see-through model.
  fog      the Cornell box of tests/transmittance_cases.py with its stack of see-through panes, in the camera's fog: one camera ray per pixel, ending after
           5.8 to 7.8 units -- inside the box (its open front is 5.8 from the camera, its back wall 7.8), so most rays end in the fog.
  random   uniformly random origins and directions in materialtest_transparency's bounds, every 7th with a finite tmax.
  plain    materialtest as shipped -- no forward lobe, no medium, so one round --: camera rays and random rays, alternated with
           tghip_query_rays TGHIP_QUERY_OCCLUDED on the same tensors; the ratio of the medians is the cost over the occlusion query.
In one process, after a warm-up of every path, `rounds` alternations; HIP-event times through the *_kernel_time getters (for the transmittance
query from its first launch to its last: the one-word read-backs between the rounds are inside).  Medians and spreads (min .. max)."""
import argparse
import ctypes as C
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scenes  # noqa: E402
import transmittance_cases as tc  # noqa: E402
import tungsten_amd as tg  # noqa: E402
from ray_query_bench import camera_rays, stats  # noqa: E402
from surface_query_bench import random_rays  # noqa: E402

LIGHT = np.array([1.5, 6.0, 2.5])
VEIL = {"type": "transparency", "alpha": 0.5, "albedo": 1, "base": {"type": "lambert", "albedo": [0.6, 0.4, 0.3]}}


def shadow_rays(r, rays):
    """From every camera ray's first hit towards LIGHT, ending there"""
    s = r.query_surface(rays)
    p = s["p"][s["rec"] >= 0].astype(np.float64)
    d = LIGHT - p
    dist = np.linalg.norm(d, axis=1)
    return np.concatenate([p, np.full((len(p), 1), 5e-4), d/dist[:, None], dist[:, None]], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    lib = tg.lib
    dev = torch.device("cuda", 0)
    ms, rounds = C.c_double(0.0), C.c_uint32(0)
    print("transmittance_query_bench: %d x %d rays on %s, library %s" % (
        a.width, a.height, torch.cuda.get_device_name(0), os.path.basename(os.environ.get("TUNGSTEN_AMD_LIB", tg.capi.LIB_PATH))))
    size = dict(resolution=(a.width, a.height), spp=1)
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []          # (label, renderer, rays, keyword arguments of the query, alternate with the occlusion query)
        veil = tg.Renderer(scenes.materialtest(tmp, name="materialtest_transparency.json", edit=scenes._mt_material(VEIL), **size))
        flat = tg.FlattenedScene(scenes.materialtest(tmp, name="materialtest_plain.json", **size))
        cam = camera_rays(flat)
        rnd = random_rays(flat, len(cam))
        flat.close()
        jobs.append(("shadow  materialtest_transparency, camera hits to a light", veil, shadow_rays(veil, cam), dict(medium=None, starts_on_surface=True), False))
        jobs.append(("random  materialtest_transparency", veil, rnd, dict(medium=None), False))
        fog_scene = scenes.cornell(tmp, name="fog_full.json", edit=tc._with(tc._panes, tc._fog), **size)
        fog_flat = tg.FlattenedScene(fog_scene)
        fog_cam = camera_rays(fog_flat)
        fog_flat.close()
        # the segments end inside the box, between its open front and its back wall: rays that end in the fog, or on a wall before they get there
        fog_cam[:, 7] = np.random.RandomState(13).uniform(5.8, 7.8, len(fog_cam)).astype(np.float32)
        fog = tg.Renderer(fog_scene)
        jobs.append(("fog     Cornell box with the pane stack in fog, camera rays that end inside the box", fog, fog_cam, dict(medium="camera"), False))
        plain = tg.Renderer(scenes.materialtest(tmp, name="materialtest_plain2.json", **size))
        jobs.append(("plain   materialtest, camera rays", plain, cam, dict(medium=None), True))
        jobs.append(("plain   materialtest, random rays", plain, rnd, dict(medium=None), True))

        for label, r, rays, kw, alternate in jobs:
            ctx, n = r.context(), len(rays)
            want = r.query_transmittance(rays, **kw)
            lib.tghip_query_transmittance_rounds(ctx, C.byref(rounds))
            lit = (want["rgb"] != 0).any(axis=1)
            print("\n%s: %d rays, %d rounds, %d lit, %d crossed something (up to %d)" % (
                label, n, rounds.value, int(lit.sum()), int((want["crossed"] > 0).sum()), int(want["crossed"].max())))
            drays = torch.from_numpy(rays).to(dev)
            dout = torch.empty((n, 4), dtype=torch.float32, device=dev)
            docc = torch.empty((n,), dtype=torch.uint8, device=dev)
            if alternate:
                occ = r.query_rays(rays, "occluded")
                same = (want["rgb"] == (1 - occ.astype(np.float32))[:, None]).all()
                print("  rgb == 1 - occluded on every ray: %s" % same)
                if not same:
                    raise SystemExit("answers differ")
            t_tr, t_occ = [], []
            for k in range(a.rounds + 1):                   # round 0 warms every path and is not counted
                if alternate:
                    r.query_rays_into(drays, docc, "occluded")
                    lib.tghip_query_rays_kernel_time(ctx, C.byref(ms))
                    if k:
                        t_occ.append(ms.value)
                r.query_transmittance_into(drays, dout, **kw)
                lib.tghip_query_transmittance_kernel_time(ctx, C.byref(ms))
                if k:
                    t_tr.append(ms.value)
            if dout.cpu().numpy().tobytes() != want.tobytes():
                raise SystemExit("device-memory answers differ from host-memory answers")
            med = float(np.median(t_tr))
            print("  query_transmittance ms          %s   %.1f Mrays/s" % (stats(t_tr), n/med/1e3))
            if alternate:
                mo = float(np.median(t_occ))
                print("  query_rays occluded kernel ms   %s   %.1f Mrays/s" % (stats(t_occ), n/mo/1e3))
                print("  query_transmittance / query_rays occluded: %.3f (%.3f ms more)" % (med/mo, med - mo))
        for r in (veil, fog, plain):
            r.close()


if __name__ == "__main__":
    main()
