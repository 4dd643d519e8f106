"""tghip_query_surface next to tghip_query_rays (closest) on two batches of materialtest, on device memory (profiles/surface_query/bench.txt).

    python tools/surface_query_bench.py [--width 1280 --height 720 --rounds 9]

Batch A: one camera ray through every pixel centre (coherent).  Batch B: as many rays with uniformly random origins in the scene's bounds and
uniformly random directions, every 7th with a finite tmax (incoherent; the rays of tests/test_gpu_ray_queries.py: make_rays).  In one process, after
a warm-up of every path, `rounds` alternations of tghip_query_rays CLOSEST and tghip_query_surface on torch tensors of the device; HIP-event times
through the *_kernel_time getters -- for the surface query both launches and, with the "surface_time_stage" option, the dense launch alone (both
figures are of the same call).  Medians and spreads (min .. max), the dense launch's share, and its bytes per second over its algorithmic bytes:
per ray 32 B of ray, 16 B of hit and 96 B of answer, per hit 48 B of record and 64 B of attributes.  The yardstick is tghip_query_rays' kernel.
The library is TUNGSTEN_AMD_LIB's (an experiment's build: make VARIANT=...), so two store forms are alternated by alternating processes."""
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
import tungsten_amd as tg  # noqa: E402
from ray_query_bench import camera_rays, stats  # noqa: E402


def random_rays(flat, n, seed=5):
    d = flat.desc.contents
    lo, hi = np.array(list(d.bounds_lo)), np.array(list(d.bounds_hi))
    rs = np.random.RandomState(seed)
    o = lo + (hi - lo)*rs.rand(n, 3)*1.2 - 0.1*(hi - lo)
    dirs = rs.randn(n, 3)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = np.concatenate([o, np.full((n, 1), 1e-4), dirs, np.full((n, 1), np.inf)], axis=1).astype(np.float32)
    rays[::7, 7] = 0.5*np.linalg.norm(hi - lo)
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    lib = tg.lib
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        path = scenes.materialtest(tmp, resolution=(a.width, a.height), spp=1)
        flat = tg.FlattenedScene(path)
        batch_a = camera_rays(flat)
        batch_b = random_rays(flat, len(batch_a))
        flat.close()
        r = tg.Renderer(path)
        ctx = r.context()
        ms = C.c_double(0.0)

        def rays_ms():
            lib.tghip_query_rays_kernel_time(ctx, C.byref(ms))
            return ms.value

        def surface_ms():
            """(both launches, the dense launch) of the last tghip_query_surface"""
            out = []
            for stage in (0, 1):
                r.set_option("surface_time_stage", stage)
                lib.tghip_query_surface_kernel_time(ctx, C.byref(ms))
                out.append(ms.value)
            r.set_option("surface_time_stage", 0)
            return out

        print("surface_query_bench: materialtest %d x %d on %s, library %s" % (
            a.width, a.height, torch.cuda.get_device_name(0), os.path.basename(os.environ.get("TUNGSTEN_AMD_LIB", tg.capi.LIB_PATH))))
        batches = (("A camera", batch_a), ("B random", batch_b))
        hits = {}
        for name, rays in batches:
            want, got = r.query_rays(rays, "closest"), r.query_surface(rays)
            hit = want["rec"] >= 0
            same = (got["rec"] == want["rec"]).all() and got["t"][hit].tobytes() == want["t"][hit].tobytes()
            hits[name] = int(hit.sum())
            print("batch %-10s %8d rays, %8d hits; rec and t equal tghip_query_rays': %s" % (name, len(rays), hits[name], same))
            if not same:
                raise SystemExit("answers differ")
        tensors = {name: (torch.from_numpy(rays).to(dev), torch.empty((len(rays), 4), dtype=torch.float32, device=dev),
                          torch.empty((len(rays), 24), dtype=torch.float32, device=dev)) for name, rays in batches}
        figures = {}
        for rnd in range(a.rounds + 1):                     # round 0 warms every path and is not counted
            for name, rays in batches:
                drays, dhits, dsurf = tensors[name]
                r.query_rays_into(drays, dhits, "closest")
                vals = [("query_rays closest kernel ms", rays_ms())]
                r.query_surface_into(drays, dsurf)
                both, dense = surface_ms()
                vals += [("query_surface both launches ms", both), ("query_surface dense launch ms", dense), ("query_surface walk launch ms", both - dense)]
                if rnd:
                    for k, v in vals:
                        figures.setdefault((name, k), []).append(v)
        for name, rays in batches:
            n = len(rays)
            print("batch %s, %d rounds:" % (name, a.rounds))
            for (b, k), v in figures.items():
                if b == name:
                    print("  %-40s %s" % (k, stats(v)))
            both = float(np.median(figures[(name, "query_surface both launches ms")]))
            dense = float(np.median(figures[(name, "query_surface dense launch ms")]))
            yard = float(np.median(figures[(name, "query_rays closest kernel ms")]))
            nbytes = n*(32 + 16 + 96) + hits[name]*(48 + 64)
            print("  query_surface / query_rays closest: %.3f; dense launch's share of query_surface: %.1f %%" % (both/yard, 100.0*dense/both))
            print("  dense launch: %.1f MB algorithmic -> %.1f GB/s, %.1f Mrays/s" % (nbytes/1e6, nbytes/dense/1e6, n/dense/1e3))
        r.close()


if __name__ == "__main__":
    main()
