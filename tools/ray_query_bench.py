"""tghip_query_rays against tghip_trace_rays on two seeded batches of materialtest (profiles/ray_query_ab.txt).

    python tools/ray_query_bench.py [--width 1280 --height 720 --rounds 7] [--sweep] [--blocks-per-cu N --refill-at K]

Batch A: one camera ray through every pixel centre (coherent).  Batch B: from every hit point of A one uniformly random direction (incoherent:
where a lock-step wave waits longest for its longest ray).  In one process, after a warm-up of every path, `rounds` alternations of
  tghip_trace_rays (repeats = 1; HIP-event time of its kernel: ms_per_launch),
  tghip_query_rays CLOSEST and OCCLUDED on host memory (HIP-event time of the kernel: tghip_query_rays_kernel_time; wall time of the whole call),
  tghip_query_rays CLOSEST and OCCLUDED on torch tensors of the device (wall time of the whole call),
on both batches; medians and spreads (min .. max).  The answers are compared first: a faster kernel with other answers is not faster.
--sweep: the kernel times on batch B over "query_blocks" (workgroups per CU) and "query_refill_at", three launches each, before the alternation."""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scenes  # noqa: E402
import tungsten_amd as tg  # noqa: E402


def camera_rays(flat):
    """One ray through every pixel centre of the scene's camera (pinhole arithmetic on the flattened camera)."""
    cam = flat.desc.contents.camera
    w, h = int(cam.res_x), int(cam.res_y)
    px, py = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    local = np.stack([-1.0 + px*2.0*cam.pixel_size_x, cam.ratio - py*2.0*cam.pixel_size_x, np.full_like(px, cam.plane_dist)], axis=-1).reshape(-1, 3)
    local /= np.linalg.norm(local, axis=1, keepdims=True)
    d = local @ np.array(list(cam.xf), np.float64).reshape(3, 3).T
    o = np.broadcast_to(np.array(list(cam.pos), np.float64), d.shape)
    n = len(d)
    return np.concatenate([o, np.full((n, 1), 1e-4), d, np.full((n, 1), np.inf)], axis=1).astype(np.float32)


def scattered_rays(rays, hits, seed=7):
    """From every hit point one uniformly random direction."""
    hit = hits["rec"] >= 0
    p = rays[hit, 0:3].astype(np.float64) + hits["t"][hit, None].astype(np.float64)*rays[hit, 4:7]
    rs = np.random.RandomState(seed)
    d = rs.randn(len(p), 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n = len(p)
    return np.concatenate([p, np.full((n, 1), 1e-3), d, np.full((n, 1), np.inf)], axis=1).astype(np.float32)


def stats(xs):
    xs = sorted(xs)
    return "median %8.3f  min %8.3f  max %8.3f" % (float(np.median(xs)), xs[0], xs[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--blocks-per-cu", type=int, default=0, help="the alternation under query_blocks = this many workgroups per CU (0: the default)")
    ap.add_argument("--refill-at", type=int, default=0, help="... and under this query_refill_at (0: the default)")
    a = ap.parse_args()
    lib = tg.lib
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        path = scenes.materialtest(tmp, resolution=(a.width, a.height), spp=1)
        flat = tg.FlattenedScene(path)
        batch_a = camera_rays(flat)
        flat.close()
        r = tg.Renderer(path)
        ctx = r.context()
        ms = C.c_double(0.0)

        def kernel_ms():
            lib.tghip_query_rays_kernel_time(ctx, C.byref(ms))
            return ms.value

        batch_b = scattered_rays(batch_a, r.trace_rays(batch_a)[0])
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        print("ray_query_bench: materialtest %d x %d on %s (%d CUs), library %s" % (a.width, a.height, torch.cuda.get_device_name(0), cus,
                                                                                 os.path.basename(os.environ.get("TUNGSTEN_AMD_LIB", tg.capi.LIB_PATH))))
        batches = (("A camera", batch_a), ("B scattered", batch_b))
        for name, rays in batches:
            want = r.trace_rays(rays)[0]
            got, occ = r.query_rays(rays, "closest"), r.query_rays(rays, "occluded")
            same = got.tobytes() == want.tobytes() and (occ == (want["rec"] >= 0)).all()
            print("batch %-12s %8d rays, %8d hits; query answers equal tghip_trace_rays': %s" % (name, len(rays), int((want["rec"] >= 0).sum()), same))
            if not same:
                raise SystemExit("answers differ")
        if a.sweep:
            print("sweep on batch B, kernel ms (median of 3): workgroups per CU x refill threshold, closest / occluded")
            for per_cu in (1, 2, 3, 4, 5, 6, 8):
                r.set_option("query_blocks", per_cu*cus)
                row = []
                for refill in (1, 8, 16, 24, 32, 40, 48, 64):
                    r.set_option("query_refill_at", refill)
                    cell = []
                    for mode in ("closest", "occluded"):
                        t = []
                        for _ in range(3):
                            r.query_rays(batch_b, mode)
                            t.append(kernel_ms())
                        cell.append(float(np.median(t)))
                    row.append("%2d: %6.3f / %6.3f" % (refill, cell[0], cell[1]))
                print("  %d per CU | %s" % (per_cu, " | ".join(row)))
            r.set_option("query_blocks", 0)
            r.set_option("query_refill_at", 0)
        r.set_option("query_blocks", a.blocks_per_cu*cus)
        r.set_option("query_refill_at", a.refill_at)
        print("alternation under query_blocks = %d (%d per CU), query_refill_at = %d (0: the defaults)" % (a.blocks_per_cu*cus, a.blocks_per_cu, a.refill_at))
        figures = {}

        def note(key, value):
            figures.setdefault(key, []).append(value)

        tensors = {name: (torch.from_numpy(rays).to(dev), torch.empty((len(rays), 4), dtype=torch.float32, device=dev),
                          torch.empty((len(rays),), dtype=torch.uint8, device=dev)) for name, rays in batches}
        for rnd in range(a.rounds + 1):                     # round 0 warms every path and is not counted
            for name, rays in batches:
                t0 = time.perf_counter()
                _, t = r.trace_rays(rays)
                vals = [("trace_rays kernel ms", t), ("trace_rays call ms", (time.perf_counter() - t0)*1e3)]
                for mode in ("closest", "occluded"):
                    t0 = time.perf_counter()
                    r.query_rays(rays, mode)
                    wall = (time.perf_counter() - t0)*1e3
                    vals += [("query %s kernel ms" % mode, kernel_ms()), ("query %s host-pointer call ms" % mode, wall)]
                    drays, dhits, docc = tensors[name]
                    t0 = time.perf_counter()
                    r.query_rays_into(drays, dhits if mode == "closest" else docc, mode)
                    vals += [("query %s device-pointer call ms" % mode, (time.perf_counter() - t0)*1e3),
                             ("query %s kernel ms (device pointers)" % mode, kernel_ms())]
                if rnd:
                    for k, v in vals:
                        note((name, k), v)
        for name, rays in batches:
            print("batch %s, %d rounds:" % (name, a.rounds))
            for (b, k), v in figures.items():
                if b == name:
                    print("  %-48s %s" % (k, stats(v)))
        r.close()


if __name__ == "__main__":
    main()
