"""What tghip_query_radiance costs against a render pass of the same paths (profiles/radiance_query/bench.txt): materialtest, 16 samples per ray.

    python tools/radiance_query_bench.py render       [--width 1280 --height 720 --spp 16 --rounds 5]    a render pass of the scene as it is
    python tools/radiance_query_bench.py render_equi  ...                                                 ... of its equirectangular variant
    python tools/radiance_query_bench.py query        ...                                                 the query on the pinhole's central rays
    ... --root DIR                                                                                        of the built checkout DIR instead of this one

One process measures one thing on the library TUNGSTEN_AMD_LIB names (default: the tree's); a session alternates the processes -- the two render
modes run on the parent commit's library as well as on the head's, `query` needs the head's.  `render_equi` has a query's launch shape (a launch that
rewrites the fresh rays in front of every closest-hit launch, k_finish on its own, no k_tail) on another workload: context, not a yardstick.
Every figure: after one warm-up, `rounds` repetitions; wall time around work that ends in a synchronise, and the HIP-event time of the launches (a pass:
TgHipCounters::ms_total; a query: tghip_query_radiance_kernel_time); median, min .. max.  Then once more with "time_kernels": the iterations and the
time of the closest-hit, shading and shadow launches of one repetition, and what is left of the event time -- k_start, the launch in front of the
walk, k_finish, k_resolve, the host checks."""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

# --root DIR: the checkout whose package, library and tests/scenes.py are measured (the parent commit's, built, for the render modes); default: this one
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(xs):
    xs = sorted(xs)
    return "median %9.3f  min %9.3f  max %9.3f" % (float(np.median(xs)), xs[0], xs[-1])


def camera_rays(flat):
    """One ray through every pixel centre of the scene's camera (pinhole arithmetic on the flattened camera), in pixel order."""
    cam = flat.desc.contents.camera
    w, h = int(cam.res_x), int(cam.res_y)
    px, py = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    local = np.stack([-1.0 + px*2.0*cam.pixel_size_x, cam.ratio - py*2.0*cam.pixel_size_x, np.full_like(px, cam.plane_dist)], axis=-1).reshape(-1, 3)
    local /= np.linalg.norm(local, axis=1, keepdims=True)
    d = local @ np.array(list(cam.xf), np.float64).reshape(3, 3).T
    o = np.broadcast_to(np.array(list(cam.pos), np.float64), d.shape)
    n = len(d)
    return np.concatenate([o, np.full((n, 1), 1e-4), d, np.full((n, 1), np.inf)], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("render", "render_equi", "query"))
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.what == "query":
        import torch      # (before the package: one HIP runtime per process)
    import scenes
    import tungsten_amd as tg
    from tungsten_amd import capi
    lib = tg.lib
    libname = os.path.relpath(os.environ.get("TUNGSTEN_AMD_LIB", capi.LIB_PATH))
    with tempfile.TemporaryDirectory() as tmp:
        edit = scenes._mt_equirectangular if a.what == "render_equi" else None
        path = scenes.materialtest(tmp, resolution=(a.width, a.height), spp=a.spp, edit=edit) if edit else scenes.materialtest(tmp, resolution=(a.width, a.height), spp=a.spp)
        r = tg.Renderer(path)
        ctx = r.context()
        samples = a.width*a.height*a.spp
        print("radiance_query_bench %s: materialtest %d x %d x %d samples, library %s" % (a.what, a.width, a.height, a.spp, libname))

        def breakdown(c0, c1, event_ms):
            it = c1.iterations - c0.iterations
            parts = [c1.ms_trace_closest - c0.ms_trace_closest, c1.ms_shade - c0.ms_shade, c1.ms_trace_shadow - c0.ms_trace_shadow]
            print("  with time_kernels: %d iterations, %d tail launches; launches of the timed check intervals (sums over all parts of the pool, which run side by "
                  "side): closest-hit %.2f ms in %d, shading %.2f ms in %d, shadow %.2f ms in %d; event time of the whole %.2f ms"
                  % (it, c1.tail_launches - c0.tail_launches, parts[0], c1.launches_trace_closest - c0.launches_trace_closest, parts[1],
                     c1.launches_shade - c0.launches_shade, parts[2], c1.launches_trace_shadow - c0.launches_trace_shadow, event_ms))

        if a.what != "query":
            def one_pass():
                p = capi.TgHipPassDesc(0, a.spp, tg.DEFAULT_SEED & 0xFFFFFFFF, 0, 1, 0)
                assert lib.tghip_clear_framebuffer(ctx) == 0
                c0 = r.counters()
                t0 = time.perf_counter()
                assert lib.tghip_render_pass(ctx, C.byref(p)) == 0 and lib.tghip_wait(ctx) == 0
                wall = (time.perf_counter() - t0)*1e3
                c1 = r.counters()
                return wall, c1.ms_total - c0.ms_total, c0, c1
            one_pass()
            walls, events = [], []
            for _ in range(a.rounds):
                w, e, _, _ = one_pass()
                walls.append(w)
                events.append(e)
            print("  pass wall ms   %s   (%.1f Msamples/s at the median)" % (stats(walls), samples/np.median(walls)/1e3))
            print("  pass event ms  %s" % stats(events))
            r.set_option("time_kernels", 1)
            one_pass()
            w, e, c0, c1 = one_pass()
            breakdown(c0, c1, e)
        else:
            flat = tg.FlattenedScene(path)
            rays = camera_rays(flat)
            flat.close()
            n = len(rays)
            dev = torch.device("cuda", 0)
            drays = torch.from_numpy(rays).to(dev)
            dsum, dcount = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
            ms = C.c_double(0.0)

            def kernel_ms():
                lib.tghip_query_radiance_kernel_time(ctx, C.byref(ms))
                return ms.value

            def host():
                t0 = time.perf_counter()
                out = r.query_radiance(rays, 0, a.spp)
                return (time.perf_counter() - t0)*1e3, kernel_ms(), out

            def device():
                t0 = time.perf_counter()
                r.query_radiance_into(drays, dsum, dcount, 0, a.spp)
                return (time.perf_counter() - t0)*1e3, kernel_ms()

            _, _, want = host()
            device()
            same = dsum.cpu().numpy().tobytes() == want[0].tobytes() and dcount.cpu().numpy().tobytes() == want[1].tobytes()
            print("  %d rays; device-pointer answers equal the host-memory ones: %s; mean radiance %s, counts all %d: %s"
                  % (n, same, want[0].mean(axis=0)/a.spp, a.spp, bool((want[1] == a.spp).all())))
            if not same:
                raise SystemExit("answers differ")
            figures = {"host wall": [], "host event": [], "device wall": [], "device event": []}
            for _ in range(a.rounds):
                w, e, _ = host()
                figures["host wall"].append(w)
                figures["host event"].append(e)
                w, e = device()
                figures["device wall"].append(w)
                figures["device event"].append(e)
            for k in ("host wall", "host event", "device wall", "device event"):
                print("  query %-13s ms  %s   (%.1f Msamples/s at the median)" % (k, stats(figures[k]), samples/np.median(figures[k])/1e3))
            r.set_option("time_kernels", 1)
            device()
            c0 = r.counters()
            _, e = device()
            breakdown(c0, r.counters(), e)
        r.close()


if __name__ == "__main__":
    main()
