"""tghip_query_direct on device memory: kernel milliseconds and (ray, sample) items per second of surface mode on the camera rays of materialtest and
of the Cornell box at 4 spp -- and, next to it, what a caller had for the same question before the call existed: tghip_query_radiance on the scene
loaded and uploaded once more with max_bounces = 2 (the camera vertex' direct light plus the first hit's emission), the time of that second load and
upload shown on its own (profiles/direct_query/bench.txt).

    python tools/direct_query_bench.py [--width 1280 --height 720 --spp 4 --rounds 9] > profiles/direct_query/bench.txt

In one process, after a warm-up of every path, `rounds` alternations of the two calls on the same ray tensor; HIP-event times through the
*_kernel_time getters (for the direct query from its first launch to its last: the one-word read-backs between its rounds and parts are inside).
Medians and spreads (min .. max)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scenes  # noqa: E402
import tungsten_amd as tg  # noqa: E402
from ray_query_bench import camera_rays, stats  # noqa: E402


def two_bounces(scene):
    scene["integrator"]["max_bounces"] = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    lib = tg.lib
    dev = torch.device("cuda", 0)
    ms = C.c_double(0.0)
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    print("direct_query_bench: %d x %d rays x %d spp on %s, library %s, commit %s + the working tree" % (
        a.width, a.height, a.spp, torch.cuda.get_device_name(0), os.path.basename(os.environ.get("TUNGSTEN_AMD_LIB", tg.capi.LIB_PATH)), commit))
    size = dict(resolution=(a.width, a.height), spp=1)
    with tempfile.TemporaryDirectory() as tmp:
        for label, make in (("materialtest", scenes.materialtest), ("Cornell box", scenes.cornell)):
            if make is scenes.materialtest and not scenes.have_materialtest():
                print("\n%s: assets not present, skipped" % label)
                continue
            path = make(tmp, name="dq_bench_%s.json" % label.split()[0], **size)
            r = tg.Renderer(path)
            flat = tg.FlattenedScene(path)
            rays = camera_rays(flat)
            flat.close()
            t0 = time.time()
            r2 = tg.Renderer(make(tmp, name="dq_bench_%s_mb2.json" % label.split()[0], edit=two_bounces, **size))
            reload_s = time.time() - t0
            n = len(rays)
            want = r.query_direct(rays, spp=a.spp, medium=None, skip=3)
            ssum, count = r2.query_radiance(rays, 0, a.spp)
            lit = (want["rgb"] != 0).any(axis=1)
            agree = (want["rgb"] == ssum).all(axis=1)
            print("\n%s: %d rays, %d hit, %d lit; the two-bounce radiance equals the direct light on %d rays (it adds the hit's emission and takes the\n"
                  "  specular and forward first hits through)" % (label, n, int((want["rec"] >= 0).sum()), int(lit.sum()), int(agree.sum())))
            drays = torch.from_numpy(rays).to(dev)
            dout = torch.empty((n, 8), dtype=torch.float32, device=dev)
            dsum = torch.empty((n, 3), dtype=torch.float32, device=dev)
            dcount = torch.empty((n,), dtype=torch.int32, device=dev)
            t_direct, t_radiance = [], []
            for k in range(a.rounds + 1):                   # round 0 warms every path and is not counted
                r2.query_radiance_into(drays, dsum, dcount, 0, a.spp)
                lib.tghip_query_radiance_kernel_time(r2.context(), C.byref(ms))
                if k:
                    t_radiance.append(ms.value)
                r.query_direct_into(drays, dout, spp=a.spp, medium=None, skip=3)
                lib.tghip_query_direct_kernel_time(r.context(), C.byref(ms))
                if k:
                    t_direct.append(ms.value)
            if dout.cpu().numpy().tobytes() != want.tobytes():
                raise SystemExit("device-memory answers differ from host-memory answers")
            md, mr = float(np.median(t_direct)), float(np.median(t_radiance))
            print("  query_direct ms                          %s   %.1f Mitems/s" % (stats(t_direct), n*a.spp/md/1e3))
            print("  query_radiance ms, max_bounces = 2       %s   %.1f Mitems/s" % (stats(t_radiance), n*a.spp/mr/1e3))
            print("  ... behind a second load and upload of the scene: %.2f s" % reload_s)
            print("  query_direct / query_radiance: %.3f" % (md/mr))
            r.close()
            r2.close()


if __name__ == "__main__":
    main()
