"""tghip_query_vertex on device memory: kernel milliseconds of whole paths on the camera rays of materialtest and of the Cornell box, one sample per ray
-- in one call (turns = max_bounces) and turn by turn from the host -- against tghip_query_radiance, the persistent loop, on the same rays; and the
turns' own times with their live-path counts (profiles/vertex_query/bench.txt).

    python tools/vertex_query_bench.py [--width 1280 --height 720 --rounds 7] > profiles/vertex_query/bench.txt

In one process, after a warm-up of every path, `rounds` alternations of the three on the same ray tensor; HIP-event times through the *_kernel_time
getters, each ending in a synchronise (for the vertex query from a call's first launch to its last: the one-word read-backs between its launches are
inside; the turn-by-turn figure is the sum over the calls of a path's life and leaves the host's time between them out).  Medians and spreads
(min .. max)."""
import argparse
import ctypes as C
import os
import subprocess
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("at least five repetitions")
    lib = tg.lib
    dev = torch.device("cuda", 0)
    ms = C.c_double(0.0)
    try:
        tree = "commit %s + the working tree" % subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        tree = "a tree without its history (the record says which)"
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    print("vertex_query_bench: %d x %d rays, one sample a ray, on %s (%s), library %s, %s" % (
        a.width, a.height, torch.cuda.get_device_name(0), arch or "arch unknown", os.path.basename(os.environ.get("TUNGSTEN_AMD_LIB", tg.capi.LIB_PATH)), tree))
    words = tg.PATH_DTYPE.itemsize//4
    with tempfile.TemporaryDirectory() as tmp:
        for label, make in (("materialtest", scenes.materialtest), ("Cornell box", scenes.cornell)):
            if make is scenes.materialtest and not scenes.have_materialtest():
                print("\n%s: assets not present, skipped" % label)
                continue
            path = make(tmp, name="vq_bench_%s.json" % label.split()[0], resolution=(a.width, a.height), spp=1)
            flat = tg.FlattenedScene(path)
            rays = camera_rays(flat)
            max_bounces = int(flat.desc.contents.settings.max_bounces)
            flat.close()
            r = tg.Renderer(path)
            ctx = r.context()
            n = len(rays)
            drays = torch.from_numpy(rays).to(dev)
            states = torch.empty((n, words), dtype=torch.float32, device=dev)
            dsum = torch.empty((n, 3), dtype=torch.float32, device=dev)
            dcount = torch.empty((n,), dtype=torch.int32, device=dev)

            def vertex_ms():
                lib.tghip_query_vertex_kernel_time(ctx, C.byref(ms))
                return ms.value

            t_once, t_turns, t_radiance, per_turn, lives = [], [], [], [], []
            for k in range(a.rounds + 1):                   # round 0 warms every path and is not counted
                r.query_radiance_into(drays, dsum, dcount, 0, 1)
                lib.tghip_query_radiance_kernel_time(ctx, C.byref(ms))
                if k:
                    t_radiance.append(ms.value)
                assert r.query_vertex_into(states, rays=drays, turns=max_bounces) == 0
                if k:
                    t_once.append(vertex_ms())
                once = states.cpu().numpy().view(tg.PATH_DTYPE).reshape(-1) if k == 0 else None
                alive, times, live = r.query_vertex_into(states, rays=drays, turns=1), [], [n]
                times.append(vertex_ms())
                while alive:
                    live.append(alive)
                    alive = r.query_vertex_into(states)
                    times.append(vertex_ms())
                if k:
                    t_turns.append(sum(times))
                    per_turn.append(times)
                    lives = live
                else:
                    chained = states.cpu().numpy().view(tg.PATH_DTYPE).reshape(-1)
                    if chained.tobytes() != once.tobytes():
                        raise SystemExit("the chain of turns differs from the one call")
                    rad = dsum.cpu().numpy()
                    if not (chained["emission"] == rad).all():
                        raise SystemExit("the paths' emission differs from tghip_query_radiance's answer")
                    census = np.bincount(chained["status"], minlength=7)
            mo, mt, mr = float(np.median(t_once)), float(np.median(t_turns)), float(np.median(t_radiance))
            print("\n%s: %d paths, max_bounces %d, %d turns; the emission equals tghip_query_radiance's answer on every path; ended: %s" % (
                label, n, max_bounces, len(lives), ", ".join("%s %d" % (tg.PATH_END_NAMES[i], census[i]) for i in range(1, 7) if census[i])))
            print("  query_radiance ms (the persistent loop)       %s   %.1f Mpaths/s" % (stats(t_radiance), n/mr/1e3))
            print("  query_vertex ms, one call, turns = %-3d        %s   %.1f Mpaths/s" % (max_bounces, stats(t_once), n/mo/1e3))
            print("  query_vertex ms, turn by turn from the host   %s   %.1f Mpaths/s" % (stats(t_turns), n/mt/1e3))
            print("  one call / query_radiance: %.2f    turn by turn / query_radiance: %.2f    turn by turn / one call: %.3f" % (mo/mr, mt/mr, mt/mo))
            print("  turn  live paths   ms (median of %d)" % a.rounds)
            for t in range(len(lives)):
                print("  %4d  %10d   %8.3f" % (t + 1, lives[t], float(np.median([p[t] for p in per_turn]))))
            r.close()


if __name__ == "__main__":
    main()
