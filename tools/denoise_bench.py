"""The NL-means filter on the device against the host comparator and the reference's own threaded nlMeans (profiles/r9_denoise.txt).

    python tools/denoise_bench.py [--sizes 1280x720,3840x2160] [--runs 10] [--warmup 2] [--cpu-runs 1] [--batches 0,1,2,4,8] [--no-cpu]

Per size and per (F, R, channels) of NFOR's stages -- (3, 5) with four packed features, (1, 9) with three channels -- the kernel's time by HIP
events (tghip_nlmeans_kernel_time; device tensors in, device tensor out: nothing crosses PCIe), median of `runs` after `warmup`; the same for
every --batches value of the "nlmeans_batch" option (0: the launcher's own choice); tgh_nlmeans_host on the same arrays; and, where
oracle/_ref/ref_nlmeans was built, the reference's nlMeans on 16 threads (three channels: nlMeans<Vec3f>; four: four nlMeans<float> runs, summed --
SimdNlMeans' float4 run is not reachable without the denoiser program).  The share of the chip's fp32 rate counts, per pixel, offset and channel,
the operations the arithmetic has: 13 for a distance and 6 for its two box-filter chains on the (32+2F)^2/32^2 padded pixels, 13 for the weight
and the two sums."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_cases as dc  # noqa: E402
import scenes  # noqa: E402
import tungsten_amd as tg  # noqa: E402
from tungsten_amd import capi  # noqa: E402

STAGES = ((3, 5, 0.5, 2.0, 4), (1, 9, 1.0, 1.0, 3))
PEAK_FP32 = 157.3e12                      # MI355X: 256 CUs x 128 lanes x 2 (FMA) x 2.4 GHz; an operation that is no FMA uses half a slot's worth


def inputs(w, h, ch, seed=5):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    ramp = (x/np.float32(w) + np.float32(0.5)*y/np.float32(h))[..., None]*np.ones(ch, np.float32)
    guide = ramp + np.float32(0.05)*rng.standard_normal((h, w, ch)).astype(np.float32)
    variance = np.float32(0.002) + np.float32(0.004)*rng.random_sample((h, w, ch)).astype(np.float32)
    return rng.random_sample((h, w, ch)).astype(np.float32), guide.astype(np.float32), variance.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1280x720,3840x2160")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-runs", type=int, default=1)
    ap.add_argument("--batches", default="0,1,2,4,8")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    lib = tg.lib
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        r = tg.Renderer(scenes.cornell(tmp, resolution=(64, 36), spp=1), seed=tg.DEFAULT_SEED)
        ctx = r.context()
        ms = C.c_double(0.0)
        print("denoise_bench: %s" % torch.cuda.get_device_name(0), flush=True)
        for size in a.sizes.split(","):
            w, h = (int(v) for v in size.split("x"))
            for F, R, k, scale, ch in STAGES:
                image, guide, variance = inputs(w, h, ch)
                tensors = [torch.from_numpy(t).to(dev).contiguous() for t in (image, guide, variance)]
                out = torch.empty_like(tensors[0])
                desc = dc.desc_for(capi, image, F, R, k, scale, capi.TGHIP_DEVELOP_DEVICE_POINTERS)
                ops = float(w)*h*ch*(2*R + 1)**2*(19.0*(32 + 2*F)**2/1024.0 + 13.0)
                first = None
                for batch in (int(b) for b in a.batches.split(",")):
                    r.set_option("nlmeans_batch", batch)
                    times = []
                    for i in range(a.warmup + a.runs):
                        rc = lib.tghip_nlmeans(ctx, C.byref(desc), tensors[0].data_ptr(), tensors[1].data_ptr(), tensors[2].data_ptr(), out.data_ptr())
                        assert rc == 0, lib.tghip_last_error(ctx)
                        lib.tghip_nlmeans_kernel_time(ctx, C.byref(ms))
                        if i >= a.warmup:
                            times.append(ms.value)
                    med = statistics.median(times)
                    print("%dx%d F %d R %d C %d batch %2d: kernel %9.3f ms (min %.3f max %.3f)  %.2f Top/s = %.1f %% of the fp32 FMA rate"
                          % (w, h, F, R, ch, batch, med, min(times), max(times), ops/med/1e9, 100.0*ops/(med*1e-3)/PEAK_FP32), flush=True)
                    got = out.cpu().numpy()
                    if first is None:
                        first = got
                    assert dc.differing_words(got, first) == 0
                r.set_option("nlmeans_batch", 0)
                if a.no_cpu:
                    continue
                host = np.empty_like(image)
                hdesc = dc.desc_for(capi, image, F, R, k, scale)
                times = []
                for _ in range(a.cpu_runs):
                    t0 = time.perf_counter()
                    assert lib.tgh_nlmeans_host(C.byref(hdesc), image.ctypes.data, guide.ctypes.data, variance.ctypes.data, host.ctypes.data) == 0
                    times.append(time.perf_counter() - t0)
                print("%dx%d F %d R %d C %d host comparator (%d threads at most): %.3f s; device result differs in %d words"
                      % (w, h, F, R, ch, min(16, os.cpu_count() or 1), statistics.median(times), dc.differing_words(first, host)), flush=True)
                if os.path.exists(dc.REF_NLMEANS):
                    src, dst = os.path.join(tmp, "in.raw"), os.path.join(tmp, "out.raw")
                    total, planes = 0.0, ([np.s_[..., c] for c in range(ch)] if ch == 4 else [np.s_[...]])
                    for sel in planes:
                        np.concatenate([np.ascontiguousarray(t[sel]).ravel() for t in (image, guide, variance)]).tofile(src)
                        o = subprocess.check_output([dc.REF_NLMEANS, str(w), str(h), str(1 if ch == 4 else ch), str(F), str(R), repr(k), repr(scale),
                                                     "16", src, dst, str(a.cpu_runs)]).decode().split()
                        total += statistics.median(float(v) for v in o)
                        ref = np.fromfile(dst, np.float32).reshape(np.ascontiguousarray(image[sel]).shape)
                        assert dc.differing_words(ref, np.ascontiguousarray(first[sel])) == 0
                    print("%dx%d F %d R %d C %d reference nlMeans, 16 threads: %.3f s; the device's bits" % (w, h, F, R, ch, total), flush=True)
        r.close()


if __name__ == "__main__":
    main()
