"""Developing a 3840 x 2160 frame on the device against the download + host loops it replaces (profiles/r8_develop.txt).

    python tools/develop_bench.py [--width 3840 --height 2160 --rounds 5]

In one process, `rounds` alternations of
  (a) tghip_develop into a host 8-bit buffer (kernel + 3 B per pixel over PCIe), and
  (b) tghip_download_framebuffer (16 B per pixel) followed by tgh_develop_host_frame: the arithmetic and the transfer of the host path;
the same for all outputs of the auxiliary buffers (five outputs x mean / A / B / variance, float and 8-bit image each, as save_outputs asks for them);
the kernels' own time by HIP events (tghip_develop_kernel_time), and next to it a device-to-device copy that moves the kernel's algorithmic bytes."""
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
from tungsten_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    n = a.width*a.height
    lib = tg.lib
    with tempfile.TemporaryDirectory() as tmp:
        r = tg.Renderer(scenes.cornell(tmp, resolution=(a.width, a.height), spp=2, edit=scenes._outputs), seed=tg.DEFAULT_SEED)
        r.render()
        ctx = r.context()
        ldr, ldr_host = np.empty((n, 3), np.uint8), np.empty((n, 3), np.uint8)
        hdr, hdr_host = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        ssum, count = np.empty((n, 3), np.float32), np.empty(n, np.uint32)
        aux = np.empty(n, tg.AUX_DTYPE)
        ms = C.c_double(0.0)

        def kernel_ms():
            lib.tghip_develop_kernel_time(ctx, C.byref(ms))
            return ms.value

        def copy_ms(nbytes):
            src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            best = 1e9
            for _ in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1))
            return best

        print("develop_bench: %d x %d (%d pixels), %s" % (a.width, a.height, n, torch.cuda.get_device_name(0)))
        op = capi.TGHIP_TONEMAP_FILMIC
        for op in (capi.TGHIP_TONEMAP_FILMIC, capi.TGHIP_TONEMAP_GAMMA):
            desc = capi.TgHipDevelopDesc(capi.TGHIP_DEVELOP_FRAME, 0, op, 0)
            lib.tghip_develop(ctx, C.byref(desc), None, ldr.ctypes.data, n)      # warm-up: staging buffer, code object
            for i in range(a.rounds):
                t0 = time.perf_counter()
                assert lib.tghip_develop(ctx, C.byref(desc), None, ldr.ctypes.data, n) == 0
                t1 = time.perf_counter()
                k = kernel_ms()
                assert lib.tghip_download_framebuffer(ctx, ssum.ctypes.data, count.ctypes.data, n) == 0
                t2 = time.perf_counter()
                assert lib.tgh_develop_host_frame(ssum.ctypes.data, count.ctypes.data, n, op, None, ldr_host.ctypes.data) == 0
                t3 = time.perf_counter()
                assert ldr.tobytes() == ldr_host.tobytes()
                print("frame %-8s round %d: (a) tghip_develop -> host 8-bit %8.2f ms (kernel %.3f ms)   (b) download %8.2f ms + host loops %8.2f ms = %8.2f ms"
                      % (tg.TONEMAP_NAMES[op], i, (t1 - t0)*1e3, k, (t2 - t1)*1e3, (t3 - t2)*1e3, (t3 - t1)*1e3))
            # the kernel alone, outputs in device memory: 16 B in, 3 B (8-bit) / 15 B (8-bit + float) out per pixel
            d_ldr, d_hdr = torch.empty((n, 3), dtype=torch.uint8, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
            ddesc = capi.TgHipDevelopDesc(capi.TGHIP_DEVELOP_FRAME, 0, op, capi.TGHIP_DEVELOP_DEVICE_POINTERS)
            for name, h, out_bytes in (("8-bit", None, 3), ("8-bit + float", d_hdr.data_ptr(), 15)):
                ks = []
                for i in range(a.rounds + 1):
                    assert lib.tghip_develop(ctx, C.byref(ddesc), h, d_ldr.data_ptr(), n) == 0
                    ks.append(kernel_ms())
                k = min(ks[1:])
                moved = (16 + out_bytes)*n
                c = copy_ms(moved//2)
                print("frame %-8s kernel, %-13s: %.3f ms for %.1f MB in + out = %.0f GB/s; a device-to-device copy moving the same bytes (%.1f MB read, as much written): %.3f ms = %.0f GB/s; kernel at %.0f %% of the copy"
                      % (tg.TONEMAP_NAMES[op], name, k, moved/1e6, moved/k/1e6, moved/2e6, c, moved/c/1e6, 100.0*c/k))
        # all outputs of the auxiliary buffers
        images = [(o, p) for o in range(5) for p in range(4)]
        aux_hdr = {o: np.empty((n, capi.TGHIP_AUX_CHANNEL_COUNT[o]), np.float32) for o in range(5)}
        aux_hdr_host = {o: np.empty((n, capi.TGHIP_AUX_CHANNEL_COUNT[o]), np.float32) for o in range(5)}
        for i in range(a.rounds + 1):
            t0 = time.perf_counter()
            k = 0.0
            for o, p in images:
                desc = capi.TgHipDevelopDesc(o, p, 0, 0)
                assert lib.tghip_develop(ctx, C.byref(desc), aux_hdr[o].ctypes.data, ldr.ctypes.data, n) == 0
                k += kernel_ms()
            t1 = time.perf_counter()
            if i == 0:
                continue                                      # warm-up
            assert lib.tghip_download_aux(ctx, aux.ctypes.data, n) == 0
            t2 = time.perf_counter()
            for o, p in images:
                assert lib.tgh_develop_host_aux(aux.ctypes.data, n, o, p, aux_hdr_host[o].ctypes.data, ldr_host.ctypes.data) == 0
            t3 = time.perf_counter()
            assert ldr.tobytes() == ldr_host.tobytes() and aux_hdr[4].tobytes() == aux_hdr_host[4].tobytes()
            print("aux, 20 images round %d: (a) tghip_develop -> host float + 8-bit %8.2f ms (kernels %.3f ms)   (b) download %8.2f ms + host loops %8.2f ms = %8.2f ms"
                  % (i - 1, (t1 - t0)*1e3, k, (t2 - t1)*1e3, (t3 - t2)*1e3, (t3 - t1)*1e3))
        r.close()


if __name__ == "__main__":
    main()
