"""Worker of tests/test_gpu_develop.py::test_device_tensors, a process of its own because torch must be imported before tungsten_amd (one HIP
runtime per process): Renderer.develop_into with torch tensors on the context's device against Renderer.develop and the host's functions.

    python tests/develop_torch_worker.py <scratch directory>      prints DEVELOP_TORCH_OK"""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import develop_cases as dc  # noqa: E402
import scenes  # noqa: E402
import tungsten_amd as tg  # noqa: E402
from tungsten_amd import capi  # noqa: E402

W, H = 67, 35
N = W*H


def raises(fn):
    try:
        fn()
    except tg.TungstenError:
        return True
    return False


def main(tmp):
    dev = torch.device("cuda", 0)
    r = tg.Renderer(scenes.cornell(tmp, resolution=(W, H), spp=1), seed=tg.DEFAULT_SEED)
    r.render()
    ctx = r.context()
    table_sum, table_count = dc.frame_table()
    ssum, count = dc.tiled(table_sum, N), dc.tiled(table_count, N)
    assert tg.lib.tghip_upload_framebuffer(ctx, ssum.ctypes.data, count.ctypes.data, N) == 0
    aux = dc.tiled(dc.aux_table(), N)
    assert tg.lib.tghip_upload_aux(ctx, aux.ctypes.data, N) == 0
    for source, part, channels in (("frame", "mean", 3), ("depth", "a", 1), ("depth", "mean", 1), ("normal", "mean", 3), ("color", "variance", 3)):
        for tonemap in ("reinhard", None) if source == "frame" else (None,):
            ldr, hdr = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev), torch.zeros((H, W, channels), dtype=torch.float32, device=dev)
            r.develop_into(ldr=ldr, hdr=hdr, source=source, part=part, tonemap=tonemap)
            desc = r._develop_desc(source, part, tonemap)
            want_hdr, want_ldr = np.empty((N, channels), np.float32), np.empty((N, 3), np.uint8)
            assert tg.lib.tghip_develop(ctx, C.byref(desc), want_hdr.ctypes.data, want_ldr.ctypes.data, N) == 0
            assert dc.same_bits(ldr.cpu().numpy().reshape(N, 3), want_ldr) and dc.same_bits(hdr.cpu().numpy().reshape(N, channels), want_hdr), (source, part, tonemap)
            if source == "frame":
                host_hdr, host_ldr = dc.host_frame(ssum, count, desc.tonemap)
            else:
                host_hdr, host_ldr = dc.host_aux(aux, desc.source, desc.part)
            assert dc.same_bits(want_ldr, host_ldr) and dc.same_bits(want_hdr, host_hdr), (source, part, tonemap)
            only = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
            r.develop_into(ldr=only, source=source, part=part, tonemap=tonemap)
            assert torch.equal(only, ldr)
    # what develop_into refuses: dtype, device, contiguity, size
    assert raises(lambda: r.develop_into(ldr=torch.zeros((H, W, 3), dtype=torch.float32, device=dev)))
    assert raises(lambda: r.develop_into(ldr=torch.zeros((H, W, 3), dtype=torch.uint8)))
    assert raises(lambda: r.develop_into(ldr=torch.zeros((H, W + 1, 3), dtype=torch.uint8, device=dev)[:, :W]))
    assert raises(lambda: r.develop_into(hdr=torch.zeros((H, W, 4), dtype=torch.float32, device=dev)))
    assert raises(lambda: r.develop_into(hdr=torch.zeros((H, W, 3), dtype=torch.float32, device=dev), source="depth"))
    r.close()

    # a torch tensor bound as framebuffer: the pass accumulates into it and the picture is developed from it
    r = tg.Renderer(scenes.cornell(tmp, resolution=(W, H), spp=2), seed=tg.DEFAULT_SEED)
    fb_sum, fb_count = torch.zeros((H, W, 3), dtype=torch.float32, device=dev), torch.zeros((H, W), dtype=torch.int32, device=dev)
    assert tg.lib.tghip_bind_framebuffer(r.context(), fb_sum.data_ptr(), fb_count.data_ptr()) == 0
    r.render()
    ldr = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    r.develop_into(ldr=ldr, tonemap="gamma")
    ssum, count = fb_sum.cpu().numpy().reshape(N, 3), fb_count.cpu().numpy().astype(np.uint32).reshape(N)
    assert (count == 2).all() and ssum.max() > 0
    assert dc.same_bits(ldr.cpu().numpy().reshape(N, 3), dc.host_frame(ssum, count, capi.TGHIP_TONEMAP_GAMMA)[1])
    assert dc.same_bits(r.develop(tonemap="gamma").reshape(N, 3), ldr.cpu().numpy().reshape(N, 3))
    assert tg.lib.tghip_bind_framebuffer(r.context(), None, None) == 0
    r.close()
    print("DEVELOP_TORCH_OK")


if __name__ == "__main__":
    main(sys.argv[1])
