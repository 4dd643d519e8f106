"""Worker of tests/test_gpu_denoise.py::test_device_tensors, a process of its own because torch must be imported before tungsten_amd (one HIP
runtime per process): tghip_nlmeans with TGHIP_DEVELOP_DEVICE_POINTERS on torch tensors against the recorded results of the reference.

    python tests/denoise_torch_worker.py <scratch directory>      prints DENOISE_TORCH_OK"""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import denoise_cases as dc  # noqa: E402
import scenes  # noqa: E402
import tungsten_amd as tg  # noqa: E402
from tungsten_amd import capi  # noqa: E402


def main(tmp):
    dev = torch.device("cuda", 0)
    r = tg.Renderer(scenes.cornell(tmp, resolution=(70, 37), spp=1), seed=tg.DEFAULT_SEED)
    ctx = r.context()
    golden = dc.load_golden()
    for name in dc.CASE_NAMES:
        _, _, _, F, R, k, scale, _ = dc.case(name)
        image, guide, variance, want = golden[name]
        tensors = [torch.from_numpy(a).to(dev).contiguous() for a in (image, guide, variance)]
        out = torch.zeros_like(tensors[0])
        desc = dc.desc_for(capi, image, F, R, k, scale, capi.TGHIP_DEVELOP_DEVICE_POINTERS)
        rc = tg.lib.tghip_nlmeans(ctx, C.byref(desc), tensors[0].data_ptr(), tensors[1].data_ptr(), tensors[2].data_ptr(), out.data_ptr())
        assert rc == 0, tg.lib.tghip_last_error(ctx)
        assert dc.differing_words(out.cpu().numpy(), want) == 0, name
        for t, a in zip(tensors, (image, guide, variance)):                 # the inputs are left as they were
            assert dc.differing_words(t.cpu().numpy(), a) == 0
    # a misaligned device array is refused: four channels take 16-byte loads
    image, guide, variance, _ = golden["packed_70x37_x4"]
    flat = torch.zeros(image.size + 1, dtype=torch.float32, device=dev)
    tensors = [torch.from_numpy(a).to(dev).contiguous() for a in (image, guide, variance)]
    desc = dc.desc_for(capi, image, 3, 5, 0.5, 2.0, capi.TGHIP_DEVELOP_DEVICE_POINTERS)
    rc = tg.lib.tghip_nlmeans(ctx, C.byref(desc), tensors[0].data_ptr(), tensors[1].data_ptr(), tensors[2].data_ptr(), flat[1:].data_ptr())
    assert rc == capi.TGHIP_E_INVALID and b"aligned" in tg.lib.tghip_last_error(ctx)
    r.close()
    print("DENOISE_TORCH_OK")


if __name__ == "__main__":
    main(sys.argv[1])
