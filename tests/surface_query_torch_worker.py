"""Worker of tests/test_gpu_surface_query.py::test_device_tensors, a process of its own because torch must be imported before tungsten_amd (one HIP
runtime per process): Renderer.query_surface_into with torch tensors on the context's device against Renderer.query_surface, on the flat list
(cornell), on instances and on the 8-wide walk (materialtest), and what query_surface_into refuses.

    python tests/surface_query_torch_worker.py <scratch directory>      prints SURFACE_QUERY_TORCH_OK"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import scenes  # noqa: E402
import tungsten_amd as tg  # noqa: E402
from ray_query_torch_worker import batch, raises, N  # noqa: E402


def main(tmp):
    dev = torch.device("cuda", 0)
    makers = [("cornell", scenes.cornell), ("instances", scenes.cornell_instances)] + ([("materialtest", scenes.materialtest)] if scenes.have_materialtest() else [])
    for name, mk in makers:
        path = mk(tmp, resolution=(64, 36), spp=1, name=name + ".json")
        rays = batch(path)
        r = tg.Renderer(path)
        want = r.query_surface(rays)
        assert (want["rec"] >= 0).sum() > N//10 and (want["rec"] < 0).sum() > N//10, name
        drays = torch.from_numpy(rays).to(dev)
        for n in (N, 257, 1):
            out = torch.full((n, 24), -7.0, dtype=torch.float32, device=dev)
            r.query_surface_into(drays[:n].contiguous(), out)
            assert out.cpu().numpy().tobytes() == want[:n].tobytes(), (name, n)
        flat_out = torch.zeros((N*24,), dtype=torch.float32, device=dev)          # any shape with N x 24 elements
        r.query_surface_into(drays, flat_out)
        assert flat_out.cpu().numpy().tobytes() == want.tobytes(), name
        if name == "cornell":
            # what query_surface_into refuses: dtype, device, contiguity, size -- and a device view that is not 16-byte aligned (the C-ABI's refusal)
            out = torch.zeros((N, 24), dtype=torch.float32, device=dev)
            assert raises(lambda: r.query_surface_into(drays.double(), out))
            assert raises(lambda: r.query_surface_into(drays, out.to(torch.int32)))
            assert raises(lambda: r.query_surface_into(drays.cpu(), out))
            assert raises(lambda: r.query_surface_into(drays, out.cpu()))
            assert raises(lambda: r.query_surface_into(torch.zeros((N, 9), dtype=torch.float32, device=dev)[:, :8], out))
            assert raises(lambda: r.query_surface_into(drays, torch.zeros((N, 25), dtype=torch.float32, device=dev)[:, :24]))
            assert raises(lambda: r.query_surface_into(drays, out[:N - 1]))
            assert raises(lambda: r.query_surface_into(drays, torch.zeros((N, 4), dtype=torch.float32, device=dev)))
            assert raises(lambda: r.query_surface_into(drays.reshape(-1), out))
            shifted = torch.zeros((N*24 + 1,), dtype=torch.float32, device=dev)[1:].reshape(N, 24)
            assert raises(lambda: r.query_surface_into(drays, shifted))
            r.query_surface_into(drays, out)                                       # ... and the context still answers
            assert out.cpu().numpy().tobytes() == want.tobytes()
        r.close()
    print("SURFACE_QUERY_TORCH_OK")


if __name__ == "__main__":
    main(sys.argv[1])
