"""Worker of tests/test_gpu_ray_queries.py::test_device_tensors, a process of its own because torch must be imported before tungsten_amd (one HIP
runtime per process): Renderer.query_rays_into with torch tensors on the context's device against Renderer.query_rays, in both modes, on the
8-wide walk (materialtest) and on the flat list (cornell), and what query_rays_into refuses.

    python tests/ray_query_torch_worker.py <scratch directory>      prints RAY_QUERY_TORCH_OK"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import scenes  # noqa: E402
import tungsten_amd as tg  # noqa: E402

N = 5000


def raises(fn):
    try:
        fn()
    except tg.TungstenError:
        return True
    return False


def batch(path):
    flat = tg.FlattenedScene(path)
    d = flat.desc.contents
    lo, hi = np.array(list(d.bounds_lo)), np.array(list(d.bounds_hi))
    flat.close()
    rs = np.random.RandomState(5)
    o = lo + (hi - lo)*rs.rand(N, 3)*1.2 - 0.1*(hi - lo)
    dirs = rs.randn(N, 3)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = np.concatenate([o, np.full((N, 1), 1e-4), dirs, np.full((N, 1), np.inf)], axis=1).astype(np.float32)
    rays[::7, 7] = 0.5*np.linalg.norm(hi - lo)
    return rays


def main(tmp):
    dev = torch.device("cuda", 0)
    makers = [("cornell", scenes.cornell)] + ([("materialtest", scenes.materialtest)] if scenes.have_materialtest() else [])
    for name, mk in makers:
        path = mk(tmp, resolution=(64, 36), spp=1, name=name + ".json")
        rays = batch(path)
        r = tg.Renderer(path)
        want_hits, want_occ = r.query_rays(rays, "closest"), r.query_rays(rays, "occluded")
        assert (want_hits["rec"] >= 0).sum() > N//10 and (want_occ == (want_hits["rec"] >= 0)).all(), name
        drays = torch.from_numpy(rays).to(dev)
        for n in (N, 257, 1):
            hits = torch.full((n, 4), -7.0, dtype=torch.float32, device=dev)
            occ = torch.full((n,), 9, dtype=torch.uint8, device=dev)
            part = drays[:n].contiguous()
            r.query_rays_into(part, hits, "closest")
            r.query_rays_into(part, occ, "occluded")
            assert hits.cpu().numpy().tobytes() == want_hits[:n].tobytes(), (name, n)
            assert occ.cpu().numpy().tobytes() == want_occ[:n].tobytes(), (name, n)
        odd = torch.full((N + 3,), 9, dtype=torch.uint8, device=dev)[3:]          # occlusion bytes need no alignment
        assert odd.data_ptr() % 4 != 0 and odd.is_contiguous()
        r.query_rays_into(drays, odd, "occluded")
        assert odd.cpu().numpy().tobytes() == want_occ.tobytes(), name
        if name == "cornell":
            # what query_rays_into refuses: dtype, device, contiguity, size -- and a device view that is not 16-byte aligned (the C-ABI's refusal)
            hits, occ = torch.zeros((N, 4), dtype=torch.float32, device=dev), torch.zeros((N,), dtype=torch.uint8, device=dev)
            assert raises(lambda: r.query_rays_into(drays.double(), hits))
            assert raises(lambda: r.query_rays_into(drays, hits.to(torch.int32)))
            assert raises(lambda: r.query_rays_into(drays, occ.float(), "occluded"))
            assert raises(lambda: r.query_rays_into(drays.cpu(), hits))
            assert raises(lambda: r.query_rays_into(drays, hits.cpu()))
            assert raises(lambda: r.query_rays_into(torch.zeros((N, 9), dtype=torch.float32, device=dev)[:, :8], hits))
            assert raises(lambda: r.query_rays_into(drays, torch.zeros((N, 5), dtype=torch.float32, device=dev)[:, :4]))
            assert raises(lambda: r.query_rays_into(drays, hits[:N - 1]))
            assert raises(lambda: r.query_rays_into(drays, occ[:N - 1], "occluded"))
            assert raises(lambda: r.query_rays_into(drays.reshape(-1), hits))
            assert raises(lambda: r.query_rays_into(drays, hits, "nearest"))
            shifted = torch.zeros((N*8 + 1,), dtype=torch.float32, device=dev)[1:].reshape(N, 8)
            assert raises(lambda: r.query_rays_into(shifted, hits))
            r.query_rays_into(drays, hits)                                         # ... and the context still answers
            assert hits.cpu().numpy().tobytes() == want_hits.tobytes()
        r.close()
    print("RAY_QUERY_TORCH_OK")


if __name__ == "__main__":
    main(sys.argv[1])
