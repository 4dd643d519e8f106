"""Worker of tests/test_gpu_transmittance_query.py::test_device_tensors, a process of its own because torch must be imported before tungsten_amd
(one HIP runtime per process): Renderer.query_transmittance_into with torch tensors on the context's device against Renderer.query_transmittance
-- on the stack of see-through panes in the fog (several rounds, a start medium per ray), on instances and on the gas scene --, guard words on both
sides of the answers, and what query_transmittance_into refuses.

    python tests/transmittance_query_torch_worker.py <scratch directory>      prints TRANSMITTANCE_QUERY_TORCH_OK"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import transmittance_cases as tc  # noqa: E402
import tungsten_amd as tg  # noqa: E402
from ray_query_torch_worker import raises  # noqa: E402

GUARD = -7.0


def main(tmp):
    dev = torch.device("cuda", 0)
    groups = tc.load_golden()
    for scene in ("tq_fog", "tq_instances", "tq_gas_davis"):
        path = tc.build_scene(scene, tmp)
        media, prims = tc.names_of(path)
        r = tg.Renderer(path)
        mine = [g for g in groups if g["scene"] == scene]
        rays = np.ascontiguousarray(np.concatenate([g["rays"] for g in mine]))
        N = len(rays)
        assert N > 129
        g = mine[0]
        medium = None if g["medium"] is None else media[g["medium"]]
        per_ray = np.full(N, -1 if medium is None else medium, np.int32)
        per_ray[::3] = -1
        kw = dict(starts_on_surface=True, ends_on_surface=g["ends"], bounce=1)
        for use_media in (False, True):
            want = r.query_transmittance(rays, media=per_ray if use_media else None, medium=medium, **kw)
            assert (want["rgb"] != 0).any(axis=1).sum() > N//10 and want["crossed"].max() >= 1, scene
            drays = torch.from_numpy(rays).to(dev)
            dmedia = torch.from_numpy(per_ray).to(dev) if use_media else None
            for n in (N, 129, 65, 1):
                # the answers in the middle of a longer tensor: 4 guard rows in front (64 bytes: the view stays 16-byte aligned) and 4 behind
                block = torch.full((n + 8, 4), GUARD, dtype=torch.float32, device=dev)
                out = block[4:n + 4]
                r.query_transmittance_into(drays[:n].contiguous(), out, media=None if dmedia is None else dmedia[:n].contiguous(), medium=medium, **kw)
                host = block.cpu().numpy()
                assert host[4:n + 4].tobytes() == want[:n].tobytes(), (scene, use_media, n)
                assert (host[:4] == GUARD).all() and (host[n + 4:] == GUARD).all(), (scene, use_media, n)
            flat_out = torch.zeros((N*4,), dtype=torch.float32, device=dev)          # any shape with N x 4 elements
            r.query_transmittance_into(drays, flat_out, media=dmedia, medium=medium, **kw)
            assert flat_out.cpu().numpy().tobytes() == want.tobytes(), scene
        if scene == "tq_fog":
            # what query_transmittance_into refuses: dtype, device, contiguity, size -- and device views that are not aligned (the C-ABI's refusal)
            out = torch.zeros((N, 4), dtype=torch.float32, device=dev)
            dmedia = torch.from_numpy(per_ray).to(dev)
            assert raises(lambda: r.query_transmittance_into(drays.double(), out))
            assert raises(lambda: r.query_transmittance_into(drays, out.to(torch.int32)))
            assert raises(lambda: r.query_transmittance_into(drays.cpu(), out))
            assert raises(lambda: r.query_transmittance_into(drays, out.cpu()))
            assert raises(lambda: r.query_transmittance_into(drays, out, media=dmedia.cpu()))
            assert raises(lambda: r.query_transmittance_into(drays, out, media=dmedia.float()))
            assert raises(lambda: r.query_transmittance_into(drays, out, media=dmedia[:N - 1]))
            assert raises(lambda: r.query_transmittance_into(torch.zeros((N, 9), dtype=torch.float32, device=dev)[:, :8], out))
            assert raises(lambda: r.query_transmittance_into(drays, torch.zeros((N, 5), dtype=torch.float32, device=dev)[:, :4]))
            assert raises(lambda: r.query_transmittance_into(drays, out[:N - 1]))
            assert raises(lambda: r.query_transmittance_into(drays.reshape(-1), out))
            shifted = torch.zeros((N*4 + 1,), dtype=torch.float32, device=dev)[1:].reshape(N, 4)
            assert raises(lambda: r.query_transmittance_into(drays, shifted))
            assert raises(lambda: r.query_transmittance_into(drays, out, medium=len(media) + 5))
            want = r.query_transmittance(rays, media=per_ray, medium=medium, **kw)
            r.query_transmittance_into(drays, out, media=dmedia, medium=medium, **kw)     # ... and the context still answers
            assert out.cpu().numpy().tobytes() == want.tobytes()
        r.close()
    print("TRANSMITTANCE_QUERY_TORCH_OK")


if __name__ == "__main__":
    main(sys.argv[1])
