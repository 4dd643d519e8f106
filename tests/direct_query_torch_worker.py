"""Worker of tests/test_gpu_direct_query.py::test_device_tensors, a process of its own because torch must be imported before tungsten_amd (one HIP
runtime per process): Renderer.query_direct_into with torch tensors on the context's device against Renderer.query_direct -- in the fogged box with
four kinds of emitter (surface mode and volume mode, a start medium per ray), under the pane stack (several rounds) and on instances --, guard words
on both sides of the answers, and what query_direct_into refuses.

    python tests/direct_query_torch_worker.py <scratch directory>      prints DIRECT_QUERY_TORCH_OK"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import direct_cases as dc  # noqa: E402
import tungsten_amd as tg  # noqa: E402
from ray_query_torch_worker import raises  # noqa: E402

GUARD = -7.0


def main(tmp):
    dev = torch.device("cuda", 0)
    groups = dc.load_golden()
    for scene, volume in (("dq_caps", False), ("dq_caps", True), ("dq_panes", False), ("dq_instances", False)):
        path = dc.build_scene(scene, tmp)
        media, prims = dc.names_of(path)
        r = tg.Renderer(path)
        mine = [g for g in groups if g["scene"] == scene and g["volume"] == volume]
        rays = np.ascontiguousarray(np.concatenate([g["rays"] for g in mine]))
        N = len(rays)
        assert N >= 64
        medium = media.get("fog")
        per_ray = np.full(N, -1 if medium is None else medium, np.int32)
        per_ray[::3] = -1
        kw = dict(spp=(1, 4), seed=11, bounce=1, skip=2, volume=volume)
        for use_media in (False, True):
            want = r.query_direct(rays, media=per_ray if use_media else None, medium=medium, **kw)
            assert (want["rgb"] != 0).any(axis=1).sum() >= 8, scene
            drays = torch.from_numpy(rays).to(dev)
            dmedia = torch.from_numpy(per_ray).to(dev) if use_media else None
            for n in sorted({N, min(N, 65), 64, 63, 1}, reverse=True):
                # the answers in the middle of a longer tensor: 2 guard rows in front (64 bytes: the view stays 16-byte aligned) and 2 behind
                block = torch.full((n + 4, 8), GUARD, dtype=torch.float32, device=dev)
                out = block[2:n + 2]
                r.query_direct_into(drays[:n].contiguous(), out, media=None if dmedia is None else dmedia[:n].contiguous(), medium=medium, **kw)
                host = block.cpu().numpy()
                assert host[2:n + 2].tobytes() == want[:n].tobytes(), (scene, use_media, n)
                assert (host[:2] == GUARD).all() and (host[n + 2:] == GUARD).all(), (scene, use_media, n)
            flat_out = torch.zeros((N*8,), dtype=torch.float32, device=dev)          # any shape with N x 8 elements
            r.query_direct_into(drays, flat_out, media=dmedia, medium=medium, **kw)
            assert flat_out.cpu().numpy().tobytes() == want.tobytes(), scene
        if scene == "dq_caps" and not volume:
            # what query_direct_into refuses: dtype, device, contiguity, size -- and device views that are not aligned (the C-ABI's refusal)
            out = torch.zeros((N, 8), dtype=torch.float32, device=dev)
            dmedia = torch.from_numpy(per_ray).to(dev)
            assert raises(lambda: r.query_direct_into(drays.double(), out))
            assert raises(lambda: r.query_direct_into(drays, out.to(torch.int32)))
            assert raises(lambda: r.query_direct_into(drays.cpu(), out))
            assert raises(lambda: r.query_direct_into(drays, out.cpu()))
            assert raises(lambda: r.query_direct_into(drays, out, media=dmedia.cpu()))
            assert raises(lambda: r.query_direct_into(drays, out, media=dmedia.float()))
            assert raises(lambda: r.query_direct_into(drays, out, media=dmedia[:N - 1]))
            assert raises(lambda: r.query_direct_into(torch.zeros((N, 9), dtype=torch.float32, device=dev)[:, :8], out))
            assert raises(lambda: r.query_direct_into(drays, torch.zeros((N, 9), dtype=torch.float32, device=dev)[:, :8]))
            assert raises(lambda: r.query_direct_into(drays, out[:N - 1]))
            assert raises(lambda: r.query_direct_into(drays.reshape(-1), out))
            shifted = torch.zeros((N*8 + 1,), dtype=torch.float32, device=dev)[1:].reshape(N, 8)
            assert raises(lambda: r.query_direct_into(drays, shifted))
            assert raises(lambda: r.query_direct_into(drays, out, medium=len(media) + 5))
            assert raises(lambda: r.query_direct_into(drays, out, light=99))
            want = r.query_direct(rays, media=per_ray, medium=medium, **kw)
            r.query_direct_into(drays, out, media=dmedia, medium=medium, **kw)     # ... and the context still answers
            assert out.cpu().numpy().tobytes() == want.tobytes()
        r.close()
    print("DIRECT_QUERY_TORCH_OK")


if __name__ == "__main__":
    main(sys.argv[1])
