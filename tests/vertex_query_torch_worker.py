"""Worker of tests/test_gpu_vertex_query.py::test_device_tensors, a process of its own because torch must be imported before tungsten_amd (one HIP
runtime per process): Renderer.query_vertex_into with torch tensors on the context's device against Renderer.start_paths / query_vertex -- in the
fogged Cornell box (media, a start medium per ray) and in the zoo of materials, begun on the rays and advanced in place, whole and turn by turn --,
guard rows on both sides of the states, and what query_vertex_into refuses.

    python tests/vertex_query_torch_worker.py <scratch directory>      prints VERTEX_QUERY_TORCH_OK"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import scenes  # noqa: E402
import tungsten_amd as tg  # noqa: E402
from ray_query_torch_worker import raises  # noqa: E402
from test_gpu_radiance_query import camera_rays  # noqa: E402

GUARD = -7.0
WORDS = tg.PATH_DTYPE.itemsize//4


def main(tmp):
    dev = torch.device("cuda", 0)
    for name in ("cornell_fog", "zoo_d"):
        mk, kw = scenes.GOLDEN_CASES[name]
        w, h = kw["resolution"]
        path = mk(tmp, name=name + "_t.json", **kw)
        flat = tg.FlattenedScene(path)
        rays = camera_rays(flat, w, h, tg.DEFAULT_SEED, 0)
        max_bounces = int(flat.desc.contents.settings.max_bounces)
        flat.close()
        N = len(rays)
        r = tg.Renderer(path)
        per_ray = np.where(np.arange(N) % 3 == 0, -1, -2).astype(np.int32)         # no medium, or the camera's
        drays = torch.from_numpy(rays).to(dev)
        for use_media in (False, True):
            kw2 = dict(sample=1, seed=11, first_index=5, first_number=2)
            first, first_alive = r.start_paths(rays, turns=1, media=per_ray if use_media else None, **kw2)
            ends, ends_alive = r.start_paths(rays, turns=max_bounces, media=per_ray if use_media else None, **kw2)
            assert 0 < first_alive <= N and ends_alive == 0 and (ends["emission"] != 0).any()      # (in the fog every path outlives its first turn)
            dmedia = torch.from_numpy(per_ray).to(dev) if use_media else None
            for n in sorted({N, 257, 65, 64, 63, 1}, reverse=True):
                # the states in the middle of a longer tensor: 4 guard rows in front (448 bytes: the view stays 16-byte aligned) and 4 behind
                block = torch.full((n + 8, WORDS), GUARD, dtype=torch.float32, device=dev)
                states = block[4:n + 4]
                alive = r.query_vertex_into(states, rays=drays[:n].contiguous(), media=None if dmedia is None else dmedia[:n].contiguous(), turns=1, **kw2)
                host = block.cpu().numpy()
                assert host[4:n + 4].tobytes() == first[:n].tobytes(), (name, use_media, n)
                assert alive == int((first[:n]["status"] == 0).sum())
                # ... advanced in place, turn by turn, to the end
                turns = 1
                while alive:
                    alive = r.query_vertex_into(states)
                    turns += 1
                assert turns <= max_bounces
                host = block.cpu().numpy()
                assert host[4:n + 4].tobytes() == ends[:n].tobytes(), (name, use_media, n)
                assert (host[:4] == GUARD).all() and (host[n + 4:] == GUARD).all(), (name, use_media, n)
            flat_states = torch.zeros((N*WORDS,), dtype=torch.int32, device=dev)          # any shape with N x 28 elements, the words as integers
            assert r.query_vertex_into(flat_states, rays=drays, media=dmedia, turns=max_bounces, **kw2) == 0
            assert flat_states.cpu().numpy().tobytes() == ends.tobytes(), name
            # states made on the host go on on the device
            dstates = torch.from_numpy(first.view(np.float32).reshape(N, WORDS).copy()).to(dev)
            assert r.query_vertex_into(dstates, turns=max_bounces) == 0
            assert dstates.cpu().numpy().tobytes() == ends.tobytes(), name
        if name == "cornell_fog":
            # what query_vertex_into refuses: dtype, device, contiguity, size -- and device views that are not aligned (the C-ABI's refusal)
            states = torch.zeros((N, WORDS), dtype=torch.float32, device=dev)
            dmedia = torch.from_numpy(per_ray).to(dev)
            assert raises(lambda: r.query_vertex_into(states, rays=drays.double()))
            assert raises(lambda: r.query_vertex_into(states.double(), rays=drays))
            assert raises(lambda: r.query_vertex_into(states, rays=drays.cpu()))
            assert raises(lambda: r.query_vertex_into(states.cpu(), rays=drays))
            assert raises(lambda: r.query_vertex_into(states.cpu()))
            assert raises(lambda: r.query_vertex_into(states.double()))
            assert raises(lambda: r.query_vertex_into(states, rays=drays, media=dmedia.cpu()))
            assert raises(lambda: r.query_vertex_into(states, rays=drays, media=dmedia.float()))
            assert raises(lambda: r.query_vertex_into(states, rays=drays, media=dmedia[:N - 1]))
            assert raises(lambda: r.query_vertex_into(states, media=dmedia))
            assert raises(lambda: r.query_vertex_into(states[:N - 1], rays=drays))
            assert raises(lambda: r.query_vertex_into(torch.zeros((N, WORDS + 1), dtype=torch.float32, device=dev)[:, :WORDS], rays=drays))
            assert raises(lambda: r.query_vertex_into(torch.zeros((N, WORDS + 1), dtype=torch.float32, device=dev)[:, :WORDS]))
            assert raises(lambda: r.query_vertex_into(torch.zeros((N*WORDS + 1,), dtype=torch.float32, device=dev)[1:]))
            shifted = torch.zeros((N*WORDS + 1,), dtype=torch.float32, device=dev)[1:].reshape(N, WORDS)
            assert raises(lambda: r.query_vertex_into(shifted, rays=drays))
            assert raises(lambda: r.query_vertex_into(states, rays=drays, medium=99))
            assert raises(lambda: r.query_vertex_into(states, rays=drays, turns=0))
            assert raises(lambda: r.query_vertex_into(states, rays=drays, first_number=1025))
            ends, _ = r.start_paths(rays, turns=max_bounces, media=per_ray)
            assert r.query_vertex_into(states, rays=drays, media=dmedia, turns=max_bounces) == 0      # ... and the context still answers
            assert states.cpu().numpy().tobytes() == ends.tobytes()
        r.close()
    print("VERTEX_QUERY_TORCH_OK")


if __name__ == "__main__":
    main(sys.argv[1])
