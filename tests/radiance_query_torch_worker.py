"""Worker of tests/test_gpu_radiance_query.py::test_device_tensors, a process of its own because torch must be imported before tungsten_amd (one HIP
runtime per process): Renderer.query_radiance_into with torch tensors on the context's device against Renderer.query_radiance, with both samplers, on
the flat list (cornell) and on the 8-wide walk (materialtest); what query_radiance_into refuses; and a framebuffer bound to torch tensors
(tghip_bind_framebuffer) that a query between two passes leaves alone.

    python tests/radiance_query_torch_worker.py <scratch directory>      prints RADIANCE_QUERY_TORCH_OK"""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import scenes  # noqa: E402
import tungsten_amd as tg  # noqa: E402
from tungsten_amd import capi  # noqa: E402

N = 2500


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
    o = lo + (hi - lo)*(0.2 + 0.6*rs.rand(N, 3))
    dirs = rs.randn(N, 3)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = np.concatenate([o, np.full((N, 1), 1e-4), dirs, np.full((N, 1), np.inf)], axis=1).astype(np.float32)
    rays[::7, 7] = 0.25*np.linalg.norm(hi - lo)
    return rays


def main(tmp):
    dev = torch.device("cuda", 0)
    makers = [("cornell", scenes.cornell)] + ([("materialtest", scenes.materialtest)] if scenes.have_materialtest() else [])
    for name, mk in makers:
        path = mk(tmp, resolution=(64, 36), spp=4, spp_step=2, name=name + ".json", renderer={"stratified_sampler": True})
        rays = batch(path)
        r = tg.Renderer(path)
        drays = torch.from_numpy(rays).to(dev)
        for sobol_seed in (None, 99):
            want_sum, want_count = r.query_radiance(rays, 1, 5, sobol_seed=sobol_seed)
            assert (want_count == 4).all() and (want_sum > 0).any(axis=-1).sum() > N//10, name
            for n in (N, 257, 1):
                ssum = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
                count = torch.full((n,), 9, dtype=torch.int32, device=dev)
                r.query_radiance_into(drays[:n].contiguous(), ssum, count, 1, 5, sobol_seed=sobol_seed)
                assert ssum.cpu().numpy().tobytes() == want_sum[:n].tobytes(), (name, n)
                assert count.cpu().numpy().tobytes() == want_count[:n].tobytes(), (name, n)
        want_sum, want_count = r.query_radiance(rays, 1, 5)
        # outputs that are 4-byte, not 16-byte aligned, with guard words around them that must stay as they are
        wide_sum = torch.full((N*3 + 2,), -7.0, dtype=torch.float32, device=dev)
        wide_count = torch.full((N + 2,), 9, dtype=torch.int32, device=dev)
        ssum, count = wide_sum[1:-1].reshape(N, 3), wide_count[1:-1]
        assert ssum.data_ptr() % 16 != 0 and ssum.is_contiguous()
        r.query_radiance_into(drays, ssum, count, 1, 5)
        assert ssum.cpu().numpy().tobytes() == want_sum.tobytes() and count.cpu().numpy().tobytes() == want_count.tobytes(), name
        assert wide_sum[0].item() == -7.0 and wide_sum[-1].item() == -7.0 and wide_count[0].item() == 9 and wide_count[-1].item() == 9
        if name == "cornell":
            # what query_radiance_into refuses: dtype, device, contiguity, size -- and device rays that are not 16-byte aligned (the C-ABI's refusal)
            ssum, count = torch.zeros((N, 3), dtype=torch.float32, device=dev), torch.zeros((N,), dtype=torch.int32, device=dev)
            assert raises(lambda: r.query_radiance_into(drays.double(), ssum, count))
            assert raises(lambda: r.query_radiance_into(drays, ssum.double(), count))
            assert raises(lambda: r.query_radiance_into(drays, ssum, count.float()))
            assert raises(lambda: r.query_radiance_into(drays, ssum, count.to(torch.int64)))
            assert raises(lambda: r.query_radiance_into(drays.cpu(), ssum, count))
            assert raises(lambda: r.query_radiance_into(drays, ssum.cpu(), count))
            assert raises(lambda: r.query_radiance_into(drays, ssum, count.cpu()))
            assert raises(lambda: r.query_radiance_into(torch.zeros((N, 9), dtype=torch.float32, device=dev)[:, :8], ssum, count))
            assert raises(lambda: r.query_radiance_into(drays, torch.zeros((N, 4), dtype=torch.float32, device=dev)[:, :3], count))
            assert raises(lambda: r.query_radiance_into(drays, ssum[:N - 1], count))
            assert raises(lambda: r.query_radiance_into(drays, ssum, count[:N - 1]))
            assert raises(lambda: r.query_radiance_into(drays.reshape(-1), ssum, count))
            assert raises(lambda: r.query_radiance_into(drays, ssum, count, 3, 3))
            shifted = torch.zeros((N*8 + 1,), dtype=torch.float32, device=dev)[1:].reshape(N, 8)
            assert raises(lambda: r.query_radiance_into(shifted, ssum, count))
            r.query_radiance_into(drays, ssum, count, 1, 5)                             # ... and the context still answers
            assert ssum.cpu().numpy().tobytes() == want_sum.tobytes()
            # a bound framebuffer: render [0, 2), query, render [2, 4) = a fresh context's [0, 4), and the query itself changes no word of it
            w, h = r.width, r.height
            images = []
            for ask in (False, True):
                r2 = tg.Renderer(path)
                fb_sum = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
                fb_count = torch.zeros((h, w), dtype=torch.int32, device=dev)
                assert tg.lib.tghip_bind_framebuffer(r2.context(), fb_sum.data_ptr(), fb_count.data_ptr()) == 0
                assert not r2.step()
                if ask:
                    before = (fb_sum.clone(), fb_count.clone())
                    got = r2.query_radiance(rays, 1, 5)
                    assert got[0].tobytes() == want_sum.tobytes() and got[1].tobytes() == want_count.tobytes()
                    r2.query_radiance_into(drays, ssum, count, 1, 5)
                    assert torch.equal(before[0], fb_sum) and torch.equal(before[1], fb_count)
                assert r2.step()
                assert int(fb_count.min()) == 4 and int(fb_count.max()) == 4
                images.append(fb_sum.cpu().numpy().tobytes())
                assert tg.lib.tghip_bind_framebuffer(r2.context(), None, None) == 0
                r2.close()
            assert images[0] == images[1]
        r.close()
    print("RADIANCE_QUERY_TORCH_OK")


if __name__ == "__main__":
    main(sys.argv[1])
