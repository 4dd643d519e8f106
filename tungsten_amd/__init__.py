"""tungsten_amd -- MI355X-native `path_tracer_hip` integrator behind Tungsten's plugin surface.

Python here is only a ctypes convenience layer over the C-ABI (include/tungsten_hip.h,
include/tungsten_host.h) for tests and bench.py; all rendering happens in the native library
(C++11 host + HIP kernels for gfx950).  Importing the package fails if that library is missing:
there is no Python or CPU fallback.

A process that also uses PyTorch-ROCm must `import torch` BEFORE this package: torch ships its own HIP / HSA runtime, and two copies in one
process do not share the device (bench.py and the tests' multi-process workers import torch first; nothing here imports it).
"""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import (TgHipCounters, TgHipDevelopDesc, TgHipHit, TgHipNlMeansDesc, TgHipPassDesc, TgHipRay, TgHipSceneDesc, TgHostSceneInfo)

lib = capi.load_library()

AUX_DTYPE = np.dtype([("a", np.float32, 11), ("b", np.float32, 11), ("variance", np.float32, 11), ("count", np.uint32, 5)])
RECORD_DTYPE = np.dtype([("sample_count", np.uint32), ("next_sample_count", np.uint32), ("sample_index", np.uint32),
                         ("adaptive_weight", np.float32), ("mean", np.float32), ("running_variance", np.float32)])
# capi.TgHipBsdfCase / TgHipBsdfResult as numpy record types (Renderer.debug_bsdf)
BSDF_CASE_DTYPE = np.dtype([("bsdf", np.int32), ("requested", np.uint32), ("wi", np.float32, 3), ("wo", np.float32, 3), ("uv", np.float32, 2),
                            ("seed", np.uint32), ("stream", np.uint32), ("variant", np.uint32), ("reserved", np.uint32)])
BSDF_RESULT_DTYPE = np.dtype([("f", np.float32, 3), ("pdf", np.float32), ("sample_ok", np.uint32), ("sample_wo", np.float32, 3),
                              ("sample_weight", np.float32, 3), ("sample_pdf", np.float32), ("sampled", np.uint32), ("next", np.float32),
                              ("reserved", np.uint32, 2)])
# capi.TgHipLightCase / TgHipLightResult (Renderer.debug_light)
LIGHT_CASE_DTYPE = np.dtype([("light", np.int32), ("variant", np.uint32), ("p", np.float32, 3), ("w", np.float32, 3), ("seed", np.uint32), ("stream", np.uint32)])
LIGHT_RESULT_DTYPE = np.dtype([("chosen", np.int32), ("choose_weight", np.float32), ("sample_ok", np.uint32), ("d", np.float32, 3), ("dist", np.float32),
                               ("pdf", np.float32), ("approx", np.float32), ("hit", np.uint32), ("t", np.float32), ("u", np.float32), ("v", np.float32),
                               ("back_side", np.uint32), ("emission", np.float32, 3), ("direct_pdf", np.float32), ("choose_next", np.float32),
                               ("sample_next", np.float32), ("reserved", np.uint32, 4)])
# capi.TgHipMediumCase / TgHipMediumResult (Renderer.debug_medium)
MEDIUM_CASE_DTYPE = np.dtype([("medium", np.int32), ("variant", np.uint32), ("seed", np.uint32), ("stream", np.uint32), ("state_bounce", np.uint32),
                              ("p", np.float32, 3), ("d", np.float32, 3), ("max_t", np.float32), ("wo", np.float32, 3), ("reserved", np.uint32)])
MEDIUM_RESULT_DTYPE = np.dtype([("ok", np.uint32), ("t", np.float32), ("weight", np.float32, 3), ("exited", np.uint32), ("bounce_after", np.uint32),
                                ("tr", np.float32, (4, 3)), ("phase_f", np.float32), ("w", np.float32, 3), ("phase_pdf", np.float32),
                                ("dist_next", np.float32), ("phase_next", np.float32), ("reserved", np.uint32, 2)])
# capi.TgHipSurface (Renderer.query_surface)
SURFACE_DTYPE = np.dtype([("p", np.float32, 3), ("t", np.float32), ("ng", np.float32, 3), ("rec", np.int32), ("ns", np.float32, 3), ("instance", np.int32),
                          ("uv", np.float32, 2), ("object", np.int32), ("bsdf", np.int32), ("albedo", np.float32, 3), ("flags", np.uint32),
                          ("emission", np.float32, 3), ("reserved", np.uint32)])
# capi.TgHipTransmittance (Renderer.query_transmittance)
TRANSMITTANCE_DTYPE = np.dtype([("rgb", np.float32, 3), ("crossed", np.uint32)])
# capi.TgHipDirect (Renderer.query_direct)
DIRECT_DTYPE = np.dtype([("rgb", np.float32, 3), ("visibility", np.float32), ("count", np.uint32), ("visibility_count", np.uint32), ("rec", np.int32),
                         ("reserved", np.uint32)])
# capi.TgHipPath (Renderer.start_paths / query_vertex): the whole state of one caller-held path, 112 B
PATH_DTYPE = np.dtype([("o", np.float32, 3), ("tmin", np.float32), ("d", np.float32, 3), ("tmax", np.float32), ("throughput", np.float32, 3),
                       ("emission", np.float32, 3), ("status", np.uint32), ("medium", np.int32), ("medium_state_bounce", np.uint32), ("bounce", np.uint32),
                       ("flags", np.uint32), ("rec", np.int32), ("t", np.float32), ("rng_state", np.uint32, 2), ("key", np.uint32), ("drawn", np.uint32),
                       ("reserved", np.uint32, 3)])
PATH_END_NAMES = ("alive", "escaped", "max_bounces", "absorbed", "zero_throughput", "roulette", "nan")   # capi.TGHIP_PATH_*
DEFAULT_SEED = 0xBA5EBA11  # src/tungsten/Shared.hpp:246
TONEMAP_NAMES = ("linear", "gamma", "reinhard", "filmic", "pbrt")           # capi.TGHIP_TONEMAP_*
QUERY_MODE_NAMES = ("closest", "occluded")                                  # capi.TGHIP_QUERY_*
DEVELOP_PART_NAMES = ("mean", "a", "b", "variance")                          # capi.TGHIP_DEVELOP_*
AUX_OUTPUT_NAMES = ("color", "depth", "normal", "albedo", "visibility")      # capi.TGHIP_AUX_*


class TungstenError(RuntimeError):
    pass


def device_count():
    return int(lib.tghip_device_count())


class FlattenedScene(object):
    """Scene::load + loadResources + TraceableScene flattening (no device needed)."""

    def __init__(self, json_path):
        err = C.create_string_buffer(1024)
        self._h = lib.tgh_scene_load(os.fsencode(json_path), err, len(err))
        if not self._h:
            raise TungstenError(err.value.decode(errors="replace"))
        self.desc = lib.tgh_scene_desc(self._h)
        info = TgHostSceneInfo()
        lib.tgh_scene_info(self._h, C.byref(info))
        self.info = info

    @property
    def width(self):
        return int(self.info.width)

    @property
    def height(self):
        return int(self.info.height)

    def items(self):
        """The items of the reference's top-level Embree geometry -- the scene's finite primitives in scene order -- as (boxes [n, 6] float32:
        each one's bounds(), object indices [n] int32)."""
        boxes, objects = C.POINTER(C.c_float)(), C.POINTER(C.c_int32)()
        n = lib.tgh_scene_items(self._h, C.byref(boxes), C.byref(objects))
        if not n:
            return np.zeros((0, 6), np.float32), np.zeros(0, np.int32)
        return (np.ctypeslib.as_array(boxes, shape=(n, 6)).copy(), np.ctypeslib.as_array(objects, shape=(n,)).copy())

    def close(self):
        if self._h:
            lib.tgh_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Renderer(object):
    """makeTraceable(seed) with the path_tracer_hip integrator + the CLI render loop."""

    def __init__(self, json_path, seed=DEFAULT_SEED, spp=0, devices=0):
        err = C.create_string_buffer(1024)
        self._err = err
        self._h = lib.tgh_renderer_open(os.fsencode(json_path), seed & 0xFFFFFFFF, int(spp), int(devices), err, len(err))
        if not self._h:
            raise TungstenError(err.value.decode(errors="replace"))
        info = TgHostSceneInfo()
        lib.tgh_renderer_info(self._h, C.byref(info))
        self.info = info
        self.width, self.height = int(info.width), int(info.height)

    def _check(self, rc):
        if rc != 0:
            raise TungstenError(self._err.value.decode(errors="replace"))

    def context(self, device=0):
        return lib.tgh_renderer_context(self._h, device)

    def set_option(self, key, value, device=0):
        rc = lib.tghip_set_option(self.context(device), key.encode(), int(value))
        if rc != 0:
            raise TungstenError(lib.tghip_last_error(self.context(device)).decode())

    def step(self):
        done = C.c_int(0)
        self._check(lib.tgh_renderer_step(self._h, C.byref(done), self._err, len(self._err)))
        return bool(done.value)

    def render(self):
        """while (!done) { startRender; waitForCompletion }; returns wall seconds of the loop."""
        secs = C.c_double(0.0)
        self._check(lib.tgh_renderer_render(self._h, C.byref(secs), self._err, len(self._err)))
        return secs.value

    def image(self):
        """(mean, sum, count): mean radiance [H,W,3], raw radiance sums [H,W,3], sample counts [H,W]."""
        n = self.width*self.height
        mean = np.empty((self.height, self.width, 3), np.float32)
        ssum = np.empty((self.height, self.width, 3), np.float32)
        count = np.empty((self.height, self.width), np.uint32)
        self._check(lib.tgh_renderer_image(self._h, mean.ctypes.data, ssum.ctypes.data, count.ctypes.data, n,
                                           self._err, len(self._err)))
        return mean, ssum, count

    def counters(self, device=0):
        c = TgHipCounters()
        lib.tghip_get_counters(self.context(device), C.byref(c))
        return c

    def reset_counters(self, device=0):
        lib.tghip_reset_counters(self.context(device))

    def trace_rays(self, rays, repeats=1, device=0):
        """Batched TraceableScene::intersect: rays [N,8] float32 (o, tmin, d, tmax) -> hits (t,u,v,rec)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        hits = np.empty(rays.shape[0], dtype=[("t", np.float32), ("u", np.float32), ("v", np.float32), ("rec", np.int32)])
        ms = C.c_double(0.0)
        self._raise_last(self.context(device), lib.tghip_trace_rays(self.context(device), rays.ctypes.data, hits.ctypes.data, rays.shape[0], int(repeats), C.byref(ms)))
        return hits, ms.value

    def _raise_last(self, ctx, rc):
        if rc != 0:
            raise TungstenError(lib.tghip_last_error(ctx).decode())

    @staticmethod
    def _query_arrays(fn, rays, media=None):
        """The host arrays of a query: rays as float32 [N,8] and, where given, media as int32 [N]."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        if media is not None:
            media = np.ascontiguousarray(media, np.int32).reshape(-1)
            if media.size != rays.shape[0]:
                raise TungstenError("%s: media must hold one entry per ray" % fn)
        return rays, media

    @staticmethod
    def _query_tensors(fn, device, tensors, shapes, n=None):
        """The torch tensors of a query_*_into: (name, tensor or None, dtypes, elements per ray), the rays first -- each of one of its dtypes, on the
        context's device, contiguous and of N x elements, which `shapes` says in words.  Returns N: the rays' [N,8], or, for a call without rays,
        the n its caller took from another tensor (below zero: a tensor of no whole number of entries)."""
        if n is None:
            rays = tensors[0][1]
            n = rays.numel()//8 if rays.dim() == 2 and rays.shape[1] == 8 else -1
        for name, t, dtypes, size in tensors:
            if t is None:
                continue
            if str(t.dtype) not in dtypes:
                raise TungstenError("%s: %s must be %s, not %s" % (fn, name, " or ".join(dtypes), t.dtype))
            if not t.is_cuda or t.get_device() != device:
                raise TungstenError("%s: %s must live on the context's device (cuda:%d)" % (fn, name, device))
            if n < 0 or not t.is_contiguous() or t.numel() != n*size:
                raise TungstenError("%s: %s" % (fn, shapes))
        return n

    @staticmethod
    def _query_medium(medium):
        """An index, or "camera" / None as the C interface spells them"""
        return capi.TGHIP_MEDIUM_OF_CAMERA if medium == "camera" else capi.TGHIP_MEDIUM_NONE if medium is None else int(medium)

    def query_rays(self, rays, mode="closest", device=0):
        """Batched TraceableScene::intersect / ::occluded (tghip_query_rays): rays [N,8] float32 (o, tmin, d, tmax) -> with mode "closest" the
        structured hits of trace_rays (t, u, v, rec; the same bits), with "occluded" uint8 [N]: 1 where the closest-hit query has a hit."""
        if mode not in QUERY_MODE_NAMES:
            raise TungstenError("query_rays: mode must be 'closest' or 'occluded', not %r" % (mode,))
        rays, _ = self._query_arrays("query_rays", rays)
        if mode == "closest":
            out = np.empty(rays.shape[0], dtype=[("t", np.float32), ("u", np.float32), ("v", np.float32), ("rec", np.int32)])
        else:
            out = np.empty(rays.shape[0], np.uint8)
        desc = capi.TgHipRayQueryDesc(QUERY_MODE_NAMES.index(mode), 0)
        ctx = self.context(device)
        self._raise_last(ctx, lib.tghip_query_rays(ctx, C.byref(desc), rays.ctypes.data, out.ctypes.data, rays.shape[0]))
        return out

    def query_rays_into(self, rays, out, mode="closest", device=0):
        """The same on torch tensors of the context's device, without a copy through the host: rays float32 [N,8], out float32 [N,4] for
        "closest" (t, u, v and in the last column rec's bits) or uint8 [N] for "occluded", both contiguous.  The answers are complete when
        the call returns."""
        if mode not in QUERY_MODE_NAMES:
            raise TungstenError("query_rays_into: mode must be 'closest' or 'occluded', not %r" % (mode,))
        closest = mode == "closest"
        n = self._query_tensors("query_rays_into", device, (("rays", rays, ("torch.float32",), 8),
                                                            ("out", out, ("torch.float32" if closest else "torch.uint8",), 4 if closest else 1)),
                                "rays must be contiguous [N, 8] and out contiguous with N x %d elements" % (4 if closest else 1))
        desc = capi.TgHipRayQueryDesc(QUERY_MODE_NAMES.index(mode), capi.TGHIP_DEVELOP_DEVICE_POINTERS)
        ctx = self.context(device)
        self._raise_last(ctx, lib.tghip_query_rays(ctx, C.byref(desc), rays.data_ptr(), out.data_ptr(), n))

    def _radiance_desc(self, flags, spp_begin, spp_end, seed, sobol_seed):
        if sobol_seed is not None:
            flags |= capi.TGHIP_RADIANCE_SOBOL
        return capi.TgHipRadianceQueryDesc(flags, int(seed) & 0xFFFFFFFF, int(spp_begin), int(spp_end), int(sobol_seed or 0) & 0xFFFFFFFF)

    def query_radiance(self, rays, spp_begin=0, spp_end=1, seed=DEFAULT_SEED, sobol_seed=None, device=0):
        """Radiance along caller-supplied rays (tghip_query_radiance): rays [N,8] float32 (o, tmin, d, tmax) -> (sum [N,3] float32, count [N] uint32):
        for every ray the sum of PathTracer::traceSample over the sample indices [spp_begin, spp_end), each path starting on the ray behind the
        camera, and the samples counted.  sobol_seed: the SobolPathSampler seed of every ray's "tile" (the scene needs its Sobol' matrices); None
        draws from the counter-based stream keyed (seed, ray index, sample index)."""
        rays, _ = self._query_arrays("query_radiance", rays)
        ssum, count = np.empty((rays.shape[0], 3), np.float32), np.empty(rays.shape[0], np.uint32)
        desc = self._radiance_desc(0, spp_begin, spp_end, seed, sobol_seed)
        ctx = self.context(device)
        self._raise_last(ctx, lib.tghip_query_radiance(ctx, C.byref(desc), rays.ctypes.data, ssum.ctypes.data, count.ctypes.data, rays.shape[0]))
        return ssum, count

    def query_radiance_into(self, rays, out_sum, out_count, spp_begin=0, spp_end=1, seed=DEFAULT_SEED, sobol_seed=None, device=0):
        """The same on torch tensors of the context's device, without a copy through the host: rays float32 [N,8], out_sum float32 with N x 3
        elements, out_count int32 or uint32 with N elements (the counts' bits either way), all contiguous.  The answers are complete when
        the call returns."""
        n = self._query_tensors("query_radiance_into", device, (("rays", rays, ("torch.float32",), 8), ("out_sum", out_sum, ("torch.float32",), 3),
                                                                ("out_count", out_count, ("torch.int32", "torch.uint32"), 1)),
                                "rays must be contiguous [N, 8], out_sum contiguous with N x 3 and out_count with N elements")
        desc = self._radiance_desc(capi.TGHIP_DEVELOP_DEVICE_POINTERS, spp_begin, spp_end, seed, sobol_seed)
        ctx = self.context(device)
        self._raise_last(ctx, lib.tghip_query_radiance(ctx, C.byref(desc), rays.data_ptr(), out_sum.data_ptr(), out_count.data_ptr(), n))

    def query_surface(self, rays, device=0):
        """What is at the closest hit of every ray (tghip_query_surface): rays [N,8] float32 (o, tmin, d, tmax) -> a structured array [N] of
        SURFACE_DTYPE: position, t, geometric and shading normal, record, instance, uv, object, bsdf, albedo, flags (capi.TGHIP_SURFACE_*) and
        emission; for a miss the infinite emitter along the ray, if there is one."""
        rays, _ = self._query_arrays("query_surface", rays)
        out = np.empty(rays.shape[0], SURFACE_DTYPE)
        desc = capi.TgHipSurfaceQueryDesc(0)
        ctx = self.context(device)
        self._raise_last(ctx, lib.tghip_query_surface(ctx, C.byref(desc), rays.ctypes.data, out.ctypes.data, rays.shape[0]))
        return out

    def query_surface_into(self, rays, out, device=0):
        """The same on torch tensors of the context's device, without a copy through the host: rays float32 [N,8], out float32 with N x 24
        elements -- the words of SURFACE_DTYPE, the integer ones as their bits --, both contiguous.  The answers are complete when the call
        returns."""
        n = self._query_tensors("query_surface_into", device, (("rays", rays, ("torch.float32",), 8), ("out", out, ("torch.float32",), 24)),
                                "rays must be contiguous [N, 8] and out contiguous with N x 24 elements")
        desc = capi.TgHipSurfaceQueryDesc(capi.TGHIP_DEVELOP_DEVICE_POINTERS)
        ctx = self.context(device)
        self._raise_last(ctx, lib.tghip_query_surface(ctx, C.byref(desc), rays.data_ptr(), out.data_ptr(), n))

    def _transmittance_desc(self, flags, medium, end_cap, bounce, starts_on_surface, ends_on_surface):
        if starts_on_surface:
            flags |= capi.TGHIP_TRANSMITTANCE_STARTS_ON_SURFACE
        if ends_on_surface:
            flags |= capi.TGHIP_TRANSMITTANCE_ENDS_ON_SURFACE
        return capi.TgHipTransmittanceQueryDesc(flags, self._query_medium(medium), int(end_cap), int(bounce))

    def query_transmittance(self, rays, media=None, medium="camera", end_cap=-1, bounce=0, starts_on_surface=False, ends_on_surface=False, device=0):
        """How much light gets along every ray (tghip_query_transmittance, TraceBase::generalizedShadowRay): rays [N,8] float32 (o, tmin, d, tmax)
        -> a structured array [N] of TRANSMITTANCE_DTYPE: rgb, and crossed, the see-through surfaces the walk went through.  medium: the medium
        every ray starts in -- an index, None, or "camera" for the one the scene's camera is in; media: int32 [N], per ray instead.  end_cap: the
        object index of the primitive the rays are aimed at, -1 = none; bounce: the bounce count the walk starts with."""
        rays, media = self._query_arrays("query_transmittance", rays, media)
        out = np.empty(rays.shape[0], TRANSMITTANCE_DTYPE)
        desc = self._transmittance_desc(0, medium, end_cap, bounce, starts_on_surface, ends_on_surface)
        ctx = self.context(device)
        self._raise_last(ctx, lib.tghip_query_transmittance(ctx, C.byref(desc), rays.ctypes.data, media.ctypes.data if media is not None else None,
                                                            out.ctypes.data, rays.shape[0]))
        return out

    def query_transmittance_into(self, rays, out, media=None, medium="camera", end_cap=-1, bounce=0, starts_on_surface=False, ends_on_surface=False,
                                 device=0):
        """The same on torch tensors of the context's device, without a copy through the host: rays float32 [N,8], out float32 with N x 4
        elements -- rgb and crossed's bits --, media None or int32 [N], all contiguous.  The answers are complete when the call returns."""
        n = self._query_tensors("query_transmittance_into", device, (("rays", rays, ("torch.float32",), 8), ("out", out, ("torch.float32",), 4),
                                                                     ("media", media, ("torch.int32",), 1)),
                                "rays must be contiguous [N, 8], out contiguous with N x 4 and media with N elements")
        desc = self._transmittance_desc(capi.TGHIP_DEVELOP_DEVICE_POINTERS, medium, end_cap, bounce, starts_on_surface, ends_on_surface)
        ctx = self.context(device)
        self._raise_last(ctx, lib.tghip_query_transmittance(ctx, C.byref(desc), rays.data_ptr(), media.data_ptr() if media is not None else None,
                                                            out.data_ptr(), n))

    def _direct_desc(self, flags, spp, seed, medium, bounce, light, skip, volume):
        if volume:
            flags |= capi.TGHIP_DIRECT_VOLUME
        begin, end = (0, spp) if np.isscalar(spp) else spp
        return capi.TgHipDirectQueryDesc(flags, int(seed) & 0xFFFFFFFF, int(begin), int(end), self._query_medium(medium), int(bounce), int(light), int(skip))

    def query_direct(self, rays, spp=1, seed=DEFAULT_SEED, medium="camera", media=None, bounce=1, light=-1, skip=0, volume=False, device=0):
        """Direct lighting at the closest hit of every ray (tghip_query_direct, TraceBase::estimateDirect), or with volume=True at the rays' origins
        inside a medium (volumeEstimateDirect): rays [N,8] float32 (o, tmin, d, tmax) -> a structured array [N] of DIRECT_DTYPE: rgb, the sum of the
        estimates of the sample indices spp (a number: 0 .. spp - 1, or a pair (begin, end)) drawn from the stream keyed (seed, ray index, sample
        index) behind `skip` discarded numbers; visibility and visibility_count, the light samples' shadow-ray transmittance as the visibility
        output takes it; count, the samples taken; rec, the hit's record.  medium: the medium every ray travels in -- an index, None, or "camera" for
        the one the scene's camera is in; media: int32 [N], per ray instead.  bounce: the bounce handed to estimateDirect; light: -1 for
        chooseLight, or a slot of the scene's lights."""
        rays, media = self._query_arrays("query_direct", rays, media)
        out = np.empty(rays.shape[0], DIRECT_DTYPE)
        desc = self._direct_desc(0, spp, seed, medium, bounce, light, skip, volume)
        ctx = self.context(device)
        self._raise_last(ctx, lib.tghip_query_direct(ctx, C.byref(desc), rays.ctypes.data, media.ctypes.data if media is not None else None,
                                                     out.ctypes.data, rays.shape[0]))
        return out

    def query_direct_into(self, rays, out, spp=1, seed=DEFAULT_SEED, medium="camera", media=None, bounce=1, light=-1, skip=0, volume=False, device=0):
        """The same on torch tensors of the context's device, without a copy through the host: rays float32 [N,8], out float32 with N x 8
        elements -- the words of DIRECT_DTYPE, the integer ones as their bits --, media None or int32 [N], all contiguous.  The answers are complete
        when the call returns."""
        n = self._query_tensors("query_direct_into", device, (("rays", rays, ("torch.float32",), 8), ("out", out, ("torch.float32",), 8),
                                                              ("media", media, ("torch.int32",), 1)),
                                "rays must be contiguous [N, 8], out contiguous with N x 8 and media with N elements")
        desc = self._direct_desc(capi.TGHIP_DEVELOP_DEVICE_POINTERS, spp, seed, medium, bounce, light, skip, volume)
        ctx = self.context(device)
        self._raise_last(ctx, lib.tghip_query_direct(ctx, C.byref(desc), rays.data_ptr(), media.data_ptr() if media is not None else None,
                                                     out.data_ptr(), n))

    def _vertex_call(self, device, desc, rays, media, paths, n):
        ctx = self.context(device)
        alive = C.c_uint32(0)
        self._raise_last(ctx, lib.tghip_query_vertex(ctx, C.byref(desc), rays, media, paths, n, C.addressof(alive)))
        return int(alive.value)

    def start_paths(self, rays, sample=0, seed=DEFAULT_SEED, first_index=0, first_number=2, medium="camera", media=None, turns=1, device=0):
        """Paths the caller holds, begun on its rays (tghip_query_vertex with TGHIP_VERTEX_START): rays [N,8] float32 (o, tmin, d, tmax) -> (paths,
        alive): a structured array [N] of PATH_DTYPE -- the state of PathTracer::traceSample behind the camera: throughput 1, wasSpecular, the stream
        keyed (seed, first_index + i, sample) behind first_number discarded numbers (2: what a pinhole camera spends) -- advanced by `turns` turns
        of the loop, and how many of them are still alive.  medium: the medium every path starts in -- an index, None, or "camera"; media: int32
        [N], per ray instead."""
        rays, media = self._query_arrays("start_paths", rays, media)
        paths = np.empty(rays.shape[0], PATH_DTYPE)
        desc = capi.TgHipVertexQueryDesc(capi.TGHIP_VERTEX_START, int(seed) & 0xFFFFFFFF, int(sample), int(first_index), int(first_number),
                                         self._query_medium(medium), int(turns), 0)
        alive = self._vertex_call(device, desc, rays.ctypes.data, media.ctypes.data if media is not None else None, paths.ctypes.data,
                                  rays.shape[0])
        return paths, alive

    def query_vertex(self, paths, turns=1, device=0):
        """`turns` more turns of traceSample's loop on caller-held paths (tghip_query_vertex): paths a structured array [N] of PATH_DTYPE -> (paths,
        alive): a new array -- a path that is not alive comes back byte for byte -- and how many are still alive.  Between calls the states may be
        reordered, dropped, split into batches or edited field by field."""
        paths = np.array(paths, PATH_DTYPE, copy=True, order="C").reshape(-1)
        desc = capi.TgHipVertexQueryDesc(0, 0, 0, 0, 0, capi.TGHIP_MEDIUM_NONE, int(turns), 0)
        alive = self._vertex_call(device, desc, None, None, paths.ctypes.data, paths.size)
        return paths, alive

    def query_vertex_into(self, paths, rays=None, sample=0, seed=DEFAULT_SEED, first_index=0, first_number=2, medium="camera", media=None, turns=1, device=0):
        """The same on torch tensors of the context's device, without a copy through the host: paths float32 (or int32) with N x 28 elements -- the words
        of PATH_DTYPE, the integer ones as their bits --, advanced in place.  rays float32 [N,8] begins the paths on them first (start_paths; media
        None or int32 [N]); None advances the states `paths` holds.  Returns how many paths are still alive; the states are complete when the call
        returns."""
        if rays is not None:
            n = self._query_tensors("query_vertex_into", device, (("rays", rays, ("torch.float32",), 8), ("paths", paths, ("torch.float32", "torch.int32"), 28),
                                                                  ("media", media, ("torch.int32",), 1)),
                                    "rays must be contiguous [N, 8], paths contiguous with N x 28 and media with N elements")
            desc = capi.TgHipVertexQueryDesc(capi.TGHIP_DEVELOP_DEVICE_POINTERS | capi.TGHIP_VERTEX_START, int(seed) & 0xFFFFFFFF, int(sample),
                                             int(first_index), int(first_number), self._query_medium(medium), int(turns), 0)
            return self._vertex_call(device, desc, rays.data_ptr(), media.data_ptr() if media is not None else None,
                                     paths.data_ptr(), n)
        if media is not None:
            raise TungstenError("query_vertex_into: media belong to the rays that begin paths")
        n = self._query_tensors("query_vertex_into", device, (("paths", paths, ("torch.float32", "torch.int32"), 28),),
                                "paths must be contiguous with N x 28 elements", n=paths.numel()//28 if paths.numel() % 28 == 0 else -1)
        desc = capi.TgHipVertexQueryDesc(capi.TGHIP_DEVELOP_DEVICE_POINTERS, 0, 0, 0, 0, capi.TGHIP_MEDIUM_NONE, int(turns), 0)
        return self._vertex_call(device, desc, None, None, paths.data_ptr(), n)

    def debug_libm(self, fn, x, device=0):
        """The device's restatement of a host libm function (capi.TGHIP_LIBM_*) evaluated on the device: float32 in, float32 out."""
        dbl = capi.TGHIP_LIBM_EXPD <= int(fn) <= capi.TGHIP_LIBM_SQRTD       # the double-precision functions: float64 in, float64 out
        x = np.ascontiguousarray(x, np.float64 if dbl else np.float32).reshape(-1)
        two = int(fn) in (capi.TGHIP_LIBM_ATAN2F, capi.TGHIP_LIBM_POWF)      # operands interleaved: x[2i], x[2i+1]
        y = np.empty(x.size//2 if two else x.size, x.dtype)
        rc = lib.tghip_debug_libm(self.context(device), int(fn), x.ctypes.data, y.ctypes.data, y.size)
        if rc != 0:
            raise TungstenError(lib.tghip_last_error(self.context(device)).decode())
        return y

    def debug_bsdf(self, cases, device=0):
        """The shading kernels' BSDF code on caller-supplied cases (tghip_debug_bsdf): `cases` an array of BSDF_CASE_DTYPE, the result an
        array of BSDF_RESULT_DTYPE of the same length."""
        cases = np.ascontiguousarray(cases, BSDF_CASE_DTYPE).reshape(-1)
        out = np.zeros(cases.size, BSDF_RESULT_DTYPE)
        rc = lib.tghip_debug_bsdf(self.context(device), cases.ctypes.data if cases.size else None, out.ctypes.data if cases.size else None, cases.size)
        if rc != 0:
            raise TungstenError(lib.tghip_last_error(self.context(device)).decode())
        return out

    def debug_bsdf_info(self, variant=capi.TGHIP_BSDF_VARIANT_ALL, device=0):
        """(type_mask, forward, covered) per bsdf of the flattened table, as the shading-class rule sees them, and the mask the variant's kernel is
        compiled for (tghip_debug_bsdf_info)."""
        n = int(self.info.num_bsdfs)
        tm, fwd, cov = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        mask = C.c_uint32(0)
        rc = lib.tghip_debug_bsdf_info(self.context(device), int(variant), tm.ctypes.data, fwd.ctypes.data, cov.ctypes.data, C.addressof(mask))
        if rc != 0:
            raise TungstenError(lib.tghip_last_error(self.context(device)).decode())
        return tm, fwd.astype(bool), cov.astype(bool), int(mask.value)

    def debug_light(self, cases, device=0):
        """The shading kernels' light code on caller-supplied cases (tghip_debug_light): `cases` an array of LIGHT_CASE_DTYPE, the result an
        array of LIGHT_RESULT_DTYPE of the same length."""
        cases = np.ascontiguousarray(cases, LIGHT_CASE_DTYPE).reshape(-1)
        out = np.zeros(cases.size, LIGHT_RESULT_DTYPE)
        rc = lib.tghip_debug_light(self.context(device), cases.ctypes.data if cases.size else None, out.ctypes.data if cases.size else None, cases.size)
        if rc != 0:
            raise TungstenError(lib.tghip_last_error(self.context(device)).decode())
        return out

    def debug_light_info(self, variant=capi.TGHIP_BSDF_VARIANT_ALL, device=0):
        """(needs, covered) per slot of the scene's sampled lights and the mask the variant's kernel is compiled for (tghip_debug_light_info)."""
        n = int(self.info.num_lights)
        needs, cov = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        mask = C.c_uint32(0)
        rc = lib.tghip_debug_light_info(self.context(device), int(variant), needs.ctypes.data, cov.ctypes.data, C.addressof(mask))
        if rc != 0:
            raise TungstenError(lib.tghip_last_error(self.context(device)).decode())
        return needs, cov.astype(bool), int(mask.value)

    def debug_medium(self, cases, device=0):
        """The shading and shadow kernels' medium code on caller-supplied cases (tghip_debug_medium): `cases` an array of MEDIUM_CASE_DTYPE, the result
        an array of MEDIUM_RESULT_DTYPE of the same length."""
        cases = np.ascontiguousarray(cases, MEDIUM_CASE_DTYPE).reshape(-1)
        out = np.zeros(cases.size, MEDIUM_RESULT_DTYPE)
        rc = lib.tghip_debug_medium(self.context(device), cases.ctypes.data if cases.size else None, out.ctypes.data if cases.size else None, cases.size)
        if rc != 0:
            raise TungstenError(lib.tghip_last_error(self.context(device)).decode())
        return out

    def trace_samples(self, spp_begin, spp_end, seed=DEFAULT_SEED, tile_seeds=None, device=0):
        """One TGHIP_PASS_SAMPLES pass on the device (into a cleared framebuffer): the radiance of every individual sample,
        [H, W, spp_end - spp_begin, 3] -- PathTracer::traceSample's return value per (pixel, sample index).  With tile_seeds
        (one per 16x16 tile) the pass draws from the Sobol' sampler (TGHIP_PASS_SOBOL)."""
        ctx = self.context(device)
        flags = capi.TGHIP_PASS_SAMPLES | (capi.TGHIP_PASS_SOBOL if tile_seeds is not None else 0)
        p = TgHipPassDesc(int(spp_begin), int(spp_end), seed & 0xFFFFFFFF, 0, 1, flags)
        if tile_seeds is not None:
            seeds = np.ascontiguousarray(tile_seeds, np.uint32)
            p.tile_seeds = seeds.ctypes.data_as(C.POINTER(C.c_uint32))
        out = np.empty((self.height, self.width, int(spp_end) - int(spp_begin), 3), np.float32)
        for rc in (lib.tghip_clear_framebuffer(ctx), lib.tghip_render_pass(ctx, C.byref(p)), lib.tghip_wait(ctx),
                   lib.tghip_download_samples(ctx, out.ctypes.data, out.size)):
            if rc != 0:
                raise TungstenError(lib.tghip_last_error(ctx).decode())
        return out

    def save_resume_data(self):
        """Integrator::saveRenderResumeData: writes renderer.resume_render_file."""
        self._check(lib.tgh_renderer_save_resume_data(self._h, self._err, len(self._err)))

    def resume(self):
        """Integrator::resumeRender: True when a saved state of this very scene was found and restored."""
        ok = C.c_int(0)
        self._check(lib.tgh_renderer_resume(self._h, C.byref(ok), self._err, len(self._err)))
        return bool(ok.value)

    @property
    def current_spp(self):
        info = TgHostSceneInfo()
        lib.tgh_renderer_info(self._h, C.byref(info))
        return int(info.current_spp)

    def records(self):
        """The integrator's SampleRecords (one per 4x4 pixels) after the last pass, as a structured array [vh, vw]."""
        vw, vh = (self.width + 3)//4, (self.height + 3)//4
        rec = np.zeros(vw*vh, RECORD_DTYPE)
        self._check(lib.tgh_renderer_records(self._h, rec.ctypes.data, rec.size, self._err, len(self._err)))
        return rec.reshape(vh, vw)

    def output_buffers(self):
        """The auxiliary output buffers (renderer.output_buffers) as a structured array [H, W] of AUX_DTYPE: per output the
        A / B halves, the Welford variance sum and the sample count (include/tungsten_hip.h: TgHipAuxPixel)."""
        aux = np.zeros(self.width*self.height, AUX_DTYPE)
        self._check(lib.tgh_renderer_output_buffers(self._h, aux.ctypes.data, aux.size, self._err, len(self._err)))
        return aux.reshape(self.height, self.width)

    def save_outputs(self):
        self._check(lib.tgh_renderer_save_outputs(self._h, self._err, len(self._err)))

    def _develop_desc(self, source, part, tonemap, flags=0):
        src = capi.TGHIP_DEVELOP_FRAME if source == "frame" else AUX_OUTPUT_NAMES.index(source)
        if tonemap is None:
            op = lib.tgh_renderer_tonemap(self._h) if source == "frame" else 0
            if op < 0:
                raise TungstenError("the scene camera's tonemap operator is unknown")
        else:
            op = TONEMAP_NAMES.index(tonemap)
        return capi.TgHipDevelopDesc(src, DEVELOP_PART_NAMES.index(part), op, flags)

    def develop(self, source="frame", part="mean", tonemap=None, hdr=False):
        """One image of the output files, developed on the device (tghip_develop): the 8-bit RGB image uint8 [H, W, 3], or with hdr=True the
        float image [H, W, channels].  source: "frame" or an auxiliary output ("color", "depth", "normal", "albedo", "visibility"); part:
        "mean", "a", "b", "variance" (the frame has its mean only); tonemap: "linear", "gamma", "reinhard", "filmic", "pbrt", None = the scene
        camera's (the frame only: auxiliary outputs are never tone-mapped)."""
        desc = self._develop_desc(source, part, tonemap)
        channels = 3 if source == "frame" else capi.TGHIP_AUX_CHANNEL_COUNT[desc.source]
        out = np.empty((self.height, self.width, channels), np.float32) if hdr else np.empty((self.height, self.width, 3), np.uint8)
        self._check(lib.tgh_renderer_develop(self._h, C.byref(desc), out.ctypes.data if hdr else None, None if hdr else out.ctypes.data,
                                             self.width*self.height, self._err, len(self._err)))
        return out

    def develop_into(self, ldr=None, hdr=None, source="frame", part="mean", tonemap=None, device=0):
        """The same into torch tensors on the context's device, without a copy through the host: ldr uint8 [H, W, 3], hdr float32 [H, W, channels],
        both contiguous; either may be None."""
        desc = self._develop_desc(source, part, tonemap, capi.TGHIP_DEVELOP_DEVICE_POINTERS)
        channels = 3 if source == "frame" else capi.TGHIP_AUX_CHANNEL_COUNT[desc.source]
        for name, t, dtype, size in (("ldr", ldr, "torch.uint8", 3), ("hdr", hdr, "torch.float32", channels)):
            if t is None:
                continue
            if str(t.dtype) != dtype:
                raise TungstenError("develop_into: %s must be %s, not %s" % (name, dtype, t.dtype))
            if not t.is_cuda or t.get_device() != device:
                raise TungstenError("develop_into: %s must live on the context's device (cuda:%d)" % (name, device))
            if not t.is_contiguous() or t.numel() != self.width*self.height*size:
                raise TungstenError("develop_into: %s must be contiguous with %d x %d x %d elements" % (name, self.height, self.width, size))
        ctx = self.context(device)
        rc = lib.tghip_develop(ctx, C.byref(desc), hdr.data_ptr() if hdr is not None else None, ldr.data_ptr() if ldr is not None else None,
                               self.width*self.height)
        if rc != 0:
            raise TungstenError(lib.tghip_last_error(ctx).decode())

    def nlmeans(self, image, guide, variance, F, R, k, variance_scale=1.0, device=0):
        """The denoiser's NL-means filter on the device (tghip_nlmeans): `image` filtered with weights from `guide` and `variance` -- float32
        arrays [H, W] or [H, W, C], C = 1..4, all of one shape -- with patch radius F, search radius R and distance scale k; returns the filtered
        array, bit for bit the reference's nlMeans."""
        image, guide, variance = (np.ascontiguousarray(a, np.float32) for a in (image, guide, variance))
        if image.ndim not in (2, 3) or guide.shape != image.shape or variance.shape != image.shape:
            raise TungstenError("nlmeans: image, guide and variance must be [H, W] or [H, W, C] arrays of one shape")
        desc = TgHipNlMeansDesc(image.shape[1], image.shape[0], image.shape[2] if image.ndim == 3 else 1, int(F), int(R), float(k),
                                float(variance_scale), capi.TGHIP_NLMEANS_POINTERS, 0, 0, 0)
        out = np.empty_like(image)
        ctx = self.context(device)
        if lib.tghip_nlmeans(ctx, C.byref(desc), image.ctypes.data, guide.ctypes.data, variance.ctypes.data, out.ctypes.data) != 0:
            raise TungstenError(lib.tghip_last_error(ctx).decode())
        return out

    def nlmeans_aux(self, output, image_part, guide_part, F, R, k, variance_scale=1.0, device=0):
        """The same on the context's auxiliary buffers, nothing but the result leaving the device: the float images develop() gives for `output`'s
        `image_part` and `guide_part` ("mean", "a", "b") and its variance are the filter's three planes.  Returns [H, W, channels]."""
        src = AUX_OUTPUT_NAMES.index(output)
        desc = TgHipNlMeansDesc(self.width, self.height, 0, int(F), int(R), float(k), float(variance_scale), src,
                                DEVELOP_PART_NAMES.index(image_part), DEVELOP_PART_NAMES.index(guide_part), 0)
        out = np.empty((self.height, self.width, capi.TGHIP_AUX_CHANNEL_COUNT[src]), np.float32)
        ctx = self.context(device)
        if lib.tghip_nlmeans(ctx, C.byref(desc), None, None, None, out.ctypes.data) != 0:
            raise TungstenError(lib.tghip_last_error(ctx).decode())
        return out

    def prefilter_features(self, outputs=("depth", "normal", "albedo", "visibility")):
        """NFOR's feature cross-prefilter (denoiser.cpp: nforDenoiser, section 5.1) on the context's auxiliary buffers: per output the A half
        filtered with weights from the B half and the B half with weights from A (F 3, R 5, k 0.5, the variance doubled).  {name: (A', B')}."""
        return {name: (self.nlmeans_aux(name, "a", "b", 3, 5, 0.5, 2.0), self.nlmeans_aux(name, "b", "a", 3, 5, 0.5, 2.0)) for name in outputs}

    def close(self):
        if self._h:
            lib.tgh_renderer_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PassScheduler(object):
    """PathTraceIntegrator's pass scheduling without a device: tile seeds + generateWork over SampleRecords."""

    def __init__(self, width, height, seed=DEFAULT_SEED):
        self._h = lib.tgh_scheduler_create(int(width), int(height), seed & 0xFFFFFFFF)
        self.num_tiles = int(lib.tgh_scheduler_num_tiles(self._h))
        self.num_records = int(lib.tgh_scheduler_num_records(self._h))

    @property
    def tile_seeds(self):
        return np.ctypeslib.as_array(lib.tgh_scheduler_tile_seeds(self._h), shape=(self.num_tiles,)).copy()

    @property
    def records(self):
        """Mutable view of the records (write sample_count / mean / running_variance, read the rest)."""
        buf = (C.c_char*(self.num_records*RECORD_DTYPE.itemsize)).from_address(
            C.addressof(lib.tgh_scheduler_records(self._h).contents))
        return np.frombuffer(buf, RECORD_DTYPE)

    def generate_work(self, current_spp, next_spp, adaptive):
        return bool(lib.tgh_scheduler_generate_work(self._h, int(current_spp), int(next_spp), int(bool(adaptive))))

    def close(self):
        if self._h:
            lib.tgh_scheduler_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sobol_matrices():
    """The 1024 x 52 Sobol' generator matrices the host hands to the device."""
    n = C.c_size_t(0)
    err = C.create_string_buffer(1024)
    p = lib.tgh_sobol_matrices(C.byref(n), err, len(err))
    if not p:
        raise TungstenError(err.value.decode(errors="replace"))
    return np.ctypeslib.as_array(p, shape=(n.value,)).reshape(1024, 52)


def load_pfm(path):
    with open(path, "rb") as f:
        magic = f.readline().strip()
        w, h = [int(v) for v in f.readline().split()]
        scale = float(f.readline())
        ch = 3 if magic == b"PF" else 1
        data = np.frombuffer(f.read(w*h*ch*4), dtype="<f4" if scale < 0 else ">f4").reshape(h, w, ch)
    return np.ascontiguousarray(data[::-1]).astype(np.float32)
