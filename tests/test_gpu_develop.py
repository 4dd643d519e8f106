"""The frame developed on the device (tghip_develop, csrc/hip/develop.hip) against the host's own functions (tgh_develop_host_frame / _aux:
what the output files were made by before), byte for byte: crafted framebuffers and auxiliary buffers at 67 x 35 -- 2 345 pixels: odd, one more
than a multiple of four, no multiple of 64, so the packed stores' tail and a partial last wave are in it --, a real render's files with the
device and the host path, torch tensors as outputs and as framebuffer, the error cases, and the reference program's own PNGs."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import develop_cases as dc
import scenes
import tungsten_amd as tg
from tungsten_amd import capi

pytestmark = pytest.mark.gpu

W, H = 67, 35
N = W*H
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BINARY = os.path.join(ROOT, "oracle", "_ref", "tungsten_hip_ref")


def _device(ctx, source, part, op, channels, flags=0):
    desc = capi.TgHipDevelopDesc(source, part, op, flags)
    hdr, ldr = np.empty((N, channels), np.float32), np.empty((N, 3), np.uint8)
    rc = tg.lib.tghip_develop(ctx, C.byref(desc), hdr.ctypes.data, ldr.ctypes.data, N)
    assert rc == 0, tg.lib.tghip_last_error(ctx)
    # each output on its own is the same image
    hdr2, ldr2 = np.empty_like(hdr), np.empty_like(ldr)
    assert tg.lib.tghip_develop(ctx, C.byref(desc), hdr2.ctypes.data, None, N) == 0 and tg.lib.tghip_develop(ctx, C.byref(desc), None, ldr2.ctypes.data, N) == 0
    assert dc.same_bits(hdr, hdr2) and dc.same_bits(ldr, ldr2)
    return hdr, ldr


@pytest.fixture(scope="module")
def renderer(tmp_path_factory):
    """The golden Cornell box at 67 x 35, one sample per pixel rendered so that the buffers exist."""
    tmp = tmp_path_factory.mktemp("develop")
    r = tg.Renderer(scenes.cornell(tmp, resolution=(W, H), spp=1), seed=tg.DEFAULT_SEED)
    r.render()
    assert (r.width, r.height) == (W, H)
    yield r
    r.close()


def test_crafted_framebuffer_every_operator(renderer):
    ctx = renderer.context()
    table_sum, table_count = dc.frame_table()
    ssum, count = dc.tiled(table_sum, N), dc.tiled(table_count, N)
    assert tg.lib.tghip_upload_framebuffer(ctx, ssum.ctypes.data, count.ctypes.data, N) == 0
    for op in range(5):
        want_hdr, want_ldr = dc.host_frame(ssum, count, op)
        hdr, ldr = _device(ctx, capi.TGHIP_DEVELOP_FRAME, capi.TGHIP_DEVELOP_MEAN, op, 3)
        bad = np.argwhere(hdr.view(np.uint32) != want_hdr.view(np.uint32))
        assert bad.size == 0, "%s: float image differs at %s: sum %s count %s" % (tg.TONEMAP_NAMES[op], bad[:4].tolist(), ssum[bad[0, 0]], count[bad[0, 0]])
        bad = np.argwhere(ldr != want_ldr)
        assert bad.size == 0, "%s: 8-bit image differs at %s: mean %s -> %s, host %s" % (
            tg.TONEMAP_NAMES[op], bad[:4].tolist(), want_hdr[bad[0, 0]], ldr[bad[0, 0]], want_ldr[bad[0, 0]])
    # the x86 conversion, spelt out: a mean of 1e8 under `linear` is black, not white
    at = int(np.argwhere((ssum[:, 0] == np.float32(1e8)) & (count == 1))[0, 0])
    assert _device(ctx, capi.TGHIP_DEVELOP_FRAME, capi.TGHIP_DEVELOP_MEAN, capi.TGHIP_TONEMAP_LINEAR, 3)[1][at, 0] == 0


def _check_aux(ctx, aux):
    assert tg.lib.tghip_upload_aux(ctx, aux.ctypes.data, N) == 0
    for output in range(5):
        for part in dc.PARTS:
            want_hdr, want_ldr = dc.host_aux(aux, output, part)
            hdr, ldr = _device(ctx, output, part, 0, dc.CHANNELS[output])
            bad = np.argwhere(hdr.view(np.uint32) != want_hdr.view(np.uint32))
            assert bad.size == 0, "%s / %s: float image differs at %s: %s" % (tg.AUX_OUTPUT_NAMES[output], tg.DEVELOP_PART_NAMES[part], bad[:4].tolist(), aux[bad[0, 0]])
            bad = np.argwhere(ldr != want_ldr)
            assert bad.size == 0, "%s / %s: 8-bit image differs at %s: %s -> %s, host %s" % (
                tg.AUX_OUTPUT_NAMES[output], tg.DEVELOP_PART_NAMES[part], bad[:4].tolist(), want_hdr[bad[0, 0]], ldr[bad[0, 0]], want_ldr[bad[0, 0]])


def test_crafted_aux_every_output_and_part(renderer):
    ctx = renderer.context()
    desc = capi.TgHipDevelopDesc(capi.TGHIP_AUX_DEPTH, capi.TGHIP_DEVELOP_MEAN, 0, 0)
    out = np.empty((N, 3), np.uint8)
    # an aux source before any aux buffer exists (the scene asks for no outputs, nothing has been uploaded)
    assert tg.lib.tghip_develop(ctx, C.byref(desc), None, out.ctypes.data, N) == capi.TGHIP_E_INVALID
    assert b"auxiliary" in tg.lib.tghip_last_error(ctx)
    aux = dc.tiled(dc.aux_table(), N)
    _check_aux(ctx, aux)
    aux["a"][:, 3], aux["b"][:, 3], aux["count"][:, 1] = np.inf, np.inf, 2          # a depth image that is all +inf: the maximum stays 0
    _check_aux(ctx, aux)
    assert (_device(ctx, capi.TGHIP_AUX_DEPTH, capi.TGHIP_DEVELOP_MEAN, 0, 1)[1] == 255).all()
    aux["a"][N - 2, 3], aux["b"][N - 2, 3] = 0.75, 0.25                             # ... and one with a single finite pixel, in the last, partial group
    _check_aux(ctx, aux)
    ldr = _device(ctx, capi.TGHIP_AUX_DEPTH, capi.TGHIP_DEVELOP_MEAN, 0, 1)[1]
    assert ldr[N - 2].tolist() == [255]*3 and (ldr == 255).all()                     # (its own maximum: 1.0 -> 255; everything else is a bad pixel)
    assert _device(ctx, capi.TGHIP_AUX_DEPTH, capi.TGHIP_DEVELOP_B, 0, 1)[0][N - 2, 0] == 0.25


def test_real_render_files_are_the_same_bytes_either_way(tmp_path):
    def edit(scene):
        scenes._outputs(scene)
        scene["camera"]["tonemap"] = "filmic"
        scene["renderer"].update(output_file="frame.png", hdr_output_file="frame.pfm", overwrite_output_files=True)
        for b in scene["renderer"]["output_buffers"]:
            b["hdr_output_file"] = b["type"] + ".pfm"
            b["ldr_output_file"] = b["type"] + ".png"
    files = {}
    for host in (0, 1):
        d = tmp_path/("host%d" % host)
        d.mkdir()
        path = scenes.cornell(d, resolution=(W, H), spp=8, edit=edit)
        cwd = os.getcwd()
        os.chdir(str(d))
        try:
            r = tg.Renderer(path, seed=tg.DEFAULT_SEED)
            r.set_option("develop_host", host)
            r.render()
            r.save_outputs()
            if host == 0:                                    # develop() is the device's image, the file's pixels
                frame = r.develop()
                depth_a = r.develop("depth", "a", hdr=True)
                aux = r.output_buffers()
            r.close()
        finally:
            os.chdir(cwd)
        files[host] = {f: open(os.path.join(str(d), f), "rb").read() for f in sorted(os.listdir(str(d))) if not f.endswith(".json")}
    want = ["frame.pfm", "frame.png"] + [t + tag + ext for t in scenes.OUTPUT_TYPES for tag in ("", "A", "B", "Variance") for ext in (".pfm", ".png")]
    assert sorted(files[0]) == sorted(want) and sorted(files[1]) == sorted(want)
    for f in want:
        assert files[0][f] == files[1][f], "%s differs between the device's and the host's development" % f
    assert frame.shape == (H, W, 3) and frame.dtype == np.uint8 and frame.max() > 100
    assert dc.same_bits(depth_a[..., 0], np.ascontiguousarray(aux["a"][..., 3]))
    assert dc.same_bits(tg.load_pfm(os.path.join(str(tmp_path/"host0"), "depthA.pfm"))[..., 0], depth_a[..., 0])


def test_device_tensors(tmp_path):
    """develop_into with torch tensors on the device equals develop, also with a torch tensor bound as framebuffer.  In a process of its own:
    torch brings its own HIP runtime and has to be imported before this package (tests/develop_torch_worker.py)."""
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "develop_torch_worker.py")
    p = subprocess.run([sys.executable, worker, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and "DEVELOP_TORCH_OK" in p.stdout, p.stdout[-4000:]


def test_error_cases_leave_the_context_working(tmp_path):
    path = scenes.cornell(tmp_path, resolution=(W, H), spp=2, spp_step=1)
    r = tg.Renderer(path, seed=tg.DEFAULT_SEED)
    r.step()
    ctx = r.context()
    out = np.empty((N, 3), np.uint8)
    frame, mean, gamma = capi.TGHIP_DEVELOP_FRAME, capi.TGHIP_DEVELOP_MEAN, capi.TGHIP_TONEMAP_GAMMA

    def fails(ctx_, desc, n=N, code=capi.TGHIP_E_INVALID):
        rc = tg.lib.tghip_develop(ctx_, C.byref(desc) if desc is not None else None, None, out.ctypes.data, n)
        assert rc == code, rc
        if ctx_ is not None:
            assert len(tg.lib.tghip_last_error(ctx_)) > 0 and tg.lib.tghip_last_error(ctx_) != b"no error"

    fails(None, capi.TgHipDevelopDesc(frame, mean, gamma, 0))
    fails(ctx, None)
    fails(ctx, capi.TgHipDevelopDesc(5, mean, gamma, 0))                              # unknown source
    fails(ctx, capi.TgHipDevelopDesc(capi.TGHIP_AUX_COLOR, 4, gamma, 0))              # unknown part
    fails(ctx, capi.TgHipDevelopDesc(frame, mean, 5, 0))                              # unknown operator
    fails(ctx, capi.TgHipDevelopDesc(frame, mean, gamma, 0), n=N - 1)                 # npixels != W*H
    fails(ctx, capi.TgHipDevelopDesc(capi.TGHIP_AUX_NORMAL, mean, gamma, 0))          # no aux buffer yet
    for part in (capi.TGHIP_DEVELOP_A, capi.TGHIP_DEVELOP_B, capi.TGHIP_DEVELOP_VARIANCE):
        fails(ctx, capi.TgHipDevelopDesc(frame, part, gamma, 0))                      # the frame has its mean only
    r.set_option("develop_host", 1)
    fails(ctx, capi.TgHipDevelopDesc(frame, mean, gamma, 0), code=capi.TGHIP_E_UNSUPPORTED)
    r.set_option("develop_host", 0)
    with pytest.raises(tg.TungstenError):
        r.develop("frame", "variance")
    # ... and the context renders a correct pass afterwards: the second sample, the image of an undisturbed render
    assert r.step()
    mean_img, ssum, count = r.image()
    developed = r.develop(tonemap="gamma")
    r.close()
    r = tg.Renderer(path, seed=tg.DEFAULT_SEED)
    r.render()
    want = r.image()
    want_developed = r.develop(tonemap="gamma")
    r.close()
    assert dc.same_bits(ssum, want[1]) and (count == want[2]).all() and (count == 2).all()
    assert dc.same_bits(developed, want_developed)
    assert dc.same_bits(developed.reshape(N, 3), dc.host_frame(ssum.reshape(N, 3), count.reshape(N), gamma)[1])


@pytest.mark.skipif(not os.path.exists(REF_BINARY), reason="oracle/_ref/tungsten_hip_ref not built (make -f oracle/Makefile.ref binding)")
@pytest.mark.parametrize("op", tg.TONEMAP_NAMES)
def test_cli_png_is_the_reference_programs_png(op, tmp_path):
    """The reference's own `tungsten` program with the plugin tone-maps with the reference's code (Integrator::writeBuffers, cameras/Tonemap.hpp)
    what the device rendered; this repository's CLI develops the same framebuffer on the device."""
    def edit(scene):
        scene["camera"]["tonemap"] = op
    path = scenes.cornell(str(tmp_path), resolution=(W, H), spp=4, edit=edit)
    d = json.load(open(path))
    d["integrator"]["type"] = "path_tracer_hip"
    hip_path = path.replace(".json", "_hip.json")
    json.dump(d, open(hip_path, "w"))
    ref_png, own_png = os.path.join(str(tmp_path), "ref.png"), os.path.join(str(tmp_path), "own.png")
    r = subprocess.run([REF_BINARY, "-t", "2", "-s", str(tg.DEFAULT_SEED), "-o", ref_png, hip_path], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(ref_png), r.stdout
    cli = os.path.join(ROOT, "tungsten_amd", "lib", "tungsten_hip")
    o = subprocess.run([cli, "-s", str(tg.DEFAULT_SEED), "-o", own_png, path], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert o.returncode == 0 and os.path.exists(own_png), o.stdout
    a, b = _png_pixels(ref_png), _png_pixels(own_png)
    assert a.shape == (H, W, 3) and a.max() > 100
    assert dc.same_bits(a, b), "%d of %d bytes differ" % (int((a != b).sum()), a.size)


def _png_pixels(path):
    """8-bit RGB / RGBA pixels of a PNG (the two programs use different encoders: the pixels are what is compared)."""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h, ch = 8, b"", 0, 0, 3
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            w, h, depth, color = struct.unpack(">IIBB", body[:10])
            assert depth == 8 and color in (2, 6)
            ch = 3 if color == 2 else 4
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w*ch)
    out = np.zeros((h, w*ch), np.uint8)
    for y in range(h):
        f, line = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        prev = out[y - 1].astype(np.int32) if y else np.zeros(w*ch, np.int32)
        cur = np.zeros(w*ch, np.int32)
        for x in range(w*ch):
            a = cur[x - ch] if x >= ch else 0
            b = prev[x]
            c = prev[x - ch] if x >= ch else 0
            if f == 0: p = 0
            elif f == 1: p = a
            elif f == 2: p = b
            elif f == 3: p = (a + b)//2
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2*c)
                p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            cur[x] = (line[x] + p) & 255
        out[y] = cur
    return np.ascontiguousarray(out.reshape(h, w, ch)[..., :3])
