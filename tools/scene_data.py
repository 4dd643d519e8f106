"""tests/golden/scene_data/: the scene files of the benchmark and the tests, stored compressed, and their unpacking into assets/.

    python tools/scene_data.py pack <scene directory> <name>     # (re)writes tests/golden/scene_data/<name>/ from an upstream copy

Every file is stored as <file>.xz (xz -9e), except Radiance .hdr images: xz gains little on their run-length-encoded RGBE scanlines, so an
.hdr is stored as <file>.rgbe.xz -- the header and the decoded RGBE planes, green subtracted from red and blue, each plane replaced by its
residual against the median edge detector prediction (LOCO-I), then xz.  unpack() inverts that and run-length encodes the scanlines again
the way the RGBE writer does, which gives the upstream file byte for byte; SHA256SUMS holds every file's digest and unpack() checks it.
__graft_entry__.build() calls unpack()."""
import hashlib
import lzma
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE = os.path.join(ROOT, "tests", "golden", "scene_data")
ASSETS = os.path.join(ROOT, "assets")
MAGIC = b"TGRGBE01"
XZ_FILTERS = [{"id": lzma.FILTER_LZMA2, "preset": 9 | lzma.PRESET_EXTREME, "lc": 4, "lp": 0, "pb": 0}]


# ---- Radiance RGBE ---------------------------------------------------------------------------------------------------------

def read_hdr(data):
    """Upstream .hdr bytes -> (header incl. the resolution line, planes uint8 [4, h, w]).  New-style RLE scanlines only."""
    import numpy as np
    end = data.index(b"\n\n") + 2
    line_end = data.index(b"\n", end) + 1
    fields = data[end:line_end].split()
    if len(fields) != 4 or fields[0] != b"-Y" or fields[2] != b"+X":
        raise ValueError("unsupported .hdr orientation %r" % data[end:line_end])
    h, w = int(fields[1]), int(fields[3])
    planes = np.zeros((4, h, w), np.uint8)
    pos = line_end
    for y in range(h):
        if data[pos] != 2 or data[pos + 1] != 2 or (data[pos + 2] << 8 | data[pos + 3]) != w:
            raise ValueError("scanline %d is not new-style RLE" % y)
        pos += 4
        for c in range(4):
            x = 0
            while x < w:
                n = data[pos]
                pos += 1
                if n > 128:
                    planes[c, y, x:x + n - 128] = data[pos]
                    pos += 1
                    x += n - 128
                else:
                    planes[c, y, x:x + n] = np.frombuffer(data[pos:pos + n], np.uint8)
                    pos += n
                    x += n
    if pos != len(data):
        raise ValueError("trailing bytes after the last scanline")
    return data[:line_end], planes


def _rle(buf):
    """One scanline channel, run-length encoded the way Greg Ward's RGBE writer does it: runs of at least 4 equal bytes, up to 127;
    literal stretches of up to 128 bytes; a short run directly in front of a long one is written as a run of its own."""
    out = bytearray()
    n, cur = len(buf), 0
    while cur < n:
        beg = cur
        cnt = old = 0
        while cnt < 4 and beg < n:
            beg += cnt
            old = cnt
            cnt = 1
            while beg + cnt < n and cnt < 127 and buf[beg] == buf[beg + cnt]:
                cnt += 1
        if old > 1 and old == beg - cur:
            out += bytes((128 + old, buf[cur]))
            cur = beg
        while cur < beg:
            k = min(128, beg - cur)
            out.append(k)
            out += buf[cur:cur + k]
            cur += k
        if cnt >= 4:
            out += bytes((128 + cnt, buf[beg]))
            cur += cnt
    return out


def write_hdr(header, planes):
    _, h, w = planes.shape
    out = bytearray(header)
    for y in range(h):
        out += bytes((2, 2, w >> 8, w & 255))
        for c in range(4):
            out += _rle(planes[c, y].tobytes())
    return bytes(out)


def _med_residual(p):
    """p int32 [4, h, w] -> residual against the LOCO-I median edge detector (neighbours outside the image are 0), mod 256."""
    import numpy as np
    q = np.zeros((p.shape[0], p.shape[1] + 1, p.shape[2] + 1), np.int32)
    q[:, 1:, 1:] = p
    a, b, c = q[:, 1:, :-1], q[:, :-1, 1:], q[:, :-1, :-1]
    pred = np.where(c >= np.maximum(a, b), np.minimum(a, b), np.where(c <= np.minimum(a, b), np.maximum(a, b), a + b - c))
    return ((p - pred) & 255).astype(np.uint8)


def _med_reconstruct(r):
    """Inverse of _med_residual, one anti-diagonal at a time (a pixel's left, upper and upper-left neighbours lie on earlier ones)."""
    import numpy as np
    ch, h, w = r.shape
    q = np.zeros((ch, h + 1, w + 1), np.int32)
    r = r.astype(np.int32)
    for k in range(h + w - 1):
        y = np.arange(max(0, k - w + 1), min(h, k + 1))
        x = k - y
        a, b, c = q[:, y + 1, x], q[:, y, x + 1], q[:, y, x]
        pred = np.where(c >= np.maximum(a, b), np.minimum(a, b), np.where(c <= np.minimum(a, b), np.maximum(a, b), a + b - c))
        q[:, y + 1, x + 1] = (r[:, y, x] + pred) & 255
    return q[:, 1:, 1:].astype(np.uint8)


def pack_hdr(data):
    import numpy as np
    header, planes = read_hdr(data)
    p = planes.astype(np.int32)
    p[0] = (p[0] - p[1]) & 255
    p[2] = (p[2] - p[1]) & 255
    _, h, w = planes.shape
    body = MAGIC + struct.pack("<III", len(header), h, w) + header + _med_residual(p).tobytes()
    return lzma.compress(body, format=lzma.FORMAT_XZ, filters=XZ_FILTERS)


def unpack_hdr(blob):
    import numpy as np
    body = lzma.decompress(blob)
    if body[:8] != MAGIC:
        raise ValueError("not a packed RGBE image")
    n, h, w = struct.unpack("<III", body[8:20])
    header = body[20:20 + n]
    p = _med_reconstruct(np.frombuffer(body[20 + n:], np.uint8).reshape(4, h, w)).astype(np.int32)
    p[0] = (p[0] + p[1]) & 255
    p[2] = (p[2] + p[1]) & 255
    return write_hdr(header, p.astype(np.uint8))


# ---- the store -------------------------------------------------------------------------------------------------------------

def _sums(scene):
    with open(os.path.join(STORE, scene, "SHA256SUMS")) as f:
        return {name: digest for digest, name in (line.split() for line in f if line.strip())}


def pack(src, scene):
    dst = os.path.join(STORE, scene)
    os.makedirs(dst, exist_ok=True)
    lines = []
    for name in sorted(os.listdir(src)):
        with open(os.path.join(src, name), "rb") as f:
            data = f.read()
        if name.endswith(".hdr"):
            stored, blob = name + ".rgbe.xz", pack_hdr(data)
            if unpack_hdr(blob) != data:
                raise SystemExit("%s: the packed image does not give the file back" % name)
        else:
            stored, blob = name + ".xz", lzma.compress(data, format=lzma.FORMAT_XZ, preset=9 | lzma.PRESET_EXTREME)
        with open(os.path.join(dst, stored), "wb") as f:
            f.write(blob)
        lines.append("%s  %s\n" % (hashlib.sha256(data).hexdigest(), name))
    with open(os.path.join(dst, "SHA256SUMS"), "w") as f:
        f.writelines(lines)


def read_stored(scene, name):
    """The bytes of upstream file `name` of `scene`, decoded from the store."""
    if name.endswith(".hdr"):
        with open(os.path.join(STORE, scene, name + ".rgbe.xz"), "rb") as f:
            return unpack_hdr(f.read())
    with lzma.open(os.path.join(STORE, scene, name + ".xz")) as f:
        return f.read()


def unpack():
    """tests/golden/scene_data/<scene>/ -> assets/<scene>/; a file already in place with the right digest is kept."""
    for scene in sorted(os.listdir(STORE)):
        if not os.path.isfile(os.path.join(STORE, scene, "SHA256SUMS")):
            continue
        dst = os.path.join(ASSETS, scene)
        os.makedirs(dst, exist_ok=True)
        for name, digest in sorted(_sums(scene).items()):
            out = os.path.join(dst, name)
            if os.path.exists(out):
                with open(out, "rb") as f:
                    if hashlib.sha256(f.read()).hexdigest() == digest:
                        continue
            data = read_stored(scene, name)
            if hashlib.sha256(data).hexdigest() != digest:
                raise RuntimeError("%s/%s: unpacked bytes do not match SHA256SUMS" % (scene, name))
            tmp = out + ".part"
            with open(tmp, "wb") as f:
                f.write(data)
            os.replace(tmp, out)


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] != "pack":
        raise SystemExit(__doc__)
    pack(sys.argv[2], sys.argv[3])
