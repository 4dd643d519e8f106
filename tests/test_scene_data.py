"""tools/scene_data.py: the stored scene files come back as the upstream files, and the RGBE image coding is lossless."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scene_data  # noqa: E402


def test_rgbe_coding_gives_the_file_back():
    """Random planes with runs of every length, including ones that straddle the 127 / 128 limits of the scanline encoding."""
    rng = np.random.default_rng(7)
    h, w = 9, 300
    planes = rng.integers(0, 256, (4, h, w), dtype=np.uint8)
    for c in range(4):
        for y in range(h):
            x = 0
            while x < w:
                n = int(rng.integers(1, 140))
                if rng.random() < 0.5:
                    planes[c, y, x:x + n] = planes[c, y, x]
                x += n
    header = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w)
    data = scene_data.write_hdr(header, planes)
    got_header, got = scene_data.read_hdr(data)
    assert got_header == header and (got == planes).all()
    assert scene_data.unpack_hdr(scene_data.pack_hdr(data)) == data


def test_stored_scenes_decode_to_their_digests():
    for scene in sorted(os.listdir(scene_data.STORE)):
        if not os.path.isfile(os.path.join(scene_data.STORE, scene, "SHA256SUMS")):
            continue
        stored = sorted(f for f in os.listdir(os.path.join(scene_data.STORE, scene)) if f.endswith(".xz"))
        sums = scene_data._sums(scene)
        assert sorted(n + (".rgbe.xz" if n.endswith(".hdr") else ".xz") for n in sums) == stored, scene
        for name, digest in sums.items():
            assert hashlib.sha256(scene_data.read_stored(scene, name)).hexdigest() == digest, "%s/%s" % (scene, name)
