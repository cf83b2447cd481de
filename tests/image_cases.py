"""Cases of the image-sequence reader (co_fusion_amd/host/ImageIO.cpp, csrc/image_decode.hip), shared by the CPU and the GPU suite and
by the generator of tests/golden/image_seq (make_image_seq_golden.py).

PNG: the files are written by co_fusion_amd.images.png_bytes and were decoded by PIL when the fixtures were generated -- the committed
.npy is PIL's answer, an independent decoder that also vouches for the writer.
OpenEXR: no independent decoder exists where the fixtures were made (no OpenEXR, OpenCV or imageio), so the expected array is the
array the writer was given, and exr_decode_numpy below restates the decoder in numpy from the "OpenEXR File Layout" document
(magic, version, attributes, offset table, blocks; ZIP: zlib, then t[i] = t[i-1] + d[i] - 128, then the two halves interleaved) --
written from that document, not from the C++."""
import os
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "image_seq")

ROLE_COLOR, ROLE_DEPTH, ROLE_MASK = 0, 1, 2


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _smooth(rng, H, W, C, hi=255):
    """a ramp plus a little noise: every PNG filter type leaves different bytes"""
    y, x = np.mgrid[0:H, 0:W]
    base = (x * 3 + y * 5)[..., None] + np.arange(C) * 40
    return ((base + rng.integers(0, 6, (H, W, C))) % (hi + 1))


def _png_image(kind, W, H, rng):
    if kind == "rgb":
        return _smooth(rng, H, W, 3).astype(np.uint8), None
    if kind == "rgba":
        return _smooth(rng, H, W, 4).astype(np.uint8), None
    if kind in ("grey", "mask"):
        return _smooth(rng, H, W, 1)[..., 0].astype(np.uint8), None
    if kind == "pal":
        pal = rng.integers(0, 256, (7, 3)).astype(np.uint8)
        return (_smooth(rng, H, W, 1)[..., 0] % 7).astype(np.uint8), pal
    assert kind == "depth"
    d = _smooth(rng, H, W, 1, hi=65535)[..., 0] * 97 % 65536
    d = d.astype(np.uint16)
    d.reshape(-1)[:5] = [0, 1, 255, 256, 65535][:min(5, W * H)]
    return d, None


# name -> (kind, W, H, filters, idat_chunks)
PNG_CASES = {}
for _k in ("rgb", "rgba", "grey", "pal", "depth", "mask"):
    PNG_CASES[f"{_k}_1x1"] = (_k, 1, 1, (0,), 1)
    PNG_CASES[f"{_k}_13x7_mixed"] = (_k, 13, 7, (4, 3, 2, 1, 0), 1)
    PNG_CASES[f"{_k}_104x72_idat5"] = (_k, 104, 72, (1, 4, 0, 3, 2), 5)
for _f in range(5):
    PNG_CASES[f"rgb_13x7_f{_f}"] = ("rgb", 13, 7, (_f,), 1)
    PNG_CASES[f"depth_13x7_f{_f}"] = ("depth", 13, 7, (_f,), 1)


def png_role(name):
    kind = PNG_CASES[name][0]
    return ROLE_DEPTH if kind == "depth" else (ROLE_MASK if kind == "mask" else ROLE_COLOR)


def png_make(name):
    """(file bytes, the image the writer was given, palette or None)"""
    from co_fusion_amd import images
    kind, W, H, filters, idat = PNG_CASES[name]
    img, pal = _png_image(kind, W, H, _rng(name))
    return images.png_bytes(img, palette=pal, filters=filters, idat_chunks=idat), img, pal


def _special_half():
    # zero, minus zero, the smallest and largest subnormal, the smallest normal, one, the largest finite, both infinities
    return np.array([0x0000, 0x8000, 0x0001, 0x03ff, 0x0400, 0x3c00, 0x7bff, 0x7c00, 0xfc00, 0x8001], np.uint16).view(np.float16)


def _exr_plane(rng, H, W, dtype, noise):
    if noise:
        bits = rng.integers(0, 1 << 16, (H, W)).astype(np.uint16)
        if dtype == np.float16:
            bits[(bits & 0x7c00) == 0x7c00] &= 0x3fff   # no NaN: its payload is no part of what is promised here
            return bits.view(np.float16)
        b32 = (rng.integers(0, 1 << 32, (H, W), dtype=np.uint64)).astype(np.uint32)
        b32[(b32 & 0x7f800000) == 0x7f800000] &= 0x3fffffff
        return b32.view(np.float32)
    y, x = np.mgrid[0:H, 0:W]
    a = (0.5 + x * 0.01 + y * 0.02).astype(dtype)
    if dtype == np.float16 and a.size >= 10:
        a.reshape(-1)[:10] = _special_half()
    return a


# name -> (W, H, dtype, channel names, compression, noise rows: None / "all" / "head")
EXR_NONE, EXR_ZIPS, EXR_ZIP = 0, 2, 3
EXR_CASES = {
    "none_f32_z_13x7": (13, 7, np.float32, ("Z",), EXR_NONE, None),
    "none_half_bgr_13x7": (13, 7, np.float16, ("B", "G", "R"), EXR_NONE, None),
    "zips_half_y_13x7": (13, 7, np.float16, ("Y",), EXR_ZIPS, None),
    "zips_f32_bgr_13x7": (13, 7, np.float32, ("B", "G", "R"), EXR_ZIPS, None),
    "zip_half_bgr_40x37": (40, 37, np.float16, ("B", "G", "R"), EXR_ZIP, None),
    "zip_f32_bgr_40x37": (40, 37, np.float32, ("B", "G", "R"), EXR_ZIP, None),
    "zip_half_z_13x37": (13, 37, np.float16, ("Z",), EXR_ZIP, None),
    "zip_f32_z_640x16": (640, 16, np.float32, ("Z",), EXR_ZIP, None),          # one 40 KB block: ten steps of the scan, nine carries
    "zip_noise_f32_z_40x37": (40, 37, np.float32, ("Z",), EXR_ZIP, "all"),      # deflate shrinks nothing: every block stored raw
    "zip_mixed_half_bgr_40x37": (40, 37, np.float16, ("B", "G", "R"), EXR_ZIP, "head"),   # block 0 raw, blocks 1 and 2 compressed
}


def exr_make(name):
    """(file bytes, the depth plane the reader must deliver)"""
    from co_fusion_amd import images
    W, H, dtype, names, comp, noise = EXR_CASES[name]
    rng = _rng(name)
    chans = {}
    for n in names:
        p = _exr_plane(rng, H, W, dtype, noise == "all")
        if noise == "head":
            p = p.copy()
            p[:16] = _exr_plane(rng, 16, W, dtype, True)
        chans[n] = p
    want = chans["B"] if len(names) > 1 else chans[names[0]]
    return images.exr_bytes(chans, compression=comp), want.astype(np.float32)


def golden(name):
    """(file bytes, expected array) of a committed fixture"""
    ext = ".exr" if name in EXR_CASES else ".png"
    with open(os.path.join(GOLDEN, name + ext), "rb") as f:
        data = f.read()
    return data, np.load(os.path.join(GOLDEN, name + ".npy"))


def rgba_of(rgb, flip=False):
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = rgb[..., ::-1] if flip else rgb
    return out


def exr_blocks_numpy(data):
    """the offset table's view of a file: [(first line, stored size, expected size)] (header parsed as exr_decode_numpy does)"""
    return _exr_parse(data)[4]


def _exr_parse(data):
    magic, version = struct.unpack_from("<II", data, 0)
    assert magic == 20000630 and version == 2
    pos, attrs = 8, {}
    while data[pos] != 0:
        e = data.index(b"\0", pos); name = data[pos:e].decode(); pos = e + 1
        e = data.index(b"\0", pos); pos = e + 1
        size, = struct.unpack_from("<i", data, pos); pos += 4
        attrs[name] = data[pos:pos + size]; pos += size
    pos += 1
    chans, p, cl = [], 0, attrs["channels"]
    while cl[p] != 0:
        e = cl.index(b"\0", p)
        ptype, = struct.unpack_from("<i", cl, e + 1)
        chans.append((cl[p:e].decode(), {1: np.dtype("<f2"), 2: np.dtype("<f4")}[ptype]))
        p = e + 17
    x0, y0, x1, y1 = struct.unpack("<iiii", attrs["dataWindow"])
    W, H = x1 - x0 + 1, y1 - y0 + 1
    comp = attrs["compression"][0]
    lpb = 16 if comp == 3 else 1
    nb = -(-H // lpb)
    offsets = struct.unpack_from("<%dQ" % nb, data, pos)
    line_bytes = sum(W * t.itemsize for _, t in chans)
    blocks = []
    for i, o in enumerate(offsets):
        y, size = struct.unpack_from("<ii", data, o)
        lines = min(lpb, H - i * lpb)
        assert y == y0 + i * lpb
        blocks.append((i * lpb, size, lines * line_bytes, o + 8))
    return W, H, chans, line_bytes, blocks


def exr_decode_numpy(data):
    """depth f32 [H, W] of a single-part scanline file: the only channel, or B where there are several"""
    W, H, chans, line_bytes, blocks = _exr_parse(data)
    pick = 0 if len(chans) == 1 else [n for n, _ in chans].index("B")
    out = np.zeros((H, W), np.float32)
    for first, size, want, at in blocks:
        payload = data[at:at + size]
        if size < want:
            d = np.frombuffer(zlib.decompress(payload), np.uint8).astype(np.int64)
            assert d.size == want
            t = (np.cumsum(d) - 128 * np.arange(want)) % 256
            half = (want + 1) // 2
            pix = np.empty(want, np.uint8)
            pix[0::2] = t[:half]
            pix[1::2] = t[half:]
        else:
            assert size == want
            pix = np.frombuffer(payload, np.uint8)
        for l in range(want // line_bytes):
            off = l * line_bytes
            for c, (_, t) in enumerate(chans):
                if c == pick:
                    out[first + l] = np.frombuffer(pix[off:off + W * t.itemsize].tobytes(), t).astype(np.float32)
                off += W * t.itemsize
    return out
