"""Image-sequence datasets (co_fusion_amd/host/ImageIO.cpp, csrc/image_decode.hip): directories of colour
.jpg/.png/.ppm, depth .exr/.png and mask .png/.pgm files as the reference's GUI/Tools/ImageLogReader.cpp reads them.

  decode_png / decode_exr / decode_ppm   the host parsers alone (no GPU)
  png_finish_host / exr_finish_host       the host statement of the device's finishing kernels
  ImageSequenceReader                     the serial reader: host buffers, everything on the calling thread
  ImageSequencePlayer / ImagePrefetcher   worker threads decode ahead, the device finishes the frames / the host half alone
  ImageDesc / ImageSlot / ExrBlock        the C-ABI structures of cf_frame_decoder_submit_images (api.FrameDecoder)
  png_bytes / exr_bytes / ppm_bytes, write_png / write_exr / write_ppm   writers for tests and tools (numpy + zlib)
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib

import numpy as np

from . import lib as _libmod

ROLE_COLOR, ROLE_DEPTH, ROLE_MASK = 0, 1, 2
IMAGE_NONE, IMAGE_PNG, IMAGE_EXR, IMAGE_JPEG, IMAGE_RAW = 0, 1, 2, 3, 4   # CF_IMAGE_*
EXR_NONE, EXR_ZIPS, EXR_ZIP = 0, 2, 3
DEFAULT_DEPTH_SCALE = float(np.float32(0.0006))   # ImageLogReader.cpp:260


class ImageError(RuntimeError):
    pass


def _host():
    return _libmod.load_host()


def _err(lib, name=None):
    msg = lib.cofusion_last_error().decode()
    return ImageError(f"{name}: {msg}" if name else msg)


# ---- C structures ----
class ExrBlock(C.Structure):
    _fields_ = [("offset", C.c_uint32), ("bytes", C.c_uint32), ("stored_raw", C.c_uint32), ("first_line", C.c_uint32)]


EXR_BLOCK = np.dtype([("offset", "<u4"), ("bytes", "<u4"), ("stored_raw", "<u4"), ("first_line", "<u4")])


class ImageDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("color_kind", C.c_int32), ("depth_kind", C.c_int32), ("mask_kind", C.c_int32),
                ("flip_colors", C.c_int32), ("png_color_type", C.c_int32), ("png_palette_entries", C.c_int32), ("depth_scale", C.c_float),
                ("exr_blocks", C.c_int32), ("exr_lines_per_block", C.c_int32), ("exr_line_bytes", C.c_int32), ("exr_chan_offset", C.c_int32),
                ("exr_chan_half", C.c_int32)]


class ImageSlot(C.Structure):
    _fields_ = [("color", C.POINTER(C.c_uint8)), ("color_bytes", C.c_uint64), ("depth", C.POINTER(C.c_uint8)), ("depth_bytes", C.c_uint64),
                ("mask", C.POINTER(C.c_uint8)), ("mask_bytes", C.c_uint64), ("palette", C.POINTER(C.c_uint8)),
                ("blocks", C.POINTER(ExrBlock)), ("max_blocks", C.c_uint32)]


class PngInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32), ("color_type", C.c_int32), ("bpp", C.c_int32),
                ("palette_entries", C.c_int32)]


class ExrInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("compression", C.c_int32), ("lines_per_block", C.c_int32), ("blocks", C.c_int32),
                ("line_bytes", C.c_int32), ("chan_offset", C.c_int32), ("chan_half", C.c_int32)]


class ImageOptions(C.Structure):
    _fields_ = [("color_dir", C.c_char_p), ("depth_dir", C.c_char_p), ("mask_dir", C.c_char_p), ("color_prefix", C.c_char_p),
                ("depth_prefix", C.c_char_p), ("mask_prefix", C.c_char_p), ("index_width", C.c_int32), ("start_index", C.c_int32),
                ("flip_colors", C.c_int32), ("depth_scale", C.c_float), ("rate_hz", C.c_float), ("max_masks", C.c_int32)]


class ImageInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("num_frames", C.c_int32), ("start_index", C.c_int32), ("has_masks", C.c_int32),
                ("max_masks", C.c_int32)]


def _png_dims(data):
    if len(data) < 24:
        return 1, 1
    w, h = struct.unpack(">II", bytes(data[16:24]))
    return (w, h) if 0 < w <= 16384 and 0 < h <= 16384 else (1, 1)


# ---- the parsers ----
def decode_png(data, role, name=None):
    """bytes of a PNG -> (PngInfo, scanlines u8 [height, 1 + bpp * width] UNFILTERED in file layout, palette u8 [entries, 3] or None)"""
    lib = _host()
    data = bytes(data)
    w, h = _png_dims(data)
    scan = np.zeros((1 + 4 * w) * h + 16, np.uint8)
    pal = np.zeros(768, np.uint8)
    info = PngInfo()
    if lib.cofusion_png_decode(data, C.c_uint64(len(data)), int(role), C.byref(info), scan.ctypes.data_as(C.c_void_p), C.c_uint64(scan.size - 16),
                               pal.ctypes.data_as(C.c_void_p)) != 0:
        raise _err(lib, name)
    stride = 1 + info.bpp * info.width
    return info, scan[:stride * info.height].reshape(info.height, stride).copy(), (pal[:3 * info.palette_entries].reshape(-1, 3).copy() if info.color_type == 3 else None)


def png_finish_host(info, scan, palette=None, role=ROLE_COLOR, flip_colors=False, depth_scale=DEFAULT_DEPTH_SCALE):
    """the device's png_finish_kernel on the host: rgba u8 [H, W, 4] / depth f32 [H, W] / mask u8 [H, W]"""
    lib = _host()
    H, W = info.height, info.width
    out = np.empty((H, W, 4), np.uint8) if role == ROLE_COLOR else np.empty((H, W), np.float32 if role == ROLE_DEPTH else np.uint8)
    pal = np.zeros(768, np.uint8)
    if palette is not None:
        pal[:palette.size] = np.asarray(palette, np.uint8).reshape(-1)
    s = np.ascontiguousarray(scan, np.uint8)
    assert s.size == (1 + info.bpp * W) * H
    if lib.cofusion_png_finish_host(C.byref(info), int(role), s.ctypes.data_as(C.c_void_p), pal.ctypes.data_as(C.c_void_p), int(bool(flip_colors)),
                                    C.c_float(depth_scale), out.ctypes.data_as(C.c_void_p)) != 0:
        raise _err(lib)
    return out


def decode_exr(data, name=None):
    """bytes of an OpenEXR file -> (ExrInfo, raw u8 [line_bytes * height]: the inflated blocks at their place, blocks EXR_BLOCK [n])"""
    lib = _host()
    data = bytes(data)
    cap = max(len(data) * 64, 1 << 16)   # deflate expands at most ~1030 : 1; the parser refuses what does not fit
    cap = min(cap, 1 << 28)
    raw = np.zeros(cap + 16, np.uint8)
    blocks = np.zeros(16384, EXR_BLOCK)
    info = ExrInfo()
    if lib.cofusion_exr_decode(data, C.c_uint64(len(data)), C.byref(info), raw.ctypes.data_as(C.c_void_p), C.c_uint64(cap),
                               blocks.ctypes.data_as(C.c_void_p), C.c_uint64(blocks.size)) != 0:
        raise _err(lib, name)
    return info, raw[:info.line_bytes * info.height].copy(), blocks[:info.blocks].copy()


def exr_finish_host(info, raw, blocks):
    """the device's exr_depth_kernel on the host: depth f32 [H, W]"""
    lib = _host()
    out = np.empty((info.height, info.width), np.float32)
    r = np.ascontiguousarray(raw, np.uint8)
    b = np.ascontiguousarray(blocks, EXR_BLOCK)
    assert r.size >= info.line_bytes * info.height and b.size == info.blocks
    if lib.cofusion_exr_finish_host(C.byref(info), r.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0:
        raise _err(lib)
    return out


def decode_ppm(data, name=None):
    """bytes of a binary PPM (P6, maxval <= 255) -> u8 [height, width, 3]"""
    lib = _host()
    data = bytes(data)
    w, h, off = C.c_int(), C.c_int(), C.c_uint64()
    if lib.cofusion_ppm_decode(data, C.c_uint64(len(data)), C.byref(w), C.byref(h), C.byref(off)) != 0:
        raise _err(lib, name)
    return np.frombuffer(data, np.uint8, w.value * h.value * 3, off.value).reshape(h.value, w.value, 3).copy()


def read_depth_png(path, depth_scale=DEFAULT_DEPTH_SCALE):
    with open(path, "rb") as f:
        info, scan, _ = decode_png(f.read(), ROLE_DEPTH, path)
    return png_finish_host(info, scan, None, ROLE_DEPTH, depth_scale=depth_scale)


def read_mask_png(path):
    with open(path, "rb") as f:
        info, scan, _ = decode_png(f.read(), ROLE_MASK, path)
    return scan[:, 1:].copy()


class ImageSequenceReader:
    """The serial reader (cofusion_image_reader_*), the counterpart of klg.KlgReader for a directory dataset.  Iterating yields
    (timestamp, depth f32 [H, W], rgb u8 [H, W, 3], mask u8 [H, W] or None)."""

    def __init__(self, color_dir, depth_dir="", mask_dir="", color_prefix="", depth_prefix="", mask_prefix="", index_width=4, start_index=-1,
                 flip_colors=False, depth_scale=0.0, rate_hz=0.0, max_masks=0):
        self.lib = _host()
        self.h = C.c_void_p()
        self._opt = _options(color_dir, depth_dir, mask_dir, color_prefix, depth_prefix, mask_prefix, index_width, start_index, flip_colors,
                             depth_scale, rate_hz, max_masks)
        info = ImageInfo()
        if self.lib.cofusion_image_reader_open(C.byref(self._opt), C.byref(self.h), C.byref(info)) != 0:
            self.h = None
            raise _err(self.lib)
        self.width, self.height, self.num_frames = info.width, info.height, info.num_frames
        self.start_index, self.has_masks, self.max_masks = info.start_index, bool(info.has_masks), info.max_masks

    def __iter__(self):
        return self

    def __next__(self):
        H, W = self.height, self.width
        depth, rgb, mask = np.empty((H, W), np.float32), np.empty((H, W, 3), np.uint8), np.empty((H, W), np.uint8)
        ts, has = C.c_int64(), C.c_int()
        rc = self.lib.cofusion_image_reader_next(self.h, C.byref(ts), depth.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p),
                                                 mask.ctypes.data_as(C.c_void_p), C.byref(has))
        if rc == 1:
            raise StopIteration
        if rc != 0:
            raise _err(self.lib)
        return ts.value, depth, rgb, (mask if has.value else None)

    def rewind(self):
        self.lib.cofusion_image_reader_rewind(self.h)

    def close(self):
        if self.h:
            self.lib.cofusion_image_reader_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()


def _options(color_dir, depth_dir, mask_dir, color_prefix, depth_prefix, mask_prefix, index_width, start_index, flip_colors, depth_scale, rate_hz,
             max_masks=0):
    enc = lambda s: str(s).encode()
    return ImageOptions(enc(color_dir), enc(depth_dir), enc(mask_dir), enc(color_prefix), enc(depth_prefix), enc(mask_prefix),
                        int(index_width), int(start_index), int(bool(flip_colors)), float(depth_scale), float(rate_hz), int(max_masks))


class ImagePrefetcher:
    """The host half of the player alone (no GPU): worker threads read the set ahead into slots from malloc; iterating yields
    (timestamp, depth f32 [H, W], rgba u8 [H, W, 4], mask u8 [H, W] or None) in order, each frame finished by the host statements of
    the device's kernels -- what the player's device frames must equal."""

    def __init__(self, color_dir, depth_dir="", mask_dir="", color_prefix="", depth_prefix="", mask_prefix="", index_width=4, start_index=-1,
                 flip_colors=False, depth_scale=0.0, rate_hz=0.0, max_masks=0, workers=4, slots=6):
        self.lib = _host()
        self.h = C.c_void_p()
        self._opt = _options(color_dir, depth_dir, mask_dir, color_prefix, depth_prefix, mask_prefix, index_width, start_index, flip_colors,
                             depth_scale, rate_hz, max_masks)
        info = ImageInfo()
        if self.lib.cofusion_image_prefetch_open(C.byref(self._opt), int(workers), int(slots), C.byref(self.h), C.byref(info)) != 0:
            self.h = None
            raise _err(self.lib)
        self.width, self.height, self.num_frames, self.max_masks = info.width, info.height, info.num_frames, info.max_masks

    def __iter__(self):
        return self

    def __next__(self):
        H, W = self.height, self.width
        depth, rgba, mask = np.empty((H, W), np.float32), np.empty((H, W, 4), np.uint8), np.empty((H, W), np.uint8)
        ts, has = C.c_int64(), C.c_int()
        rc = self.lib.cofusion_image_prefetch_next(self.h, C.byref(ts), depth.ctypes.data_as(C.c_void_p), rgba.ctypes.data_as(C.c_void_p),
                                                   mask.ctypes.data_as(C.c_void_p), C.byref(has))
        if rc == 1:
            raise StopIteration
        if rc != 0:
            raise _err(self.lib)
        return ts.value, depth, rgba, (mask if has.value else None)

    def rewind(self):
        self.lib.cofusion_image_prefetch_rewind(self.h)

    def close(self):
        if self.h:
            self.lib.cofusion_image_prefetch_close(self.h)
            self.h = None

    def __del__(self):
        self.close()


class ImageSequencePlayer:
    """Plays an image directory into a facade.CoFusion at tracker speed (cofusion_image_player_*): `workers` host threads read, inflate
    and unfilter ahead, the device finishes the frames.  Iterating yields (timestamp, depth_ptr, rgba_ptr, mask_ptr): device addresses
    of the frame (depth f32 [H, W], rgba u8 [H, W, 4], mask u8 [H, W] or None), intact until the next step; process() plays one frame
    into the instance (False at the end), play(n) up to n frames and returns how many.  Close the player before the instance."""

    def __init__(self, cf, color_dir, depth_dir="", mask_dir="", color_prefix="", depth_prefix="", mask_prefix="", index_width=4, start_index=-1,
                 flip_colors=False, depth_scale=0.0, rate_hz=0.0, max_masks=0, workers=4):
        self.lib = _host()
        self.cf = cf
        self.h = C.c_void_p()
        self._opt = _options(color_dir, depth_dir, mask_dir, color_prefix, depth_prefix, mask_prefix, index_width, start_index, flip_colors,
                             depth_scale, rate_hz, max_masks)
        info = ImageInfo()
        if self.lib.cofusion_image_player_open(cf.h, C.byref(self._opt), int(workers), C.byref(self.h), C.byref(info)) != 0:
            self.h = None
            raise _err(self.lib)
        self.width, self.height, self.num_frames = info.width, info.height, info.num_frames
        self.has_masks, self.max_masks = bool(info.has_masks), info.max_masks

    def set_limits(self, frame_limit=-1):
        self.lib.cofusion_image_player_set_limits(self.h, int(frame_limit))

    def __iter__(self):
        return self

    def __next__(self):
        ts, d, c, m = C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.cofusion_image_player_next(self.h, C.byref(ts), C.byref(d), C.byref(c), C.byref(m))
        if rc == 1:
            raise StopIteration
        if rc != 0:
            raise _err(self.lib)
        return ts.value, d.value, c.value, m.value

    def process(self):
        rc = self.lib.cofusion_image_player_process(self.h)
        if rc not in (0, 1):
            raise _err(self.lib)
        return rc == 0

    def play(self, n=-1):
        done = 0
        while (n < 0 or done < n) and self.process():
            done += 1
        return done

    def rewind(self):
        if self.lib.cofusion_image_player_rewind(self.h) != 0:
            raise _err(self.lib)

    def times(self):
        """seconds the workers spent so far (all workers summed): dict(read, inflate -- zlib's inflate() alone --, unfilter, parse)"""
        r, i, u, p = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        self.lib.cofusion_image_player_times(self.h, C.byref(r), C.byref(i), C.byref(u), C.byref(p))
        return dict(read=r.value, inflate=i.value, unfilter=u.value, parse=p.value)

    def close(self):
        if self.h:
            self.lib.cofusion_image_player_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()


# ---- writers (tests and tools) ----
def png_chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def png_filter_rows(rows, bpp, filters):
    """rows u8 [H, row_bytes] -> the filtered scanlines u8 [H, 1 + row_bytes], row y with filter type filters[y % len(filters)]"""
    rows = np.ascontiguousarray(rows, np.uint8)
    H, rb = rows.shape
    out = np.zeros((H, rb + 1), np.uint8)
    zero = np.zeros(rb, np.int32)
    for y in range(H):
        f = int(filters[y % len(filters)])
        cur = rows[y].astype(np.int32)
        up = rows[y - 1].astype(np.int32) if y else zero
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        upleft = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        pred = [zero, left, up, (left + up) >> 1, _paeth(left, up, upleft)][f]
        out[y, 0] = f
        out[y, 1:] = ((cur - pred) & 255).astype(np.uint8)
    return out


def png_bytes(image, palette=None, filters=(0,), idat_chunks=1, level=6, interlace=0, extra_chunks=()):
    """A PNG of `image`: u8 [H, W] grey (or palette indices when `palette` u8 [n, 3] is given), u16 [H, W] 16-bit grey, u8 [H, W, 3] RGB,
    u8 [H, W, 4] RGBA, u16 [H, W, 3] 16-bit RGB.  filters: the filter type forced on row y is filters[y % len(filters)]; idat_chunks:
    the zlib stream is cut into so many IDAT chunks; extra_chunks: (kind, body) pairs placed before the first IDAT."""
    a = np.asarray(image)
    assert a.dtype in (np.uint8, np.uint16) and a.ndim in (2, 3)
    H, W = a.shape[:2]
    channels = 1 if a.ndim == 2 else a.shape[2]
    color_type = {1: 3 if palette is not None else 0, 3: 2, 4: 6}[channels]
    depth = 16 if a.dtype == np.uint16 else 8
    rows = (a.astype(">u2").view(np.uint8) if depth == 16 else a).reshape(H, -1)
    scan = png_filter_rows(rows, channels * depth // 8, filters)
    z = zlib.compress(scan.tobytes(), level)
    out = [PNG_SIGNATURE, png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, color_type, 0, 0, interlace))]
    if palette is not None:
        out.append(png_chunk(b"PLTE", np.asarray(palette, np.uint8).reshape(-1, 3).tobytes()))
    out += [png_chunk(k, b) for k, b in extra_chunks]
    n = max(1, int(idat_chunks))
    cuts = [len(z) * i // n for i in range(n + 1)]
    out += [png_chunk(b"IDAT", z[cuts[i]:cuts[i + 1]]) for i in range(n)]
    out.append(png_chunk(b"IEND"))
    return b"".join(out)


def _exr_attr(name, kind, body):
    return name.encode() + b"\0" + kind.encode() + b"\0" + struct.pack("<i", len(body)) + body


def exr_zip_forward(pixels):
    """OpenEXR's ZIP pre-processing of a block's pixel bytes: even bytes to the first half, odd bytes to the second, then every byte
    replaced by its difference to the one before plus 128 (modulo 256)"""
    p = np.frombuffer(pixels, np.uint8)
    t = np.concatenate([p[0::2], p[1::2]]).astype(np.int32)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128) & 255
    return d.astype(np.uint8).tobytes()


def exr_bytes(channels, compression=EXR_ZIP, level=6, store_raw=(), version_flags=0, compression_code=None, line_order=0, extra_attrs=(),
              data_window=None):
    """A single-part scanline OpenEXR file.  channels: {name: f16 or f32 array [H, W]} (stored in alphabetical order, as the format
    wants); compression EXR_NONE / EXR_ZIPS / EXR_ZIP.  A block deflate does not shrink is stored raw, as the format says; store_raw
    names further block indices to store raw.  The remaining arguments write headers the reader must refuse."""
    names = sorted(channels)
    arrs = [np.ascontiguousarray(channels[n]) for n in names]
    H, W = arrs[0].shape
    for a in arrs:
        assert a.shape == (H, W) and a.dtype in (np.float16, np.float32)
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", 1 if a.dtype == np.float16 else 2, 0, 1, 1) for n, a in zip(names, arrs)) + b"\0"
    box = struct.pack("<iiii", 0, 0, W - 1, H - 1)
    head = struct.pack("<II", 20000630, 2 | version_flags)
    head += _exr_attr("channels", "chlist", chlist)
    head += _exr_attr("compression", "compression", bytes([compression if compression_code is None else compression_code]))
    head += _exr_attr("dataWindow", "box2i", box if data_window is None else struct.pack("<iiii", *data_window))
    head += _exr_attr("displayWindow", "box2i", box)
    head += _exr_attr("lineOrder", "lineOrder", bytes([line_order]))
    head += _exr_attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    head += _exr_attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0))
    head += _exr_attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
    for name, kind, body in extra_attrs:
        head += _exr_attr(name, kind, body)
    head += b"\0"
    lpb = 16 if compression == EXR_ZIP else 1
    nblocks = -(-H // lpb)
    body, offsets = [], []
    pos = len(head) + 8 * nblocks
    for i in range(nblocks):
        y0, y1 = i * lpb, min(H, (i + 1) * lpb)
        pix = b"".join(a[y].astype(a.dtype.newbyteorder("<")).tobytes() for y in range(y0, y1) for a in arrs)
        data = pix
        if compression != EXR_NONE and i not in store_raw:
            z = zlib.compress(exr_zip_forward(pix), level)
            if len(z) < len(pix):
                data = z
        offsets.append(pos)
        blk = struct.pack("<ii", y0, len(data)) + data
        body.append(blk)
        pos += len(blk)
    return head + struct.pack("<%dQ" % nblocks, *offsets) + b"".join(body)


def ppm_bytes(rgb, comment=None):
    a = np.ascontiguousarray(rgb, np.uint8)
    assert a.ndim == 3 and a.shape[2] == 3
    head = b"P6\n" + (b"# " + comment.encode() + b"\n" if comment else b"") + b"%d %d\n255\n" % (a.shape[1], a.shape[0])
    return head + a.tobytes()


def pgm_bytes(grey):
    a = np.ascontiguousarray(grey, np.uint8)
    assert a.ndim == 2
    return b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + a.tobytes()


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)


def write_png(path, image, **kw):
    _write(path, png_bytes(image, **kw))


def write_exr(path, channels, **kw):
    _write(path, exr_bytes(channels, **kw))


def write_ppm(path, rgb, **kw):
    _write(path, ppm_bytes(rgb, **kw))
