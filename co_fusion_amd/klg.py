"""ctypes view of the .klg RGB-D log reader / writer (co_fusion_amd/host/KlgIO.cpp; format of the reference's
GUI/Tools/KlgLogReader.cpp:22-87).  Host-only code: works without a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _libmod


class KlgError(RuntimeError):
    pass


def _host():
    return _libmod.load_host()


class KlgReader:
    def __init__(self, path, width, height, flip_colors=False):
        self.lib = _host()
        self.h = C.c_void_p()
        n = C.c_int()
        if self.lib.cofusion_klg_open(str(path).encode(), width, height, int(flip_colors), C.byref(self.h), C.byref(n)) != 0:
            raise KlgError(self.lib.cofusion_last_error().decode())
        self.num_frames, self.width, self.height = n.value, width, height

    def __iter__(self):
        return self

    def __next__(self):
        depth = np.empty((self.height, self.width), np.float32)
        rgb = np.empty((self.height, self.width, 3), np.uint8)
        ts = C.c_int64()
        rc = self.lib.cofusion_klg_next(self.h, C.byref(ts), depth.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p))
        if rc == 1:
            raise StopIteration
        if rc != 0:
            raise KlgError(self.lib.cofusion_last_error().decode())
        return ts.value, depth, rgb

    def close(self):
        if self.h:
            self.lib.cofusion_klg_close(self.h)
            self.h = None

    def __del__(self):
        self.close()


class KlgWriter:
    def __init__(self, path, width, height, compress_depth=True):
        self.lib = _host()
        self.h = C.c_void_p()
        if self.lib.cofusion_klg_create(str(path).encode(), width, height, int(compress_depth), C.byref(self.h)) != 0:
            raise KlgError(self.lib.cofusion_last_error().decode())
        self.width, self.height = width, height

    def write(self, timestamp, depth_m, rgb):
        d = np.ascontiguousarray(depth_m, np.float32)
        c = np.ascontiguousarray(rgb, np.uint8)
        assert d.shape == (self.height, self.width) and c.shape == (self.height, self.width, 3)
        if self.lib.cofusion_klg_write(self.h, C.c_int64(int(timestamp)), d.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)) != 0:
            raise KlgError(self.lib.cofusion_last_error().decode())

    def close(self):
        if self.h:
            self.lib.cofusion_klg_finish(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()


# ---- the log player (host/KlgPlayer.h, csrc/frame_decode.hip) ----
COLOR_NONE, COLOR_JPEG, COLOR_RAW, COLOR_DECODED = 0, 1, 2, 3   # CF_FRAME_COLOR_*


class JpegComp(C.Structure):
    _fields_ = [("h", C.c_int32), ("v", C.c_int32), ("bw", C.c_int32), ("bh", C.c_int32), ("first", C.c_int32)]


class JpegHeader(C.Structure):
    """cf_jpeg_header: what the JPEG front end leaves beside the quantised coefficients"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("hmax", C.c_int32), ("vmax", C.c_int32),
                ("total_blocks", C.c_int32), ("comp", JpegComp * 3), ("qt", (C.c_uint8 * 64) * 3)]


class FrameDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("color_kind", C.c_int32), ("flip_colors", C.c_int32)]


class FrameSlot(C.Structure):
    _fields_ = [("header", C.POINTER(JpegHeader)), ("coef", C.POINTER(C.c_int16)), ("coef_blocks", C.c_uint64),
                ("depth", C.POINTER(C.c_uint16)), ("rgb", C.POINTER(C.c_uint8))]


def jpeg_max_blocks(width, height):
    """CF_JPEG_MAX_BLOCKS: the blocks a frame of this size can have, whatever its sampling factors"""
    return 48 * ((width + 31) // 32) * ((height + 31) // 32)


def jpeg_header(width, height, sampling, qt=None):
    """a cf_jpeg_header for a frame of this size: sampling = [(h, v)] per component, qt = [64 values] per component (default 1)"""
    hd = JpegHeader()
    hd.width, hd.height, hd.ncomp = width, height, len(sampling)
    hd.hmax, hd.vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mx, my = -(-width // (8 * hd.hmax)), -(-height // (8 * hd.vmax))
    first = 0
    for c, (h, v) in enumerate(sampling):
        hd.comp[c] = JpegComp(h, v, mx * h, my * v, first)
        first += mx * h * my * v
        for i in range(64):
            hd.qt[c][i] = 1 if qt is None else int(qt[c][i])
    hd.total_blocks = first
    return hd


def jpeg_front(stream, width, height):
    """the JPEG front end (cofusion_jpeg_front): (status, header, coef int16 [total_blocks, 64]); status 0 = decoded, 1 = refused
    (the device path does not promise to reproduce this stream); a decoding error raises"""
    lib = _host()
    hd = JpegHeader()
    coef = np.zeros((jpeg_max_blocks(width, height), 64), np.int16)
    data = bytes(stream)
    rc = lib.cofusion_jpeg_front(data, C.c_uint64(len(data)), width, height, C.byref(hd), coef.ctypes.data_as(C.c_void_p), C.c_uint64(coef.shape[0]))
    if rc < 0:
        raise KlgError(lib.cofusion_last_error().decode())
    return rc, hd, coef[:hd.total_blocks] if rc == 0 else coef[:0]


def jpeg_finish_host(header, coef):
    """the host back end (cofusion_jpeg_finish_host): rgb u8 [H, W, 3] in libjpeg's channel order"""
    lib = _host()
    c = np.ascontiguousarray(coef, np.int16)
    assert c.size == header.total_blocks * 64
    rgb = np.empty((header.height, header.width, 3), np.uint8)
    if lib.cofusion_jpeg_finish_host(C.byref(header), c.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p)) != 0:
        raise KlgError(lib.cofusion_last_error().decode())
    return rgb


class KlgPrefetcher:
    """The host half of the player alone (no GPU): worker threads read the log ahead into slots from malloc.  Iterating yields
    (timestamp, depth_mm u16 [H, W], color_kind, colour) in log order, where colour is (header, coef) for COLOR_JPEG, the log's bytes
    [H, W, 3] for COLOR_RAW, a host-decoded JPEG in libjpeg's order for COLOR_DECODED, None for COLOR_NONE -- copies, valid for good."""

    def __init__(self, path, width, height, workers=4, slots=6):
        self.lib = _host()
        self.h = C.c_void_p()
        n = C.c_int()
        if self.lib.cofusion_klg_prefetch_open(str(path).encode(), width, height, int(workers), int(slots), C.byref(self.h), C.byref(n)) != 0:
            raise KlgError(self.lib.cofusion_last_error().decode())
        self.num_frames, self.width, self.height = n.value, width, height

    def __iter__(self):
        return self

    def __next__(self):
        ts, kind, s = C.c_int64(), C.c_int(), FrameSlot()
        rc = self.lib.cofusion_klg_prefetch_next(self.h, C.byref(ts), C.byref(kind), C.byref(s))
        if rc == 1:
            raise StopIteration
        if rc != 0:
            raise KlgError(self.lib.cofusion_last_error().decode())
        H, W = self.height, self.width
        depth = np.ctypeslib.as_array(s.depth, shape=(H, W)).copy()
        colour = None
        if kind.value == COLOR_JPEG:
            hd = JpegHeader.from_buffer_copy(s.header.contents)
            colour = (hd, np.ctypeslib.as_array(s.coef, shape=(hd.total_blocks, 64)).copy())
        elif kind.value in (COLOR_RAW, COLOR_DECODED):
            colour = np.ctypeslib.as_array(s.rgb, shape=(H, W, 3)).copy()
        return ts.value, depth, kind.value, colour

    def rewind(self):
        self.lib.cofusion_klg_prefetch_rewind(self.h)

    def close(self):
        if self.h:
            self.lib.cofusion_klg_prefetch_close(self.h)
            self.h = None

    def __del__(self):
        self.close()


class KlgPlayer:
    """Plays a log into a facade.CoFusion at tracker speed (cofusion_klg_player_*): `workers` host threads inflate and entropy-decode
    ahead, the device finishes the frames.  Iterating yields (timestamp, depth_ptr, rgba_ptr): device addresses of the frame (depth f32
    [H, W] metres, rgba u8 [H, W, 4]), intact until the next step; process() plays one frame into the instance (False at the end of
    the log), play(n) up to n frames (all by default) and returns how many.  Close the player before the instance."""

    def __init__(self, cf, path, flip_colors=False, workers=4):
        self.lib = _host()
        self.cf = cf
        self.h = C.c_void_p()
        n = C.c_int()
        if self.lib.cofusion_klg_player_open(cf.h, str(path).encode(), int(flip_colors), int(workers), C.byref(self.h), C.byref(n)) != 0:
            raise KlgError(self.lib.cofusion_last_error().decode())
        self.num_frames = n.value

    def set_limits(self, reference_compatible=False, frame_limit=-1):
        self.lib.cofusion_klg_player_set_limits(self.h, int(reference_compatible), int(frame_limit))

    def __iter__(self):
        return self

    def __next__(self):
        ts, d, c = C.c_int64(), C.c_void_p(), C.c_void_p()
        rc = self.lib.cofusion_klg_player_next(self.h, C.byref(ts), C.byref(d), C.byref(c))
        if rc == 1:
            raise StopIteration
        if rc != 0:
            raise KlgError(self.lib.cofusion_last_error().decode())
        return ts.value, d.value, c.value

    def process(self):
        rc = self.lib.cofusion_klg_player_process(self.h)
        if rc not in (0, 1):
            raise KlgError(self.lib.cofusion_last_error().decode())
        return rc == 0

    def play(self, n=-1):
        done = 0
        while (n < 0 or done < n) and self.process():
            done += 1
        return done

    def rewind(self):
        if self.lib.cofusion_klg_player_rewind(self.h) != 0:
            raise KlgError(self.lib.cofusion_last_error().decode())

    def close(self):
        if self.h:
            self.lib.cofusion_klg_player_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()
