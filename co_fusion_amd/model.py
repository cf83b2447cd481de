"""Python mirror of the surfel Model (Core/Model/Model.h:117-235) over the C-ABI (per-call access for tests and tools;
the frame loop itself is the C++ facade, co_fusion_amd/host/CoFusion.cpp)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .api import Context, Odometry, _f, _p

SURFEL = 12
TIME_DELTA = 2 ** 31 // 2 - 1  # openLoop: INT_MAX / 2 (GUI/MainController.cpp:328)

class ModelPass(C.Structure):
    """cf_model_pass (include/cofusion_hip.h)"""
    _fields_ = [("model", C.c_void_p), ("pose", C.POINTER(C.c_float)), ("rgba", C.c_void_p), ("mask", C.c_void_p), ("depth_raw", C.c_void_p),
                ("depth_filtered", C.c_void_p), ("do_fuse", C.c_int), ("time", C.c_int), ("fuse_max_depth", C.c_float), ("weighting", C.c_float),
                ("mask_id", C.c_int), ("conf_threshold", C.c_float), ("fill_in", C.c_int), ("passthrough_geom", C.c_int),
                ("passthrough_rgb", C.c_int)]


class ModelPreindex(C.Structure):
    """cf_model_preindex (include/cofusion_hip.h)"""
    _fields_ = [("model", C.c_void_p), ("odom", C.c_void_p), ("time", C.c_int)]


def frame_passes(ctx: Context, items, depth_cutoff, outlier_coeff, time_delta=None):
    """cf_models_frame_passes.  items: dicts with model (a Model), pose, rgba, depth_filt, time, conf_threshold and, for do_fuse (default 1),
    mask, depth_raw, fuse_max_depth, weighting, mask_id; the images are device tensors.  fill_in (default 0) with passthrough_geom /
    passthrough_rgb: the fill-in maps and the fill ratio of the model out of the same chain"""
    n = len(items)
    arr = (ModelPass * n)()
    keep = []
    for a, it in zip(arr, items):
        pose = _f(np.asarray(it["pose"], np.float32).reshape(16))
        keep.append(pose)
        a.model = it["model"].h
        a.pose = C.cast(pose, C.POINTER(C.c_float))
        a.rgba, a.mask = _p(it["rgba"]), _p(it.get("mask"))
        a.depth_raw, a.depth_filtered = _p(it.get("depth_raw")), _p(it["depth_filt"])
        a.do_fuse = int(it.get("do_fuse", 1))
        a.time = int(it["time"])
        a.fuse_max_depth = float(it.get("fuse_max_depth", depth_cutoff))
        a.weighting = float(it.get("weighting", 1.0))
        a.mask_id = int(it.get("mask_id", 0))
        a.conf_threshold = float(it["conf_threshold"])
        a.fill_in, a.passthrough_geom, a.passthrough_rgb = int(it.get("fill_in", 0)), int(it.get("passthrough_geom", 0)), int(it.get("passthrough_rgb", 0))
    ctx._check(ctx.lib.cf_models_frame_passes(ctx.h, arr, n, C.c_float(depth_cutoff), C.c_float(outlier_coeff),
                                              int(TIME_DELTA if time_delta is None else time_delta)))


def preindex(ctx: Context, items, depth_cutoff, time_delta=None):
    """cf_models_preindex.  items: (Model, Odometry, time) triples"""
    n = len(items)
    arr = (ModelPreindex * n)()
    for a, (m, od, time) in zip(arr, items):
        a.model, a.odom, a.time = m.h, od.h, int(time)
    ctx._check(ctx.lib.cf_models_preindex(ctx.h, arr, n, C.c_float(depth_cutoff), int(TIME_DELTA if time_delta is None else time_delta)))


def set_extent_culling(ctx: Context, on=True):
    """cf_set_extent_culling: the batched passes (frame_passes, preindex) skip the texels outside the models' extents; default on"""
    ctx._check(ctx.lib.cf_set_extent_culling(ctx.h, int(bool(on))))


_BUF = {0: (np.uint32, 1), 1: (np.float32, 4), 2: (np.float32, 4), 3: (np.float32, 4), 4: (np.uint8, 4), 5: (np.float32, 4),
        6: (np.float32, 4), 7: (np.uint16, 1), 8: (np.float32, 4), 9: (np.float32, 4), 10: (np.uint8, 4),
        15: (np.uint8, 4), 16: (np.float32, 4), 17: (np.float32, 4), 18: (np.uint16, 1)}   # 15..18: the inactive prediction


def bilateral(ctx: Context, depth, max_d):
    rows, cols = depth.shape
    out = ctx.empty((rows, cols))
    ctx._check(ctx.lib.cf_bilateral(ctx.h, _p(depth), cols, rows, C.c_float(max_d), _p(out)))
    return out


def fusion_weight(ctx: Context, pose, last_pose, mult):
    ctx.lib.cf_fusion_weight.restype = C.c_float
    return float(ctx.lib.cf_fusion_weight(_f(np.asarray(pose, np.float32).reshape(16)), _f(np.asarray(last_pose, np.float32).reshape(16)),
                                          C.c_float(mult)))


class Model:
    def __init__(self, ctx: Context, max_surfels=1 << 20):
        self.ctx = ctx
        self.h = C.c_void_p()
        ctx._check(ctx.lib.cf_model_create(ctx.h, int(max_surfels), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.cf_model_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _pose(self, pose):
        return _f(np.asarray(pose, np.float32).reshape(16))

    def initialise(self, rgba, depth_raw, depth_filt, time, max_depth):
        self.ctx._check(self.ctx.lib.cf_model_initialise(self.h, _p(rgba), _p(depth_raw), _p(depth_filt), time, C.c_float(max_depth)))

    def count(self):
        c = C.c_uint32()
        self.ctx._check(self.ctx.lib.cf_model_count(self.h, C.byref(c)))
        return c.value

    def predict_indices(self, pose, time, max_depth, time_delta=TIME_DELTA):
        self.ctx._check(self.ctx.lib.cf_model_predict_indices(self.h, self._pose(pose), time, C.c_float(max_depth), time_delta))

    def index_keys(self, pose, time, max_depth, surfel_begin, surfel_end, time_delta=TIME_DELTA):
        """first half of predict_indices for the surfel range [begin, end): int64 view of the u64 z-keys, [H, W] on the device"""
        keys = torch.empty((self.ctx.height, self.ctx.width), dtype=torch.int64, device=self.ctx.device)
        self.ctx._check(self.ctx.lib.cf_model_index_keys(self.h, self._pose(pose), time, C.c_float(max_depth), time_delta,
                                                         int(surfel_begin), int(surfel_end), C.c_void_p(keys.data_ptr())))
        return keys

    def index_resolve(self, pose, keys):
        """second half: resolve a (reduced) key map into the index-map textures"""
        self.ctx._check(self.ctx.lib.cf_model_index_resolve(self.h, self._pose(pose), C.c_void_p(keys.data_ptr())))

    def combined_predict(self, pose, max_depth, conf_threshold, time, max_time, time_delta=TIME_DELTA):
        self.ctx._check(self.ctx.lib.cf_model_combined_predict(self.h, self._pose(pose), C.c_float(max_depth), C.c_float(conf_threshold),
                                                               time, max_time, time_delta))

    def predict_inactive(self, pose, max_depth, conf_threshold, max_time, time_delta):
        """the INACTIVE prediction (buffers 15..18: image, vertexConf, normalRad, time) and its covered count (inactive_covered)"""
        self.ctx._check(self.ctx.lib.cf_model_predict_inactive(self.h, self._pose(pose), C.c_float(max_depth), C.c_float(conf_threshold),
                                                               int(max_time), int(time_delta)))

    def inactive_covered(self):
        """texels of the last inactive prediction with time > 0 (waits for the stream)"""
        ptr, nbytes = self.tensor(19)
        host = np.empty(1, np.uint32)
        self.ctx._check(self.ctx.lib.cf_memcpy_d2h(self.ctx.h, host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_uint64(nbytes)))
        return int(host[0])

    def synthesize_depth(self, pose, max_depth, conf_threshold, time, max_time, time_delta, out):
        """ModelProjection::synthesizeDepth into `out`, a device tensor f32 [rows, cols]; enqueued"""
        assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() == self.ctx.width * self.ctx.height
        self.ctx._check(self.ctx.lib.cf_model_synthesize_depth(self.h, self._pose(pose), C.c_float(max_depth), C.c_float(conf_threshold),
                                                               int(time), int(max_time), int(time_delta), _p(out)))

    def perform_fill_in(self, rgba, depth_filt, pass_geom=False, pass_rgb=False):
        self.ctx._check(self.ctx.lib.cf_model_perform_fill_in(self.h, _p(rgba), _p(depth_filt), int(pass_geom), int(pass_rgb)))

    def prefetch_fill_ratio(self):
        self.ctx._check(self.ctx.lib.cf_model_prefetch_fill_ratio(self.h))

    def fill_counts_device(self):
        """the (covered, total) counts of the pending fill-ratio prefetch as they stand in device memory, or None without one"""
        ptr = C.c_void_p()
        self.ctx._check(self.ctx.lib.cf_model_fill_ratio_device(self.h, C.byref(ptr)))
        if not ptr.value:
            return None
        host = np.empty(2, np.uint32)
        self.ctx._check(self.ctx.lib.cf_memcpy_d2h(self.ctx.h, host.ctypes.data_as(C.c_void_p), ptr, C.c_uint64(8)))
        return host

    def requires_fill_in(self, ratio=0.75):
        out = C.c_int()
        self.ctx._check(self.ctx.lib.cf_model_requires_fill_in(self.h, C.c_float(ratio), C.byref(out)))
        return bool(out.value)

    def fuse(self, pose, time, rgba, mask, depth_raw, depth_filt, max_depth, weighting, mask_id):
        self.ctx._check(self.ctx.lib.cf_model_fuse(self.h, self._pose(pose), time, _p(rgba), _p(mask), _p(depth_raw), _p(depth_filt),
                                                   C.c_float(max_depth), C.c_float(weighting), mask_id))

    def clean(self, pose, time, conf_threshold, outlier_coeff, depth_filt, mask, mask_id, time_delta=TIME_DELTA):
        c = C.c_uint32()
        self.ctx._check(self.ctx.lib.cf_model_clean(self.h, self._pose(pose), time, C.c_float(conf_threshold), C.c_float(outlier_coeff),
                                                    time_delta, _p(depth_filt), _p(mask), mask_id, C.byref(c)))
        return c.value

    def download_map(self):
        n = self.count()
        out = np.zeros((max(n, 1), SURFEL), np.float32)
        c = C.c_uint32()
        self.ctx._check(self.ctx.lib.cf_model_download_map(self.h, out.ctypes.data_as(C.c_void_p), n, C.byref(c)))
        return out[:n]

    def upload_map(self, surfels):
        s = np.ascontiguousarray(surfels, np.float32).reshape(-1, SURFEL)
        self.ctx._check(self.ctx.lib.cf_model_upload_map(self.h, s.ctypes.data_as(C.c_void_p), s.shape[0]))

    def extents_unknown(self):
        """cf_model_extents_unknown: the caller wrote the model's device buffers itself"""
        self.ctx._check(self.ctx.lib.cf_model_extents_unknown(self.h))

    def tensor(self, which):
        """Zero-copy torch view of a projection buffer (stays valid while the model lives)."""
        ptr = C.c_void_p(); nbytes = C.c_uint64()
        self.ctx._check(self.ctx.lib.cf_model_buffer(self.h, which, C.byref(ptr), C.byref(nbytes)))
        return ptr.value, nbytes.value

    def buffer(self, which):
        ptr, nbytes = self.tensor(which)
        host = np.empty(nbytes, np.uint8)
        if nbytes:
            self.ctx._check(self.ctx.lib.cf_memcpy_d2h(self.ctx.h, host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_uint64(nbytes)))
        h, w = self.ctx.height, self.ctx.width
        if which in (11, 12):   # the surfels; the new unstable surfels of the last fuse
            return host.view(np.float32).reshape(-1, SURFEL)
        if which == 13:         # the clean stage's packed texel records
            return host.view(np.float32).reshape(h, w, 8)
        if which == 14:         # the rasterisers' z-keys
            return host.view(np.uint64).reshape(h, w)
        dt, ch = _BUF[which]
        a = host.view(dt)
        return a.reshape(h, w, ch) if ch > 1 else a.reshape(h, w)


class _DevView:
    """Minimal stand-in that lets _p() pass a raw device pointer owned by the library."""

    def __init__(self, ptr):
        self._ptr = ptr
        self.is_cuda = True

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self._ptr
