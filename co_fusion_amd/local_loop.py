"""ctypes binding of the constraint stage of local loop closure (cf_local_loop_* in include/cofusion_loop.h; csrc/local_loop.hip,
DESIGN.md 4.14 "The local half"): the accept rule on the model-to-model tracker's result and the surface constraints, one launch."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .api import _p


class Thresholds(C.Structure):
    """cf_local_loop_thresholds"""
    _fields_ = [("cov_thresh", C.c_float), ("icp_count_thresh", C.c_int32), ("icp_err_thresh", C.c_float)]


class Track(C.Structure):
    """cf_local_loop_track"""
    _fields_ = [("rot", C.c_float * 9), ("trans", C.c_float * 3), ("icp_error", C.c_float), ("icp_count", C.c_float), ("lastA", C.c_double * 36)]


class Record(C.Structure):
    """cf_local_loop_record"""
    _fields_ = [("accepted", C.c_int32), ("n_constraints", C.c_int32), ("max_covariance", C.c_double), ("icp_error", C.c_float),
                ("icp_count", C.c_float), ("est_pose", C.c_float * 16), ("covered", C.c_uint32), ("serial", C.c_uint32)]


_V, _I = C.c_void_p, C.c_int
SIGNATURES = {
    "cf_local_loop_create": (_I, [_V, C.POINTER(_V)]),
    "cf_local_loop_destroy": (None, [_V]),
    "cf_local_loop_constraints_async": (_I, [_V, _V, C.POINTER(Track), _V, _V, _V, C.POINTER(C.c_float), _I, C.c_float, _I, C.POINTER(Thresholds)]),
    "cf_local_loop_wait": (_I, [_V, C.POINTER(Record)]),
    "cf_local_loop_constraint_buffers": (_I, [_V, C.POINTER(_V), C.POINTER(_V), C.POINTER(_V)]),
    "cf_local_loop_target_times": (_I, [_V, C.POINTER(_V)]),
}


def bind(lib):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class LocalLoop:
    """cf_local_loop on an api.Context"""

    def __init__(self, ctx):
        self.ctx, self.lib = ctx, bind(ctx.lib)
        self.h = C.c_void_p()
        ctx._check(self.lib.cf_local_loop_create(ctx.h, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.cf_local_loop_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def constraints_async(self, vertex_conf, old_time, curr_pose, tick, max_depth, pin, odom=None, track=None, covered=None,
                          cov_thresh=1e-5, icp_count_thresh=40000, icp_err_thresh=5e-5):
        """vertex_conf, old_time: device tensors or raw addresses; the tracker's result from `odom` (an api.Odometry) or from `track`:
        dict(rot 3x3, trans 3, icp_error, icp_count, lastA 6x6)"""
        addr = lambda a: None if a is None else (C.c_void_p(a) if isinstance(a, int) else _p(a))
        tr = None
        if track is not None:
            tr = Track((C.c_float * 9)(*[float(x) for x in np.asarray(track["rot"], np.float32).reshape(9)]),
                       (C.c_float * 3)(*[float(x) for x in np.asarray(track["trans"], np.float32).reshape(3)]),
                       float(track["icp_error"]), float(track["icp_count"]),
                       (C.c_double * 36)(*[float(x) for x in np.asarray(track["lastA"], np.float64).reshape(36)]))
        th = Thresholds(float(cov_thresh), int(icp_count_thresh), float(icp_err_thresh))
        pose = (C.c_float * 16)(*[float(x) for x in np.asarray(curr_pose, np.float32).reshape(16)])
        self.ctx._check(self.lib.cf_local_loop_constraints_async(self.h, None if odom is None else odom.h, None if tr is None else C.byref(tr),
                                                                 addr(vertex_conf), addr(old_time), addr(covered), pose, int(tick),
                                                                 float(max_depth), int(bool(pin)), C.byref(th)))

    def wait(self):
        r = Record()
        self.ctx._check(self.lib.cf_local_loop_wait(self.h, C.byref(r)))
        return dict(accepted=bool(r.accepted), n_constraints=r.n_constraints, max_covariance=float(r.max_covariance),
                    icp_error=np.float32(r.icp_error), icp_count=np.float32(r.icp_count),
                    est_pose=np.array(list(r.est_pose), np.float32).reshape(4, 4), covered=int(r.covered), serial=int(r.serial))

    def buffers(self):
        """device addresses of src, dst [1536][3] and time [1536]"""
        s, d, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ctx._check(self.lib.cf_local_loop_constraint_buffers(self.h, C.byref(s), C.byref(d), C.byref(t)))
        return s.value, d.value, t.value

    def target_times_buffer(self):
        """device address of target_time [768]: the old time of every constraint (pin rows not counted)"""
        t = C.c_void_p()
        self.ctx._check(self.lib.cf_local_loop_target_times(self.h, C.byref(t)))
        return t.value

    def target_times(self, n):
        """the old times of the first n constraints, downloaded"""
        host = np.zeros(max(n, 1), np.float32)
        self.ctx._check(self.ctx.lib.cf_memcpy_d2h(self.ctx.h, host.ctypes.data_as(C.c_void_p), C.c_void_p(self.target_times_buffer()), C.c_uint64(4 * max(n, 1))))
        return host[:n]

    def rows(self, n):
        """the first n rows, downloaded: src [n, 3], dst [n, 3], time [n]"""
        out = []
        for ptr, width in zip(self.buffers(), (3, 3, 1)):
            host = np.zeros((max(n, 1), width), np.float32)
            self.ctx._check(self.ctx.lib.cf_memcpy_d2h(self.ctx.h, host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_uint64(4 * width * max(n, 1))))
            out.append(host[:n] if width > 1 else host[:n, 0])
        return out
