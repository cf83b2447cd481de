"""ctypes binding of the fern keyframe database (cf_ferns_* in include/cofusion_hip.h; csrc/ferns.hip).

ElasticFusion's random-fern relocaliser (Core/Ferns.cpp), device resident: `Ferns.add` is Ferns::addFrame without a host wait,
`Ferns.relocalise` is Ferns::findFrame.  The loop-closure seam (include/cofusion_loop.h): `gate_async` / `gate_wait` after a search,
`find_frame` for a camera that is not lost, `constraints` for its device part alone.  Tensors are torch CUDA tensors handed over as raw
device pointers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _libmod

FERN = np.dtype([("x", "<i4"), ("y", "<i4"), ("r", "<i4"), ("g", "<i4"), ("b", "<i4"), ("d", "<i4")])
FERNS_MAX = 2048


class FernsConfig(C.Structure):
    _fields_ = [("n_ferns", C.c_int), ("capacity", C.c_int), ("max_depth_mm", C.c_int), ("photo_threshold", C.c_float)]


class FernsResult(C.Structure):
    _fields_ = [("accepted", C.c_int), ("keyframe", C.c_int), ("dissimilarity", C.c_float), ("overlap", C.c_float),
                ("pose", C.c_float * 16), ("icp_error", C.c_float), ("icp_count", C.c_float), ("icp_ran", C.c_int),
                ("photo_count", C.c_int), ("photo_error", C.c_double)]


# the documented signatures (tests/test_cpu_ferns.py holds include/cofusion_hip.h against them)
_V, _I, _F, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_uint64
SIGNATURES = {
    "cf_ferns_table": (_I, [_U64, _I, _I, _I, _I, _V]),
    "cf_ferns_create": (_I, [_V, C.POINTER(FernsConfig), _V, _U64, C.POINTER(_V)]),
    "cf_ferns_destroy": (None, [_V]),
    "cf_ferns_get_table": (_I, [_V, _V]),
    "cf_ferns_encode": (_I, [_V, _V, _V, _V]),
    "cf_ferns_search": (_I, [_V, _I, _I]),
    "cf_ferns_append": (_I, [_V, _V, _I, _F]),
    "cf_ferns_add_async": (_I, [_V, _V, _V, _V, _V, _I, _F]),
    "cf_ferns_relocalise": (_I, [_V, _V, _I, _I, _I, C.POINTER(FernsResult)]),
    "cf_ferns_count": (_I, [_V, C.POINTER(_I), C.POINTER(_I)]),
    "cf_ferns_download": (_I, [_V, _I, _V, C.POINTER(_I), _V, C.POINTER(_I), _V, _V, _V]),
    "cf_ferns_last_search": (_I, [_V, _V, _I, C.POINTER(_I), C.POINTER(_F), C.POINTER(_F), C.POINTER(_I), C.POINTER(_I)]),
}


class FernsGate(C.Structure):
    """cf_ferns_gate (include/cofusion_loop.h): 32 bytes"""
    _fields_ = [("serial", C.c_uint32), ("match_id", C.c_int32), ("dissimilarity", C.c_float), ("overlap", C.c_float),
                ("good_q", C.c_int32), ("keyframe_time", C.c_int32), ("count", C.c_int32), ("keyframes", C.c_int32)]


class FernsClosure(C.Structure):
    """cf_ferns_closure: 48 bytes"""
    _fields_ = [("accepted", C.c_int32), ("n_constraints", C.c_int32), ("photo_sum", C.c_int64), ("photo_count", C.c_int64),
                ("photo_error", C.c_double), ("keyframe", C.c_int32), ("keyframe_time", C.c_int32), ("icp_error", C.c_float),
                ("icp_count", C.c_float)]


MAX_SAMPLES = 64
MAX_CONSTRAINTS = 128
# the loop-closure seam (include/cofusion_loop.h)
LOOP_SIGNATURES = {
    "cf_ferns_gate_async": (_I, [_V]),
    "cf_ferns_gate_wait": (_I, [_V, C.POINTER(FernsGate)]),
    "cf_ferns_constraints": (_I, [_V, _I, _V, _V, _F, _F, _I, _I, C.POINTER(FernsClosure)]),
    "cf_ferns_find_frame": (_I, [_V, _V, _I, _I, _I, C.POINTER(FernsResult), C.POINTER(FernsClosure)]),
    "cf_ferns_constraint_buffers": (_I, [_V, C.POINTER(_V), C.POINTER(_V), C.POINTER(_V)]),
    "cf_ferns_keyframe_buffers": (_I, [_V, C.POINTER(_V), C.POINTER(_V)]),
}


def loop_samples(n_ferns):
    """samples loop closure draws from n_ferns ferns (Ferns.cpp:240), or None where it is refused (fewer than 50 ferns, more than 64 samples)"""
    if n_ferns < 50:
        return None
    step = n_ferns // 50
    m = (n_ferns + step - 1) // step
    return m if m <= MAX_SAMPLES else None


def bind(lib):
    for name, (res, args) in list(SIGNATURES.items()) + list(LOOP_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def make_table(seed, n_ferns, reduced_width, reduced_height, max_depth_mm):
    """the table cf_ferns_create generates from `seed` (host arithmetic only: works without a GPU)"""
    lib = bind(_libmod.load())
    out = np.zeros(n_ferns, FERN)
    rc = lib.cf_ferns_table(seed, n_ferns, reduced_width, reduced_height, max_depth_mm, out.ctypes.data)
    if rc != 0:
        raise ValueError(f"cf_ferns_table: error {rc}")
    return out


def _dp(t):
    assert t.is_cuda and t.is_contiguous()
    return t.data_ptr()


def _pose(p):
    return np.ascontiguousarray(p, np.float32).reshape(16)


class Ferns:
    """cf_ferns on an api.Context of the full frame size (width % 128 == 0, height % 32 == 0)."""

    def __init__(self, ctx, n_ferns=500, capacity=1024, max_depth_mm=5000, photo_threshold=115.0, table=None, seed=0):
        self.ctx, self.lib = ctx, bind(ctx.lib)
        self.n, self.capacity = int(n_ferns), int(capacity)
        self.rw, self.rh = ctx.width // 8, ctx.height // 8
        cfg = FernsConfig(self.n, self.capacity, int(max_depth_mm), float(photo_threshold))
        tab = None
        if table is not None:
            tab = np.ascontiguousarray(table, FERN)
            assert tab.shape == (self.n,)
        self.h = C.c_void_p()
        ctx._check(self.lib.cf_ferns_create(ctx.h, C.byref(cfg), None if tab is None else tab.ctypes.data, seed, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.cf_ferns_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def table(self):
        out = np.zeros(self.n, FERN)
        self.ctx._check(self.lib.cf_ferns_get_table(self.h, out.ctypes.data))
        return out

    def encode(self, vertex4, normal4, rgba):
        self.ctx._check(self.lib.cf_ferns_encode(self.h, _dp(vertex4), _dp(normal4), _dp(rgba)))

    def search(self, time, min_age):
        self.ctx._check(self.lib.cf_ferns_search(self.h, int(time), int(min_age)))

    def append(self, pose, src_time, threshold):
        p = _pose(pose)
        self.ctx._check(self.lib.cf_ferns_append(self.h, p.ctypes.data, int(src_time), float(threshold)))

    def add(self, vertex4, normal4, rgba, pose, src_time, threshold):
        """Ferns::addFrame, enqueued only: read the outcome with count() / last_search()"""
        p = _pose(pose)
        self.ctx._check(self.lib.cf_ferns_add_async(self.h, _dp(vertex4), _dp(normal4), _dp(rgba), p.ctypes.data, int(src_time), float(threshold)))

    def relocalise(self, curr_pose, time, min_age=300, lost=True):
        res = FernsResult()
        p = _pose(curr_pose)
        self.ctx._check(self.lib.cf_ferns_relocalise(self.h, p.ctypes.data, int(time), int(min_age), int(bool(lost)), C.byref(res)))
        return self._result(res)

    @staticmethod
    def _result(res):
        return dict(accepted=bool(res.accepted), keyframe=res.keyframe, dissimilarity=np.float32(res.dissimilarity), overlap=np.float32(res.overlap),
                    pose=np.array(res.pose, np.float32).reshape(4, 4), icp_error=np.float32(res.icp_error), icp_count=np.float32(res.icp_count),
                    icp_ran=bool(res.icp_ran), photo_count=res.photo_count, photo_error=float(res.photo_error))

    @staticmethod
    def _closure(c):
        return dict(accepted=bool(c.accepted), n_constraints=c.n_constraints, photo_sum=c.photo_sum, photo_count=c.photo_count,
                    photo_error=float(c.photo_error), keyframe=c.keyframe, keyframe_time=c.keyframe_time, icp_error=np.float32(c.icp_error),
                    icp_count=np.float32(c.icp_count))

    def gate_async(self):
        """blockHDAware of the current slot against the match of the last search: one launch, enqueued"""
        self.ctx._check(self.lib.cf_ferns_gate_async(self.h))

    def gate_wait(self):
        g = FernsGate()
        self.ctx._check(self.lib.cf_ferns_gate_wait(self.h, C.byref(g)))
        return dict(serial=g.serial, match_id=g.match_id, dissimilarity=np.float32(g.dissimilarity), overlap=np.float32(g.overlap), good_q=g.good_q,
                    keyframe_time=g.keyframe_time, count=g.count, keyframes=g.keyframes)

    def constraints(self, keyframe, curr_pose, est_pose, icp_error, icp_count, lost, time):
        """photometric check, accept rule and surface constraints against `keyframe`, the tracker's results handed in"""
        c = FernsClosure()
        cp, ep = _pose(curr_pose), _pose(est_pose)
        self.ctx._check(self.lib.cf_ferns_constraints(self.h, int(keyframe), cp.ctypes.data, ep.ctypes.data, float(icp_error), float(icp_count),
                                                      int(bool(lost)), int(time), C.byref(c)))
        return self._closure(c)

    def find_frame(self, curr_pose, time, min_age=300, lost=False):
        """Ferns::findFrame for a slot that has been encoded, searched and gated -> (result as relocalise gives it, closure)"""
        res, c = FernsResult(), FernsClosure()
        p = _pose(curr_pose)
        self.ctx._check(self.lib.cf_ferns_find_frame(self.h, p.ctypes.data, int(time), int(min_age), int(bool(lost)), C.byref(res), C.byref(c)))
        return self._result(res), self._closure(c)

    def constraint_buffers(self):
        """device addresses of src, dst f32 [128][3] and time f32 [128]"""
        s, d, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ctx._check(self.lib.cf_ferns_constraint_buffers(self.h, C.byref(s), C.byref(d), C.byref(t)))
        return s.value, d.value, t.value

    def keyframe_buffers(self):
        """device addresses of the database's poses f32 [capacity][16] and times i32 [capacity]"""
        p, t = C.c_void_p(), C.c_void_p()
        self.ctx._check(self.lib.cf_ferns_keyframe_buffers(self.h, C.byref(p), C.byref(t)))
        return p.value, t.value

    def download_constraints(self, n):
        """the first n rows of the constraint buffers -> src [n, 3], dst [n, 3], time [n] (host)"""
        s, d, t = self.constraint_buffers()
        src = np.zeros((n, 3), np.float32); dst = np.zeros((n, 3), np.float32); tm = np.zeros(n, np.float32)
        for a, p in ((src, s), (dst, d), (tm, t)):
            if n:
                self.ctx._check(self.ctx.lib.cf_memcpy_d2h(self.ctx.h, a.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_uint64(a.nbytes)))
        return src, dst, tm

    def count(self):
        c, f = C.c_int(), C.c_int()
        self.ctx._check(self.lib.cf_ferns_count(self.h, C.byref(c), C.byref(f)))
        return c.value, bool(f.value)

    def download(self, index=-1):
        """index -1: the current slot"""
        npx = self.rw * self.rh
        codes = np.zeros(self.n, np.uint8); pose = np.zeros(16, np.float32)
        v = np.zeros((3 * self.rh, self.rw), np.float32); n = np.zeros((3 * self.rh, self.rw), np.float32); rgb = np.zeros((self.rh, self.rw, 3), np.uint8)
        good, time = C.c_int(), C.c_int()
        assert v.size == 3 * npx
        self.ctx._check(self.lib.cf_ferns_download(self.h, int(index), codes.ctypes.data, C.byref(good), pose.ctypes.data, C.byref(time),
                                                   v.ctypes.data, n.ctypes.data, rgb.ctypes.data))
        return dict(codes=codes, good=good.value, pose=pose.reshape(4, 4), time=time.value, vmap=v, nmap=n, rgb=rgb)

    def last_search(self):
        co = np.zeros(max(self.capacity, 1), np.int32)
        searched, match, appended = C.c_int(), C.c_int(), C.c_int()
        ma, mm = C.c_float(), C.c_float()
        self.ctx._check(self.lib.cf_ferns_last_search(self.h, co.ctypes.data, co.size, C.byref(searched), C.byref(ma), C.byref(mm), C.byref(match),
                                                      C.byref(appended)))
        return dict(co=co[:searched.value].copy(), searched=searched.value, min_all=np.float32(ma.value), min_match=np.float32(mm.value),
                    match_id=match.value, appended=bool(appended.value))
