"""ctypes binding of the deformation graph (cf_deform_* in include/cofusion_hip.h; csrc/deform.hip): loop closure of one
surfel map from absolute constraints -- sample the graph, weight the constraint points, optimise, move the map and the keyframe poses.
The graph's local mode (a last_deform_time: only younger nodes are free) is the *_local calls, behind the same methods.
Maps are a model.Model or a torch CUDA tensor f32 [S, 12]; poses and times are torch CUDA tensors."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .api import Cam, _p

MAX_NODES = 1024
MAX_CONSTRAINTS = 128
MAX_CONSTRAINTS_SIZED = 1536
MAX_RELATIVE = 128
BAND = 240
VARS = 12
STEP_FIELDS = ("error", "delta_norm", "failed", "mean_cons_error")
RESULT_FIELDS = ("optimised", "accepted", "failed", "iterations", "error_before", "mean_cons_error_before", "error", "mean_cons_error")


class Thresholds(C.Structure):
    """cf_deform_thresholds"""
    _fields_ = [("min_cons_error", C.c_float), ("max_iterations", C.c_int), ("min_delta", C.c_float), ("min_error", C.c_float),
                ("min_change", C.c_float), ("max_first_error", C.c_float), ("accept_cons_error", C.c_float), ("accept_error", C.c_float)]


class Step(C.Structure):
    """cf_deform_step"""
    _fields_ = [("error", C.c_float), ("delta_norm", C.c_double), ("failed", C.c_int), ("mean_cons_error", C.c_float)]


class Result(C.Structure):
    """cf_deform_result"""
    _fields_ = [("optimised", C.c_int), ("accepted", C.c_int), ("failed", C.c_int), ("iterations", C.c_int), ("error_before", C.c_float),
                ("mean_cons_error_before", C.c_float), ("error", C.c_float), ("mean_cons_error", C.c_float)]


class Reactivate(C.Structure):
    """cf_deform_reactivate"""
    _fields_ = [("pose", C.c_float * 16), ("cam", Cam), ("cols", C.c_int), ("rows", C.c_int), ("max_depth", C.c_float), ("depth", C.c_void_p),
                ("conf_threshold", C.c_float), ("tick", C.c_int)]


_V, _I, _F = C.c_void_p, C.c_int, C.c_float
_PI = C.POINTER(C.c_int)
SIGNATURES = {
    "cf_deform_create": (_I, [_V, C.POINTER(_V)]),
    "cf_deform_create_sized": (_I, [_V, _I, C.POINTER(_V)]),
    "cf_deform_assemble_local": (_I, [_V, _I]),
    "cf_deform_iterate_local": (_I, [_V, _I, C.POINTER(Step)]),
    "cf_deform_optimise_local": (_I, [_V, _I, C.POINTER(Thresholds), C.POINTER(Result)]),
    "cf_deform_destroy": (None, [_V]),
    "cf_deform_default_thresholds": (None, [C.POINTER(Thresholds)]),
    "cf_deform_sample": (_I, [_V, _V, C.c_uint32, _I, _PI, _PI, _PI]),
    "cf_deform_set_nodes": (_I, [_V, _V, _V, _I]),
    "cf_deform_weights": (_I, [_V, _V, _V, _V, _I]),
    "cf_deform_weights_device": (_I, [_V, _V, _V, _V, _I]),
    "cf_deform_assemble": (_I, [_V]),
    "cf_deform_iterate": (_I, [_V, C.POINTER(Step)]),
    "cf_deform_optimise": (_I, [_V, C.POINTER(Thresholds), C.POINTER(Result)]),
    "cf_deform_apply": (_I, [_V, _V, C.c_uint32, C.POINTER(Reactivate)]),
    "cf_deform_apply_poses": (_I, [_V, _V, _V, _I]),
    "cf_deform_download": (_I, [_V, _PI, _PI, _V, _V, _V, _V, _V, _V, _V]),
    "cf_deform_enable_relative": (_I, [_V, _I]),
    "cf_deform_set_relative": (_I, [_V, _V, _V, _V, _V, _I, _I]),
    "cf_deform_set_relative_device": (_I, [_V, _V, _V, _V, _V, _I, _I]),
    "cf_deform_pick_relative": (_I, [_V, _V, _V, _V, _V, _V, _I, _I, _PI]),
    "cf_deform_download_out": (_I, [_V, _V]),
    "cf_deform_bench_relative_y": (_I, [_V]),
    "cf_deform_download_relative": (_I, [_V, _PI, _PI, C.POINTER(C.c_int64), _PI, _V, _V, _V, _V, _V, _V, _V]),
}


def bind(lib):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def default_thresholds(lib):
    t = Thresholds()
    bind(lib).cf_deform_default_thresholds(C.byref(t))
    return t


def _map(m):
    """-> (device address, surfel count) of a Model or a tensor [S, 12]"""
    if hasattr(m, "tensor"):
        ptr, nbytes = m.tensor(11)
        return C.c_void_p(ptr), nbytes // 48
    assert m.is_cuda and m.is_contiguous() and m.dtype.is_floating_point and m.element_size() == 4 and m.numel() % 12 == 0
    return C.c_void_p(m.data_ptr()), m.numel() // 12


def _host(a, dtype, shape):
    a = np.ascontiguousarray(a, dtype).reshape(shape)
    return a, a.ctypes.data_as(C.c_void_p)


class Deform:
    """cf_deform on an api.Context; max_constraints: None (128, cf_deform_create) or a capacity up to MAX_CONSTRAINTS_SIZED"""

    def __init__(self, ctx, max_constraints=None):
        self.ctx, self.lib = ctx, bind(ctx.lib)
        self.h = C.c_void_p()
        if max_constraints is None:
            ctx._check(self.lib.cf_deform_create(ctx.h, C.byref(self.h)))
        else:
            ctx._check(self.lib.cf_deform_create_sized(ctx.h, int(max_constraints), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.cf_deform_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sample(self, surfel_map, sample_rate=25000):
        """-> (nodes, stride, monotone)"""
        ptr, count = _map(surfel_map)
        n, s, m = C.c_int(), C.c_int(), C.c_int()
        self.ctx._check(self.lib.cf_deform_sample(self.h, ptr, count, int(sample_rate), C.byref(n), C.byref(s), C.byref(m)))
        return n.value, s.value, bool(m.value)

    def set_nodes(self, nodes, params=None):
        nodes, pn = _host(nodes, np.float32, (-1, 4))
        pp = None
        if params is not None:
            params, pp = _host(params, np.float32, (len(nodes), VARS))
        self.ctx._check(self.lib.cf_deform_set_nodes(self.h, pn, pp, len(nodes)))

    def weights(self, src, dst, src_time):
        src, ps = _host(src, np.float32, (-1, 3)); dst, pd = _host(dst, np.float32, (-1, 3)); tm, pt = _host(src_time, np.float32, (-1,))
        assert len(src) == len(dst) == len(tm)
        self.ctx._check(self.lib.cf_deform_weights(self.h, ps, pd, pt, len(src)))

    def weights_device(self, src, dst, src_time, n):
        """the same from device arrays (tensors or raw addresses) f32 [>= n, 3], [>= n, 3], [>= n]: no host-to-device copy"""
        addr = lambda a: C.c_void_p(a) if isinstance(a, int) else _p(a)
        self.ctx._check(self.lib.cf_deform_weights_device(self.h, addr(src), addr(dst), addr(src_time), int(n)))

    def assemble(self, last_deform_time=None):
        """last_deform_time None: every node is free (cf_deform_assemble); an int: the local mode (cf_deform_assemble_local)"""
        if last_deform_time is None:
            self.ctx._check(self.lib.cf_deform_assemble(self.h))
        else:
            self.ctx._check(self.lib.cf_deform_assemble_local(self.h, int(last_deform_time)))

    def iterate(self, last_deform_time=None):
        st = Step()
        if last_deform_time is None:
            self.ctx._check(self.lib.cf_deform_iterate(self.h, C.byref(st)))
        else:
            self.ctx._check(self.lib.cf_deform_iterate_local(self.h, int(last_deform_time), C.byref(st)))
        return dict(error=np.float32(st.error), delta_norm=float(st.delta_norm), failed=bool(st.failed), mean_cons_error=np.float32(st.mean_cons_error))

    def optimise(self, thresholds=None):
        r = Result()
        self.ctx._check(self.lib.cf_deform_optimise(self.h, None if thresholds is None else C.byref(thresholds), C.byref(r)))
        return self._result(r)

    def optimise_local(self, last_deform_time, thresholds=None):
        """the graph's local mode: no 0.06 gate, no `error > 10` stop, accepted unless a step failed or no node is enabled"""
        r = Result()
        self.ctx._check(self.lib.cf_deform_optimise_local(self.h, int(last_deform_time), None if thresholds is None else C.byref(thresholds), C.byref(r)))
        return self._result(r)

    @staticmethod
    def _result(r):
        out = {k: getattr(r, k) for k in RESULT_FIELDS}
        for k in ("optimised", "accepted", "failed"):
            out[k] = bool(out[k])
        for k in RESULT_FIELDS[4:]:
            out[k] = np.float32(out[k])
        return out

    def apply(self, surfel_map, reactivate=None):
        """the map pass, in place, enqueued.  reactivate: dict(pose 4x4, cam (fx, fy, cx, cy), depth: device tensor [rows, cols], max_depth,
        conf_threshold, tick)"""
        ptr, count = _map(surfel_map)
        re = None
        if reactivate is not None:
            a = reactivate
            rows, cols = a["depth"].shape
            re = Reactivate((C.c_float * 16)(*[float(x) for x in np.asarray(a["pose"], np.float32).reshape(16)]), Cam(*[float(x) for x in a["cam"]]),
                            cols, rows, float(a["max_depth"]), _p(a["depth"]), float(a["conf_threshold"]), int(a["tick"]))
        self.ctx._check(self.lib.cf_deform_apply(self.h, ptr, count, None if re is None else C.byref(re)))

    def apply_poses(self, poses, times):
        """poses: device tensor f32 [n, 16] (row-major 4x4), times: device tensor i32 [n]; in place, enqueued"""
        n = times.numel()
        assert poses.numel() == 16 * n and times.element_size() == 4
        self.ctx._check(self.lib.cf_deform_apply_poses(self.h, _p(poses), _p(times), n))

    def counts(self):
        n, c = C.c_int(), C.c_int()
        self.ctx._check(self.lib.cf_deform_download(self.h, C.byref(n), C.byref(c), None, None, None, None, None, None, None))
        return n.value, c.value

    def download(self, system=False):
        """nodes, params, edges, ids, weights; with system: A in band form [12 n, 240] and b [12 n] too"""
        n, c = self.counts()
        nodes = np.zeros((n, 4), np.float32); params = np.zeros((n, VARS), np.float32); edges = np.zeros((n, 4), np.int32)
        ids = np.zeros((c, 4), np.int32); w = np.zeros((c, 4), np.float32)
        A = np.zeros((VARS * n, BAND)) if system else None
        b = np.zeros(VARS * n) if system else None
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self.ctx._check(self.lib.cf_deform_download(self.h, None, None, vp(nodes), vp(params), vp(edges), vp(ids), vp(w), vp(A), vp(b)))
        out = dict(nodes=nodes, params=params, edges=edges, ids=ids, weights=w)
        if system:
            out.update(A=A, b=b)
        return out

    # ---------------------------------------------------------------------------------------------- relative constraints
    def enable_relative(self, capacity=MAX_RELATIVE):
        """allocate the ring of relative pairs and the storage of the step that takes them (cf_deform_enable_relative)"""
        self.ctx._check(self.lib.cf_deform_enable_relative(self.h, int(capacity)))

    def set_relative(self, pairs, append=False):
        """pairs [n, 8] (source xyz, srcTime, target xyz, dstTime) from the host; append False: the ring is emptied first"""
        p = np.ascontiguousarray(pairs, np.float32).reshape(-1, 8)
        cols = [np.ascontiguousarray(p[:, 0:3]), np.ascontiguousarray(p[:, 4:7]), np.ascontiguousarray(p[:, 3]), np.ascontiguousarray(p[:, 7])]
        ptr = [a.ctypes.data_as(C.c_void_p) for a in cols]
        self.ctx._check(self.lib.cf_deform_set_relative(self.h, ptr[0], ptr[1], ptr[2], ptr[3], len(p), 1 if append else 0))

    def set_relative_device(self, src, dst, src_time, dst_time, n, append=False):
        """the same from device tensors f32 [>= n, 3], [>= n, 3], [>= n], [>= n]"""
        self.ctx._check(self.lib.cf_deform_set_relative_device(self.h, _p(src), _p(dst), _p(src_time), _p(dst_time), int(n), 1 if append else 0))

    def pick_relative(self, closure, src, dst, time, dst_time, n, row_stride=1):
        """append what the accepted closure `closure` (a Deform) leaves of its n constraints (device tensors; rows row_stride * i of src, dst,
        time; dst_time one per constraint) -> the number of pairs appended"""
        k = C.c_int()
        self.ctx._check(self.lib.cf_deform_pick_relative(self.h, closure.h, _p(src), _p(dst), _p(time), _p(dst_time), int(n), int(row_stride), C.byref(k)))
        return k.value

    def relative_counts(self):
        """-> dict(capacity, count, appended, used)"""
        cap, cnt, used, app = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        self.ctx._check(self.lib.cf_deform_download_relative(self.h, C.byref(cap), C.byref(cnt), C.byref(app), C.byref(used), None, None, None, None, None, None, None))
        return dict(capacity=cap.value, count=cnt.value, appended=app.value, used=used.value)

    def download_relative(self, system=False):
        """pairs [count, 8]; with system (after assemble / iterate): the weight sets of sources and targets, U in compact form, the relative
        residuals and C = I + Y^T Y [3 count, 3 count] with Y^T y [3 count]"""
        c = self.relative_counts()["count"]
        pairs = np.zeros((c, 8), np.float32)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        ids = w = uid = uval = rr = Cm = None
        if system:
            ids = np.zeros((2, c, 4), np.int32); w = np.zeros((2, c, 4), np.float32); uid = np.zeros((c, 8), np.int32)
            uval = np.zeros((c, 8, 4)); rr = np.zeros(3 * c); Cm = np.zeros((3 * c + 1, 3 * c))
        self.ctx._check(self.lib.cf_deform_download_relative(self.h, None, None, None, None, vp(pairs), vp(ids), vp(w), vp(uid), vp(uval), vp(rr), vp(Cm)))
        out = dict(pairs=pairs)
        if system:
            out.update(ids=ids, weights=w, u_ids=uid, u_vals=uval, r_rel=rr, C=Cm[:3 * c], z=Cm[3 * c])
        return out

    def download_out(self):
        """the 32-byte record the last residual pass / solve left on the device, as bytes"""
        buf = (C.c_ubyte * 32)()
        self.ctx._check(self.lib.cf_deform_download_out(self.h, buf))
        return bytes(buf)

    def bench_relative_y(self):
        """benchmark access: only the launch Y = L^-1 U^T, on the state the last iterate with pairs left.  Enqueued only."""
        self.ctx._check(self.lib.cf_deform_bench_relative_y(self.h))
