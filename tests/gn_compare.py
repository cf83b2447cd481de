"""Bit-for-bit comparison helpers of the stage suites that read a tracker state back through the C-ABI (plain helper module, no tests
in here): tests/test_gn_solve_gpu.py and tests/test_so3_prealign_gpu.py."""
import ctypes as C

import numpy as np


def raw(v):
    return bytes(v) if isinstance(v, (C.Array, C.Structure)) else np.asarray(v).tobytes()


def show(v):
    return list(v) if isinstance(v, C.Array) else v


def same(a, b):
    """bit equality of two ctypes values (float / int scalars or arrays), NaN equal to NaN"""
    if isinstance(a, C.Array):
        t = {C.c_float: np.float32, C.c_double: np.float64, C.c_int32: np.int32, C.c_int: np.int32}[a._type_]
        x, y = np.frombuffer(bytes(a), t), np.frombuffer(bytes(b), t)
    else:
        t = np.float32 if isinstance(a, float) else np.int64
        x, y = np.array([a], t), np.array([b], t)
    if x.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
        return bool(np.all((x.view(u) == y.view(u)) | (np.isnan(x) & np.isnan(y))))
    return bool(np.array_equal(x, y))


def expected_hot(s):
    """refresh_hot (csrc/cf_kernels.h, GnHot) of a state, as 48 words: line 0 {icp, level_done, cull_z[2], Rcurr[9], tcurr[3]}, line 1
    {Rprev_inv[9], tprev[3], cull_box[4]}, line 2 {rgb, rgbOnly, level_done, 0, krkInv[9], kt[3]}"""
    i32 = lambda *v: np.array(v, np.int32).view(np.uint32)
    f32 = lambda a: np.frombuffer(bytes(a), np.uint32)
    return np.concatenate([i32(s.icp, s.level_done), f32(s.cull_z), f32(s.Rcurr), f32(s.tcurr), f32(s.Rprev_inv), f32(s.tprev), f32(s.stats.cull_box),
                           i32(s.rgb, s.rgbOnly, s.level_done, 0), f32(s.krkInv), f32(s.kt)])
