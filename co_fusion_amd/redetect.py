"""Python mirror of the re-detection entries of the C-ABI (cf_redetect_score, cf_relabel; include/cofusion_hip.h):
per-call access for tests and tools -- the frame loop calls them from the C++ facade (CoFusion::redetectModels)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .api import Cam, Context, _p

MAX_CANDIDATES = 16   # kRedetectBatch (csrc/cf_kernels.h)
COUNT_FIELDS = ("projected", "occluded", "seen_through", "agree", "agree_on_label", "covered")


class Counts(C.Structure):
    """cf_redetect_counts"""
    _fields_ = [(k, C.c_uint32) for k in COUNT_FIELDS]


class Candidate(C.Structure):
    """cf_redetect_candidate"""
    _fields_ = [("model", C.c_void_p), ("pose", C.c_float * 16), ("conf_threshold", C.c_float)]


class Frame(C.Structure):
    """cf_redetect_frame"""
    _fields_ = [("depth", C.c_void_p), ("label", C.c_void_p), ("cols", C.c_int), ("rows", C.c_int), ("cam", Cam), ("new_label", C.c_int),
                ("depth_cutoff", C.c_float), ("depth_tol", C.c_float)]


def score(ctx: Context, candidates, depth, label, cam, new_label, depth_cutoff, depth_tol):
    """cf_redetect_score.  candidates: (Model, pose 4x4, conf_threshold) triples; depth f32 [H, W] and label u8 [H, W]: device tensors;
    cam: (fx, fy, cx, cy).  Returns ([dict of the six counts per candidate], label_pixels)."""
    n = len(candidates)
    arr = (Candidate * n)()
    for a, (m, pose, theta) in zip(arr, candidates):
        a.model = m.h
        a.pose = (C.c_float * 16)(*[float(x) for x in np.asarray(pose, np.float32).reshape(16)])
        a.conf_threshold = float(theta)
    rows, cols = depth.shape
    assert tuple(label.shape) == (rows, cols)
    f = Frame(_p(depth), _p(label), cols, rows, Cam(*[float(x) for x in cam]), int(new_label), float(depth_cutoff), float(depth_tol))
    out = (Counts * n)()
    px = C.c_uint32()
    ctx._check(ctx.lib.cf_redetect_score(ctx.h, arr, n, C.byref(f), out, C.byref(px)))
    return [{k: int(getattr(o, k)) for k in COUNT_FIELDS} for o in out], int(px.value)


def timing(ctx: Context, on=True):
    """cf_redetect_timing: device events around the launches of every later score(); returns what the last one took, in milliseconds"""
    ms = C.c_float()
    ctx._check(ctx.lib.cf_redetect_timing(ctx.h, int(bool(on)), C.byref(ms)))
    return float(ms.value)


def relabel(ctx: Context, label, src, dst):
    """cf_relabel on a flat device tensor u8 (16-byte aligned storage), in place; enqueued on the context's stream"""
    ctx._check(ctx.lib.cf_relabel(ctx.h, _p(label), C.c_uint64(label.numel()), int(src), int(dst)))
