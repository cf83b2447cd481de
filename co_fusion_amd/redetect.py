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


BINS = 512            # CF_REDETECT_BINS


class Registration(C.Structure):
    """cf_redetect_registration"""
    _fields_ = [("ok", C.c_int), ("iterations", C.c_int), ("first_inliers", C.c_uint32), ("last_inliers", C.c_uint32), ("rms", C.c_float),
                ("cam_from_model", C.c_float * 16)]


def _frame(depth, label, cam, new_label, depth_cutoff, depth_tol):
    rows, cols = depth.shape
    assert tuple(label.shape) == (rows, cols)
    return Frame(_p(depth), _p(label), cols, rows, Cam(*[float(x) for x in cam]), int(new_label), float(depth_cutoff), float(depth_tol))


def _f32s(values, n):
    return (C.c_float * n)(*[float(x) for x in np.asarray(values, np.float32).reshape(n)])


def frame_moments(ctx: Context, depth, label, rgba, cam, new_label, depth_cutoff):
    """cf_redetect_frame_moments.  depth f32 [H, W], label u8 [H, W], rgba u8 [H, W, 4]: device tensors.  Returns (moments int64 [4]: the
    number of the label's valid pixels and their vertex sums on the 2^-16 m grid, hist uint32 [512])."""
    f = _frame(depth, label, cam, new_label, depth_cutoff, 0.0)
    assert tuple(rgba.shape) == tuple(depth.shape) + (4,)
    m = np.zeros(4, np.int64); h = np.zeros(BINS, np.uint32)
    ctx._check(ctx.lib.cf_redetect_frame_moments(ctx.h, C.byref(f), _p(rgba), m.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p)))
    return m, h


def model_moments(ctx: Context, candidates, dhat):
    """cf_redetect_model_moments.  candidates: (Model, pose 4x4, conf_threshold) triples as score() takes them (the static hypotheses); dhat:
    the unit vector towards the label's centroid.  Returns (moments int64 [n, 4] of the front-facing stable surfels, hist uint32 [n, 512]
    of all stable surfels)."""
    n = len(candidates)
    arr = (Candidate * n)()
    for a, (m, pose, theta) in zip(arr, candidates):
        a.model = m.h
        a.pose = _f32s(pose, 16)
        a.conf_threshold = float(theta)
    mm = np.zeros((n, 4), np.int64); h = np.zeros((n, BINS), np.uint32)
    ctx._check(ctx.lib.cf_redetect_model_moments(ctx.h, arr, n, _f32s(dhat, 3), mm.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p)))
    return mm, h


def register_step(ctx: Context, model, theta, cam_from_model, depth, label, cam, new_label, depth_cutoff, depth_tol, centre):
    """cf_redetect_register_step: the 29 sums (int64 [32]) of one step of `model` at T(camera <- model) = cam_from_model"""
    f = _frame(depth, label, cam, new_label, depth_cutoff, depth_tol)
    s = np.zeros(32, np.int64)
    ctx._check(ctx.lib.cf_redetect_register_step(ctx.h, model.h, C.c_float(theta), _f32s(cam_from_model, 16), C.byref(f), _f32s(centre, 3),
                                                 s.ctypes.data_as(C.c_void_p)))
    return s


def register(ctx: Context, model, theta, seed_cam_from_model, depth, label, cam, new_label, depth_cutoff, depth_tol, centre, iterations=10):
    """cf_redetect_register: the whole loop.  Returns dict(ok, iterations, first_inliers, last_inliers, rms, cam_from_model f32 [4, 4])."""
    f = _frame(depth, label, cam, new_label, depth_cutoff, depth_tol)
    r = Registration()
    ctx._check(ctx.lib.cf_redetect_register(ctx.h, model.h, C.c_float(theta), _f32s(seed_cam_from_model, 16), C.byref(f), _f32s(centre, 3),
                                            int(iterations), C.byref(r)))
    return dict(ok=bool(r.ok), iterations=int(r.iterations), first_inliers=int(r.first_inliers), last_inliers=int(r.last_inliers), rms=float(r.rms),
                cam_from_model=np.array(list(r.cam_from_model), np.float32).reshape(4, 4))


def timing(ctx: Context, on=True):
    """cf_redetect_timing: device events around the launches of every later score(); returns what the last one took, in milliseconds"""
    ms = C.c_float()
    ctx._check(ctx.lib.cf_redetect_timing(ctx.h, int(bool(on)), C.byref(ms)))
    return float(ms.value)


def relabel(ctx: Context, label, src, dst):
    """cf_relabel on a flat device tensor u8 (16-byte aligned storage), in place; enqueued on the context's stream"""
    ctx._check(ctx.lib.cf_relabel(ctx.h, _p(label), C.c_uint64(label.numel()), int(src), int(dst)))
