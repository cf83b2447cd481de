"""The static synthetic room of the relocalisation tests (co_fusion_amd/synth.py, no moving objects, no noise) seen from chosen
viewpoints: rendered once per process and shared by tests/test_ferns_reloc_gpu.py and tests/test_reloc_facade_gpu.py."""
from __future__ import annotations

import functools
import math

import numpy as np

from co_fusion_amd import synth

W, H = 640, 480
CAM = synth.Camera.scaled(W, H)
KEYFRAME_TIMES = (0, 40, 80, 120, 160)   # along Scene.camera_pose: up to 0.25 m and 10 degrees apart
QUERY_TIME = 94                          # 3.5 cm and 0.58 degrees from keyframe 2 (t = 80)
QUERY_KEYFRAME = 2
# The CPU oracle's own pose error on this query (tests/test_ferns_reloc_gpu.py states how it was measured), and the bound the tests
# allow: twice that, for the choice of query
ORACLE_TRANS_ERR_M, ORACLE_ROT_ERR_DEG = 1.2575e-3, 0.03287
POSE_BOUND_M, POSE_BOUND_DEG = 2 * ORACLE_TRANS_ERR_M, 2 * ORACLE_ROT_ERR_DEG


def _pose_far(which):
    """"far": looking at the opposite wall, "far2": at a side wall -- nothing in common with the approach, nor with each other"""
    T = np.eye(4)
    if which == "far":
        T[:3, :3] = synth._rot_axis([0, 1, 0], math.pi) @ synth._rot_axis([1, 0, 0], 0.15)
        T[:3, 3] = [0.1, 0.0, 0.6]
    else:
        T[:3, :3] = synth._rot_axis([0, 1, 0], 0.5 * math.pi) @ synth._rot_axis([1, 0, 0], -0.3)
        T[:3, 3] = [-0.9, -0.2, 1.4]
    return T


@functools.lru_cache(maxsize=64)
def view(t):
    """t: a frame number of the scene's smooth trajectory, or "far" / "far2".  -> depth f32, rgb u8, pose f32 T(world <- camera)"""
    sc = synth.Scene(n_obj=0, seed=1234)
    if isinstance(t, str):
        sc.camera_pose = lambda _t: _pose_far(t)
    d, rgb, _, T = sc.render(CAM, 0 if isinstance(t, str) else t, noise=False)
    return d, rgb, T.astype(np.float32)


@functools.lru_cache(maxsize=64)
def maps(t):
    """the frame's own geometry as fill-in maps: f32x4 vertex, f32x4 normal, rgba8 (synth.ideal_prediction)"""
    d, rgb, _ = view(t)
    return synth.ideal_prediction(CAM, d, rgb)


def pose_error(est, gt):
    """translation distance (m), rotation angle (degrees)"""
    est = np.asarray(est, np.float64).reshape(4, 4); gt = np.asarray(gt, np.float64).reshape(4, 4)
    dR = gt[:3, :3].T @ est[:3, :3]
    ang = math.degrees(2.0 * math.asin(min(1.0, float(np.linalg.norm(dR - np.eye(3))) / (2.0 * math.sqrt(2.0)))))   # (well conditioned near 0)
    return float(np.linalg.norm(est[:3, 3] - gt[:3, 3])), ang
