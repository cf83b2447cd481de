"""The scenario of local loop closure in the frame loop (tests/test_local_loop_closure_gpu.py, DESIGN.md 4.14 "The local half") and its
statement on the CPU: the room and the yaw turn of tests/test_loop_closure_gpu.py with a smaller drift.

synth.Scene(n_obj=0, seed=1234) at 640x480, noise off, the camera at (0, 0, 0.9) turning about the vertical axis by 3 degrees per frame.
Frames are fed in pose-input mode at poses whose yaw is DRIFT x the true yaw.  time_delta = 60 ticks: a wall leaves the 62-degree view
after 21 frames and comes back 99 frames later, inactive.  A view that returns after a full turn (120 frames) sits 360 (DRIFT - 1)
degrees from where the map has it.

The drift factor.  It must keep the global path silent (a mean constraint error below 0.06 with pins, that is constraints shorter than
0.12 m) and lie inside the tracker's 0.10 m correspondence gate when the old wall comes back.  DRIFT = 1.004 gives 1.44 degrees: 0.05 m
at 2 m, 0.10 m only beyond 4 m (the room's far corners).  The surfels of the first pass were fused at yaw DRIFT x their true yaw and
the fresh ones at DRIFT x (true yaw + 360), so seen from the fed pose the inactive map is the room seen from a camera turned by the
drift angle: `oracle_registration` renders the two views, makes their ideal predictions and runs the oracle tracker in the call order of
CoFusion.cpp:396-405 on them (frame side written through orc_odom_buffer, as tests/test_local_tracker_gpu.py does)."""
import ctypes as C
import math

import numpy as np

f32 = np.float32
TURN_DEG, DRIFT, TIME_DELTA = 3.0, 1.004, 60
RATE = 5000                 # sample rate of the local graph, the default of setLocalLoopClosure
EYE_AT = (0.0, 0.0, 0.9)
# The confidence threshold of the background map.  At 3 degrees per frame a surface stays in the 62-degree view for 21 frames and a
# surfel gains at most 1 per frame: at the default of 10 only the strip of the view that has been seen longest is stable, the active
# prediction covers a seventh of the image (measured: 42 000 texels matched, against the accept rule's 40 000) and the registration of
# such a strip leaves yaw and sideways translation coupled (covariance 3e-4 .. 3e-3 against 1e-5).  At 2 the active prediction covers
# what the statement's ideal prediction assumes, nearly the whole view.
CONF = 2.0
RETURN_FRAME = 105          # a frame in which the first pass's surface is in view again (from frame 100 on)
MAX_DEPTH_RGB = 6.0         # RGBDOdometry::maxDepthRGB
DRIFT_DEG = 360.0 * (DRIFT - 1.0)


def yaw_pose(deg):
    from co_fusion_amd import synth
    T = np.eye(4)
    T[:3, :3] = synth._rot_axis([0, 1, 0], math.radians(deg))
    T[:3, 3] = EYE_AT
    return T


def angle_between(a, b):
    r = np.asarray(a, np.float64)[:3, :3].T @ np.asarray(b, np.float64)[:3, :3]
    return math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(r) - 1) / 2))))


def make_views():
    """-> view(k): depth, rgb of frame k (the true view of frame k is the view of frame k mod 120), rendered once"""
    from co_fusion_amd import synth
    scene = synth.Scene(n_obj=0, seed=1234)
    scene.camera_pose = lambda t: yaw_pose(TURN_DEG * t)
    cam = synth.Camera()
    cache = {}

    def view(k):
        if k % 120 not in cache:
            cache[k % 120] = scene.render(cam, k % 120, noise=False)[:2]
        return cache[k % 120]
    return view


def wanted_pose(k):
    """the pose at which frame k's view agrees with the first pass's map: (old-view pose . true relative motion), the old view being
    the one a full turn earlier, whose true relative motion to frame k is the identity"""
    return yaw_pose(DRIFT * TURN_DEG * (k - 120))


def oracle_registration(k=RETURN_FRAME):
    """the model-to-model registration of frame k on ideal predictions -> the fed pose, the estimated pose, the oracle's statistics"""
    import orc
    from co_fusion_amd import synth
    scene = synth.Scene(n_obj=0, seed=1234)
    scene.camera_pose = lambda t: yaw_pose(TURN_DEG * t)
    cam = synth.Camera()
    W, H = cam.width, cam.height
    fed = f32(yaw_pose(DRIFT * TURN_DEG * k))
    # the active map is where the fed pose puts frame k's view; the inactive map, fused a full turn earlier, is the room turned back by
    # the drift angle, that is the room seen from true yaw 3 k + DRIFT_DEG
    d_act, rgb_act = scene.render(cam, k, noise=False)[:2]
    d_old, rgb_old = scene.render(cam, k + DRIFT_DEG / TURN_DEG, noise=False)[:2]
    v_act, n_act, img_act = synth.ideal_prediction(cam, d_act, rgb_act)
    v_old, n_old, img_old = synth.ideal_prediction(cam, d_old, rgb_old)
    od = orc.Odometry(W, H, cam.cx, cam.cy, cam.fx, cam.fy)
    od.init_icp_model(f32(v_old), f32(n_old), fed)
    od.init_rgb_model(img_old)
    v, n = orc.copy_maps(f32(v_act), f32(n_act))
    vs, ns = [v], [n]
    for _ in range(2):
        vs.append(orc.resize_map(vs[-1], False)); ns.append(orc.resize_map(ns[-1], True))
    od.init_rgb(img_act)
    ds = [orc.vertices_to_depth(f32(v_act), MAX_DEPTH_RGB)]
    for _ in range(2):
        ds.append(orc.pyrdown_gauss_f32(ds[-1]))
    for level in range(3):
        for which, arr in ((0, vs[level]), (1, ns[level]), (5, ds[level])):
            arr = np.ascontiguousarray(arr, f32)
            C.memmove(orc.lib.orc_odom_buffer(C.c_void_p(od.h_), which, level), arr.ctypes.data, arr.nbytes)
    tr, rot, st = od.track(fed[:3, 3], fed[:3, :3], rgb_only=False, icp_weight=10.0, pyramid=True, fast_odom=False, so3=False)
    est = np.eye(4, dtype=f32)
    est[:3, :3] = np.asarray(rot, f32).reshape(3, 3); est[:3, 3] = np.asarray(tr, f32)
    return fed, est, st
