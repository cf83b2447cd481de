"""GPU suite of loop closure in the frame loop (cofusion_set_loop_closure): a camera that returns with drift.

Scenario.  synth.Scene(n_obj=0, seed=1234) at 640x480, noise off, the camera at (0, 0, 0.9) turning about the vertical axis by 3 degrees per
frame, up to 450 degrees.  Frames are fed in pose-input mode at poses whose yaw is 1.012 x the true yaw, so a view that returns after a
full turn sits 4.32 degrees from where the map has it: about 0.14 m at the walls, which the 0.06 gate needs (pins count in the mean
constraint error, so the non-pin constraints must be more than 0.12 m off).  reloc = 1, set_relocalisation(min_age=60),
set_loop_closure(sample_rate=10000): at the reference's 25 000 the first frame's nodes of this noise-free room are collinear and the
normal equations singular (tests/test_cpu_loop_ref.py).  time_delta = 60 ticks: a wall leaves the 62-degree view after 21 frames and
comes back 99 frames later, so the first pass is inactive when the camera returns and the return view fuses fresh surfels next to the
old ones; without them the newest graph nodes are metres from the constraint points.  max_surfels 2^22 (about 3 M are fused).

The run stops feeding poses at the first accepted graph.  The map before that closure is the map of the same sequence without the
setter at the same frame (the gate changes no map, which the byte comparison of the two switched-off runs with each other and of
their counts with the closure run's shows).

The pose check.  The turn is about the camera's own centre, so the injected drift has no translation: it is the rotation of 4.32
degrees, and at the surface the displacement 2 x mean_cons_error_before.  The corrected pose must be within a quarter of the rotation
of (keyframe pose . true relative motion) and its translation within a quarter of the surface displacement."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
TURN_DEG, DRIFT, LAST = 3.0, 1.012, 150
MIN_AGE, RATE, TIME_DELTA = 60, 10000, 60
EYE_AT = (0.0, 0.0, 0.9)


def yaw_pose(deg):
    from co_fusion_amd import synth
    T = np.eye(4)
    T[:3, :3] = synth._rot_axis([0, 1, 0], math.radians(deg))
    T[:3, 3] = EYE_AT
    return T


def angle_between(a, b):
    r = np.asarray(a, np.float64)[:3, :3].T @ np.asarray(b, np.float64)[:3, :3]
    return math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(r) - 1) / 2))))


@pytest.fixture(scope="module")
def views():
    """the rendered views, once: the true view of frame k is the view of frame k mod 120"""
    from co_fusion_amd import synth
    scene = synth.Scene(n_obj=0, seed=1234)
    scene.camera_pose = lambda t: yaw_pose(TURN_DEG * t)
    cam = synth.Camera()
    cache = {}

    def view(k):
        if k % 120 not in cache:
            d, rgb, _, _ = scene.render(cam, k % 120, noise=False)
            cache[k % 120] = (d, rgb)
        return cache[k % 120]
    return view


def run(views, mode, stop=None):
    """mode 'on' / 'off' (the setter called, then switched off) / 'never'.  Feeds frames 0 .. stop (or up to the first accepted graph)
    -> rows per frame, the map after the last fed frame, the loop statistics, and for 'on' the state after two tracked frames"""
    from co_fusion_amd import facade
    cf = facade.CoFusion(reloc=1, enable_multiple_models=0, max_models=2, max_surfels=1 << 22, time_delta=TIME_DELTA)
    try:
        cf.set_relocalisation(True, min_age=MIN_AGE, seed=3)
        if mode != "never":
            cf.set_loop_closure(True, sample_rate=RATE)
        if mode == "off":
            cf.set_loop_closure(False)
        rows = []
        for k in range(LAST + 1 if stop is None else stop + 1):
            d, rgb = views(k)
            cf.process_frame(d, rgb, timestamp=k, in_pose=yaw_pose(DRIFT * TURN_DEG * k))
            info = cf.model_info(0)
            rows.append(dict(tick=cf.tick, pose=info["pose"].copy(), count=info["count"]))
            if mode == "on" and cf.loop_stats()["accepted"]:
                break
        out = dict(rows=rows, map=cf.model_download(0), stats=cf.loop_stats(), reloc=cf.reloc_stats())
        if mode == "on":
            later = []
            for k in range(len(rows), len(rows) + 2):
                d, rgb = views(k)
                cf.process_frame(d, rgb, timestamp=k)
                later.append(dict(tick=cf.tick, count=cf.model_info(0)["count"], lost=cf.lost))
            out["later"] = later
        return out
    finally:
        cf.close()


@pytest.fixture(scope="module")
def runs(views):
    on = run(views, "on")
    stop = len(on["rows"]) - 1
    return dict(on=on, off=run(views, "off", stop), never=run(views, "never", stop), stop=stop)


def test_the_returning_camera_closes_the_loop(runs):
    on, stop = runs["on"], runs["stop"]
    s = on["stats"]
    print("stats", s, "reloc", on["reloc"], "closing frame", stop, "surfels", len(on["map"]))
    assert s["accepted"] >= 1 and s["fern_accepts"] >= 1 and s["candidates"] >= s["fern_accepts"] and s["gated"] >= s["candidates"]
    assert s["last_tick"] == on["rows"][stop]["tick"] - 1 and 5 <= s["last_nodes"] <= 1024
    r = s["last"]
    assert r["optimised"] and r["accepted"] and not r["failed"]
    assert r["mean_cons_error"] < 3e-4 and r["error"] < 0.12 and r["mean_cons_error_before"] >= 0.06
    # the keyframe is the view of a full turn earlier
    kf_time = keyframe_time(runs)
    true_now, true_kf = TURN_DEG * stop, TURN_DEG * (kf_time - 1)
    print("keyframe", s["last_keyframe"], "time", kf_time, "true views", true_now, true_kf)
    apart = (true_now - true_kf) % 360.0
    assert stop - (kf_time - 1) > MIN_AGE and min(apart, 360.0 - apart) <= 6.0


def keyframe_time(runs):
    """srcTime of the keyframe the closure matched: a tick, one more than the number of the frame it was made from"""
    return runs["on"]["stats"]["last_keyframe_time"]


def test_the_pose_is_corrected(runs):
    on, stop = runs["on"], runs["stop"]
    fed = yaw_pose(DRIFT * TURN_DEG * stop)
    kf_frame = keyframe_time(runs) - 1
    want = yaw_pose(DRIFT * TURN_DEG * kf_frame) @ np.linalg.inv(yaw_pose(TURN_DEG * kf_frame)) @ yaw_pose(TURN_DEG * stop)   # keyframe pose . true relative motion
    want[:3, 3] = EYE_AT   # (the turn is about the camera's centre)
    got = on["rows"][stop]["pose"]
    injected = angle_between(fed, want)
    surface = 2.0 * float(on["stats"]["last"]["mean_cons_error_before"])
    print("injected rotation", injected, "left", angle_between(got, want), "translation off", np.linalg.norm(got[:3, 3] - want[:3, 3]), "surface drift", surface)
    assert injected > 3.0
    assert angle_between(got, want) <= injected / 4
    assert np.linalg.norm(got[:3, 3] - want[:3, 3]) <= surface / 4


def test_the_map_moves_where_it_is_new_and_stays_where_it_is_pinned(runs):
    before, after = runs["never"]["map"], runs["on"]["map"]
    assert len(before) == len(after) and after.tobytes() != before.tobytes()
    assert np.array_equal(after[:, [3, 4, 5, 6, 11]], before[:, [3, 4, 5, 6, 11]])   # confidence, colour, init_time, radius
    move = np.linalg.norm(after[:, 0:3] - before[:, 0:3], axis=1)
    drift = 2.0 * float(runs["on"]["stats"]["last"]["mean_cons_error_before"])      # mean |dst - src| of the non-pin constraints
    born = before[:, 6]
    now, kf = runs["on"]["stats"]["last_tick"], keyframe_time(runs)
    fresh, pinned = born > now - 5, np.abs(born - kf) <= 5
    print("drift", drift, "fresh", fresh.sum(), move[fresh].mean(), "pinned", pinned.sum(), move[pinned].mean())
    assert fresh.sum() > 1000 and pinned.sum() > 1000
    assert 0.5 * drift <= move[fresh].mean() <= 1.5 * drift
    assert move[pinned].mean() < 0.1 * drift
    assert np.abs(np.linalg.norm(after[:, 8:11], axis=1) - 1).max() < 1e-4


def test_the_frame_loop_goes_on(runs):
    on, stop = runs["on"], runs["stop"]
    later = on["later"]
    print("later", later)
    assert later[-1]["tick"] == on["rows"][stop]["tick"] + 2 and not later[-1]["lost"]
    assert later[-1]["count"] >= on["rows"][stop]["count"]


def test_switched_off_is_the_frame_loop_without_the_setter(runs):
    off, never, on = runs["off"], runs["never"], runs["on"]
    assert off["stats"]["gated"] == 0 and never["stats"]["gated"] == 0
    assert off["map"].tobytes() == never["map"].tobytes()
    for i, (a, b, c) in enumerate(zip(off["rows"], never["rows"], on["rows"])):
        assert a["tick"] == b["tick"] == c["tick"] and a["count"] == b["count"] == c["count"], i
        assert a["pose"].tobytes() == b["pose"].tobytes(), i
    assert off["reloc"] == never["reloc"]


def test_refusals():
    from co_fusion_amd import facade
    kw = dict(enable_multiple_models=0, max_models=2, max_surfels=1 << 16)
    cf = facade.CoFusion(128, 64, 100.0, 100.0, 64.0, 32.0, reloc=1, **kw)
    try:
        with pytest.raises(facade.CoFusionError, match="setRelocalisation"):
            cf.set_loop_closure(True)
        cf.set_relocalisation(True, n_ferns=99)
        with pytest.raises(facade.CoFusionError, match="fern count"):
            cf.set_loop_closure(True)
        cf.set_relocalisation(True, n_ferns=127)
        cf.set_loop_closure(True, sample_rate=RATE)
        assert cf.loop_stats()["gated"] == 0 and cf.loop_stats()["last_keyframe"] == -1
        cf.set_loop_closure(False)
    finally:
        cf.close()
    g = facade.CoFusionGroup(2, 128, 64, 100.0, 100.0, 64.0, 32.0, **kw)
    try:
        with pytest.raises(facade.CoFusionError, match="group"):
            g.sequences[0].set_loop_closure(True)
    finally:
        g.close()
