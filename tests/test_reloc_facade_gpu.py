"""GPU suite of the relocalisation switch of the facade (cofusion_set_relocalisation): a 640x480 static room with reloc = 1.  A short
smooth approach builds keyframes, twelve frames that jump between the opposite wall and a side wall make the camera lost (the ten-frame rule of CoFusion.cpp:312-317
needs eleven), then three views that continue the approach.  The approach is fed with its ground-truth poses (the reference's
pose-input mode), so the keyframes sit at known poses and the recovered pose can be held against the ground truth without the drift of
a tracked approach; every later frame is tracked.  With the switch on the camera recovers; with it off the frame loop is
what it is without the setter, frame for frame."""
import numpy as np
import pytest

import ferns_scene as fs

pytestmark = pytest.mark.gpu

APPROACH = tuple(range(0, 24, 3))      # 8 frames
FAR_FRAMES = 12
NEAR = (22, 23, 24)
# (the far views alternate between two unrelated viewpoints: a repeated view would track against its own fill-in and count as good)
FRAMES = APPROACH + ("far", "far2") * (FAR_FRAMES // 2) + NEAR


def run(mode):
    """mode: "on", "off" (the setter called with on = 0) or "never".  -> per frame dict(lost, tick, pose, count) + final stats"""
    from co_fusion_amd import facade
    c = fs.CAM
    cf = facade.CoFusion(fs.W, fs.H, c.fx, c.fy, c.cx, c.cy, reloc=1, enable_multiple_models=0, max_models=2, max_surfels=1 << 20)
    try:
        if mode == "on":
            cf.set_relocalisation(True, n_ferns=500, fern_threshold=0.05, photo_threshold=115.0, min_age=3, seed=11, capacity=64)
        elif mode == "off":
            cf.set_relocalisation(False)
        rows = []
        for i, t in enumerate(FRAMES):
            d, rgb, gt = fs.view(t)
            cf.process_frame(d, rgb, timestamp=i, in_pose=gt if i < len(APPROACH) else None)
            info = cf.model_info(0)
            rows.append(dict(lost=cf.lost, tick=cf.tick, pose=info["pose"].copy(), count=info["count"]))
        return rows, cf.reloc_stats()
    finally:
        cf.close()


@pytest.fixture(scope="module")
def runs():
    return {m: run(m) for m in ("on", "off", "never")}


def test_a_lost_camera_recovers(runs):
    rows, stats = runs["on"]
    n0 = len(APPROACH) + FAR_FRAMES
    print("stats", stats, "lost", [int(r["lost"]) for r in rows], "counts", [r["count"] for r in rows])
    print("approach pose errors", [fs.pose_error(rows[i]["pose"], fs.view(FRAMES[i])[2]) for i in range(len(APPROACH))])
    assert rows[n0 - 1]["lost"], "the far views did not make the camera lost"
    assert stats["keyframes"] >= 2 and not stats["database_full"]
    assert not rows[n0 + 2]["lost"], "still lost three frames after the views returned"
    assert stats["recoveries"] >= 1 and stats["last_closest"] >= 0
    back = next(i for i in range(n0, len(rows)) if not rows[i]["lost"])
    assert rows[-1]["count"] > rows[n0 - 1]["count"] or rows[back]["count"] > rows[n0 - 1]["count"], "fusion did not resume"
    assert rows[-1]["tick"] > rows[n0 - 1]["tick"], "the clock did not resume"
    for i in range(back, len(rows)):
        dt, dr = fs.pose_error(rows[i]["pose"], fs.view(FRAMES[i])[2])
        print("frame", i, "pose error", dt, dr)
    for i in range(back, len(rows)):
        dt, dr = fs.pose_error(rows[i]["pose"], fs.view(FRAMES[i])[2])
        assert dt < fs.POSE_BOUND_M and dr < fs.POSE_BOUND_DEG, (i, dt, dr)


def test_switch_off_is_the_frame_loop_without_the_setter(runs):
    off, off_stats = runs["off"]
    never, never_stats = runs["never"]
    assert off[-1]["lost"] and never[-1]["lost"]
    assert off_stats == never_stats == dict(keyframes=0, last_closest=-1, recoveries=0, database_full=False)
    for i, (a, b) in enumerate(zip(off, never)):
        assert a["lost"] == b["lost"] and a["tick"] == b["tick"] and a["count"] == b["count"], i
        assert a["pose"].tobytes() == b["pose"].tobytes(), i
    # ... and until the camera is lost the database only listens: the run with the switch on has the same poses and counts
    on, _ = runs["on"]
    first_lost = next(i for i, r in enumerate(never) if r["lost"])
    assert first_lost > len(APPROACH)
    for i in range(first_lost):
        assert on[i]["lost"] == never[i]["lost"] and on[i]["count"] == never[i]["count"] and on[i]["pose"].tobytes() == never[i]["pose"].tobytes(), i


def test_setter_is_refused_where_the_header_says():
    from co_fusion_amd import facade
    c = fs.CAM
    cf = facade.CoFusion(fs.W, fs.H, c.fx, c.fy, c.cx, c.cy, reloc=0, enable_multiple_models=0, max_models=2, max_surfels=1 << 16)
    try:
        with pytest.raises(facade.CoFusionError, match="reloc"):
            cf.set_relocalisation(True)
    finally:
        cf.close()
    g = facade.CoFusionGroup(2, 128, 64, 100.0, 100.0, 64.0, 32.0, reloc=1, enable_multiple_models=0, max_models=2, max_surfels=1 << 16)
    try:
        with pytest.raises(facade.CoFusionError, match="group"):
            g.sequences[0].set_relocalisation(True)
    finally:
        g.close()
