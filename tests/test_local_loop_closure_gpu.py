"""GPU suite of local loop closure in the frame loop (cofusion_set_local_loop_closure, DESIGN.md 4.14 "The local half"): a camera that
returns with a drift too small for the global path.

Scenario (tests/local_loop_scene.py): the room and the yaw turn of tests/test_loop_closure_gpu.py, no fern database, time_delta = 60,
poses fed at DRIFT = 1.004 x the true yaw: 1.44 degrees after a full turn, about 0.05 m at the walls -- inside the tracker's 0.10 m gate
and far below the 0.12 m the global path's 0.06 gate needs.  The first pass's surface comes back into view from frame 100 on.

Three runs of the same frames, which are bit-identical where they do the same (the existing scenario relies on that too):
  A      the switch on, up to the second accepted closure (at most MAX_FRAMES frames);
  never  no setter, up to the frame of A's first closure: the map that closure found;
  B      as A up to the frame before A's second closure, then switched off for that frame: the map the second closure found.

The oracle's figures for the chosen drift (tests/test_cpu_local_loop_ref.py::test_the_scenarios_drift_registers_and_is_accepted, frame 105
on ideal predictions): rotation left 0.200 of 1.440 degrees, translation off 1e-4 m, ICP error 7.4e-6, count 294 993, largest covariance
diagonal 4.5e-6 -- accepted by the default thresholds (1e-5, 40 000, 5e-5)."""
import numpy as np
import pytest

import local_loop_scene as sc

pytestmark = pytest.mark.gpu
f32 = np.float32
MAX_FRAMES = 240
KW = dict(enable_multiple_models=0, max_models=2, max_surfels=1 << 22, time_delta=sc.TIME_DELTA, conf_global_init=sc.CONF)


def feed(cf, views, k):
    d, rgb = views(k)
    cf.process_frame(d, rgb, timestamp=k, in_pose=sc.yaw_pose(sc.DRIFT * sc.TURN_DEG * k))


def run_on(views, closures, switch_off_at=None):
    """frames until `closures` local closures have been accepted -> per-frame rows, the maps after each closing frame"""
    from co_fusion_amd import facade
    cf = facade.CoFusion(**KW)
    try:
        cf.set_local_loop_closure(True, sample_rate=sc.RATE)
        rows, maps = [], []
        for k in range(MAX_FRAMES):
            if k == switch_off_at:
                cf.set_local_loop_closure(False)
            feed(cf, views, k)
            s = cf.local_loop_stats()
            rows.append(dict(tick=cf.tick, pose=cf.model_info(0)["pose"].copy(), stats=s))
            if k == switch_off_at:
                maps.append(cf.model_download(0))
                break
            if s["deforms"] > len(maps):
                maps.append(cf.model_download(0))
            if len(maps) == closures:
                break
        return dict(rows=rows, maps=maps)
    finally:
        cf.close()


def run_never(views, stop):
    from co_fusion_amd import facade
    cf = facade.CoFusion(**KW)
    try:
        for k in range(stop + 1):
            feed(cf, views, k)
        return cf.model_download(0)
    finally:
        cf.close()


@pytest.fixture(scope="module")
def runs():
    views = sc.make_views()
    a = run_on(views, 2)
    deforms = [r["stats"]["deforms"] for r in a["rows"]]
    closing = [k for k in range(len(deforms)) if deforms[k] > (deforms[k - 1] if k else 0)]
    for k, r in enumerate(a["rows"]):
        s = r["stats"]
        if s["examined"] and (s["last_covered"] or s["last_tracker_accepted"]):
            print(k, "covered", s["last_covered"], "accepted", s["last_tracker_accepted"], "err %.3g count %.0f cov %.3g" %
                  (s["last_icp_error"], s["last_icp_count"], s["last_max_covariance"]), "deforms", s["deforms"], "cons", s["last_constraints"], "nodes", s["last_nodes"])
    out = dict(a=a, closing=closing)
    if closing:
        out["before_first"] = run_never(views, closing[0])
    if len(closing) > 1:
        out["before_second"] = run_on(views, 2, switch_off_at=closing[1])["maps"][-1]
    return out


def test_a_local_closure_is_accepted_and_none_before_the_old_surface_is_in_view(runs):
    rows, closing = runs["a"]["rows"], runs["closing"]
    print("closing frames", closing, "last stats", rows[-1]["stats"])
    assert len(closing) >= 1
    for k, r in enumerate(rows):
        s = r["stats"]
        if k < 99:   # the view of frame k reaches the view of frame 0 when 3 k + 31 >= 360 - 31
            assert s["tracker_accepts"] == 0 and s["deforms"] == 0, k
        # the clock: nothing can be inactive before tick time_delta + 1, and every later frame is examined (no fern seam here)
        assert s["examined"] == max(0, k + 1 - sc.TIME_DELTA), k
    assert closing[0] >= 99


def test_the_stats_are_consistent(runs):
    rows, closing = runs["a"]["rows"], runs["closing"]
    prev = None
    for k, r in enumerate(rows):
        s = r["stats"]
        assert s["deforms"] == s["accepted"] <= s["optimised"] <= s["tracker_accepts"] <= s["examined"] - s["skipped_by_gate"], k
        assert s["failed"] + s["accepted"] <= s["optimised"], k
        if k in closing:
            assert s["last_deform_time"] == s["last_tick"] == r["tick"] - 1, k
            assert s["last"]["optimised"] and s["last"]["accepted"] and not s["last"]["failed"], k
            assert 5 <= s["last_nodes"] <= 1024 and 1 <= s["last_constraints"] <= 1536, k
            assert s["last_tracker_accepted"] and s["last_covered"] >= 40000, k
            assert s["last_icp_count"] > 40000 and s["last_icp_error"] < 5e-5 and s["last_max_covariance"] <= 1e-5, k
        elif prev is not None:
            assert s["last_deform_time"] == prev["last_deform_time"] and s["deforms"] == prev["deforms"], k
        prev = s


def test_pins_are_used_for_the_first_closure_only(runs):
    rows, closing = runs["a"]["rows"], runs["closing"]
    assert len(closing) >= 2
    first, second = rows[closing[0]]["stats"], rows[closing[1]]["stats"]
    assert first["last_pinned"] and first["last_constraints"] % 2 == 0
    assert not second["last_pinned"]
    for k in range(closing[0] + 1, len(rows)):   # every tracker accept behind the first closure
        s = rows[k]["stats"]
        if s["last_tick"] == rows[k]["tick"] - 1:
            assert not s["last_pinned"], k


def test_the_pose_improves(runs):
    rows, k = runs["a"]["rows"], runs["closing"][0]
    fed, got, want = sc.yaw_pose(sc.DRIFT * sc.TURN_DEG * k), rows[k]["pose"], sc.wanted_pose(k)
    before, after = sc.angle_between(fed, want), sc.angle_between(got, want)
    print("frame", k, "rotation off before", before, "after", after, "translation off", np.linalg.norm(got[:3, 3] - want[:3, 3]))
    assert np.array_equal(f32(got), rows[k]["stats"]["last_est_pose"])
    assert after < before


def test_fresh_surfels_move_towards_their_targets(runs):
    k = runs["closing"][0]
    before, after = runs["before_first"], runs["a"]["maps"][0]
    s = runs["a"]["rows"][k]["stats"]
    assert len(before) == len(after) and after.tobytes() != before.tobytes()
    assert np.array_equal(after[:, [3, 4, 5, 6, 11]], before[:, [3, 4, 5, 6, 11]])   # confidence, colour, init_time, radius
    fresh = before[:, 6] > s["last_tick"] - 5
    # a constraint takes curr_pose . v to est_pose . v: the target of a fresh surfel p is est . curr^-1 . p
    M = np.float64(s["last_est_pose"]) @ np.linalg.inv(sc.yaw_pose(sc.DRIFT * sc.TURN_DEG * k))
    target = before[fresh, 0:3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    off_before = np.linalg.norm(before[fresh, 0:3] - target, axis=1).mean()
    off_after = np.linalg.norm(after[fresh, 0:3] - target, axis=1).mean()
    print("fresh", fresh.sum(), "mean distance to the target before", off_before, "after", off_after)
    assert fresh.sum() > 1000
    assert off_after < off_before


def test_old_surfels_in_view_are_reactivated(runs):
    k = runs["closing"][0]
    before, after = runs["before_first"], runs["a"]["maps"][0]
    tick = runs["a"]["rows"][k]["stats"]["last_tick"]
    old = before[:, 6] <= tick - sc.TIME_DELTA - 21   # born in the first pass over the wall that is back in view
    print("old", old.sum(), "stamped before", (before[old, 7] == tick).sum(), "after", (after[old, 7] == tick).sum())
    assert (before[old, 7] > tick - sc.TIME_DELTA).sum() == 0          # all inactive when the closure found them
    assert (after[old, 7] == tick).sum() > 1000
    assert np.isin(after[old, 7], (tick,)).sum() + (after[old, 7] == before[old, 7]).sum() == old.sum()


def test_surfels_older_than_the_last_deformation_stay_exactly_still(runs):
    closing = runs["closing"]
    assert len(closing) >= 2
    before, after = runs["before_second"], runs["a"]["maps"][1]
    ldt = runs["a"]["rows"][closing[0]]["stats"]["last_deform_time"]
    s = runs["a"]["rows"][closing[1]]["stats"]
    assert len(before) == len(after)
    # the nodes are every stride-th surfel of the map the closure found, in time order; a surfel is moved by nodes out of a window of at
    # most 20 consecutive nodes around its own time, so a surfel born before the 20th node below the first enabled one reaches none
    stride = sc.RATE * -(-len(before) // (sc.RATE * 1024))
    node_time = before[::stride, 6]
    assert len(node_time) == s["last_nodes"] and np.all(np.diff(node_time) >= 0)
    first_enabled = int(np.searchsorted(node_time, ldt, side="right"))
    assert 20 <= first_enabled < len(node_time)
    old = before[:, 6] < node_time[first_enabled - 20]
    young = before[:, 6] > ldt
    moved = np.any(after[:, [0, 1, 2, 8, 9, 10]] != before[:, [0, 1, 2, 8, 9, 10]], axis=1)
    print("second closure at frame", closing[1], "last_deform_time before it", ldt, "old", old.sum(), "of them moved", moved[old].sum(),
          "young", young.sum(), "of them moved", moved[young].sum())
    assert old.sum() > 100000 and moved[old].sum() == 0
    assert moved[young].sum() > 0


def test_refusals():
    from co_fusion_amd import facade
    kw = dict(enable_multiple_models=0, max_models=2, max_surfels=1 << 16)
    cf = facade.CoFusion(128, 64, 100.0, 100.0, 64.0, 32.0, **kw)
    try:
        with pytest.raises(facade.CoFusionError, match="timeDelta"):
            cf.set_local_loop_closure(True)
    finally:
        cf.close()
    cf = facade.CoFusion(128, 64, 100.0, 100.0, 64.0, 32.0, time_delta=60, **kw)
    try:
        cf.set_local_loop_closure(True)      # needs no fern database
        s = cf.local_loop_stats()
        assert s["examined"] == 0 and s["deforms"] == 0 and s["last_deform_time"] == 0 and s["last_tick"] == -1
        cf.set_local_loop_closure(False)
    finally:
        cf.close()
    cf = facade.CoFusion(128, 64, 100.0, 100.0, 64.0, 32.0, rank=0, world=2, time_delta=60, **kw)
    try:
        with pytest.raises(facade.CoFusionError, match="single-GPU"):
            cf.set_local_loop_closure(True)
    finally:
        cf.close()
    g = facade.CoFusionGroup(2, 128, 64, 100.0, 100.0, 64.0, 32.0, time_delta=60, **kw)
    try:
        with pytest.raises(facade.CoFusionError, match="group"):
            g.sequences[0].set_local_loop_closure(True)
    finally:
        g.close()
