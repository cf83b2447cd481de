"""GPU suite of relative constraints at the facade (cofusion_set_relative_constraints and its companions, DESIGN.md 4.14 "Relative rows").

deform_background at 160x128: six frames of synth.Scene fused at their ground-truth poses, a graph of every 500th surfel, forty
constraints that shift the map by 0.07 m and three stored pairs seeded through cofusion_add_relative_constraints.  The entry must give
the map and the outcome the cf_deform_* calls give on a copy of the map (those are held against the numpy statement in
test_deform_rel_gpu.py); with the switch off again, or never on, it gives today's bytes.

The frame loop on tests/local_loop_scene.py (unchanged): with both switches on, the first accepted local closure leaves the picks of its
constraints in the store and the statistics count them.  The closure's rows, its target times and its accepted graph are read back
(cofusion_local_closure_download) and the stored pairs are exactly deform_rel_ref.closure_pairs of them, bit for bit; the moved sources
lie nearer their targets than the fed pose put them."""
import numpy as np
import pytest

import deform_rel_ref as rel
import local_loop_scene as sc

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 160, 128
FRAMES = tuple(range(0, 18, 3))
RATE = 500
SHIFT = f32([0.07, 0.0, 0.0])


def _cam():
    from co_fusion_amd import synth
    return synth.Camera.scaled(W, H)


def _open():
    from co_fusion_amd import facade
    c = _cam()
    return facade.CoFusion(W, H, c.fx, c.fy, c.cx, c.cy, enable_multiple_models=0, max_models=2, max_surfels=1 << 18)


def _run(frames, mode):
    """mode "pairs": the switch on and three pairs stored; "off": the same, then switched off; "never": no call at all"""
    cf = _open()
    try:
        for i, (d, rgb, gt) in enumerate(frames):
            cf.process_frame(d, rgb, timestamp=i, in_pose=gt)
        before = cf.model_download(0)
        pick = np.linspace(0, len(before) - 1, 40).astype(np.int64)
        src = before[pick, 0:3].copy(); tm = before[pick, 6].copy()
        at = np.array([len(before) // 7, len(before) // 2, len(before) - 9])
        to = np.array([5, len(before) // 3, len(before) // 5])
        pairs = np.concatenate([before[at, 0:3], before[at, 6:7], before[at, 0:3] + f32([0.002, -0.001, 0.001]), before[to, 6:7]], 1).astype(f32)
        stats = []
        if mode != "never":
            cf.set_relative_constraints(True)
            stats.append(cf.relative_stats())
            cf.add_relative_constraints(pairs[:2, 0:3], pairs[:2, 4:7], pairs[:2, 3], pairs[:2, 7])
            cf.add_relative_constraints(pairs[2:, 0:3], pairs[2:, 4:7], pairs[2:, 3], pairs[2:, 7])
            stats.append(cf.relative_stats())
            stored = cf.relative_constraints()
        else:
            stored = None
        if mode == "off":
            cf.set_relative_constraints(False)
        out = cf.deform_background(src, src + SHIFT, tm, sample_rate=RATE)
        after = cf.model_download(0)
        if mode == "pairs":
            stats.append(cf.relative_stats())
        return dict(before=before, src=src, tm=tm, pairs=pairs, stored=stored, out=out, after=after, stats=stats)
    finally:
        cf.close()


@pytest.fixture(scope="module")
def runs():
    from co_fusion_amd import synth
    scene = synth.Scene(n_obj=0, seed=1234)
    cam = _cam()
    frames = []
    for t in FRAMES:
        d, rgb, _, pose = scene.render(cam, t, noise=False)
        frames.append((d, rgb, pose))
    return {m: _run(frames, m) for m in ("pairs", "off", "never")}


def test_the_store_takes_caller_supplied_pairs(runs):
    r = runs["pairs"]
    assert r["stats"][0] == dict(appended=0, overwritten=0, stored=0, used_by_last_closure=0, last_picked=0)
    assert r["stats"][1] == dict(appended=3, overwritten=0, stored=3, used_by_last_closure=0, last_picked=0)
    assert r["stored"].tobytes() == r["pairs"].tobytes()
    assert r["stats"][2]["used_by_last_closure"] == 3 and r["stats"][2]["stored"] == 3


def test_the_pairs_count_below_the_line_and_the_closure_is_accepted(runs):
    o, plain = runs["pairs"]["out"], runs["never"]["out"]
    print("with pairs", o, "\nwithout", plain)
    assert runs["pairs"]["before"].tobytes() == runs["never"]["before"].tobytes()
    assert abs(plain["mean_cons_error_before"] - 0.07) < 1e-5
    assert abs(o["mean_cons_error_before"] - 0.07 * 40 / 43) < 1e-5            # 40 absolute constraints over 43 constraints in all
    assert o["optimised"] and o["accepted"] and not o["failed"] and o["error_before"] > plain["error_before"]
    move = runs["pairs"]["after"][:, 0:3] - runs["pairs"]["before"][:, 0:3]
    assert np.linalg.norm(move - SHIFT, axis=1).mean() < 1e-3


def test_the_entry_equals_the_deform_calls_on_a_copy(runs):
    from co_fusion_amd import api, deform
    r = runs["pairs"]
    c = _cam()
    ctx = api.Context(W, H, c.fx, c.fy, c.cx, c.cy, max_models=2, max_surfels=1 << 16)
    d = deform.Deform(ctx)
    try:
        d.enable_relative()
        dev = ctx.to_device(r["before"])
        n, stride, mono = d.sample(dev, RATE)
        assert (n, stride, mono) == (r["out"]["nodes"], RATE, True) and n >= 20
        d.weights(r["src"], r["src"] + SHIFT, r["tm"])
        d.set_relative(r["pairs"])
        got = d.optimise()
        for k in deform.RESULT_FIELDS:
            assert np.asarray(got[k]).tobytes() == np.asarray(type(got[k])(r["out"][k])).tobytes(), k
        d.apply(dev)
        ctx.synchronize()
        cols = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11]
        assert dev.cpu().numpy()[:, cols].tobytes() == r["after"][:, cols].tobytes()
    finally:
        d.close()
        ctx.close()


def test_switched_off_it_is_todays_result(runs):
    off, never = runs["off"], runs["never"]
    assert off["out"] == never["out"]
    assert off["after"].tobytes() == never["after"].tobytes()
    assert runs["pairs"]["after"].tobytes() != never["after"].tobytes()


def test_refusals():
    from co_fusion_amd import facade
    cf = _open()
    try:
        p = np.zeros((1, 3), f32)
        with pytest.raises(facade.CoFusionError, match="setRelativeConstraints"):
            cf.add_relative_constraints(p, p, [1], [1])
        assert len(cf.relative_constraints()) == 0 and cf.relative_stats()["stored"] == 0
        cf.set_relative_constraints(True)
        with pytest.raises(facade.CoFusionError, match="pairs"):
            cf.add_relative_constraints(np.zeros((129, 3), f32), np.zeros((129, 3), f32), np.zeros(129), np.zeros(129))
    finally:
        cf.close()
    g = facade.CoFusionGroup(2, 128, 64, 100.0, 100.0, 64.0, 32.0, enable_multiple_models=0, max_models=2, max_surfels=1 << 16)
    try:
        with pytest.raises(facade.CoFusionError, match="group"):
            g.sequences[0].set_relative_constraints(True)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ the frame loop
def test_an_accepted_local_closure_leaves_its_picks_in_the_store():
    from co_fusion_amd import facade
    views = sc.make_views()
    cf = facade.CoFusion(enable_multiple_models=0, max_models=2, max_surfels=1 << 22, time_delta=sc.TIME_DELTA, conf_global_init=sc.CONF)
    try:
        cf.set_local_loop_closure(True, sample_rate=sc.RATE)
        cf.set_relative_constraints(True)
        closing = None
        for k in range(240):
            d, rgb = views(k)
            cf.process_frame(d, rgb, timestamp=k, in_pose=sc.yaw_pose(sc.DRIFT * sc.TURN_DEG * k))
            s = cf.local_loop_stats()
            if s["deforms"]:
                closing = k
                break
            assert cf.relative_stats()["appended"] == 0, k
        assert closing is not None and closing >= 99
        n = s["last_constraints"] // (2 if s["last_pinned"] else 1)
        picks = len(rel.pick_indices(n))
        rs = cf.relative_stats()
        print("closing frame", closing, "constraints", n, "stats", rs)
        assert s["last_pinned"] and n >= 3 and picks in (3, 4)
        assert rs == dict(appended=picks, overwritten=0, stored=picks, used_by_last_closure=0, last_picked=picks)
        pairs = cf.relative_constraints()
        assert pairs.shape == (picks, 8)
        # exactly the statement's picks of that closure's rows, moved by that closure's accepted graph
        cl = cf.local_closure()
        assert cl["pinned"] and len(cl["src"]) == s["last_constraints"] and len(cl["target_time"]) == n and len(cl["nodes"]) == s["last_nodes"]
        assert np.array_equal(cl["src"][1::2], cl["dst"][1::2]) and np.array_equal(cl["time"][1::2], cl["target_time"])      # the pin rows
        want = rel.closure_pairs(cl["src"], cl["dst"], cl["time"], cl["target_time"], True, cl["nodes"], cl["params"], cl["last_deform_time"])
        assert pairs.tobytes() == want.tobytes()
        assert (pairs[:, 3] == s["last_tick"]).all()                              # srcTime: the closing frame's tick
        assert (pairs[:, 7] >= 1).all() and (pairs[:, 7] <= s["last_tick"] - sc.TIME_DELTA).all() and (pairs[:, 7] == np.round(pairs[:, 7])).all()
        # target = est * p and the un-moved source = fed pose * p for the same camera point p: the accepted graph moved the source towards it
        est = s["last_est_pose"].astype(np.float64); fed = sc.yaw_pose(sc.DRIFT * sc.TURN_DEG * closing)
        p = (np.linalg.inv(est) @ np.concatenate([pairs[:, 4:7], np.ones((picks, 1))], 1).T).T
        unmoved = (fed @ p.T).T[:, :3]
        gap_before = np.linalg.norm(unmoved - pairs[:, 4:7], axis=1); gap_after = np.linalg.norm(pairs[:, 0:3].astype(np.float64) - pairs[:, 4:7], axis=1)
        print("gap before", gap_before, "after", gap_after)
        assert (gap_before > 1e-3).all() and (gap_after < gap_before).all()
    finally:
        cf.close()
