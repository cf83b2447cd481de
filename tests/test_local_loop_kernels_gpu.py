"""GPU suite: the splat passes of local loop closure (cf_model_predict_inactive, cf_model_synthesize_depth in csrc/cabi_model.hip; the
resolve modes of csrc/surf_splat_dev.h) at 256x160 against the CPU oracle on the crafted maps of tests/local_loop_cases.py.

Inactive prediction: bit for bit orc_combined_predict(time = 0, maxTime, timeDelta); the ACTIVE buffers byte-identical before and after;
the covered count exact; twice, identical bytes.  Depth synthesis: splat.vert + depth_splat.frag accept what the colour splat accepts
(one vertex stage, the same disc test and depth range), so its statement is the z channel of orc_combined_predict for the same
arguments: bit for bit, exactly 0 where nothing lands, and no other buffer of the model written.

The constraint stage (cf_local_loop_* in csrc/local_loop.hip) against tests/local_loop_ref.py: one named case per branch of the accept
rule and of the sampling (tests/local_loop_cases.py; 12 x 8 = 96 samples, two waves), record and rows exact, the covariance figure and
the coordinates bit for bit, twice each; and the tracker's result read from its device state after a real tracking call."""
import numpy as np
import pytest

import local_loop_cases as lc
import orc
import orc_pipeline as op

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = lc.SHAPE
POSE = np.eye(4, dtype=f32)
ACTIVE, OLD = (4, 5, 6, 7), (15, 16, 17, 18)


@pytest.fixture(scope="module")
def rig():
    from co_fusion_amd import api, model as M
    ctx = api.Context(W, H, *lc.CAM, max_models=2)
    m = M.Model(ctx, 1 << 12)
    yield ctx, m
    m.close()
    ctx.close()


def _oracle(surfels, conf, time, max_time, delta, pose=POSE):
    return op.combined_predict(surfels, pose, orc.Cam(*lc.CAM), W, H, lc.SPLAT_DEPTH, conf, time, max_time, delta)


def _same(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want).astype(got.dtype, copy=False).reshape(got.shape)
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1))[:5])


def test_no_inactive_prediction_yet_is_an_error():
    from co_fusion_amd import api, model as M
    ctx = api.Context(W, H, *lc.CAM, max_models=2)
    m = M.Model(ctx, 1 << 10)
    try:
        for which in OLD + (19,):
            with pytest.raises(api.CofusionError):
                m.tensor(which)
    finally:
        m.close(); ctx.close()


@pytest.mark.parametrize("kind", lc.SPLAT_MAPS)
def test_inactive_prediction_is_the_oracle_bit_for_bit(rig, kind):
    ctx, m = rig
    surfels = lc.splat_map(kind)
    want = _oracle(surfels, lc.SPLAT_CONF, 0, lc.MAX_TIME, lc.SPLAT_DELTA)
    m.upload_map(surfels)
    m.combined_predict(POSE, lc.SPLAT_DEPTH, lc.SPLAT_CONF, lc.TICK, lc.TICK, lc.SPLAT_DELTA)
    ctx.synchronize()
    active = [m.buffer(k).tobytes() for k in ACTIVE]
    for k, a in zip(ACTIVE, _oracle(surfels, lc.SPLAT_CONF, lc.TICK, lc.TICK, lc.SPLAT_DELTA)):
        _same(m.buffer(k), a, f"active {k}")
    runs = []
    for _ in range(2):
        m.predict_inactive(POSE, lc.SPLAT_DEPTH, lc.SPLAT_CONF, lc.MAX_TIME, lc.SPLAT_DELTA)
        covered = m.inactive_covered()
        got = [m.buffer(k) for k in OLD]
        for k, g, a in zip(OLD, got, want):
            _same(g, a, f"{kind}: buffer {k}")
        assert covered == int((want[3] > 0).sum()) and (kind == "all_active") == (covered == 0)
        assert [m.buffer(k).tobytes() for k in ACTIVE] == active
        assert not (m.buffer(14) != np.uint64(0xFFFFFFFFFFFFFFFF)).any()          # the z-buffer is left cleared for the next pass
        runs.append([g.tobytes() for g in got] + [covered])
    assert runs[0] == runs[1]


def test_inactive_prediction_from_another_pose(rig):
    ctx, m = rig
    surfels = lc.splat_map("mixed")
    pose = np.eye(4, dtype=f32)
    pose[:3, :3] = f32([[0.9950042, 0.0, 0.0998334], [0.0, 1.0, 0.0], [-0.0998334, 0.0, 0.9950042]])
    pose[:3, 3] = f32([0.125, -0.0625, 0.25])
    want = _oracle(surfels, lc.SPLAT_CONF, 0, lc.MAX_TIME, lc.SPLAT_DELTA, pose)
    m.upload_map(surfels)
    m.predict_inactive(pose, lc.SPLAT_DEPTH, lc.SPLAT_CONF, lc.MAX_TIME, lc.SPLAT_DELTA)
    for k, a in zip(OLD, want):
        _same(m.buffer(k), a, f"buffer {k}")
    assert m.inactive_covered() == int((want[3] > 0).sum()) > 1000


# (confidence, time, maxTime, timeDelta): what CoFusion.cpp:481 passes (everything not older than tick - timeDelta), the inactive set, and
# the full map
DEPTH_ARGS = [(lc.SPLAT_CONF, lc.TICK, lc.TICK - lc.SPLAT_DELTA, 65535), (lc.SPLAT_CONF, 0, lc.MAX_TIME, lc.SPLAT_DELTA), (0.0, lc.TICK, lc.TICK, 65535)]


@pytest.mark.parametrize("kind", lc.SPLAT_MAPS)
def test_depth_synthesis_is_the_z_channel_of_the_splat(rig, kind):
    ctx, m = rig
    surfels = lc.splat_map(kind)
    m.upload_map(surfels)
    m.combined_predict(POSE, lc.SPLAT_DEPTH, lc.SPLAT_CONF, lc.TICK, lc.TICK, lc.SPLAT_DELTA)
    m.predict_inactive(POSE, lc.SPLAT_DEPTH, lc.SPLAT_CONF, lc.MAX_TIME, lc.SPLAT_DELTA)
    ctx.synchronize()
    before = [m.buffer(k).tobytes() for k in ACTIVE + OLD] + [m.inactive_covered()]
    for conf, time, max_time, delta in DEPTH_ARGS:
        want = _oracle(surfels, conf, time, max_time, delta)
        z = np.ascontiguousarray(want[1][..., 2], f32)
        runs = []
        for _ in range(2):
            out = ctx.to_device(np.full((H, W), 7.0, f32))
            m.synthesize_depth(POSE, lc.SPLAT_DEPTH, conf, time, max_time, delta, out)
            ctx.synchronize()
            got = out.cpu().numpy()
            _same(got, z, f"{kind}: depth {conf, time, max_time, delta}")
            assert (got[want[3] == 0].view(np.uint32) == 0).all() and ((got > 0) == (z > 0)).all()
            runs.append(got.tobytes())
        assert runs[0] == runs[1]
    assert [m.buffer(k).tobytes() for k in ACTIVE + OLD] + [m.inactive_covered()] == before
    assert not (m.buffer(14) != np.uint64(0xFFFFFFFFFFFFFFFF)).any()


# ------------------------------------------------------------------------------------------------ the constraint stage
@pytest.fixture(scope="module")
def loop(rig):
    from co_fusion_amd import local_loop
    ctx, _ = rig
    l = local_loop.LocalLoop(ctx)
    yield ctx, l
    l.close()


def _run_constraints(ctx, l, track, v, t, pose, pin, th, covered=None):
    import local_loop_ref as lref
    want = lref.local_constraints(track, v, t, pose, lc.CONS_TICK, lc.CONS_MAX_DEPTH, pin, th)
    dv, dt = ctx.to_device(v), ctx.to_device(t)
    runs = []
    for _ in range(2):
        l.constraints_async(dv, dt, pose, lc.CONS_TICK, lc.CONS_MAX_DEPTH, pin, track=track, covered=covered, **th)
        rec = l.wait()
        assert rec["accepted"] == want["accepted"] and rec["n_constraints"] == want["n"]
        assert rec["est_pose"].tobytes() == want["est_pose"].tobytes()
        assert rec["icp_error"] == f32(track["icp_error"]) and rec["icp_count"] == f32(track["icp_count"])
        wc = want["max_covariance"]
        assert (np.isnan(rec["max_covariance"]) and np.isnan(wc)) or rec["max_covariance"] == wc      # f64, to the bit
        src, dst, tm = l.rows(want["n"])
        assert src.tobytes() == want["src"].tobytes() and dst.tobytes() == want["dst"].tobytes() and tm.tobytes() == want["time"].tobytes()
        runs.append((rec["accepted"], rec["n_constraints"], src.tobytes(), dst.tobytes(), tm.tobytes()))
    assert runs[0] == runs[1]
    return rec


@pytest.mark.parametrize("name", list(lc.ACCEPT_CASES))
def test_accept_rule(loop, name):
    ctx, l = loop
    track, th = lc.ACCEPT_CASES[name]
    v, t = lc.cons_maps("all_valid")
    rec = _run_constraints(ctx, l, track, v, t, lc.cons_pose(0), True, th)
    assert rec["accepted"] == lc.ACCEPT_WANT[name] and rec["n_constraints"] == (192 if lc.ACCEPT_WANT[name] else 0)


@pytest.mark.parametrize("pin", [False, True], ids=["no_pins", "pins"])
@pytest.mark.parametrize("kind", lc.SAMPLE_CASES)
def test_constraint_rows(loop, kind, pin):
    ctx, l = loop
    v, t = lc.cons_maps(kind)
    _run_constraints(ctx, l, lc.good_track(), v, t, lc.cons_pose(0), pin, {})


def test_constraint_rows_feed_the_graph_and_carry_the_covered_word(rig, loop):
    from co_fusion_amd import deform
    import deform_cases as dc
    import deform_ref as ref
    ctx, l = loop
    _, m = rig
    m.upload_map(lc.splat_map("mixed"))
    m.predict_inactive(POSE, lc.SPLAT_DEPTH, lc.SPLAT_CONF, lc.MAX_TIME, lc.SPLAT_DELTA)
    covered = m.inactive_covered()
    v, t = lc.cons_maps("old_time_zero")
    rec = _run_constraints(ctx, l, lc.good_track(), v, t, lc.cons_pose(0), True, {}, covered=m.tensor(19)[0])
    assert rec["covered"] == covered > 0
    # the rows go to a sized graph object without a host copy, and weigh as the same rows uploaded from the host
    n = rec["n_constraints"]
    src, dst, tm = l.rows(n)
    nodes = dc.make_nodes(21)
    d = deform.Deform(ctx, deform.MAX_CONSTRAINTS_SIZED)
    try:
        d.set_nodes(nodes)
        d.weights_device(*l.buffers(), n)
        got = d.download()
        ids, w, ok = ref.weights(nodes, src, tm)
        assert np.array_equal(got["ids"], ids) and got["weights"][ok].tobytes() == w[ok].tobytes()
    finally:
        d.close()


def test_constraints_read_the_trackers_result_on_the_device():
    """the tracker's pose and statistics are taken from its device state: the record carries what cf_odom_fetch_result returns"""
    import common
    from co_fusion_amd import api, local_loop
    import local_loop_ref as lref
    W2, H2 = 320, 240
    fp = common.frame_pair(W2, H2, noise=True)
    cam = fp["cam"]
    pose = common.perturbed_pose(2)
    ctx = api.Context(W2, H2, cam.fx, cam.fy, cam.cx, cam.cy)
    g = api.Odometry(ctx)
    l = local_loop.LocalLoop(ctx)
    try:
        d = ctx.to_device
        g.init_first_rgb(d(fp["rgba0"]))
        g.init_icp_model(d(fp["v4"]), d(fp["n4"]), pose)
        g.init_rgb_model(d(fp["img"]))
        g.init_icp(ctx.depth_pyramid(d(fp["d1"])), 20.0)
        g.init_rgb(d(fp["rgba1"]))
        tr, rot, st = g.track(pose[:3, 3], pose[:3, :3])
        track = dict(rot=rot, trans=tr, icp_error=st.last_icp_error, icp_count=st.last_icp_count, lastA=np.array(list(st.lastA)).reshape(6, 6))
        v = np.ascontiguousarray(fp["v4"], f32).reshape(H2, W2, 4)
        t = np.full((H2, W2), 7, np.uint16)
        th = dict(cov_thresh=1.0, icp_count_thresh=1000, icp_err_thresh=1.0)
        want = lref.local_constraints(track, v, t, pose, 9, 20.0, True, th)
        assert want["accepted"] and want["n"] > 100
        l.constraints_async(d(v), d(t), pose, 9, 20.0, True, odom=g, **th)
        rec = l.wait()
        assert rec["accepted"] and rec["n_constraints"] == want["n"] and rec["est_pose"].tobytes() == want["est_pose"].tobytes()
        assert rec["max_covariance"] == want["max_covariance"] and rec["icp_count"] == f32(st.last_icp_count)
        src, dst, tm = l.rows(want["n"])
        assert src.tobytes() == want["src"].tobytes() and dst.tobytes() == want["dst"].tobytes() and tm.tobytes() == want["time"].tobytes()
    finally:
        l.close(); g.close(); ctx.close()
