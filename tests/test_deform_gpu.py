"""GPU suite: the deformation graph (csrc/deform.hip through cf_deform_*) stage by stage against the numpy statement tests/deform_ref.py
on the cases of tests/deform_cases.py.

Exact: nodes, count, monotone flag, edges, window node ids.  Bit for bit (f32, stated order): weights, map positions, normals, time
stamps, pose translations.  A and b: every entry within (m - 1) 2^-53 sum|terms| of the f64 statement (the bound of a sum taken in
another order; both sides computed here).  Solve: |delta_dev - delta*|_inf <= max(8 e, 4 2^-53 |delta*|_inf) with e = numpy's own
Cholesky error against the extended-precision solution delta*.  One iteration: every parameter within 1 ulp of f32.  Free-running
optimise: same flags and iteration count, errors within a relative 1e-5.  Every stage twice: identical bytes."""
import numpy as np
import pytest

import deform_cases as dc
import deform_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
SOLVABLE = [(n, k) for n, k in dc.SYSTEMS if k not in dc.GAUGE_FREE]
CAM = (60.0, 60.0, 32.0, 24.0)


@pytest.fixture(scope="module")
def rig():
    from co_fusion_amd import api, deform
    ctx = api.Context(64, 48, *CAM, max_models=2, max_surfels=8192)
    d = deform.Deform(ctx)
    yield ctx, d
    d.close()
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def within_ulps(a, b, ulps=1):
    a = np.asarray(a, f32); b = np.asarray(b, f32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def device_weights(d, nodes, pts, times):
    """weight sets of any number of points, MAX_CONSTRAINTS at a time"""
    ids, w = [], []
    for at in range(0, len(pts), ref.MAX_CONS):
        p = pts[at:at + ref.MAX_CONS]
        d.weights(p, p, times[at:at + ref.MAX_CONS])
        got = d.download()
        ids.append(got["ids"]); w.append(got["weights"])
    return np.concatenate(ids), np.concatenate(w)


# ------------------------------------------------------------------------------------------------ sample
@pytest.mark.parametrize("name", list(dc.MAPS) + ["non_monotone"])
def test_sample_is_exact(rig, name):
    ctx, d = rig
    c = dc.non_monotone_map() if name == "non_monotone" else dc.get_map(name)
    want, stride, mono = ref.sample(c.surfels, c.sample_rate)
    dev = ctx.to_device(c.surfels)
    for _ in range(2):
        assert d.sample(dev, c.sample_rate) == (len(want), stride, mono)
        got = d.download()
        assert got["nodes"].tobytes() == want.tobytes()
        assert got["params"].tobytes() == ref.identity_params(len(want)).tobytes()
        if len(want) >= 5:
            assert np.array_equal(got["edges"], ref.edges(len(want)))


def test_no_graph_is_refused(rig):
    from co_fusion_amd import api
    ctx, d = rig
    c = dc.get_map("four_nodes")
    assert d.sample(ctx.to_device(c.surfels), c.sample_rate)[0] == 4
    with pytest.raises(api.CofusionError):
        d.weights(np.zeros((1, 3)), np.zeros((1, 3)), [0])
    with pytest.raises(api.CofusionError):
        d.optimise()
    with pytest.raises(api.CofusionError):
        d.apply(ctx.to_device(c.surfels))
    with pytest.raises(api.CofusionError):
        d.weights(np.zeros((129, 3)), np.zeros((129, 3)), np.zeros(129))


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("n", dc.NODE_COUNTS)
def test_window_ids_exact_weights_bit_for_bit(rig, n):
    _, d = rig
    nodes = dc.make_nodes(n)
    pts = dc.window_points(nodes)
    ids, w, ok = ref.weights(nodes, pts[:, :3], pts[:, 3])
    d.set_nodes(nodes)
    assert np.array_equal(d.download()["edges"], ref.edges(n))
    for _ in range(2):
        gi, gw = device_weights(d, nodes, pts[:, :3], pts[:, 3])
        assert np.array_equal(gi, ids)
        assert np.array_equal(bits(gw), bits(w))


def test_ties_and_degenerate_sets(rig):
    _, d = rig
    nodes = dc.tie_nodes()
    d.set_nodes(nodes)
    for t in (9, 12):
        ids, w, ok = ref.weights(nodes, np.zeros((1, 3), f32), [t])
        gi, gw = device_weights(d, nodes, np.zeros((1, 3), f32), np.array([t], f32))
        assert np.array_equal(gi, ids) and np.array_equal(bits(gw), bits(w))
    for coincident in (False, True):
        nodes = dc.degenerate_nodes(coincident)
        d.set_nodes(nodes, dc.bent_params(5))
        _, gw = device_weights(d, nodes, np.zeros((1, 3), f32), np.array([2], f32))
        assert np.isnan(gw).all()


# ------------------------------------------------------------------------------------------------ apply
def _reactivate(ctx, surfels, seed):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.5, 3.0, (48, 64)).astype(f32)
    depth[rng.uniform(size=depth.shape) < 0.2] = 0
    pose = np.eye(4, dtype=f32); pose[:3, 3] = surfels[:, :3].mean(0) - f32([0, 0, 1.2])
    host = dict(t_inv=np.linalg.inv(pose.astype(np.float64)).astype(f32), cam=CAM, cols=64, rows=48, max_depth=3.0, depth=depth, threshold=10.0, tick=777)
    return host, dict(pose=pose, cam=CAM, depth=ctx.to_device(depth), max_depth=3.0, conf_threshold=10.0, tick=777)


@pytest.mark.parametrize("stamp", [False, True], ids=["move", "stamp"])
@pytest.mark.parametrize("name", ["first_of_stride", "full_stride", "five_nodes", "workgroups", "stride_rule", "one_frame"])
def test_map_pass_bit_for_bit(rig, name, stamp):
    ctx, d = rig
    c = dc.get_map(name)
    nodes = ref.sample(c.surfels, c.sample_rate)[0]
    params = dc.bent_params(len(nodes), seed=len(name))
    host_re, dev_re = _reactivate(ctx, c.surfels, len(name)) if stamp else (None, None)
    if stamp:
        # the pose's translation is exact in f32 and its rotation the identity: the inverse the library takes is the statement's
        assert np.array_equal(host_re["t_inv"][:3, :3], np.eye(3, dtype=f32)) and np.array_equal(host_re["t_inv"][:3, 3], -dev_re["pose"][:3, 3])
    want = ref.apply_map(nodes, params, c.surfels, host_re)
    if stamp:
        assert (want[:, 7] == 777).sum() > 0 and (want[:, 7] != 777).sum() > 0
    for _ in range(2):
        dev = ctx.to_device(c.surfels)
        assert d.sample(dev, c.sample_rate)[0] == len(nodes)
        d.set_nodes(d.download()["nodes"], params)
        d.apply(dev, dev_re)
        ctx.synchronize()
        got = dev.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]


def test_map_pass_leaves_degenerate_surfels_alone(rig):
    ctx, d = rig
    m = dc.make_map(300, 3)
    m[:, :3] = 0
    for coincident in (False, True):
        d.set_nodes(dc.degenerate_nodes(coincident), dc.bent_params(5))
        dev = ctx.to_device(m)
        d.apply(dev)
        ctx.synchronize()
        assert np.array_equal(bits(dev.cpu().numpy()), bits(m))


# ------------------------------------------------------------------------------------------------ assemble
def _upload(d, s, params=None):
    d.set_nodes(s["nodes"], params)
    d.weights(s["src"], s["dst"], s["tm"])


def _check_system(got, n, jr, r, A, b):
    mA, sA, mb, sb = ref.sum_bounds(n, jr, r)
    want = ref.to_band(A)
    errA = np.abs(got["A"] - want); errb = np.abs(got["b"] - b)
    assert (errA <= np.maximum(mA - 1, 0) * 2.0 ** -53 * sA).all(), np.argwhere(errA > np.maximum(mA - 1, 0) * 2.0 ** -53 * sA)[:5]
    assert (errb <= np.maximum(mb - 1, 0) * 2.0 ** -53 * sb).all()
    assert (mA > 0).sum() > 100 and np.abs(want).max() > 1


@pytest.mark.parametrize("n,kind", dc.SYSTEMS, ids=[f"{n}-{k}" for n, k in dc.SYSTEMS])
def test_normal_equations_within_the_summation_bound(rig, n, kind):
    _, d = rig
    s = dc.system(n, kind)
    first = None
    for _ in range(2):
        _upload(d, s)
        d.assemble()
        got = d.download(system=True)
        if len(s["src"]):
            assert np.array_equal(got["ids"], s["opt"]["ids"]) and np.array_equal(bits(got["weights"]), bits(s["opt"]["w"]))
        _check_system(got, n, s["jr"], s["r"], s["A"], s["b"])
        first = first or (got["A"].tobytes(), got["b"].tobytes())
        assert first == (got["A"].tobytes(), got["b"].tobytes())


def test_normal_equations_at_a_bent_state(rig):
    """general rotations in every Jacobian row: the state the accepted 21-node shift ends in"""
    _, d = rig
    s = dc.system(21, "shift")
    o = s["opt"]
    jr, r = ref.rows(s["nodes"], o["params"], s["src"], s["dst"], o["ids"], o["w"], o["ok"])
    _, A, b = ref.dense_system(21, jr, r)
    _upload(d, s, o["params"])
    d.assemble()
    _check_system(d.download(system=True), 21, jr, r, A, b)


# ------------------------------------------------------------------------------------------------ solve, iterate, optimise
def test_solve_and_one_iteration(rig):
    _, d = rig
    print("\n   case        e = |numpy - star|   |device - star|   ratio   allowed")
    for n, kind in SOLVABLE:
        s = dc.system(n, kind)
        o = s["opt"]
        states = [ref.identity_params(n)]
        step1 = ref.iterate(s["nodes"], states[0], s["src"], s["dst"], o["ids"], o["w"], o["ok"])
        if kind == "shift":
            states.append(step1["params"])       # ... and from the statement's own f32 state after its first iteration
        for k, P in enumerate(states):
            want = step1 if k == 0 else ref.iterate(s["nodes"], P, s["src"], s["dst"], o["ids"], o["w"], o["ok"])
            jr, r = (s["jr"], s["r"]) if k == 0 else ref.rows(s["nodes"], P, s["src"], s["dst"], o["ids"], o["w"], o["ok"])
            A, b = (s["A"], s["b"]) if k == 0 else ref.dense_system(n, jr, r)[1:]
            star = ref.solve_star(ref.to_band(A), b)
            e = float(np.abs(want["delta"] - star).max())
            runs = []
            for _ in range(2):
                _upload(d, s, P)
                got = d.iterate()
                dl = d.download(system=True)
                runs.append((dl["b"].tobytes(), dl["params"].tobytes(), got["error"].tobytes()))
            assert runs[0] == runs[1]
            err = float(np.abs(dl["b"] - star).astype(np.float64).max())
            allowed = max(8 * e, 4 * 2.0 ** -53 * float(np.abs(star).max()))
            print(f"   {n:4d}-{kind:6s}{k}  {e:.3e}            {err:.3e}        {err / e if e else float('inf'):6.2f}   {allowed:.3e}")
            assert not got["failed"] and err <= allowed
            assert within_ulps(dl["params"], want["params"]).all()
            assert abs(float(got["error"]) - float(want["error"])) <= 1e-5 * float(want["error"])
            assert abs(got["delta_norm"] - want["delta_norm"]) <= 1e-9 * want["delta_norm"]


# (one constraint passes the 0.06 gate and then solves a system that is singular to rounding: no yardstick, see deform_cases.GAUGE_FREE)
FREE_RUNNING = [(n, k) for n, k in dc.SYSTEMS if k != "one"]


@pytest.mark.parametrize("n,kind", FREE_RUNNING, ids=[f"{n}-{k}" for n, k in FREE_RUNNING])
def test_free_running_optimise(rig, n, kind):
    _, d = rig
    s = dc.system(n, kind)
    o = s["opt"]
    runs = []
    for _ in range(2):
        _upload(d, s)
        got = d.optimise()
        runs.append((sorted((k, np.asarray(v).tobytes()) for k, v in got.items()), d.download()["params"].tobytes()))
    assert runs[0] == runs[1]
    for k in ("optimised", "accepted", "failed", "iterations"):
        assert got[k] == o[k], (k, got, {k: o[k] for k in got})
    for k in ("error_before", "mean_cons_error_before", "error", "mean_cons_error"):
        if np.isnan(o[k]):
            assert np.isnan(got[k])
        else:
            assert abs(float(got[k]) - float(o[k])) <= 1e-5 * abs(float(o[k])), (k, got[k], o[k])


def test_thresholds_are_parameters(rig):
    from co_fusion_amd import deform
    ctx, d = rig
    s = dc.system(21, "shift")
    th = deform.default_thresholds(ctx.lib)
    assert (round(th.min_cons_error, 6), th.max_iterations, round(th.accept_cons_error, 7), round(th.accept_error, 6)) == (0.06, 3, 3e-4, 0.12)
    for field, value in (("min_cons_error", 0.2), ("max_iterations", 1), ("accept_error", 1e-4)):   # gated; one step; optimised and rejected
        th = deform.default_thresholds(ctx.lib)
        setattr(th, field, value)
        o = ref.optimise(s["nodes"], s["src"], s["dst"], s["tm"], th={field: value})
        want = {k: o[k] for k in ("optimised", "accepted", "iterations")}
        assert want != {k: s["opt"][k] for k in want}
        _upload(d, s)
        got = d.optimise(th)
        assert {k: got[k] for k in want} == want, (field, got)


def test_a_non_positive_pivot_fails_the_step(rig):
    _, d = rig
    nodes, params = dc.singular_state()
    d.set_nodes(nodes, params)
    d.weights(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0))
    got = d.iterate()
    assert got["failed"]
    assert d.download()["params"].tobytes() == params.tobytes()


# ------------------------------------------------------------------------------------------------ keyframe poses
@pytest.mark.parametrize("kind", ["rotation", "half"])
def test_keyframe_poses(rig, kind):
    ctx, d = rig
    nodes = dc.make_nodes(21)
    poses, times, params = dc.poses_case(nodes, kind)
    t, M, ok = ref.apply_poses(nodes, params, poses, times)
    assert ok.all()
    d.set_nodes(nodes, params)
    runs = []
    for _ in range(2):
        dp = ctx.to_device(poses.reshape(-1, 16)); dt = ctx.to_device(times)
        d.apply_poses(dp, dt)
        ctx.synchronize()
        runs.append(dp.cpu().numpy().reshape(-1, 4, 4))
    assert runs[0].tobytes() == runs[1].tobytes()
    got = runs[0]
    assert np.array_equal(bits(got[:, :3, 3]), bits(t))
    assert np.array_equal(got[:, 3], poses[:, 3])
    for g, m in zip(got, M):
        assert within_ulps(g[:3, :3], ref.polar_svd(m).astype(f32)).all()


# ------------------------------------------------------------------------------------------------ the allocation limit
def test_1024_nodes_assemble_and_solve_once(rig):
    """CF_DEFORM_MAX_NODES nodes, one constraint at every 16th: the whole band of A (12288 x 240), the solve over 1024 block columns and
    the map pass with every node slot of its LDS stage in use.  (Numpy's yardstick here is LAPACK's band Cholesky where scipy is
    installed, the statement's own loops otherwise; no 1-ulp parameter comparison: e is not below a quarter ulp of f32 on a chain this long.)"""
    ctx, d = rig
    n = dc.BIG
    nodes = dc.make_nodes(n)
    src, dst, tm = dc.constraints("anchored", nodes)
    ids, w, ok = ref.weights(nodes, src, tm)
    assert ok.all()
    jr, r = ref.rows(nodes, ref.identity_params(n), src, dst, ids, w, ok)
    AB, b = ref.band_system(n, jr, r)
    mA, sA, mb, sb = ref.sum_bounds(n, jr, r)
    d.set_nodes(nodes)
    d.weights(src, dst, tm)
    d.assemble()
    got = d.download(system=True)
    assert np.array_equal(got["ids"], ids) and np.array_equal(bits(got["weights"]), bits(w)) and np.array_equal(got["edges"], ref.edges(n))
    assert (np.abs(got["A"] - AB) <= np.maximum(mA - 1, 0) * 2.0 ** -53 * sA).all() and (np.abs(got["b"] - b) <= np.maximum(mb - 1, 0) * 2.0 ** -53 * sb).all()
    star = ref.solve_star(AB, b)
    e = float(np.abs(ref.band_factor(AB)(b) - star).max())
    step = d.iterate()
    delta = d.download(system=True)["b"]
    err = float(np.abs(delta - star).astype(np.float64).max())
    allowed = max(8 * e, 4 * 2.0 ** -53 * float(np.abs(star).max()))
    print(f"\n   1024-anchored  e {e:.3e}  device {err:.3e}  ratio {err / e:.2f}  allowed {allowed:.3e}  error {step['error']}")
    assert not step["failed"] and err <= allowed
    # the map pass over a graph of 1024 nodes sampled from 2048 surfels
    m = dc.make_map(2 * n, 4, seed=3)
    sampled = ref.sample(m, 2)[0]
    assert len(sampled) == n
    params = dc.bent_params(n, seed=9)
    dev = ctx.to_device(m)
    assert d.sample(dev, 2) == (n, 2, True)
    d.set_nodes(sampled, params)
    d.apply(dev)
    ctx.synchronize()
    assert np.array_equal(bits(dev.cpu().numpy()), bits(ref.apply_map(sampled, params, m)))
