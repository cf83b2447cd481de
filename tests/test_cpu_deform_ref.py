"""CPU suite: the numpy statement of the deformation graph (tests/deform_ref.py) is sane on its own, and every case of
tests/deform_cases.py keeps the conditions the GPU comparisons (test_deform_gpu.py) rest on.  A case that breaks a condition is changed;
the bound is not."""
import numpy as np
import pytest

import deform_cases as dc
import deform_ref as ref

f32 = np.float32
system, SYSTEMS = dc.system, dc.SYSTEMS
IDS = [f"{n}-{k}" for n, k in SYSTEMS]


def test_edges_are_connect_graph_seq():
    assert ref.edges(5).tolist() == [[1, 2, 3, 4], [0, 2, 3, 4], [1, 3, 0, 4], [0, 1, 2, 4], [0, 1, 2, 3]]
    e = ref.edges(9)
    assert e[0].tolist() == [1, 2, 3, 4] and e[4].tolist() == [3, 5, 2, 6] and e[7].tolist() == [4, 5, 6, 8] and e[8].tolist() == [4, 5, 6, 7]
    for n in dc.NODE_COUNTS:
        e = ref.edges(n)
        assert (e != np.arange(n)[:, None]).all() and (np.abs(e - np.arange(n)[:, None]) <= 4).all()


def test_sampling_and_the_stride_rule():
    for name in dc.MAPS:
        c = dc.get_map(name)
        nodes, stride, mono = ref.sample(c.surfels, c.sample_rate)
        assert mono and len(nodes) <= ref.MAX_NODES and stride % c.sample_rate == 0
        assert len(nodes) == -(-len(c.surfels) // stride)
        assert stride == c.sample_rate or -(-len(c.surfels) // (stride - c.sample_rate)) > ref.MAX_NODES
    assert len(ref.sample(dc.get_map("four_nodes").surfels, dc.R)[0]) == 4
    assert ref.sample(dc.get_map("stride_rule").surfels, 2)[1] == 4
    assert not ref.sample(dc.non_monotone_map().surfels, dc.R)[2]
    assert ref.stride_for(10 ** 6, 25000) == 25000 and ref.stride_for(3 * 10 ** 7, 25000) == 50000


def test_window_branches_and_ties():
    T = [0, 10, 10, 10, 20, 30, 30, 40]
    assert ref.window(T, 10)[0] in (1, 2, 3) and ref.window(T, -7)[0] == 0 and ref.window(T, 99)[0] == 7
    assert ref.window(T, 15)[0] in (3, 4) and ref.window(T, 14)[0] in (1, 2, 3) and ref.window(T, 16)[0] == 4
    found, cand = ref.window(list(range(40)), 25)
    assert found == 25 and cand == list(range(25, 15, -1)) + list(range(26, 36))
    assert ref.window(list(range(40)), 3)[1] == [3, 2, 1, 0] + list(range(4, 20))
    assert ref.window(list(range(40)), 38)[1] == list(range(38, 28, -1)) + [39]
    # the crafted tie: nodes 3 and 4 at distance 1; the earlier candidate is the 4th, the later one the 5th (dMax)
    nodes = dc.tie_nodes()
    for t, want in ((9, [0, 1, 2, 3]), (12, [0, 1, 2, 4])):      # found = 3: candidates 3, 2, 1, 0, 4, 5; found = 4: 4, 3, 2, 1, 0, 5
        ids, w, ok, ds = ref.weights(nodes, np.zeros((1, 3), f32), [t], with_dists=True)
        assert ds[0, 3] == ds[0, 4] == 1 and ids[0].tolist() == want and ok[0] and w[0, 3] == 0
    for coincident in (False, True):
        ids, w, ok = ref.weights(dc.degenerate_nodes(coincident), np.zeros((1, 3), f32), [2])
        assert not ok[0]
        m = ref.move_points(dc.degenerate_nodes(coincident), dc.bent_params(5), np.zeros((1, 3), f32), ids, w, ok)
        assert np.array_equal(m, np.zeros((1, 3), f32))


@pytest.mark.parametrize("n", dc.NODE_COUNTS)
def test_no_unintended_distance_ties(n):
    nodes = dc.make_nodes(n)
    pts = dc.window_points(nodes)
    ids, w, ok, ds = ref.weights(nodes, pts[:, :3], pts[:, 3], with_dists=True)
    assert ok.all() and (ds[:, 3] < ds[:, 4]).all()
    assert np.allclose(w.sum(1), 1, atol=1e-6) and (np.diff(ids, axis=1) > 0).all()
    for name in ("workgroups", "full_stride", "one_frame"):
        c = dc.get_map(name)
        nd = ref.sample(c.surfels, c.sample_rate)[0]
        ds = ref.weights(nd, c.surfels[:, :3], c.surfels[:, 6], with_dists=True)[3]
        assert (ds[:, 3] < ds[:, 4]).all(), name


@pytest.mark.parametrize("n,kind", SYSTEMS, ids=IDS)
def test_conditions_of_the_gpu_comparisons(n, kind):
    s = system(n, kind)
    if len(s["src"]):
        ds = ref.weights(s["nodes"], s["src"], s["tm"], with_dists=True)[3]
        assert s["opt"]["ok"].all() and (ds[:, 3] < ds[:, 4]).all()
    for value, threshold in s["trace"]:          # no stop or accept rule is decided by the last digits
        assert not np.isfinite(value) or abs(value - threshold) > 1e-5 * max(abs(threshold), abs(value)), (value, threshold)
    # A is zero outside the stated band, symmetric positive definite, and numpy's Cholesky solves it far below f32 resolution
    A, b = s["A"], s["b"]
    i, j = np.indices(A.shape)
    assert not A[np.abs(i - j) > ref.HALF_BAND].any()
    assert not A[np.abs(i // 12 - j // 12) > ref.HALF_BLOCKS].any()
    AB = ref.to_band(A)
    AB2, b2 = ref.band_system(n, s["jr"], s["r"])
    mA, sA, mb, sb = ref.sum_bounds(n, s["jr"], s["r"])
    assert (np.abs(AB - AB2) <= np.maximum(mA - 1, 0) * 2.0 ** -53 * sA).all() and (np.abs(b - b2) <= np.maximum(mb - 1, 0) * 2.0 ** -53 * sb).all()
    if kind in dc.GAUGE_FREE:
        return
    star = ref.solve_star(AB, b)
    d_np = ref._tri(np.linalg.cholesky(A), b)
    e = np.abs(d_np - star).astype(np.float64)
    new = ref.identity_params(n).reshape(-1).astype(np.float64) + d_np
    quarter_ulp = np.spacing(np.abs(new).astype(f32)).astype(np.float64) / 4
    assert (e < quarter_ulp).all(), (e.max(), quarter_ulp.min())
    # ... and the band routine of the statement agrees with it
    d_band = ref.band_solve(ref.band_cholesky(AB), b)
    assert np.abs(d_band - star).max() <= max(8 * e.max(), 4 * 2.0 ** -53 * float(np.abs(star).max()))


def test_the_shift_is_accepted_and_lands():
    for n in (5, 6, 12):      # too few nodes between the pinned and the shifted part: optimised, and rejected
        o = system(n, "shift")["opt"]
        assert o["optimised"] and not o["accepted"] and not o["failed"] and o["iterations"] == 3
    assert system(21, "shift")["opt"]["accepted"]
    for n in (45,):
        s = system(n, "shift")
        o = s["opt"]
        assert o["optimised"] and o["accepted"] and not o["failed"] and 1 <= o["iterations"] <= 3
        assert o["mean_cons_error_before"] > 0.06 and o["mean_cons_error"] < 3e-4 and o["error"] < 0.12
        moved = ref.move_points(s["nodes"], o["params"], s["src"], o["ids"], o["w"], o["ok"])
        assert np.linalg.norm(moved[0::2] - s["dst"][0::2], axis=1).max() < 3e-4      # the sources land on their targets
        assert np.linalg.norm(moved[1::2] - s["src"][1::2], axis=1).max() < 3e-4      # the pinned points stay


def test_the_other_outcomes():
    assert not system(6, "none")["opt"]["optimised"]
    small = system(12, "small")["opt"]
    assert not small["optimised"] and small["mean_cons_error_before"] < 0.06 and np.array_equal(small["params"], ref.identity_params(12))
    wild = system(21, "wild")["opt"]
    assert wild["optimised"] and wild["iterations"] == 1 and wild["error"] > 10 and not wild["accepted"]
    nodes, params = dc.singular_state()
    step = ref.iterate(nodes, params, np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros((0, 4), np.int32), np.zeros((0, 4), f32), np.zeros(0, bool))
    assert step["failed"] and np.array_equal(step["params"], params)
    jr, r = ref.rows(nodes, params, np.zeros((0, 3), f32), np.zeros((0, 3), f32), None, None, None)
    assert ref.band_cholesky(ref.band_system(len(nodes), jr, r)[0]) is None


def test_map_pass_moves_with_the_graph():
    c = dc.get_map("full_stride")
    nodes = ref.sample(c.surfels, c.sample_rate)[0]
    same = ref.apply_map(nodes, ref.identity_params(len(nodes)), c.surfels)
    assert np.allclose(same[:, :3], c.surfels[:, :3], atol=2e-6) and np.allclose(same[:, 8:11], c.surfels[:, 8:11], atol=1e-6)
    P = ref.identity_params(len(nodes)); P[:, 9:] = f32([0.1, -0.2, 0.05])
    moved = ref.apply_map(nodes, P, c.surfels)
    assert np.allclose(moved[:, :3], c.surfels[:, :3] + f32([0.1, -0.2, 0.05]), atol=2e-6)
    assert np.array_equal(moved[:, [3, 4, 5, 6, 7, 11]], c.surfels[:, [3, 4, 5, 6, 7, 11]])
    assert np.allclose(np.linalg.norm(ref.apply_map(nodes, dc.bent_params(len(nodes)), c.surfels)[:, 8:11], axis=1), 1, atol=1e-6)


@pytest.mark.parametrize("kind", ["rotation", "half"])
def test_polar_factor_is_orthogonal(kind):
    nodes = dc.make_nodes(21)
    poses, times, params = dc.poses_case(nodes, kind)
    t, M, ok = ref.apply_poses(nodes, params, poses, times)
    assert ok.all()
    for m in M:
        if kind == "half":
            assert 0.35 < np.linalg.det(m.astype(np.float64)) < 0.65
        Q = ref.polar_newton(m)
        assert np.abs(Q.T @ Q - np.eye(3)).max() < 1e-15 and np.linalg.det(Q) > 0
        assert np.abs(Q - ref.polar_svd(m)).max() < 1e-14
        Y = ref.inv_t_3x3(m.astype(np.float64))
        assert np.abs(Y - np.linalg.inv(m.astype(np.float64)).T).max() < 1e-13
