"""CPU suite: the numpy statement of the relative constraints (tests/deform_rel_ref.py) on the cases of tests/deform_rel_cases.py -- its own
rules, the property the rows exist for, and the conditions the GPU comparisons of test_deform_rel_gpu.py rest on.

Ratios |stated direct method - star| / e with e = |numpy's dense Cholesky of A - star| (star: the extended-precision solution of the full
system), first iteration from the identity, as measured where this suite was written (the figures move with the BLAS in use; the GPU suite
computes them again and takes kappa = max(8, 2 * the largest)):

    loop1 6.5   loop3 4.8e3   loop4 1.3e3   path5 0.9   path6 2.1   path12 1.9   path21 2.9   overlap 6.9   same 1.2   nan 1.6

The loop cases are where the method costs digits: the oldest nodes hang on the pinned middle of the loop by eighteen regularisation edges
only, so B alone is soft exactly where the pairs pull, Y^T Y is of the order of 1e3, and y - Y t cancels that many digits.  The absolute
error stays near 5e-11; on loop3 and loop4 that is no longer a quarter ulp below the smallest f32 parameters it is added to, so the
1-ulp comparison of one iteration is made on the other cases (deform_rel_cases.ONE_ULP, checked below).  The device forms C and Y^T y
with compensated sums for this reason and lands below the figures of this f64 statement."""
import numpy as np
import pytest

import deform_cases as dc
import deform_ref as ref
import deform_rel_cases as rc
import deform_rel_ref as rel

f32 = np.float32


# ------------------------------------------------------------------------------------------------ pick and ring
def test_pick_rule():
    want = {1: [0], 2: [0, 1], 3: [0, 1, 2], 4: [0, 1, 2, 3], 5: [0, 1, 2, 3, 4], 8: [0, 2, 4, 6], 11: [0, 3, 6, 9], 767: [0, 255, 510, 765]}
    assert set(want) == set(rc.PICK_COUNTS)
    for n, idx in want.items():
        assert rel.pick_indices(n) == idx
    assert rel.pick_indices(0) == []
    assert max(len(rel.pick_indices(n)) for n in range(1, 1600)) == 5      # what one launch of the pick kernel may append


@pytest.mark.parametrize("n", rc.PICK_COUNTS)
def test_pick_moves_the_sources_by_the_map_rule(n):
    nodes, params, src, dst, ts, td = rc.closure_rows(n)
    got = rel.pick(nodes, params, src, dst, ts, td)
    idx = rel.pick_indices(n)
    surfels = np.zeros((len(idx), 12), f32); surfels[:, 0:3] = src[idx]; surfels[:, 6] = ts[idx]; surfels[:, 8] = 1
    assert np.array_equal(got[:, 0:3], ref.apply_map(nodes, params, surfels)[:, 0:3])      # what the map pass does to a surfel there
    assert np.array_equal(got[:, 4:7], dst[idx]) and np.array_equal(got[:, 3], ts[idx]) and np.array_equal(got[:, 7], td[idx])
    assert not np.array_equal(got[:, 0:3], src[idx])


@pytest.mark.parametrize("appends", [127, 128, 129])
def test_ring(appends):
    ring = rel.Ring()
    rows = np.arange(appends * 8, dtype=f32).reshape(-1, 8)
    for k in range(appends):
        ring.append(rows[k])
    assert ring.total == appends and ring.count == min(appends, 128) and ring.overwritten == max(appends - 128, 0)
    want = rows[:128].copy()
    if appends == 129:
        want[0] = rows[128]
    assert np.array_equal(ring.pairs(), want[:ring.count])


# ------------------------------------------------------------------------------------------------ rows
def test_rows_are_off_band_on_the_loop_only():
    c = rc.case("loop3")
    uid = c["sys"]["uid"]
    assert (uid >= 0).all()
    assert (uid[:, :4].min(1) - uid[:, 4:].max(1) >= 20).all()             # source and target sets >= 20 blocks apart: outside the band
    i, j = np.nonzero(c["sys"]["U"].T @ c["sys"]["U"])
    assert np.abs(i - j).max() > ref.HALF_BAND
    # the straight path cannot produce it: a target stamped with the oldest time but placed at node 22 takes the window's last nodes
    nodes = dc.make_nodes(45)
    ids, _, ok = ref.weights(nodes, nodes[22:23, :3], nodes[0:1, 3])
    assert ok.all() and ids.max() <= 19
    for name in ("path5", "path6", "path12", "path21", "overlap", "same"):
        u = rc.case(name)["sys"]["uid"]
        assert np.ptp(np.where(u >= 0, u, u[:, :1]), axis=1).max() <= ref.HALF_BLOCKS


def test_merged_and_empty_rows():
    o = rc.case("overlap"); s = rc.case("same"); n = rc.case("nan")
    shared = [len(set(a) & set(b)) for a, b in zip(o["opt"]["ws"][0], o["opt"]["wt"][0])]
    assert min(shared) >= 1 and max(shared) <= 3                            # some nodes in both sets, not all
    assert [(u >= 0).sum() for u in o["sys"]["uid"]] == [8 - k for k in shared]
    assert np.array_equal(s["opt"]["ws"][0], s["opt"]["wt"][0]) and ((s["sys"]["uid"] >= 0).sum(1) == 4).all()
    assert np.abs(s["sys"]["uval"][:, :4, 3].sum(1)).max() < 1e-5           # the weights of both sets sum to one: the merged ones cancel
    assert list(n["opt"]["ws"][2]) == [True, False, True] and n["opt"]["wt"][2].all()
    assert (n["sys"]["uid"][1] == -1).all() and not n["sys"]["U"][3:6].any() and np.abs(n["sys"]["r_rel"][3:6]).min() > 0
    for name in rc.CASES:                                                    # a merged slot holds source + (-target), columns are unique
        sy = rc.case(name)["sys"]
        for u in sy["uid"]:
            assert len(set(u[u >= 0])) == (u >= 0).sum()
        c = rc.case(name)
        jr = rel.sparse_rows(sy["uid"], sy["uval"])
        assert len(jr) == 3 * len(c["pairs"]) and np.array_equal(rel.dense_rows(len(c["nodes"]), sy["uid"], sy["uval"]), sy["U"])


def test_mean_constraint_error_counts_every_constraint_below_the_line():
    nodes, src, dst, tm, pairs = rc.gate_case()
    without = ref.optimise(nodes, src, dst, tm)
    with_pair = rel.optimise(nodes, src, dst, tm, pairs)
    assert abs(float(without["mean_cons_error_before"]) - 0.07) < 1e-6 and without["optimised"]
    assert with_pair["mean_cons_error_before"] == f32(without["mean_cons_error_before"] / f32(2)) and not with_pair["optimised"]
    assert abs(float(with_pair["mean_cons_error_before"]) - 0.06) > 1e-5 * 0.06


# ------------------------------------------------------------------------------------------------ the conditions of the GPU comparisons
@pytest.mark.parametrize("name", rc.CASES)
def test_conditions_of_the_gpu_comparisons(name):
    c = rc.case(name); s = c["sys"]; o = c["opt"]
    for pts, tms in ((c["src"], c["tm"]), (c["pairs"][:, 0:3], c["pairs"][:, 3]), (c["pairs"][:, 4:7], c["pairs"][:, 7])):
        ok, ds = (lambda r: (r[2], r[3]))(ref.weights(c["nodes"], pts, tms, with_dists=True))
        assert (ds[ok, 3] < ds[ok, 4]).all()                                 # no 4th / 5th distance tie decides a weight set
    for value, threshold in c["trace"]:                                      # no stop or accept rule is decided by the last digits
        assert not np.isfinite(value) or abs(value - threshold) > 1e-5 * max(abs(threshold), abs(value)), (value, threshold)
    A = s["A"]
    assert np.array_equal(A, A.T) or np.abs(A - A.T).max() <= 2.0 ** -50 * np.abs(A).max()
    star, direct, dense = rc.solved(name)
    e = float(np.abs(dense - star).max()); ed = float(np.abs(direct - star).max())
    print(f"\n   {name:8s} e {e:.3e}  stated method {ed:.3e}  ratio {ed / e:.1f}")
    assert np.isfinite(ed) and ed < 1e-9
    new = ref.identity_params(len(c["nodes"])).reshape(-1).astype(np.float64) + direct
    quarter_ulp = np.spacing(np.abs(new).astype(f32)).astype(np.float64) / 4
    assert (4 * np.abs(direct - star).astype(np.float64) < quarter_ulp).all() == (name in rc.ONE_ULP)
    # the relative residual rows are in the error
    P0 = ref.identity_params(len(c["nodes"]))
    assert o["error_before"] == rel.error_of(s["r"], s["r_rel"]) and o["error_before"] > ref.error_of(s["r"])
    assert np.array_equal(rel.rel_residual(c["nodes"], P0, c["pairs"], o["ws"], o["wt"]), s["r_rel"])


def test_the_pairs_keep_what_a_local_closure_registered():
    """the loop with the shift constraints: both closures are accepted; without the pairs the newest part moves by 15 cm and leaves the
    oldest part, which it lay on, behind; with them it takes it along"""
    c = rc.case("loop3"); o = c["opt"]
    plain = ref.optimise(c["nodes"], c["src"], c["dst"], c["tm"])
    assert o["accepted"] and plain["accepted"]
    before = rel.gap(c["nodes"], ref.identity_params(45), c["pairs"], o["ws"], o["wt"])
    with_pairs = rel.gap(c["nodes"], o["params"], c["pairs"], o["ws"], o["wt"])
    without = rel.gap(c["nodes"], plain["params"], c["pairs"], o["ws"], o["wt"])
    print(f"\n   |phi(src) - phi(tgt)|  before {before.max():.4f}  without the pairs {without.max():.4f}  with {with_pairs.max():.4f}")
    assert (with_pairs < without).all() and with_pairs.max() < 0.01 < 0.1 < without.min()
    moved = ref.move_points(c["nodes"], o["params"], c["src"], o["ids"], o["w"], o["ok"])
    assert np.linalg.norm(moved - c["dst"], axis=1).max() < 2e-3             # the absolute constraints are still met


def test_target_times_are_the_pin_rows_times():
    """deform_rel_ref.target_times restates the sampling of local_loop_ref.local_constraints: with pins its values are the times of the pin
    rows, and there is one per constraint with or without pins"""
    import local_loop_cases as lc
    import local_loop_ref as lref
    for kind in lc.SAMPLE_CASES:
        v, t = lc.cons_maps(kind)
        want = rel.target_times(v, t, lc.CONS_MAX_DEPTH)
        pinned = lref.local_constraints(lc.good_track(), v, t, lc.cons_pose(0), lc.CONS_TICK, lc.CONS_MAX_DEPTH, True)
        plain = lref.local_constraints(lc.good_track(), v, t, lc.cons_pose(0), lc.CONS_TICK, lc.CONS_MAX_DEPTH, False)
        assert want.tobytes() == pinned["time"][1::2].tobytes() and len(want) == plain["n"] == pinned["n"] // 2
    assert len(rel.target_times(*lc.cons_maps("all_valid"), lc.CONS_MAX_DEPTH)) == 96
