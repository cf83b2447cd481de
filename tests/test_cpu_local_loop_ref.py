"""CPU suite: the numpy statement of the graph's local mode (tests/local_loop_ref.py) is sane on its own, and every case of
tests/local_loop_cases.py keeps the conditions the GPU comparisons (test_local_deform_gpu.py) rest on: the comparison a case is meant
to hit exactly is hit exactly, and no stop rule of a free-running case is decided by the last digits.  A case that breaks a condition is
changed; the bound is not."""
import math

import numpy as np
import pytest

import deform_cases as dc
import deform_ref as ref
import local_loop_cases as lc
import local_loop_ref as lref

f32 = np.float32
ident = lambda cases: ["-".join(str(x) for x in c) for c in cases]


@pytest.mark.parametrize("n,kind,which", lc.IDENTICAL, ids=ident(lc.IDENTICAL))
def test_every_node_enabled_is_the_global_system(n, kind, which):
    s, g = lc.system(n, kind, which), dc.system(n, kind)
    assert s["ldt"] == 0 and s["nodes"][:, 3].min() >= 1 and s["en"].all() and s["keep"].all()
    assert np.array_equal(s["A"], g["A"]) and np.array_equal(s["b"], g["b"]) and np.array_equal(s["r"], g["r"])
    assert len(s["jr"]) == len(g["jr"]) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(s["jr"], g["jr"]))


@pytest.mark.parametrize("n,kind,which", lc.DISABLED, ids=ident(lc.DISABLED))
def test_conditions_of_the_disabled_cases(n, kind, which):
    s = lc.system(n, kind, which)
    nodes, en, keep, ldt = s["nodes"], s["en"], s["keep"], s["ldt"]
    t = nodes[:, 3].astype(np.int64)
    # the enable rule is hit exactly: a node AT last_deform_time is disabled, and the enabled nodes are a suffix
    assert (t == ldt).any() and not en[t == ldt].any() and np.array_equal(en, t > ldt) and (np.diff(en.astype(int)) >= 0).all()
    rot, edge, con = keep[:6 * n], keep[6 * n:18 * n], keep[18 * n:]
    assert not rot.all() and not edge.all()
    if which == "half":
        assert en.any() and rot.any() and 0 < en.sum() < n
        # an edge between a disabled and an enabled node stays, with the enabled end's columns only
        E = ref.edges(n)
        mixed = [(j, k) for j in range(n) for k in range(4) if en[j] != en[E[j, k]]]
        assert mixed and all(edge[3 * (4 * j + k)] for j, k in mixed)
    else:
        assert not en.any() and not keep.any() and len(s["jr"]) == 0
    if len(s["src"]):
        ds = ref.weights(nodes, s["src"], s["tm"], with_dists=True)[3]
        assert s["opt"]["ok"].all() and (ds[:, 3] < ds[:, 4]).all()
    if kind == "dead_one":       # the last constraint's weight set is wholly disabled: its rows are dropped, and absent from the error
        assert not en[s["opt"]["ids"][-1]].any() and not con[-3:].any()
        if which == "half":
            assert con[:-3].all()
            full = dc_rows_error(s)
            gone = float(np.sum((f32(10.0) * (s["src"][-1] - s["dst"][-1]).astype(np.float64)) ** 2))
            assert gone > 1 and abs((full - float(ref.error_of(s["r"]))) - gone) < 1e-4 * gone
    if kind == "shift" and which == "half":   # every pin lies in the disabled part
        assert not con.reshape(-1, 3)[1::2].any() and con.reshape(-1, 3)[0::2].all()
    # no column of a disabled node is left in J; A carries exact identity blocks there; the enabled part is positive definite
    on = np.repeat(en, 12)
    assert all(on[c].all() for c, _ in s["jr"])
    A, b = s["A"], s["b"]
    assert np.array_equal(A[np.ix_(~on, ~on)], np.eye(int((~on).sum()))) and not A[np.ix_(on, ~on)].any() and not b[~on].any()
    i, j = np.indices(A.shape)
    assert not A[np.abs(i - j) > ref.HALF_BAND].any()
    if not en.any():
        return
    star = ref.solve_star(ref.to_band(A), b)
    assert not star[~on].any()
    d_np = ref._tri(np.linalg.cholesky(A), b)
    e = np.abs(d_np - star).astype(np.float64)
    new = ref.identity_params(n).reshape(-1).astype(np.float64) + d_np
    assert (e < np.spacing(np.abs(new).astype(f32)).astype(np.float64) / 4).all()
    # ... and one step of the statement (Cholesky of the enabled part alone) is that solution
    step = lref.iterate(nodes, ref.identity_params(n), s["src"], s["dst"], s["opt"]["ids"], s["opt"]["w"], s["opt"]["ok"], ldt)
    assert not step["delta"][~on].any() and np.abs(step["delta"] - star).max() <= max(8 * e.max(), 4 * 2.0 ** -53 * float(np.abs(star).max()))
    assert np.array_equal(step["params"][~en], ref.identity_params(n)[~en])


def dc_rows_error(s):
    """the error of the same state with every row kept"""
    n = len(s["nodes"])
    _, r = ref.rows(s["nodes"], ref.identity_params(n), s["src"], s["dst"], s["opt"]["ids"], s["opt"]["w"], s["opt"]["ok"])
    en = s["en"]
    keep_but_last = lref.kept_rows(s["nodes"], s["opt"]["ids"], len(s["src"]), en)
    keep_but_last[-3:] = True
    return float(ref.error_of(r[keep_but_last]))


@pytest.mark.parametrize("n,kind,which", lc.FREE_RUNNING, ids=ident(lc.FREE_RUNNING))
def test_no_stop_rule_is_decided_by_the_last_digits(n, kind, which):
    s = lc.system(n, kind, which)
    o = s["opt"]
    assert not o["failed"] and o["optimised"] == bool(s["en"].any()) and o["accepted"] == o["optimised"]
    assert (len(s["trace"]) > 0) == o["optimised"]
    for value, threshold in s["trace"]:
        assert abs(value - threshold) > 1e-5 * max(abs(threshold), abs(value)), (value, threshold)


def test_the_local_mode_takes_what_the_global_mode_turns_away():
    g, l = dc.system(12, "small")["opt"], lc.system(12, "small", "zero")["opt"]
    assert not g["optimised"] and g["mean_cons_error_before"] < 0.06
    assert l["optimised"] and l["accepted"] and l["iterations"] >= 1 and l["error"] < l["error_before"]
    far = lc.system(21, "far", "zero")
    g, l = ref.optimise(far["nodes"], far["src"], far["dst"], far["tm"]), far["opt"]
    assert g["optimised"] and g["iterations"] == 1 and 10 < g["error"] < g["error_before"] and not g["accepted"]   # stopped by `error > 10` alone
    assert l["iterations"] == 3 and l["accepted"] and l["error"] < 0.1 * g["error"]
    wild = lc.system(21, "wild", "zero")["opt"]      # ... and a set whose first iteration raises the error stops there in either mode
    assert wild["iterations"] == 1 and wild["error"] > wild["error_before"] and wild["accepted"]


def test_the_other_outcomes():
    off = lc.system(21, "shift", "all_off")["opt"]
    assert not off["optimised"] and not off["accepted"] and off["enabled"] == 0 and off["iterations"] == 0
    assert np.array_equal(off["params"], ref.identity_params(21)) and off["error_before"] == 0 and off["mean_cons_error_before"] > 0.06
    half = lc.system(45, "shift", "half")
    moved = ref.move_points(half["nodes"], half["opt"]["params"], half["src"], half["opt"]["ids"], half["opt"]["w"], half["opt"]["ok"])
    before = np.linalg.norm(half["src"][0::2] - half["dst"][0::2], axis=1).max()
    assert np.linalg.norm(moved[0::2] - half["dst"][0::2], axis=1).max() < 0.2 * before          # the sources move to their targets
    assert np.allclose(moved[1::2], half["src"][1::2], rtol=0, atol=2e-6)                         # what only disabled nodes carry stays (identity parameters, f32 rounding)
    assert np.array_equal(half["opt"]["params"][~half["en"]], ref.identity_params(45)[~half["en"]])
    nodes, params, ldt = lc.singular_half()
    en = lref.enabled(nodes, ldt)
    assert en.tolist() == [False, False, False, True, True, True]
    none = (np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, f32))
    o = lref.optimise(nodes, *none, ldt, params=params)
    assert o["optimised"] and o["failed"] and not o["accepted"] and o["iterations"] == 1 and np.array_equal(o["params"], params)
    jr, r, _, _ = lref.rows(nodes, params, none[0], none[1], np.zeros((0, 4), np.int32), None, None, ldt)
    AB, _ = lref.band_system(len(nodes), jr, r, en)
    assert AB[36, 0] == 0 and ref.band_cholesky(AB) is None and ref.band_cholesky(AB[:36]) is not None


@pytest.mark.parametrize("n,which", lc.BIG, ids=[f"{n}-{w}" for n, w in lc.BIG])
def test_conditions_of_the_1536_constraint_cases(n, which):
    s = lc.big_system(n, which)
    assert len(s["src"]) == 2 * 768 == lref.MAX_CONS_SIZED and s["ok"].all()
    ds = ref.weights(s["nodes"], s["src"], s["tm"], with_dists=True)[3]
    assert (ds[:, 3] < ds[:, 4]).all()
    assert (s["ids"][:, 3] - s["ids"][:, 0] <= ref.HALF_BLOCKS).all()     # the band does not grow with the constraint count
    assert len(s["keep"]) == 18 * n + 3 * 1536 and len(s["jr"]) == int(s["keep"].sum())
    on = np.repeat(s["en"], 12)
    assert np.array_equal(s["AB"][~on, 0], np.ones(int((~on).sum()))) and not s["AB"][~on, 1:].any() and not s["b"][~on].any()
    assert (which == "zero") == bool(s["en"].all()) and s["keep"].all() == (which == "zero")
    assert ref.band_cholesky(s["AB"]) is not None


# ------------------------------------------------------------------------------------------------ the crafted maps of the splat passes
def _predict(surfels, time, max_time):
    import orc
    import orc_pipeline as op
    w, h = lc.SHAPE
    return op.combined_predict(surfels, np.eye(4, dtype=f32), orc.Cam(*lc.CAM), w, h, lc.SPLAT_DEPTH, lc.SPLAT_CONF, time, max_time, lc.SPLAT_DELTA)


def test_the_crafted_maps_take_the_branches_they_are_meant_to():
    assert lc.MAX_TIME == lc.TICK - lc.SPLAT_DELTA
    w, h = lc.SHAPE
    assert (w // 20) * (h // 20) == 96 and w * h % 256 == 0 and (w * h // 256) > 1
    m = lc.splat_map("mixed")
    at = m[m[:, 7] == lc.MAX_TIME]; above = at.copy(); above[:, 7] = lc.MAX_TIME + 1
    assert len(at) >= 40 and (m[:, 7] < lc.MAX_TIME).sum() > 50 and (m[:, 7] > lc.MAX_TIME).sum() > 50 and (m[:, 3] < lc.SPLAT_CONF).sum() > 10
    # `last_time > maxTime` is out: a surfel exactly AT maxTime is kept, one tick later it is not
    assert (_predict(at[at[:, 3] > lc.SPLAT_CONF], 0, lc.MAX_TIME)[3] > 0).sum() > 100 and (_predict(above, 0, lc.MAX_TIME)[3] > 0).sum() == 0
    old, act = _predict(m, 0, lc.MAX_TIME), _predict(m, lc.TICK, lc.TICK)
    assert 1000 < (old[3] > 0).sum() < w * h and 1000 < (act[3] > 0).sum() < w * h
    assert ((old[3] > 0) & (act[3] == 0)).sum() > 100 and ((old[3] == 0) & (act[3] > 0)).sum() > 100
    assert (_predict(lc.splat_map("all_active"), 0, lc.MAX_TIME)[3] > 0).sum() == 0
    centre = (slice(h // 2 - 10, h // 2 + 10), slice(w // 2 - 10, w // 2 + 10))
    for kind, old_front in (("old_in_front", True), ("active_in_front", False)):
        old, act = _predict(lc.splat_map(kind), 0, lc.MAX_TIME), _predict(lc.splat_map(kind), lc.TICK, lc.TICK)
        zo, za = old[1][..., 2][centre], act[1][..., 2][centre]
        near, far = (zo, za) if old_front else (za, zo)
        assert (near > 0).all() and (near < 1.7).all() and (far > 1.8).all()      # each prediction sees through the other's surfels


# ------------------------------------------------------------------------------------------------ the constraint stage
def test_covariance_statement_is_the_oracles():
    import ctypes as C
    import orc
    for name, (track, _) in lc.ACCEPT_CASES.items():
        a = np.ascontiguousarray(track["lastA"], np.float64).reshape(36)
        want = np.zeros(36)
        with np.errstate(all="ignore"):
            orc.lib.orc_covariance(a.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p))
            got = lref.covariance(track["lastA"]).reshape(36)
        assert (np.isnan(got) == np.isnan(want)).all() and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]), name


def test_accept_cases_hit_their_thresholds_exactly():
    v, t = lc.cons_maps("all_valid")
    got = {}
    for name, (track, th) in lc.ACCEPT_CASES.items():
        got[name] = lref.local_constraints(track, v, t, lc.cons_pose(0), lc.CONS_TICK, lc.CONS_MAX_DEPTH, True, th)
        assert got[name]["accepted"] == lc.ACCEPT_WANT[name], name
        assert got[name]["n"] == (192 if lc.ACCEPT_WANT[name] else 0)
    diag = lambda name: np.diagonal(lref.covariance(lc.ACCEPT_CASES[name][0]["lastA"]))
    thr = np.float64(f32(lc.COV_POW2))
    assert (diag("cov_exactly_at_threshold") == thr).all()                       # equality passes
    d = diag("cov_one_ulp_above")
    assert d[4] == np.nextafter(thr, 1.0) and (np.delete(d, 4) == thr).all()     # one entry one ulp above: rejected by it alone
    assert lc.ACCEPT_CASES["count_exactly_at_threshold"][0]["icp_count"] == f32(40000) and lc.ACCEPT_CASES["count_one_above"][0]["icp_count"] == f32(40001)
    assert lc.ACCEPT_CASES["error_exactly_at_threshold"][0]["icp_error"] == f32(5e-5)
    assert lc.ACCEPT_CASES["error_one_ulp_below"][0]["icp_error"] == np.nextafter(f32(5e-5), f32(0))
    assert np.isnan(diag("singular_zero")).any() and not np.isfinite(diag("singular_one_column")).all()
    assert np.isnan(got["singular_zero"]["max_covariance"])
    piv = lc.ACCEPT_CASES["pivoting_lastA"][0]["lastA"]
    assert np.abs(piv[:, 0]).argmax() != 0 and 0 < diag("pivoting_lastA").max() < 1e-5
    assert np.allclose(lref.covariance(piv), np.linalg.inv(piv), rtol=1e-8, atol=0)


def test_sample_cases_take_their_branches():
    pose, track = lc.cons_pose(0), lc.good_track()
    n = {}
    for kind in lc.SAMPLE_CASES:
        v, t = lc.cons_maps(kind)
        for pin in (False, True):
            r = lref.local_constraints(track, v, t, pose, lc.CONS_TICK, lc.CONS_MAX_DEPTH, pin)
            assert r["accepted"] and r["n"] % (2 if pin else 1) == 0
            n[kind, pin] = r["n"]
            if pin and r["n"]:
                assert np.array_equal(r["src"][1::2], r["dst"][1::2]) and np.array_equal(r["dst"][0::2], r["dst"][1::2])
                assert (r["time"][0::2] == lc.CONS_TICK).all() and (r["time"][1::2] > 0).all() and (r["time"][1::2] < 100).all()
                assert np.abs(r["src"][0::2] - r["dst"][0::2]).max() > 0.01       # constraints of non-zero length: estPose, not currPose
    assert n["all_valid", False] == 96 and n["all_valid", True] == 192 and n["none_valid", True] == 0
    assert n["gaps_across_the_wave", False] == 96 - 9
    v, t = lc.cons_maps("z_at_max_depth")
    assert n["z_at_max_depth", False] == 96 - len(range(0, 96, 5)) - 2           # exactly maxDepth, negative and NaN out; one ulp below in
    assert n["old_time_zero", False] == 96 - len(range(3, 96, 7)) - 1
    # column by column: the second valid row is the sample one ROW down, not one column along
    v, t = lc.cons_maps("all_valid")
    r = lref.local_constraints(track, v, t, np.eye(4, dtype=f32), lc.CONS_TICK, lc.CONS_MAX_DEPTH, False)
    assert np.array_equal(r["src"][1], v[30, 10, :3]) and np.array_equal(r["src"][8], v[10, 30, :3])


def test_the_scenarios_drift_registers_and_is_accepted():
    """The drift factor of tests/test_local_loop_closure_gpu.py, chosen here: local_loop_scene.DRIFT = 1.004 (1.44 degrees after a full
    turn).  The oracle tracker on the ideal predictions of frame 105 and of the same view turned by the drift, in the call order of
    CoFusion.cpp:396-405: the registration converges (0.200 degrees left of 1.440, translation off 1e-4 m) and the accept rule passes with
    the default thresholds (ICP error 7.38e-6 < 5e-5, count 294 993 > 40 000, largest covariance diagonal 4.47e-6 <= 1e-5).  Frames that
    look at one flat wall head-on (115 .. 125) leave yaw and sideways translation coupled: their covariance is 2e-5 .. 4e-5 and the rule
    turns them away, as it should."""
    import local_loop_scene as sc
    fed, est, st = sc.oracle_registration()
    want = sc.wanted_pose(sc.RETURN_FRAME)
    before, after = sc.angle_between(fed, want), sc.angle_between(est, want)
    off = float(np.linalg.norm(est[:3, 3] - want[:3, 3]))
    lastA = np.array(st.lastA, np.float64).reshape(6, 6)
    diag = np.diag(np.asarray(lref.covariance(lastA), np.float64).reshape(6, 6))
    print("rotation off before", before, "after", after, "translation off", off, "icp error", st.last_icp_error, "count", st.last_icp_count,
          "covariance diagonal", diag)
    assert abs(before - sc.DRIFT_DEG) < 1e-3
    assert 2.0 * math.tan(math.radians(sc.DRIFT_DEG)) * 2.0 < 0.12      # constraints at 2 m are shorter than the global gate needs, with pins
    assert after < before / 4 and off < 0.01                            # it converges
    th = lref.LOCAL_DEFAULTS
    assert diag.max() <= th["cov_thresh"] and st.last_icp_count > th["icp_count_thresh"] and st.last_icp_error < th["icp_err_thresh"]
