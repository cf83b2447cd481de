"""GPU suite: relative constraints of the deformation graph (csrc/deform.hip through cf_deform_*_relative and the calls that take the
ring's pairs) stage by stage against the numpy statement tests/deform_rel_ref.py on the cases of tests/deform_rel_cases.py.

Exact: picked indices, ring contents, weight ids.  Bit for bit: weights, the entries and node slots of U, the relative residuals, the
inputs of mean_cons_error.  B (the band) and b: every entry within (m - 1) 2^-53 sum|terms| of the f64 statement.  Solve:
|delta_dev - delta*|_inf <= max(kappa e, 4 2^-53 |delta*|_inf), e = the error of numpy's dense Cholesky of A = B + U^T U against the
extended-precision solution delta*, kappa = max(8, 2 * the largest ratio of the STATED method's own error to e over the cases), computed
here on the machine the test runs on (table: test_cpu_deform_rel_ref.py).  One iteration: parameters within 1 ulp of f32 on the cases of
deform_rel_cases.ONE_ULP.  Free-running optimise: same flags and iteration count, errors within a relative 1e-5.  Every stage twice:
identical bytes.  An empty ring, or a ring whose only pair has no weight set: the bytes of an object without relative constraints."""
import numpy as np
import pytest

import deform_cases as dc
import deform_ref as ref
import deform_rel_cases as rc
import deform_rel_ref as rel

pytestmark = pytest.mark.gpu
f32 = np.float32
CAM = (60.0, 60.0, 32.0, 24.0)


@pytest.fixture(scope="module")
def rig():
    from co_fusion_amd import api, deform
    ctx = api.Context(64, 48, *CAM, max_models=2, max_surfels=8192)
    d = deform.Deform(ctx); d.enable_relative()
    plain = deform.Deform(ctx)
    yield ctx, d, plain
    d.close(); plain.close()
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def within_ulps(a, b, ulps=1):
    a = np.asarray(a, f32); b = np.asarray(b, f32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def _upload(d, c, params=None, pairs=True):
    d.set_nodes(c["nodes"], params)
    d.weights(c["src"], c["dst"], c["tm"])
    if pairs:
        d.set_relative(c["pairs"])


@pytest.fixture(scope="module")
def kappa():
    worst = 0.0
    for name in rc.CASES:
        star, direct, dense = rc.solved(name)
        worst = max(worst, float(np.abs(direct - star).max()) / float(np.abs(dense - star).max()))
    return max(8.0, 2.0 * worst)


# ------------------------------------------------------------------------------------------------ ring and pick
@pytest.mark.parametrize("appends", [127, 128, 129])
def test_ring_wraps_at_its_capacity(rig, appends):
    ctx, d, _ = rig
    rows = np.random.default_rng(appends).normal(size=(appends, 8)).astype(f32)
    want = rel.Ring(); want.append(rows)
    d.set_relative(rows[:100])
    dev = [ctx.to_device(rows[100:, 0:3].copy()), ctx.to_device(rows[100:, 4:7].copy()), ctx.to_device(rows[100:, 3].copy()), ctx.to_device(rows[100:, 7].copy())]
    d.set_relative_device(*dev, appends - 100, append=True)       # (enqueued: the arrays live until the download below has waited)
    assert d.relative_counts() == dict(capacity=128, count=want.count, appended=appends, used=d.relative_counts()["used"])
    assert np.array_equal(bits(d.download_relative()["pairs"]), bits(want.pairs()))
    d.set_relative(np.zeros((0, 8)))
    assert d.relative_counts()["count"] == 0


@pytest.mark.parametrize("pinned", [False, True], ids=["rows", "pinned"])
@pytest.mark.parametrize("n", rc.PICK_COUNTS)
def test_pick_appends_the_statements_pairs(rig, n, pinned):
    ctx, d, closure = rig
    nodes, params, src, dst, ts, td = rc.closure_rows(n)
    stride = 2 if pinned else 1
    S = np.full((stride * n, 3), 9.0, f32); D = np.full((stride * n, 3), 9.0, f32); T = np.full(stride * n, 9.0, f32)
    S[::stride] = src; D[::stride] = dst; T[::stride] = ts
    want = rel.Ring()
    want.append(np.full((126, 8), 1.0, f32))                     # the picks of the larger closures wrap the ring
    want.append(rel.pick(nodes, params, src, dst, ts, td))
    closure.set_nodes(nodes, params)
    dev = [ctx.to_device(a) for a in (S, D, T, td)]
    runs = []
    for _ in range(2):
        d.set_relative(np.full((126, 8), 1.0, f32))
        assert d.pick_relative(closure, *dev, n, stride) == len(rel.pick_indices(n))
        ctx.synchronize()
        runs.append(d.download_relative()["pairs"])
        assert d.relative_counts()["appended"] == want.total
    assert runs[0].tobytes() == runs[1].tobytes()
    assert np.array_equal(bits(runs[0]), bits(want.pairs()))
    d.set_relative(np.zeros((0, 8)))


# ------------------------------------------------------------------------------------------------ rows, residuals, the system
def _check_rows(got, sy, opt):
    assert np.array_equal(got["ids"][0], opt["ws"][0]) and np.array_equal(got["ids"][1], opt["wt"][0])
    for k, ws in enumerate((opt["ws"], opt["wt"])):
        assert np.array_equal(np.isnan(got["weights"][k]).all(1), ~ws[2])
        assert np.array_equal(bits(got["weights"][k][ws[2]]), bits(ws[1][ws[2]]))
    assert np.array_equal(got["u_ids"], sy["uid"])
    assert got["u_vals"].tobytes() == sy["uval"].tobytes()
    assert got["r_rel"].tobytes() == sy["r_rel"].tobytes()


def _check_system(got, n, sy):
    mA, sA, _, _ = ref.sum_bounds(n, sy["jr"], sy["r"])
    assert (np.abs(got["A"] - ref.to_band(sy["B"])) <= np.maximum(mA - 1, 0) * 2.0 ** -53 * sA).all()
    urows = rel.sparse_rows(sy["uid"], sy["uval"])
    mb, sb = rel.rhs_bounds(n, sy["jr"] + urows, np.concatenate([sy["r"], sy["r_rel"]]))
    assert (np.abs(got["b"] - sy["b"]) <= np.maximum(mb - 1, 0) * 2.0 ** -53 * sb).all()
    assert np.abs(sy["b"] - sy["b_B"]).max() > 0


@pytest.mark.parametrize("name", rc.CASES)
def test_rows_residuals_and_system(rig, name):
    _, d, _ = rig
    c = rc.case(name)
    first = None
    for _ in range(2):
        _upload(d, c)
        d.assemble()
        got = d.download(system=True); gr = d.download_relative(system=True)
        assert np.array_equal(got["ids"], c["opt"]["ids"]) and np.array_equal(bits(got["weights"]), bits(c["opt"]["w"]))
        _check_rows(gr, c["sys"], c["opt"])
        _check_system(got, len(c["nodes"]), c["sys"])
        run = (got["A"].tobytes(), got["b"].tobytes(), gr["u_vals"].tobytes(), gr["r_rel"].tobytes())
        first = first or run
        assert first == run


def test_rows_at_a_bent_state(rig):
    """general rotations under the relative residuals: the state the accepted loop closure ends in"""
    _, d, _ = rig
    c = rc.case("loop3"); o = c["opt"]
    sy = rel.system(c["nodes"], o["params"], c["src"], c["dst"], o["ids"], o["w"], o["ok"], c["pairs"], o["ws"], o["wt"])
    _upload(d, c, o["params"])
    d.assemble()
    _check_rows(d.download_relative(system=True), sy, o)
    _check_system(d.download(system=True), 45, sy)


# ------------------------------------------------------------------------------------------------ nothing changes without pairs
def test_an_empty_ring_is_the_plain_object_byte_for_byte(rig):
    _, d, plain = rig
    c = rc.case("loop3")
    outs = []
    for obj in (d, plain):
        _upload(obj, c, pairs=False)
        if obj is d:
            d.set_relative(np.zeros((0, 8)))
        obj.assemble()
        sysm = obj.download(system=True)
        step = obj.iterate()
        after = obj.download(system=True)
        outs.append((sysm["A"].tobytes(), sysm["b"].tobytes(), after["b"].tobytes(), after["params"].tobytes(), after["A"].tobytes(),
                     step["error"].tobytes(), step["mean_cons_error"].tobytes(), step["delta_norm"], step["failed"], obj.download_out()))
    assert outs[0] == outs[1] and len(outs[0][-1]) == 32


def test_a_pair_without_weights_leaves_delta_to_the_split_solve(rig):
    """one pair whose source has no weight set: U is empty, so the factor / finish halves of the solve kernel, with Y, C and the correction
    between them, must leave the bytes of the unsplit kernel -- while the pair's residual and its count in the mean are present"""
    _, d, plain = rig
    c = rc.case("nan")
    outs = []
    for obj in (d, plain):
        _upload(obj, c, pairs=False)
        if obj is d:
            d.set_relative(c["pairs"][1:2])
        step = obj.iterate()
        after = obj.download(system=True)
        outs.append((after["A"].tobytes(), after["b"].tobytes(), after["params"].tobytes(), step["delta_norm"], step["failed"]))
        if obj is d:
            gr = d.download_relative(system=True)
            assert (gr["u_ids"] == -1).all() and np.array_equal(gr["C"], np.eye(3)) and not gr["z"].any()
            rel_step = step
    assert outs[0] == outs[1]
    assert rel_step["error"] > step["error"]
    assert abs(float(rel_step["mean_cons_error"]) - float(step["mean_cons_error"]) * 100 / 101) <= 1e-6 * float(step["mean_cons_error"])


# ------------------------------------------------------------------------------------------------ solve, iterate, optimise
def test_solve_and_one_iteration(rig, kappa):
    _, d, _ = rig
    print(f"\n   kappa {kappa:.1f}\n   case      e = |numpy - star|   |stated - star|   |device - star|   allowed")
    for name in rc.CASES:
        c = rc.case(name); o = c["opt"]
        star, direct, dense = rc.solved(name)
        want = rel.iterate(c["nodes"], ref.identity_params(len(c["nodes"])), c["src"], c["dst"], o["ids"], o["w"], o["ok"], c["pairs"], o["ws"], o["wt"])
        e = float(np.abs(dense - star).max())
        runs = []
        for _ in range(2):
            _upload(d, c)
            got = d.iterate()
            dl = d.download(system=True); gr = d.download_relative(system=True)
            runs.append((dl["b"].tobytes(), dl["params"].tobytes(), got["error"].tobytes(), gr["C"].tobytes(), gr["z"].tobytes()))
        assert runs[0] == runs[1]
        err = float(np.abs(dl["b"] - star).astype(np.float64).max())
        allowed = max(kappa * e, 4 * 2.0 ** -53 * float(np.abs(star).max()))
        print(f"   {name:8s}  {e:.3e}            {float(np.abs(direct - star).max()):.3e}         {err:.3e}         {allowed:.3e}")
        assert not got["failed"] and err <= allowed
        C = c["C"]
        assert np.abs(gr["C"] - C).max() <= 1e-9 * np.abs(C).max()          # (a derived quantity: Y carries the forward substitution's error)
        if name in rc.ONE_ULP:
            assert within_ulps(dl["params"], want["params"]).all()
        assert abs(float(got["error"]) - float(want["error"])) <= 1e-5 * float(want["error"])
        assert abs(got["delta_norm"] - want["delta_norm"]) <= 1e-6 * want["delta_norm"]


@pytest.mark.parametrize("name", rc.CASES)
def test_free_running_optimise(rig, name):
    _, d, _ = rig
    c = rc.case(name); o = c["opt"]
    runs = []
    for _ in range(2):
        _upload(d, c)
        got = d.optimise()
        runs.append((sorted((k, np.asarray(v).tobytes()) for k, v in got.items()), d.download()["params"].tobytes()))
    assert runs[0] == runs[1]
    assert d.relative_counts()["used"] == len(c["pairs"])
    for k in ("optimised", "accepted", "failed", "iterations"):
        assert got[k] == o[k], (k, got, {k: o[k] for k in got})
    for k in ("error_before", "mean_cons_error_before", "error", "mean_cons_error"):
        assert abs(float(got[k]) - float(o[k])) <= 1e-5 * abs(float(o[k])), (k, got[k], o[k])


def test_the_pairs_keep_what_a_local_closure_registered(rig):
    _, d, plain = rig
    c = rc.case("loop3"); o = c["opt"]
    _upload(d, c)
    assert d.optimise()["accepted"]
    _upload(plain, c, pairs=False)
    assert plain.optimise()["accepted"]
    with_pairs = rel.gap(c["nodes"], d.download()["params"], c["pairs"], o["ws"], o["wt"])
    without = rel.gap(c["nodes"], plain.download()["params"], c["pairs"], o["ws"], o["wt"])
    want = rel.gap(c["nodes"], o["params"], c["pairs"], o["ws"], o["wt"])
    print(f"\n   |phi(src) - phi(tgt)|  without the pairs {without.max():.4f}  with {with_pairs.max():.4f}  (statement {want.max():.4f})")
    assert (with_pairs < without).all() and np.abs(with_pairs - want).max() < 1e-5


def test_the_denominator_alone_closes_the_gate(rig):
    _, d, _ = rig
    nodes, src, dst, tm, pairs = rc.gate_case()
    want = rel.optimise(nodes, src, dst, tm, pairs)
    d.set_nodes(nodes); d.weights(src, dst, tm); d.set_relative(pairs)
    got = d.optimise()
    assert not got["optimised"] and got["iterations"] == 0
    assert got["mean_cons_error_before"].tobytes() == want["mean_cons_error_before"].tobytes()      # the inputs are equal bit for bit
    d.set_relative(np.zeros((0, 8)))
    d.set_nodes(nodes); d.weights(src, dst, tm)
    assert d.optimise()["optimised"]


def test_the_local_mode_refuses_pairs(rig):
    from co_fusion_amd import api
    _, d, plain = rig
    c = rc.case("path21")
    _upload(d, c)
    for call in (lambda: d.assemble(0), lambda: d.iterate(0), lambda: d.optimise_local(0)):
        with pytest.raises(api.CofusionError):
            call()
    with pytest.raises(api.CofusionError):
        plain.set_relative(c["pairs"])                            # not enabled
    with pytest.raises(api.CofusionError):
        d.set_relative(np.zeros((129, 8)))
    d.set_relative(np.zeros((0, 8)))
    assert not d.iterate(0)["failed"]                             # an empty ring: the local mode as ever


# ------------------------------------------------------------------------------------------------ the allocation limit
def test_1024_nodes_128_pairs(rig):
    """every slot of the ring in use on CF_DEFORM_MAX_NODES nodes: 384 columns of Y over 1024 block rows, C of 384 x 384.  A of 12288^2
    is not held densely: delta* comes from refinement in extended precision (deform_rel_ref.solve_star_band), and the yardstick e is the
    error of the stated method itself (deform_ref's band routines), as the 1024-node test of test_deform_gpu.py takes the band routine.
    That yardstick already carries the method's loss of digits, so the factor is the existing direct-solve one, 8, not kappa."""
    _, d, _ = rig
    c = rc.big_case(); n = dc.BIG
    nodes, pairs = c["nodes"], c["pairs"]
    ids, w, ok = ref.weights(nodes, c["src"], c["tm"])
    ws, wt = rel.rel_weights(nodes, pairs)
    assert ok.all() and ws[2].all() and wt[2].all()
    P0 = ref.identity_params(n)
    jr, r = ref.rows(nodes, P0, c["src"], c["dst"], ids, w, ok)
    AB, bB = ref.band_system(n, jr, r)
    uid, uval = rel.compact_rows(nodes, pairs, ws, wt)
    assert (uid[:, :4].min(1) - uid[:, 4:].max(1) > 900).all()
    U = rel.dense_rows(n, uid, uval)
    rr = rel.rel_residual(nodes, P0, pairs, ws, wt)
    b = rel.rel_rhs(bB, U, rr)
    _upload(d, c)
    d.assemble()
    got = d.download(system=True); gr = d.download_relative(system=True)
    _check_rows(gr, dict(uid=uid, uval=uval, r_rel=rr), dict(ws=ws, wt=wt))
    mA, sA, _, _ = ref.sum_bounds(n, jr, r)
    mb, sb = rel.rhs_bounds(n, jr + rel.sparse_rows(uid, uval), np.concatenate([r, rr]))
    assert (np.abs(got["A"] - AB) <= np.maximum(mA - 1, 0) * 2.0 ** -53 * sA).all() and (np.abs(got["b"] - b) <= np.maximum(mb - 1, 0) * 2.0 ** -53 * sb).all()
    star = rel.solve_star_band(AB, U, b)
    direct, _ = rel.solve(AB, U, b)
    e = float(np.abs(direct - star).max())
    step = d.iterate()
    delta = d.download(system=True)["b"]
    err = float(np.abs(delta - star).astype(np.float64).max())
    allowed = max(8 * e, 4 * 2.0 ** -53 * float(np.abs(star).max()))
    print(f"\n   1024 nodes, 128 pairs  e {e:.3e}  device {err:.3e}  ratio {err / e:.2f}  allowed {allowed:.3e}  error {step['error']}")
    assert not step["failed"] and err <= allowed
