"""GPU suite: the local mode of the deformation graph (cf_deform_create_sized, cf_deform_assemble_local / _iterate_local /
_optimise_local in csrc/cabi_deform.hip, the kernels of csrc/deform.hip) against the numpy statement tests/local_loop_ref.py on the cases
of tests/local_loop_cases.py, which reuse the node sets of tests/deform_cases.py.

last_deform_time = 0 on node times >= 1: A_band, b and the first iterate byte-identical to cf_deform_assemble / cf_deform_iterate of a
128-capacity object.  Disabled nodes: enabled entries within (m - 1) 2^-53 sum|terms| of the statement's f64 J^T J (the bound of a sum
taken in another order), disabled blocks exactly identity / zero, delta of disabled nodes exactly 0, dropped rows absent from `error`.
Solve: |delta_dev - delta*|_inf <= max(8 e, 4 2^-53 |delta*|_inf) with e = numpy's own Cholesky error on the same system against the
extended-precision solution delta*.  768 + 768 constraints: weight sets exact / bit for bit, the system within the summation bound.
Free-running cf_deform_optimise_local: same flags and iteration count, errors within a relative 1e-5.  Every stage twice: identical
bytes."""
import numpy as np
import pytest

import deform_cases as dc
import deform_ref as ref
import local_loop_cases as lc
import local_loop_ref as lref

pytestmark = pytest.mark.gpu
f32 = np.float32
ident = lambda cases: ["-".join(str(x) for x in c) for c in cases]


@pytest.fixture(scope="module")
def rig():
    from co_fusion_amd import api, deform
    ctx = api.Context(64, 48, 60.0, 60.0, 32.0, 24.0, max_models=2, max_surfels=8192)
    small, big = deform.Deform(ctx), deform.Deform(ctx, deform.MAX_CONSTRAINTS_SIZED)
    yield ctx, small, big
    small.close(); big.close()
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _upload(d, s, params=None):
    d.set_nodes(s["nodes"], params)
    d.weights(s["src"], s["dst"], s["tm"])


def _within_bound(got, n, jr, r, want_AB, want_b):
    mA, sA, mb, sb = ref.sum_bounds(n, jr, r)
    errA = np.abs(got["A"] - want_AB); errb = np.abs(got["b"] - want_b)
    assert (errA <= np.maximum(mA - 1, 0) * 2.0 ** -53 * sA).all(), np.argwhere(errA > np.maximum(mA - 1, 0) * 2.0 ** -53 * sA)[:5]
    assert (errb <= np.maximum(mb - 1, 0) * 2.0 ** -53 * sb).all()
    return mA


def test_capacity_is_checked(rig):
    from co_fusion_amd import api, deform
    ctx, small, big = rig
    for bad in (0, deform.MAX_CONSTRAINTS_SIZED + 1):
        with pytest.raises(api.CofusionError):
            deform.Deform(ctx, bad)
    nodes = dc.make_nodes(12)
    big.set_nodes(nodes)
    with pytest.raises(api.CofusionError):
        big.weights(np.zeros((1537, 3)), np.zeros((1537, 3)), np.zeros(1537))
    small.set_nodes(nodes)
    with pytest.raises(api.CofusionError):
        small.weights(np.zeros((129, 3)), np.zeros((129, 3)), np.zeros(129))
    few = deform.Deform(ctx, 7)
    few.set_nodes(nodes)
    few.weights(np.zeros((7, 3)), np.zeros((7, 3)), np.zeros(7))
    with pytest.raises(api.CofusionError):
        few.weights(np.zeros((8, 3)), np.zeros((8, 3)), np.zeros(8))
    few.close()


# ------------------------------------------------------------------------------------------------ every node enabled
@pytest.mark.parametrize("n,kind,which", lc.IDENTICAL, ids=ident(lc.IDENTICAL))
def test_last_deform_time_zero_is_the_global_mode_byte_for_byte(rig, n, kind, which):
    _, small, big = rig
    s = lc.system(n, kind, which)
    assert s["ldt"] == 0
    _upload(small, s)
    small.assemble()
    g = small.download(system=True)
    want = [g["ids"].tobytes(), g["weights"].tobytes(), g["A"].tobytes(), g["b"].tobytes()]
    gauge_free = kind in dc.GAUGE_FREE
    if not gauge_free:
        st = small.iterate()
        g = small.download(system=True)
        want += [g["b"].tobytes(), g["params"].tobytes(), np.asarray([st["error"], st["mean_cons_error"]], f32).tobytes(),
                 np.float64(st["delta_norm"]).tobytes(), st["failed"]]
    for d in (small, big):
        for _ in range(2):
            _upload(d, s)
            d.assemble(0)
            l = d.download(system=True)
            got = [l["ids"].tobytes(), l["weights"].tobytes(), l["A"].tobytes(), l["b"].tobytes()]
            if not gauge_free:
                st = d.iterate(0)
                l = d.download(system=True)
                got += [l["b"].tobytes(), l["params"].tobytes(), np.asarray([st["error"], st["mean_cons_error"]], f32).tobytes(),
                        np.float64(st["delta_norm"]).tobytes(), st["failed"]]
            assert got == want


# ------------------------------------------------------------------------------------------------ disabled nodes
@pytest.mark.parametrize("n,kind,which", lc.DISABLED, ids=ident(lc.DISABLED))
def test_disabled_nodes_leave_the_system(rig, n, kind, which):
    _, _, d = rig
    s = lc.system(n, kind, which)
    on = np.repeat(s["en"], 12)
    first = None
    for _ in range(2):
        _upload(d, s)
        d.assemble(s["ldt"])
        got = d.download(system=True)
        if len(s["src"]):
            assert np.array_equal(got["ids"], s["opt"]["ids"]) and np.array_equal(bits(got["weights"]), bits(s["opt"]["w"]))
        _within_bound(got, n, s["jr"], s["r"], ref.to_band(s["A"]), s["b"])
        # a disabled node: the identity on the diagonal of its rows, exact zeros in the rest of them and in its columns, zero in b
        assert np.array_equal(got["A"][~on, 0], np.ones(int((~on).sum()))) and not got["A"][~on, 1:].any() and not got["b"][~on].any()
        i, dd = np.indices(got["A"].shape)
        col = i - dd
        assert not got["A"][(col >= 0) & ~on[np.clip(col, 0, None)] & (dd > 0)].any()
        first = first or (got["A"].tobytes(), got["b"].tobytes())
        assert first == (got["A"].tobytes(), got["b"].tobytes())


def test_dropped_rows_are_absent_from_the_error(rig):
    _, _, d = rig
    s = lc.system(45, "dead_one", "half")
    o = s["opt"]
    assert float(o["error_before"]) == float(ref.error_of(s["r"]))
    _upload(d, s)
    th = None
    got = d.optimise_local(s["ldt"], th)
    want = float(o["error_before"])
    assert abs(float(got["error_before"]) - want) <= 1e-5 * want
    # with every row kept the dead constraint alone adds (10 * 0.3)^2 = 9: far outside that tolerance
    _, r_all = ref.rows(s["nodes"], ref.identity_params(45), s["src"], s["dst"], o["ids"], o["w"], o["ok"])
    assert float(ref.error_of(r_all)) - want > 8.9
    # ... and the mean constraint error still counts it
    assert abs(float(got["mean_cons_error_before"]) - float(o["mean_cons_error_before"])) <= 1e-5 * float(o["mean_cons_error_before"])


HALF = [c for c in lc.DISABLED if c[2] == "half"]


def test_solve_with_disabled_nodes(rig):
    _, _, d = rig
    print("\n   case                 e = |numpy - star|   |device - star|   ratio   allowed")
    for n, kind, which in HALF:
        s = lc.system(n, kind, which)
        o = s["opt"]
        on = np.repeat(s["en"], 12)
        want = lref.iterate(s["nodes"], ref.identity_params(n), s["src"], s["dst"], o["ids"], o["w"], o["ok"], s["ldt"])
        star = ref.solve_star(ref.to_band(s["A"]), s["b"])
        e = float(np.abs(ref._tri(np.linalg.cholesky(s["A"]), s["b"]) - star).max())
        runs = []
        for _ in range(2):
            _upload(d, s)
            got = d.iterate(s["ldt"])
            dl = d.download(system=True)
            runs.append((dl["b"].tobytes(), dl["params"].tobytes(), got["error"].tobytes()))
        assert runs[0] == runs[1]
        err = float(np.abs(dl["b"] - star).astype(np.float64).max())
        allowed = max(8 * e, 4 * 2.0 ** -53 * float(np.abs(star).max()))
        print(f"   {n:4d}-{kind:8s}-{which}  {e:.3e}            {err:.3e}        {err / e if e else float('inf'):6.2f}   {allowed:.3e}")
        assert not got["failed"] and err <= allowed
        assert not dl["b"][~on].any()                                                     # delta of a disabled node: exactly 0
        assert dl["params"][~s["en"]].tobytes() == ref.identity_params(n)[~s["en"]].tobytes()
        a = np.asarray(dl["params"], f32); b = np.asarray(want["params"], f32)
        assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)).all()
        assert abs(float(got["error"]) - float(want["error"])) <= 1e-5 * float(want["error"])
        assert abs(got["delta_norm"] - want["delta_norm"]) <= 1e-9 * want["delta_norm"]


# ------------------------------------------------------------------------------------------------ 768 + 768 constraints
@pytest.mark.parametrize("n,which", lc.BIG, ids=[f"{n}-{w}" for n, w in lc.BIG])
def test_1536_constraints(rig, n, which):
    ctx, _, d = rig
    s = lc.big_system(n, which)
    on = np.repeat(s["en"], 12)
    dev = [ctx.to_device(np.ascontiguousarray(s[k], f32)) for k in ("src", "dst", "tm")]
    first = None
    for k in range(2):
        d.set_nodes(s["nodes"])
        if k == 0:
            d.weights(s["src"], s["dst"], s["tm"])
        else:
            d.weights_device(*dev, len(s["src"]))          # the packing launch over twelve workgroups
        d.assemble(s["ldt"])
        got = d.download(system=True)
        assert got["ids"].shape == (1536, 4) and np.array_equal(got["ids"], s["ids"]) and np.array_equal(bits(got["weights"]), bits(s["w"]))
        _within_bound(got, n, s["jr"], s["r"], s["AB"], s["b"])
        assert np.array_equal(got["A"][~on, 0], np.ones(int((~on).sum()))) and not got["A"][~on, 1:].any() and not got["b"][~on].any()
        first = first or (got["A"].tobytes(), got["b"].tobytes())
        assert first == (got["A"].tobytes(), got["b"].tobytes())
    # the residual pass over all 1536: error and mean constraint error of the statement
    st = d.optimise_local(s["ldt"], _one_iteration(ctx))
    want_mean = float(ref.cons_error(s["nodes"], ref.identity_params(n), s["src"], s["dst"], s["ids"], s["w"], s["ok"]))
    assert abs(float(st["error_before"]) - float(ref.error_of(s["r"]))) <= 1e-5 * float(ref.error_of(s["r"]))
    assert abs(float(st["mean_cons_error_before"]) - want_mean) <= 1e-5 * want_mean
    assert st["optimised"] and st["accepted"] and not st["failed"] and float(st["error"]) < float(st["error_before"])


def _one_iteration(ctx):
    from co_fusion_amd import deform
    th = deform.default_thresholds(ctx.lib)
    th.max_iterations = 1
    return th


# ------------------------------------------------------------------------------------------------ optimise
@pytest.mark.parametrize("n,kind,which", lc.FREE_RUNNING, ids=ident(lc.FREE_RUNNING))
def test_free_running_optimise_local(rig, n, kind, which):
    _, _, d = rig
    s = lc.system(n, kind, which)
    o = s["opt"]
    runs = []
    for _ in range(2):
        _upload(d, s)
        got = d.optimise_local(s["ldt"])
        runs.append((sorted((k, np.asarray(v).tobytes()) for k, v in got.items()), d.download()["params"].tobytes()))
    assert runs[0] == runs[1]
    for k in ("optimised", "accepted", "failed", "iterations"):
        assert got[k] == o[k], (k, got, {k: o[k] for k in got})
    for k in ("error_before", "mean_cons_error_before", "error", "mean_cons_error"):
        assert abs(float(got[k]) - float(o[k])) <= 1e-5 * abs(float(o[k])), (k, got[k], o[k])
    if not o["optimised"]:
        assert d.download()["params"].tobytes() == ref.identity_params(n).tobytes()


def test_the_local_mode_takes_what_the_global_mode_turns_away(rig):
    _, small, _ = rig
    s = lc.system(12, "small", "zero")
    _upload(small, s)
    assert not small.optimise()["optimised"]                       # the 0.06 gate
    got = small.optimise_local(0)
    assert got["optimised"] and got["accepted"] and got["iterations"] == s["opt"]["iterations"]
    s = lc.system(21, "far", "zero")
    _upload(small, s)
    g = small.optimise()
    assert g["optimised"] and g["iterations"] == 1 and float(g["error"]) > 10 and not g["accepted"]     # `error > 10` after the first iteration
    _upload(small, s)
    got = small.optimise_local(0)
    assert got["iterations"] == 3 and got["accepted"] and float(got["error"]) < 0.1 * float(g["error"])


def test_a_failed_step_and_no_enabled_node_leave_the_parameters(rig):
    _, _, d = rig
    nodes, params, ldt = lc.singular_half()
    none = (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0))
    d.set_nodes(nodes, params)
    d.weights(*none)
    got = d.optimise_local(ldt)
    assert got["optimised"] and got["failed"] and not got["accepted"] and got["iterations"] == 1
    assert d.download()["params"].tobytes() == params.tobytes()
    # no node enabled, from parameters away from the identity: not optimised, nothing written
    s = lc.system(21, "shift", "half")
    bent = dc.bent_params(21, seed=4)
    _upload(d, s, bent)
    got = d.optimise_local(int(s["nodes"][-1, 3]))
    assert not got["optimised"] and not got["accepted"] and not got["failed"] and got["iterations"] == 0
    assert d.download()["params"].tobytes() == bent.tobytes()
