"""CPU suite: what the case table of the SO(3) pre-alignment (tests/so3_cases.py) covers, from the oracle's trace.

orc_so3_prealign is the loop of the oracle's tracking function (the existing tracking pins prove the extraction changed nothing); its
trace records error, count, branch and zero pivots of every iteration.  Here every case is shown to take the exit, at the iteration,
its row of so3_cases.EXPECT claims, and to have the property it is named for; the table as a whole is shown to cover exits at
iterations 2, 3, >= 4 and 10, a count of 0, a NaN error, a singular matrix and an identity result after a revert.  The rotated pairs
are checked against the TRUE rotation in float64; orc_so3_prealign_state against the identity hand-over."""
import ctypes as C
import math

import numpy as np
import pytest

import orc
import so3_cases as sc

ALL = [(c.name, c.shape) for c in sc.content_cases()]
IDS = [c.key for c in sc.content_cases()]
EYE = np.eye(3)


def _bits(v):
    return np.float32(v).tobytes()


def _exit(trace):
    return "ten" if trace[-1]["branch"] == "step" else trace[-1]["branch"]


def test_the_table_is_complete():
    assert set(sc.EXPECT) == set(sc.CONTENT) and len(set(sc.CONTENT)) == len(sc.CONTENT)
    assert all(len(v) == len(sc.SHAPES) for v in sc.EXPECT.values())
    for name, members in sc.BATCHES.items():
        assert len(members) == int(name[1:]) and all(n in sc.CONTENT and s in sc.SHAPES for n, s in members)
    assert sorted(len(m) for m in sc.BATCHES.values()) == [1, 3, 9, 16]
    for w, h in sc.SHAPES:      # what cf_so3_prealign_step accepts
        assert w % 16 == 0 and h % 4 == 0
    assert set(sc.level2(s) for s in sc.SHAPES) == {(40, 30), (44, 33), (160, 120)}


@pytest.mark.parametrize("name,shape", ALL, ids=IDS)
def test_case_takes_the_exit_its_row_claims(name, shape):
    c = sc.case(name, shape)
    R, st, trace = sc.reference(name, shape)
    print(c.key, [(t["err"], t["count"], t["branch"], t["zero_pivots"]) for t in trace])
    iterations, how = c.expect
    assert (st.so3_iterations, _exit(trace)) == (iterations, how) and len(trace) == iterations
    assert all(t["branch"] == "step" for t in trace[:-1])
    if how == "reverted":       # the statistics are those of the iteration before, and the error did rise by more than 0.001
        assert _bits(st.last_so3_error) == _bits(trace[-2]["err"]) and _bits(st.last_so3_count) == _bits(trace[-2]["count"])
        assert float(trace[-1]["err"]) > float(trace[-2]["err"]) + 0.001
    else:
        assert _bits(st.last_so3_error) == _bits(trace[-1]["err"]) and _bits(st.last_so3_count) == _bits(trace[-1]["count"])
    # the camera the table promises, at level 2
    cols, rows = sc.level2(shape)
    il = c.intr.level(2)
    scale = sc.CAMERA_SCALE.get(name, 1.0)
    assert (il.fx, il.fy, il.cx, il.cy) == (np.float32(0.825 * cols * scale), np.float32(0.825 * cols * scale), np.float32((cols - 1) / 2 - 0.375),
                                            np.float32((rows - 1) / 2 - 0.375))


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_named_properties(shape):
    cols, rows = sc.level2(shape)
    inner = (cols - 2) * (rows - 2)
    ref = lambda n: sc.reference(n, shape)

    R, st, tr = ref("identical")
    assert np.array_equal(sc.case("identical", shape).last, sc.case("identical", shape).next)
    assert all(t["err"] == 0 and t["count"] == inner and t["zero_pivots"] == 0 for t in tr) and R.tobytes() == EYE.tobytes()

    for name in ("rot_small", "rot_mid", "rot_large", "rot_wide"):
        R, st, tr = ref(name)
        assert all(t["zero_pivots"] == 0 for t in tr) and not np.array_equal(R, EYE), name
        assert len({t["count"] for t in tr}) >= 2, name                      # accepted steps moved pixels across the border

    R, st, tr = ref("noise")
    same = [k for k in range(1, len(tr)) if _bits(tr[k]["err"]) == _bits(tr[0]["err"]) and tr[k]["count"] == tr[0]["count"]]
    assert same[:3] == [1, 2, 3], "the first steps change nothing the rounding sees"
    assert not np.array_equal(R, EYE)                                        # ... while the rotation accumulates

    R, st, tr = ref("stripes")
    last, nxt = sc.case("stripes", shape).last, sc.case("stripes", shape).next
    assert np.array_equal(last[:, :-1], nxt[:, 1:]) and (last == last[:1]).all()    # shifted one column; no gradient along y
    assert tr[0]["err"] > 0 and all(t["err"] == 0 for t in tr[1:]) and len(tr) == 10

    for name, err in (("flat", lambda n: 0.0), ("flat_offset", lambda n: 8.0 / math.sqrt(n)), ("extreme", lambda n: 255.0 / math.sqrt(n))):
        R, st, tr = ref(name)
        assert all(t["zero_pivots"] == 3 and t["count"] == inner for t in tr), name          # the all-zero matrix
        assert all(_bits(t["err"]) == _bits(tr[0]["err"]) for t in tr) and abs(tr[0]["err"] - err(inner)) <= 1e-6 * err(inner), name
        assert R.tobytes() == EYE.tobytes(), name                                            # zero pivots give a zero update

    R, st, tr = ref("ejected")
    assert tr[0]["count"] == inner and tr[0]["zero_pivots"] == 0
    assert all(t["count"] == 0 and math.isnan(t["err"]) and t["zero_pivots"] == 3 for t in tr[1:]) and len(tr) == 10
    assert math.isnan(st.last_so3_error) and st.last_so3_count == 0 and not np.array_equal(R, EYE)

    c = sc.case("saturated", shape)
    J = np.abs(sc.first_rows(c))
    over = int((J.max(axis=-1) > sc.CLAMP).sum())
    print("saturated", shape, "row entries up to %.4g (clamp %g) in %d of %d pixels" % (J.max(), sc.CLAMP, over, J.shape[0] * J.shape[1]))
    assert J.max() > 1.5 * sc.CLAMP and 0 < over * 2.0 ** 50 < 2.0 ** 62     # far beyond the clamp; the 64-bit sums cannot wrap
    J1 = np.abs(sc.first_rows(sc.case("rot_wide", shape)))
    assert J1.max() < sc.CLAMP / 16                                          # ... and no other camera of the table comes near it


def test_revert_to_identity():
    shape = sc.SHAPES[0]
    R, st, tr = sc.reference("revert_to_identity", shape)
    assert [t["branch"] for t in tr] == ["step", "reverted"] and st.so3_iterations == 2
    assert R.tobytes() == EYE.tobytes()                                      # lastResultR of iteration 1
    assert tr[0]["zero_pivots"] == 0                                         # a real step was taken and thrown away
    assert _bits(st.last_so3_error) == _bits(tr[0]["err"]) and _bits(st.last_so3_count) == _bits(tr[0]["count"])


def test_what_the_table_covers():
    exits = {}
    for c in sc.content_cases():
        R, st, tr = sc.reference(c.name, c.shape)
        exits.setdefault((_exit(tr), st.so3_iterations), []).append(c.key)
    reverted = sorted(k for how, k in exits if how == "reverted")
    assert 2 in reverted and 3 in reverted and any(k >= 4 for k in reverted), reverted
    assert ("ten", 10) in exits
    traces = [sc.reference(c.name, c.shape) for c in sc.content_cases()]
    assert any(t["count"] == 0 for _, _, tr in traces for t in tr)
    assert any(math.isnan(t["err"]) for _, _, tr in traces for t in tr)
    assert any(t["zero_pivots"] == 3 for _, _, tr in traces for t in tr)
    assert any(tr[-1]["branch"] == "reverted" and R.tobytes() == EYE.tobytes() for R, _, tr in traces)
    # known gap (so3_cases docstring): no case takes the "converged" exit
    assert not any(t["branch"] == "converged" for _, _, tr in traces for t in tr)
    # every batch mixes exits where it has more than one model; models 0 and 8 of the nine leave at different iterations
    for name, members in sc.BATCHES.items():
        its = [sc.reference(n, s)[1].so3_iterations for n, s in members]
        assert len(members) == 1 or len(set(its)) > 1, name
    n3 = [sc.reference(n, s) for n, s in sc.BATCHES["n3"]]
    assert n3[0][1].so3_iterations < 10 and n3[1][1].so3_iterations == 10 and math.isnan(n3[2][1].last_so3_error)
    n9 = [sc.reference(n, s)[1].so3_iterations for n, s in sc.BATCHES["n9"]]
    assert n9[0] != n9[8]


@pytest.mark.parametrize("name,shape", [k for k in ALL if k[0].startswith("rot_")], ids=[i for i in IDS if i.startswith("rot_")])
def test_rotated_pairs_against_the_true_rotation(name, shape):
    """independent of the oracle's arithmetic: the float64 geodesic distance between the oracle's rotation and the rotation the pair
    was generated with is below half the true angle -- the pre-alignment beats doing nothing by 2x"""
    R, st, tr = sc.reference(name, shape)
    angle = sc.ANGLES[name]
    true = sc.rotation(sc.AXIS, angle)
    assert abs(sc.geodesic(EYE, true) - angle) < 1e-12
    assert not np.array_equal(R, EYE)
    d = sc.geodesic(R, true)
    print("%s@%dx%d: geodesic distance %.3e rad = %.3f of the true angle" % (name, shape[0], shape[1], d, d / angle))
    assert abs(np.linalg.det(R) - 1) < 1e-5 and np.abs(R.dot(R.T) - EYE).max() < 1e-5       # a rotation, to float32
    assert d < sc.GEODESIC_CAP * angle


@pytest.mark.parametrize("first_level", [0, 1, 2])
def test_state_without_prealignment_is_the_identity_hand_over(first_level):
    c = sc.case("rot_mid", sc.SHAPES[1])
    s = orc.GnState()
    C.memset(C.byref(s), 0x5A, C.sizeof(s))
    s.intr = c.intr; s.width, s.height = c.shape
    out = orc.so3_prealign_state(s, None, None, False, first_level)
    assert np.array(out.resultRt).tobytes() == np.eye(4).reshape(16).tobytes()
    # as VALUES: the affine inverse negates a zero translation, kt holds -0.0f (the GPU suite compares the bits with the device's)
    assert np.array_equal(np.array(out.krkInv, np.float32).reshape(3, 3), np.eye(3, dtype=np.float32))
    assert np.array_equal(np.array(out.kt, np.float32), np.zeros(3, np.float32))
    assert out.lastRGBError == np.finfo(np.float32).max and out.level_done == 0 and list(out.residual) == [0.0, 0.0]
    assert (out.stats.so3_iterations, out.stats.last_so3_error, out.stats.last_so3_count) == (0, 0.0, 0.0)
    # nothing else is written
    for f in ("Rprev", "tprev", "Rcurr", "tcurr"):
        assert bytes(getattr(out, f)) == bytes(getattr(s, f)), f
    assert (out.solves, out.icp, out.rgb, out.rgbOnly) == (s.solves, s.icp, s.rgb, s.rgbOnly)


@pytest.mark.parametrize("first_level", [0, 2])
def test_state_with_prealignment_carries_the_loop_result(first_level):
    c = sc.case("rot_large", sc.SHAPES[0])
    R, st, _ = sc.reference(c.name, c.shape)
    s = orc.GnState()
    s.intr = c.intr; s.width, s.height = c.shape
    out = orc.so3_prealign_state(s, c.last, c.next, True, first_level)
    Rt = np.array(out.resultRt).reshape(4, 4)
    assert Rt[:3, :3].tobytes() == R.tobytes() and Rt[:, 3].tolist() == [0, 0, 0, 1] and Rt[3].tolist() == [0, 0, 0, 1]
    assert (out.stats.so3_iterations, _bits(out.stats.last_so3_error), out.stats.last_so3_count) == (st.so3_iterations, _bits(st.last_so3_error), st.last_so3_count)
    # krkInv = K R^-1 K^-1 at first_level, kt = 0: checked in float64 to float32 rounding
    il = c.intr.level(first_level)
    K = np.array([[il.fx, 0, il.cx], [0, il.fy, il.cy], [0, 0, 1]], np.float64)
    want = K.dot(np.linalg.inv(R)).dot(np.linalg.inv(K))
    got = np.array(out.krkInv, np.float64).reshape(3, 3)
    assert np.abs(got - want).max() <= 2.0 ** -22 * np.abs(want).max()
    assert list(out.kt) == [0.0, 0.0, 0.0]
