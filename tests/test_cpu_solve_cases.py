"""CPU suite: the cases of tests/solve_cases.py visit the branches of the Gauss-Newton solve they were built for -- asserted from the
oracle's trace alone, so that a case which silently stops taking a branch fails here and not unnoticed on the GPU --, the oracle's
solve itself is held against exact rational arithmetic, the chain of 19 solves reproduces the oracle's tracking loop, and the
ctypes mirrors of cf_gn_state / cf_gn_system have the layout of the header."""
import ctypes as C
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import orc
import solve_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _traces(family=None):
    for c in (sc.family(family) if family else sc.cases().values()):
        for step, (state, tr) in zip(c.steps, sc.reference(c.name)):
            yield c, step, state, tr


def test_every_transposition_is_visited():
    seen = set()
    for c, _, _, tr in _traces("pivots"):
        assert tr.active and not any(tr.zero), c.name
        seen |= {(k, tr.pivot[k]) for k in range(6) if tr.pivot[k] != k}
    assert len(sc.family("pivots")) == 720
    assert seen == {(k, p) for k in range(6) for p in range(k + 1, 6)}


def test_ties_occur_at_every_step_and_the_first_wins():
    steps = set()
    for c, _, _, tr in _traces("ties"):
        steps |= {k for k in range(6) if tr.tie[k]}
    assert steps >= {0, 1, 2, 3, 4}
    ref = lambda n: sc.reference("ties-" + n)[0][1]
    assert list(ref("all-equal").pivot) == [0, 1, 2, 3, 4, 5] and list(ref("all-equal").tie) == [1, 1, 1, 1, 1, 0]   # no swap is allowed
    assert ref("all-equal-coupled").tie[0] and ref("all-equal-coupled").pivot[0] == 0
    assert ref("first-of-two").tie[0] and ref("first-of-two").pivot[0] == 2                                          # of 2 and 4
    assert ref("last-then-equal").pivot[0] == 5 and list(ref("last-then-equal").tie)[1:5] == [1, 1, 1, 1]
    assert list(ref("late-pair").tie) == [0, 0, 0, 0, 1, 0] and list(ref("late-triple").tie) == [0, 0, 0, 1, 1, 0]
    assert list(ref("late-coupled").tie) == [0, 0, 0, 1, 0, 0] and ref("late-coupled").pivot[3] == 4
    assert ref("opposite-signs").tie[0] and ref("opposite-signs").pivot[0] == 0
    assert ref("opposite-signs-late").tie[0] and ref("opposite-signs-late").pivot[0] == 2                            # -8 in front of 8


def test_every_count_of_zero_pivots_is_present():
    counts = {}
    for c, _, state, tr in _traces("zero pivots"):
        n = sum(tr.zero)
        counts.setdefault(n, []).append(c.name)
        # a zero pivot gives a zero solution component: the update of an empty system is the identity
        if n == 6:
            assert tr.identity and np.array_equal(np.array(state.resultRt), np.eye(4).reshape(16)), c.name
    assert set(counts) >= {1, 2, 3, 4, 5, 6}, counts
    for c, _, _, tr in _traces("near-singular"):
        # rank deficiency by rounding: more pivots pass the zero test than the rank -- tiny ones, and the update is huge or NaN
        assert 6 - sum(tr.zero) > c.meta["rank"], c.name
        assert not (c.meta.get("huge") and max(abs(v) for v in tr.result) < 1e12), c.name
    assert max(tr.theta for _, _, _, tr in _traces("near-singular")) > 1e12                 # far beyond any octant


def test_rotations_reach_the_thetas_they_name():
    got = {c.name: tr for c, _, _, tr in _traces("rotations")}
    for c in sc.family("rotations"):
        if "theta" in c.meta:
            assert got[c.name].theta == c.meta["theta"], c.name     # exactly: the neighbours of epsilon and of pi / 4 are one ulp apart
    assert got["rotation-0"].identity and got["rotation-0"].theta == 0.0
    assert got["rotation-1e-17"].identity and got["rotation-1e-17"].theta > 0 and got["rotation-eps-pred"].identity
    assert not got["rotation-eps"].identity and not got["rotation-eps-succ"].identity
    assert got["rotation-eps-pred"].theta == math.nextafter(sc.EPS, 0) and got["rotation-eps-succ"].theta == math.nextafter(sc.EPS, 1)
    octants = {int(tr.theta / (math.pi / 4)) for tr in got.values() if not tr.identity and tr.theta < 7}
    assert octants >= {0, 1, 2, 3, 4, 8}, octants                   # det_sincos beyond the first octant, every quadrant of the reduction
    assert max(tr.theta for tr in got.values()) == 100.0


def test_both_sides_of_the_guard_fire():
    fired = {c.name: tr.guard for c, _, _, tr in _traces("guard")}
    for c, step, state, tr in _traces("guard"):
        above, rgb, end = "above" in c.name, c.state["rgb"], step.next_level < 0
        assert bool(tr.guard) == bool(above and rgb and end), c.name
        want = 0.0 if tr.guard else -c.meta["t"]
        assert list(state.tcurr) == [want, 0.0, 0.0], c.name        # tcurr - tprev is exactly -t
    assert any(fired.values()) and not all(fired.values())
    assert float(np.float32(0.3)) > 0.3 > float(np.nextafter(np.float32(0.3), np.float32(0)))


def test_both_sides_of_the_stop_rule_fire():
    run = lambda n: sc.reference("stop-" + n)
    (s1, t1), (s2, t2), (s3, t3), (s4, t4) = run("above")
    assert t1.stop and not t1.active and s1.level_done == 1 and s1.solves == 1
    assert not t2.active and not t2.stop and s2.level_done == 1 and s2.solves == 2       # inactive while level_done is set
    for f in ("Rcurr", "tcurr", "resultRt", "krkInv", "kt", "residual", "stats"):
        assert bytes(getattr(s1, f)) == bytes(getattr(s2, f)), f                           # ... the pose and the statistics are untouched
    assert s1.lastRGBError == s2.lastRGBError
    assert not t3.active and s3.level_done == 0 and s3.lastRGBError == np.float32(sc.FLT_MAX) and s3.solves == 3   # last_of_level re-arms
    assert t4.active and s4.solves == 4 and bytes(s4.resultRt) != bytes(s3.resultRt)
    for n in ("equal", "below"):
        for k, (s, t) in enumerate(run(n)):
            assert t.active and not t.stop and s.solves == k + 1, (n, k)
    for c in sc.family("stop rule"):
        if "inactive" in c.name:
            (s, t), = sc.reference(c.name)
            assert not t.active and s.solves == 4 and bytes(s.Rcurr) == np.asarray(c.state["Rcurr"], np.float32).tobytes()


def test_identity_branch_is_taken_and_not_taken():
    ident = {bool(tr.identity) for _, _, _, tr in _traces() if tr.active}
    assert ident == {True, False}


def test_every_rgb_format_occurs_and_the_statistics_degenerate():
    bits = {c.meta["rgb_bits"] for c in sc.family("modes") if c.meta.get("rgb_bits") is not None}
    assert bits >= set(range(8, 33, 2)), bits
    st = lambda n: sc.reference("modes-" + n)[0][0].stats
    assert math.isnan(st("count0-sigma0").last_rgb_error) and math.isinf(st("count0-sigma77").last_rgb_error)
    assert math.isinf(st("no-inliers").last_icp_error) and math.isnan(st("no-inliers-no-residual").last_icp_error)
    # fixed and Gram ICP words carry the same values
    for w in ("icp-only", "both-w10", "both-w100", "both-w0.5"):
        a, b = st(w + "-fixed"), st(w + "-gram")
        assert bytes(a.lastA) == bytes(b.lastA) and bytes(a.lastb) == bytes(b.lastb), w


def test_group_layouts_sum_to_the_same_totals():
    tot = [(sc.totals(c.steps[0].icp).tobytes(), sc.totals(c.steps[0].rgb).tobytes()) for c in sc.family("groups")]
    assert len(tot) == 6 and len(set(tot)) == 1
    wrap = sc.cases()["groups-wrap63"].steps[0].icp
    with np.errstate(over="ignore"):
        assert (np.abs(wrap.astype(np.float64)).max() >= 2.0 ** 62) and (sc.totals(wrap) < 0).any()
    states = {bytes(sc.reference(c.name)[0][0]) for c in sc.family("groups")}
    assert len(states) == 1


def test_levels_cover_the_schedule():
    seen = {(s.next_level, bool(s.last_of_level)) for c in sc.family("levels") for s in c.steps}
    assert seen == {(l, b) for l in (2, 1, 0, -1) for b in (False, True)}
    c = sc.family("levels")[0]
    fx, fy, cx, cy = c.state["intr"]
    assert fx != fy and cx != c.state["width"] / 2 and cy != c.state["height"] / 2


def test_chain_is_the_oracles_tracking_loop():
    """the 19 steps through orc_gn_solve_step, fed with sums taken step by step, end where the oracle's own loop ends: bit for bit"""
    c = sc.cases()["chain-4-5-10"]
    assert len(c.steps) == 19 and [s.next_level for s in c.steps] == [2, 2, 2, 1, 1, 1, 1, 1, 0] + [0] * 9 + [-1]
    s, _ = sc.reference(c.name)[-1]
    od, cam, pose = sc.chain_tracker()
    t, R, st = od.track(pose[:3, 3], pose[:3, :3], so3=False)
    assert np.array(s.tcurr, np.float32).tobytes() == t.tobytes() and np.array(s.Rcurr, np.float32).tobytes() == R.tobytes()
    assert bytes(s.stats) == bytes(st) and s.solves == 19
    assert st.last_icp_count > 1000 and st.last_rgb_count > 1000


# ------------------------------------------------------------------------------------------ the oracle against exact rationals
def _solve_exact(A, b):
    """Gaussian elimination with exact rationals"""
    n = len(b)
    M = [[Fraction(A[i][j]) for j in range(n)] + [Fraction(b[i])] for i in range(n)]
    for k in range(n):
        p = max(range(k, n), key=lambda r: abs(M[r][k]))
        assert M[p][k] != 0
        M[k], M[p] = M[p], M[k]
        for r in range(k + 1, n):
            f = M[r][k] / M[k][k]
            M[r] = [a - f * c for a, c in zip(M[r], M[k])]
    x = [Fraction(0)] * n
    for k in range(n - 1, -1, -1):
        x[k] = (M[k][n] - sum(M[k][j] * x[j] for j in range(k + 1, n))) / M[k][k]
    return x


def test_oracle_backward_error_against_exact_rationals():
    """The kernel and the oracle were restated from the same text, so the oracle's solve is held against something else: on the
    well-conditioned systems of `pivots` and `modes`, lastA and lastb (exact dyadic rationals) are solved with Fraction arithmetic and
    the backward error of the oracle's LDL^T, ||A x - b||inf / (||A||inf ||x||inf + ||b||inf), is computed exactly.  Measured maximum:
    solve_cases.BACKWARD_ERROR_MAX; asserted: the next power of two above four times that."""
    worst = {}
    for fam in ("pivots", "modes"):
        for c in sc.family(fam):
            (state, tr), = sc.reference(c.name)
            A = np.array(state.stats.lastA).reshape(6, 6); b = np.array(state.stats.lastb)
            x = np.array(tr.result)                                           # the oracle's own solution of this system
            Af = [[Fraction(v) for v in row] for row in A]; bf = [Fraction(v) for v in b]; xf = [Fraction(v) for v in x]
            r = max(abs(sum(Af[i][j] * xf[j] for j in range(6)) - bf[i]) for i in range(6))
            nA = max(sum(abs(v) for v in row) for row in Af)
            eta = r / (nA * max(abs(v) for v in xf) + max(abs(v) for v in bf))
            worst[fam] = max(worst.get(fam, 0.0), float(eta))
            if fam == "pivots" and c.name.endswith(("012345", "543210", "305142")):
                # and the forward error on a sample, against the exact solution: the condition numbers are around 1e11 here (column
                # scales up to 2^15, squared), times a backward error of 1e-16 that is 1e-5 relative; asserted: 1e-4
                xe = _solve_exact(Af, bf)
                assert max(abs(a - e) for a, e in zip(xf, xe)) <= Fraction(1, 10 ** 4) * max(abs(e) for e in xe), c.name
            # the translation the step applied to the identity the cases start from is x[0:3] as it stands
            assert np.array(state.resultRt).reshape(4, 4)[:3, 3].tobytes() == x[:3].tobytes(), c.name
    print("oracle backward error, maximum per family:", worst)
    m = max(worst.values())
    assert m <= 1e-12, "implausible for a 6x6 factorisation: find out why before asserting anything"
    assert m <= sc.BACKWARD_ERROR_BOUND, worst
    assert sc.BACKWARD_ERROR_BOUND == 2.0 ** math.ceil(math.log2(4 * sc.BACKWARD_ERROR_MAX))


# ------------------------------------------------------------------------------------------------- layout of the ctypes mirrors
def test_struct_mirrors_match_the_header(tmp_path):
    from co_fusion_amd import api
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler (the build of the oracle needs one too)"
    mirrors = {"cf_gn_state": api.GnState, "cf_gn_system": api.GnSystem, "cf_track_stats": api.TrackStats, "cf_so3_system": api.So3System}
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"cofusion_hip.h\"\nint main(void) {\n"
    for s, m in mirrors.items():
        src += f'  printf("{s} %zu\\n", sizeof({s}));\n'
        for f, *_ in m._fields_:
            src += f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));\n'
    src += "  return 0;\n}\n"
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = str(tmp_path / "layout")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    for s, m in mirrors.items():
        assert int(got[s]) == C.sizeof(m), s
        for f, *_ in m._fields_:
            assert int(got[f"{s}.{f}"]) == getattr(m, f).offset, f"{s}.{f}"
    assert set(sc.STATE_FIELDS) | {"cull_z", "stats"} == {f for f, *_ in api.GnState._fields_}
