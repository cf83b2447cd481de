"""CPU suite: the numpy statement of the re-detection search (tests/redetect_search_ref.py) against the cases of
tests/redetect_search_cases.py -- counts and sums known by construction, and the registration loop against the crafted moves.

Bounds.  (a), (b): the loop must end within HALF the tracker's gates of the crafted move -- 0.05 m of the object's centre, 10 degrees --
so that the next frame's tracker can pull the model in.  (c): a single plane leaves the slide inside it unobservable; the damping keeps
the seed's in-plane position, within 1 mm, and the loop must not fail.  1 mm is a tenth of a pixel's footprint at these sizes (1.5 m /
128 = 11.7 mm), so only surfels on the label's one-pixel border can change sides: at most the border's share of the label, below a
fifth for the 25 x 20 pixel (160x128) and a third for the 13 x 10 pixel (70x46) plane -- the bounds on the last step's inliers."""
import numpy as np
import pytest

import redetect_search_cases as sc
import redetect_search_ref as ref


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sc.NAMES)
def test_statement_against_the_construction(name, size):
    case = sc.get(name, size)
    st = sc.statement(case)
    if case.expect_frame is not None:
        n, bins = case.expect_frame
        assert st["frame"][0][0] == n
        assert {int(b): int(c) for b, c in enumerate(st["frame"][1]) if c} == bins
    assert int(st["frame"][1].sum()) == st["frame"][0][0]
    for k, c in enumerate(st["cands"]):
        s = case.models[case.cands[k][0]]
        assert int(c["hist"].sum()) == int(np.count_nonzero(s[:, 3] >= case.cands[k][1])), "the histogram counts every stable surfel"
        assert 0 <= c["moments"][0] <= int(c["hist"].sum())
        if case.expect_model[k] is not None:
            n_front, bins = case.expect_model[k]
            if n_front is not None:
                assert c["moments"][0] == n_front
            if bins is not None:
                assert {int(b): int(v) for b, v in enumerate(c["hist"]) if v} == bins
        if case.expect_step[k] is not None:
            for word, value in case.expect_step[k].items():
                assert c["step_T0"][word] == value, f"candidate {k} word {word}"
        for sums in (c["step_T0"], c["step_seed"]):
            if sums is not None:
                assert sums[29:] == [0, 0, 0] and sums[28] >= 0 and sums[27] >= 0
                assert all(sums[w] >= 0 for w in (0, 7, 13, 18, 22, 25)), "the diagonal of J^T J"


def test_the_gate_is_inclusive_and_sharp():
    """|v - p| = tol - k ulp: in for k >= 0, out for k < 0, at both sizes"""
    for size in sc.SIZES:
        got = [sc.statement(sc.get(f"gate_{k}", size))["cands"][0]["step_T0"][28] for k in sc.GATE_K]
        assert got == [0, 0, 70, 70, 70], got


def _pose_error(T, truth):
    D = T.astype(np.float64) @ np.linalg.inv(truth)
    ang = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(T[:3, 3].astype(np.float64) - truth[:3, 3])), float(ang)   # (the model's origin is the box's centre)


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["box_moved", "box_turned"])
def test_the_loop_ends_within_half_the_trackers_gates(name, size):
    case = sc.get(name, size)
    c = sc.statement(case)["cands"][0]
    assert c["seed"] is not None and c["colour"] > 0.5
    reg = c["reg"]
    dist, ang = _pose_error(reg["cam_from_model"], case.truth)
    d0, a0 = _pose_error(c["seed"].reshape(4, 4), case.truth)
    s0, _ = _pose_error(c["T0"].reshape(4, 4), case.truth)
    print(f"{name} {size}: static {s0:.3f} m, seed {d0 * 1e3:.1f} mm {a0:.2f} deg -> {dist * 1e3:.2f} mm {ang:.2f} deg in {reg['iterations']} steps, "
          f"inliers {reg['first_inliers']} -> {reg['last_inliers']}, rms {reg['rms'] * 1e3:.2f} mm")
    assert abs(s0 - 0.3) < 1e-3, "the static hypothesis is 0.3 m off: three times the gate"
    assert reg["ok"] and reg["iterations"] <= 10
    assert dist <= 0.05 and ang <= 10.0


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_single_plane_keeps_the_seeds_in_plane_position(size):
    case = sc.get("plane", size)
    c = sc.statement(case)["cands"][0]
    reg = c["reg"]
    assert reg["ok"] and reg["first_inliers"] >= 6
    seed = c["seed"].reshape(4, 4).astype(np.float64); T = reg["cam_from_model"].astype(np.float64)
    mbar = np.array([np.ldexp(float(c["moments"][1 + a]), -16) / c["moments"][0] for a in range(3)] + [1.0])
    moved = (T @ mbar - seed @ mbar)[:3]
    print(f"plane {size}: centroid moved {moved * 1e3} mm in {reg['iterations']} steps, inliers {reg['first_inliers']} -> {reg['last_inliers']}")
    assert abs(moved[0]) <= 1e-3 and abs(moved[1]) <= 1e-3, "the plane's normal is the camera's z: x and y are the unobservable slide"
    share = 0.2 if size[0] >= 128 else 1.0 / 3.0
    assert reg["last_inliers"] >= (1.0 - share) * reg["first_inliers"], "the plane stayed on the label"
    assert abs((T @ mbar)[2] - 1.5) <= 0.005, "and went onto the measured surface (3 mm noise, 2 mm in the map)"


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nothing_to_register_is_not_registered(size):
    case = sc.get("empty", size)
    st = sc.statement(case)
    assert st["frame"][0] == [0, 0, 0, 0] and ref.frame_centroid(st["frame"][0]) == (None, None)
    assert [c["seed"] for c in st["cands"]] == [None, None] and [c["colour"] for c in st["cands"]] == [0.0, 0.0]
    # an empty map against a frame that has the label, and a map against an empty label: the loop says "failed", nothing is divided by zero
    box = sc.get("box_moved", size)
    bst = sc.statement(box)
    args = (box.depth, box.label, box.new_label, box.cam, box.cutoff, box.tol, bst["centre"])
    with np.errstate(all="raise"):
        r = ref.register(np.zeros((0, 12), np.float32), sc.THETA, bst["cands"][0]["seed"], *args)
        assert not r["ok"] and r["iterations"] == 0 and r["first_inliers"] == 0 and r["rms"] == 0
        assert ref.seed(bst["cands"][0]["T0"], [0, 0, 0, 0], [0.0, 0.0, 1.5]) is None
        r = ref.register(case.models[1], sc.THETA, sc.I4.reshape(16), case.depth, case.label, case.new_label, case.cam, case.cutoff, case.tol, [0, 0, 1.5])
        assert not r["ok"] and r["iterations"] == 0 and r["last_inliers"] == 0
    assert ref.solve_step([0] * 32, [0.0, 0.0, 1.5], [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], [0.0, 0.0, 0.0]) is None


def test_a_model_listed_twice_is_two_candidates():
    case = sc.get("batch_9", (70, 46))
    st = sc.statement(case)
    assert case.cands[3][0] == case.cands[6][0] == 6
    assert st["cands"][3]["moments"] != st["cands"][6]["moments"], "another pose and threshold: other sums"
    assert int(st["cands"][3]["hist"].sum()) > int(st["cands"][6]["hist"].sum()) > 0
    assert st["cands"][1]["moments"] == [0, 0, 0, 0]
