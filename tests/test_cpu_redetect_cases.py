"""CPU suite: the numpy statement of the re-detection score (tests/redetect_ref.py) against cases whose counts are known by construction
(tests/redetect_cases.py), the decision rule, and the two thresholds against synthetic frames of the scenarios the GPU suite runs
(tests/test_redetect_facade_gpu.py): the true candidate and the strongest false one must lie on the intended sides."""
import numpy as np
import pytest

import redetect_cases as rc
import redetect_ref as ref
from co_fusion_amd import synth


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", rc.NAMES)
def test_statement_gives_the_constructed_counts(name, size):
    case = rc.get(name, size)
    assert (size[0] * size[1]) % 32 != 0 or size == (64, 48)
    for k, (s, theta, pose) in enumerate(case.cands):
        got = ref.score(s, theta, pose, case.depth, case.label, case.new_label, case.cam, case.cutoff, case.tol)
        assert got["occluded"] + got["seen_through"] + got["agree"] <= got["projected"] <= s.shape[0]
        assert got["covered"] <= got["agree_on_label"] <= got["agree"]
        if case.expect[k] is not None:
            assert got == case.expect[k], f"{name} candidate {k}"
    if case.label_pixels is not None:
        assert ref.label_pixels(case.label, case.new_label) == case.label_pixels


def test_cases_exercise_what_they_are_named_for():
    for size in rc.SIZES:
        g = rc.get("behind_gate", size).expect, rc.get("before_gate", size).expect
        assert [e["occluded"] > 0 for e in g[0]] == [k > 0 for k in rc.GATE_K]          # d < z - tol is strict
        assert [e["seen_through"] > 0 for e in g[1]] == [k < 0 for k in rc.GATE_K]      # d > z + tol is strict
        assert [c[0].shape[0] for c in rc.get("counts", size).cands] == list(rc.COUNT_SIZES)
        assert [c[0].shape[0] for c in rc.get("batch_mixed_9", size).cands].count(0) == 1
        assert rc.get("counts", size).expect[-1]["covered"] < rc.get("counts", size).expect[-1]["agree_on_label"]
        w, h = size
        assert rc.get("rejects", size).cands[0][0].shape[0] > rc.get("rejects", size).expect[0]["projected"]
    assert (70 * 46) % 32 != 0 and (70 * 46) % 16 != 0


def _c(agree_on_label, agree, seen_through, covered):
    return dict(projected=agree + seen_through, occluded=0, seen_through=seen_through, agree=agree, agree_on_label=agree_on_label, covered=covered)


def test_decision_rule():
    # thresholds are inclusive
    rows, win = ref.decide([_c(50, 100, 0, 50)], 100, 0.5, 0.5)
    assert rows[0]["eligible"] and win == 0 and rows[0]["fit"] == 0.5 and rows[0]["cover"] == 0.5
    assert ref.decide([_c(49, 100, 0, 50)], 100, 0.5, 0.5)[1] == -1          # fit just below
    assert ref.decide([_c(50, 100, 0, 49)], 100, 0.5, 0.5)[1] == -1          # cover just below
    # seen-through surfels count against the fit, occluded ones do not
    assert ref.decide([_c(50, 50, 51, 50)], 100, 0.5, 0.5)[1] == -1
    occ = _c(50, 50, 0, 50); occ["occluded"] = 1000; occ["projected"] = 1050
    assert ref.decide([occ], 100, 0.5, 0.5)[1] == 0
    # zero denominators are never eligible, whatever the thresholds
    assert ref.decide([_c(0, 0, 0, 0)], 100, 0.0, 0.0) == ([dict(fit=0, cover=0, eligible=False)], -1)
    assert ref.decide([_c(10, 10, 0, 10)], 0, 0.0, 0.0)[1] == -1
    # the largest agree_on_label among the eligible wins; a larger one that is not eligible does not; ties go to the earlier position
    cands = [_c(60, 100, 0, 60), _c(90, 200, 0, 90), _c(80, 100, 0, 80), _c(80, 90, 0, 80)]
    rows, win = ref.decide(cands, 100, 0.5, 0.5)
    assert [r["eligible"] for r in rows] == [True, False, True, True] and win == 2
    assert ref.decide([], 10, 0.5, 0.5) == ([], -1)


# ---- the thresholds against the scenarios of the GPU suite, on synthetic frames -------------------------------------------------
W, H = 160, 128


def _ideal_map(cam, depth, label, value, T_cam, T_obj):
    """the surfels a perfect fusion of one frame would hold for the object labelled `value`, in the object's frame"""
    v, u = np.nonzero((label == value) & (depth > 0))
    z = depth[v, u].astype(np.float64)
    pc = np.stack([(u + 0.5 - cam.cx) * z / cam.fx, (v + 0.5 - cam.cy) * z / cam.fy, z, np.ones_like(z)], axis=1)
    po = pc @ (np.linalg.inv(T_obj) @ T_cam).T
    s = np.zeros((len(z), 12), np.float32)
    s[:, :3] = po[:, :3]
    s[:, 3] = 1.0
    return s


def _fit_cover(s, pose, depth, label, value, cam):
    c = ref.score(s, 0.5, pose, depth, label, value, (cam.fx, cam.fy, cam.cx, cam.cy), 20.0, 0.10)
    rows, _ = ref.decide([c], ref.label_pixels(label, value), 0.5, 0.5)
    return float(rows[0]["fit"]), float(rows[0]["cover"])


def test_thresholds_separate_the_scenarios():
    """object 2 of Scene(n_obj=2) mapped at frame 5 and scored at frame 9: parked (true candidate), the OTHER object's map under its own
    static hypothesis (the strongest false candidate: a different, moving object elsewhere in the image), and parked but come back 0.5 m
    away.  0.5 / 0.5 must lie between the true candidate's figures and the others'."""
    cam = synth.Camera.scaled(W, H)
    sc = synth.Scene(n_obj=2)
    d5, _, l5, G5 = sc.render(cam, 5, noise=True)
    O2, O1 = sc.object_pose(1, 5), sc.object_pose(0, 5)
    map2 = _ideal_map(cam, d5, l5, 2, G5, O2)
    map1 = _ideal_map(cam, d5, l5, 1, G5, O1)
    assert map2.shape[0] > 256 and map1.shape[0] > 256

    class Parked(synth.Scene):
        shift = np.zeros(3)

        def object_pose(self, i, t):
            T = synth.Scene.object_pose(self, i, min(t, 4) if i == 1 else t)
            if i == 1 and t >= 9:
                T = T.copy(); T[:3, 3] += self.shift
            return T

    parked = Parked(n_obj=2)
    O2p = parked.object_pose(1, 5)
    d5p, _, l5p, _ = parked.render(cam, 5, noise=True)
    map2p = _ideal_map(cam, d5p, l5p, 2, G5, O2p)
    d9, _, l9, G9 = parked.render(cam, 9, noise=True)
    # the hypothesis M_now = O^-1 G_now with O = the object's world pose at deactivation (here: the truth at frame 5)
    true_fit, true_cover = _fit_cover(map2p, np.linalg.inv(O2p) @ G9, d9, l9, 2, cam)
    false_fit, false_cover = _fit_cover(map1, np.linalg.inv(O1) @ G9, d9, l9, 2, cam)
    assert true_fit > 0.5 and true_cover > 0.5, (true_fit, true_cover)
    assert min(false_fit, false_cover) < 0.5, (false_fit, false_cover)
    moved = Parked(n_obj=2); moved.shift = np.array([0.5, 0.0, 0.0])
    d9m, _, l9m, _ = moved.render(cam, 9, noise=True)
    if ref.label_pixels(l9m, 2):
        mf, mc = _fit_cover(map2p, np.linalg.inv(O2p) @ G9, d9m, l9m, 2, cam)
        assert min(mf, mc) < 0.5, (mf, mc)
    print(f"true {true_fit:.3f}/{true_cover:.3f}  false {false_fit:.3f}/{false_cover:.3f}")
