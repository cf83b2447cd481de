"""The case table of tests/track_cases.py, checked on the CPU: the oracle is the reference of tests/test_track_batch_gpu.py, and a case
whose reference result is degenerate tests nothing.  For every case, step and tracker the oracle alone must give what the GPU test
relies on: plenty of ICP inliers, RGB correspondences, a pose that moved -- plus the geometric precondition each case is named after."""
import itertools

import numpy as np
import pytest

import track_cases as tc


def _steps(case):
    return [(k, s) for s in range(case.steps) for k in range(len(case.trackers))]


@pytest.mark.parametrize("name", [c.name for c in tc.CASES])
def test_oracle_result_is_not_degenerate(name):
    case = tc.BY_NAME[name]
    for k, s in _steps(case):
        ti = tc.tracker_inputs(case, k, s)
        o = tc.oracle_step(case, k, s)
        what = f"{name} tracker {k} step {s}"
        if case.trackers[k].masks[s] == tc.EMPTY:
            assert ti["n_valid"] == 0 and o["icp_count"] == 0, what
            continue
        assert ti["n_valid"] > 0, what
        if tc.uses_icp(case):
            assert o["icp_count"] >= 100, f"{what}: {o['icp_count']} ICP inliers"
        if tc.uses_rgb(case):
            assert o["rgb_count"] > 0, f"{what}: no RGB correspondence"
        start = ti["start"]
        moved = o["trans"].tobytes() != start[:3, 3].tobytes() or o["rot"].tobytes() != np.ascontiguousarray(start[:3, :3]).tobytes()
        assert moved, f"{what}: the tracked pose is the start pose"
        if case.err:
            assert np.count_nonzero(o["err"]) >= 100, what


@pytest.mark.parametrize("name", [c.name for c in tc.CASES if c.batched])
def test_trackers_of_a_batch_differ(name):
    """two identical trackers would hide a slot mix-up: masks, start poses and oracle results are pairwise different"""
    case = tc.BY_NAME[name]
    assert len({t.seed for t in case.trackers}) == len(case.trackers)
    for s in range(case.steps):
        for a, b in itertools.combinations(range(len(case.trackers)), 2):
            oa, ob = tc.oracle_step(case, a, s), tc.oracle_step(case, b, s)
            assert oa["trans"].tobytes() != ob["trans"].tobytes() and oa["rot"].tobytes() != ob["rot"].tobytes(), (name, s, a, b)
            assert not np.array_equal(oa["lastA"], ob["lastA"]), (name, s, a, b)
            assert not np.array_equal(tc.tracker_inputs(case, a, s)["start"], tc.tracker_inputs(case, b, s)["start"])
            assert case.trackers[a].masks[s] != case.trackers[b].masks[s]


def test_level_geometry_of_the_size_cases():
    """the sizes hit the run-table edges they are named after, and the library's tiled model-map pass (width % 16, height % 4) feeds the box"""
    for c in tc.CASES:
        W, H = c.size
        assert W % 16 == 0 and H % 4 == 0, c.name
    W, H = tc.BY_NAME["narrow_208x156"].size
    assert all((W >> l) % 64 != 0 for l in range(3)) and ((W >> 2) * (H >> 2)) % 64 != 0
    W, H = tc.BY_NAME["odd_336x252"].size
    assert all(((W >> l) * (H >> l)) % 64 != 0 for l in (1, 2))
    W, H = tc.BY_NAME["batch_mixed_5"].size
    assert all((W >> l) % 64 == 0 for l in range(3))
    W, H = tc.BY_NAME["corner_tl"].size
    assert tc.keep_mask(tc.BY_NAME["corner_tl"], 0, 1)[0, 0]
    c = tc.BY_NAME["corner_br"]
    assert tc.keep_mask(c, 0, 1)[c.size[1] - 1, c.size[0] - 1]
    x0, x1, y0, y1 = tc.BY_NAME["sliver_v"].trackers[0].masks[1]
    assert x1 - x0 == tc.SLIVER_V_WIDTH <= 8 and (y0, y1) == (0, 240)
    x0, x1, y0, y1 = tc.BY_NAME["sliver_h"].trackers[0].masks[1]
    assert y1 - y0 == tc.SLIVER_H_HEIGHT <= 8 and (x0, x1) == (0, 320) and x1 - x0 > 64
    assert tc.BY_NAME["whole_image"].trackers[0].masks[1] is tc.FULL and tc.BY_NAME["whole_image"].trackers[0].cull
    assert len(tc.BY_NAME["batch_9"].trackers) == 9 and len(tc.BY_NAME["batch_16"].trackers) == 16


def test_grown_moved_vanished_preconditions():
    g = tc.BY_NAME["grown"]
    a0, a1 = tc.keep_mask(g, 0, 0).sum(), tc.keep_mask(g, 0, 1).sum()
    assert a1 >= 6 * a0, (a0, a1)
    m = tc.BY_NAME["moved"]
    assert not (tc.keep_mask(m, 0, 0) & tc.keep_mask(m, 0, 1)).any()
    v = tc.BY_NAME["vanished"]
    assert tc.tracker_inputs(v, 0, 0)["n_valid"] > 0 and tc.tracker_inputs(v, 0, 1)["n_valid"] == 0
    assert tc.oracle_step(v, 0, 1)["icp_count"] == 0


def test_neg_zero_pose_precondition():
    c = tc.BY_NAME["neg_zero_pose"]
    ti = tc.tracker_inputs(c, 0, 1)
    neg = np.signbit(ti["start"]) & (ti["start"] == 0)
    assert neg.any(), "the start pose holds no -0.0"
    assert np.array_equal(ti["start"], ti["pose"]) and ti["start"].tobytes() != ti["pose"].tobytes(), "same values, other bits"


def test_depth_split_precondition():
    """per 64-pixel run of the current frame's level 0, the interval of its valid depths (numpy, from the depth image): inside the
    object's rectangle at least one run misses the depth interval of the model and at least one overlaps it"""
    c = tc.BY_NAME["depth_split"]
    W, H = c.size
    for s in range(c.steps):
        d = tc.frame_inputs(c, s)["d_cur"]
        ti = tc.tracker_inputs(c, 0, s)
        z = ti["v4"][..., 2][ti["v4"][..., 2] > 0]
        zlo, zhi = float(z.min()) - 0.2, float(z.max()) + 0.2   # the model's depths, dilated far beyond the 5 mm / 0.5 deg of the start pose
        x0, y0, x1, y1 = ti["rect"]
        runs = d.reshape(-1, 64)
        miss = hit = 0
        for r in range(runs.shape[0]):
            y, xa = divmod(r * 64, W)
            if not (y0 <= y <= y1 and xa + 63 >= x0 and xa <= x1):
                continue
            v = runs[r][runs[r] > 0]
            if len(v) == 0 or v.min() > zhi or v.max() < zlo:
                miss += 1
            else:
                hit += 1
        assert miss >= 1 and hit >= 1, (s, miss, hit)
        y0o, y1o, zo = c.occluder
        assert y0 < y0o and y1o < y1 and zo < zlo, "the band lies inside the box and in front of the model"
