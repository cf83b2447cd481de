"""GPU suite of the loop-closure seam of the fern database (csrc/ferns.hip: ferns_gate_kernel, ferns_close_kernel; cf_deform_weights_device)
against the numpy statement tests/loop_ref.py on the case table tests/loop_cases.py.

Everything is exact.  Gate record: match, dissimilarity and overlap bit for bit (NaN included), counts and the keyframe's time.  Closure
record: photometric sum and count, the f64 error, `accepted`, `n_constraints`.  Constraint rows: byte for byte (f32 in the stated
association, no contraction).  Each twice.  cf_ferns_find_frame against cf_ferns_relocalise on the same state at 640x480: the same result,
the photometric error to the bit."""
import numpy as np
import pytest

import deform_cases as dc
import ferns_scene as fs
import loop_cases as lc

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def rig():
    from co_fusion_amd import api, ferns
    ctx = api.Context(lc.W, lc.H, *lc.CAM, max_models=1, max_surfels=1024)
    made = {}

    def scene(name):
        """the scene's database with the query encoded and searched"""
        if name not in made:
            sc = lc.scenes()[name]
            f = ferns.Ferns(ctx, n_ferns=sc.n, capacity=4, max_depth_mm=lc.MAX_DEPTH_MM, photo_threshold=sc.photo_threshold, table=sc.table)
            for maps, p, t in sc.keyframes:
                f.add(*(ctx.to_device(a) for a in maps), p, t, -1.0)
            assert f.count() == (len(sc.keyframes), False)
            f.encode(*(ctx.to_device(a) for a in sc.query))
            made[name] = f
        return made[name]

    yield ctx, scene
    for f in made.values():
        f.close()
    ctx.close()


@pytest.mark.parametrize("name", list(lc.CASES))
def test_gate_record_is_the_statements(rig, name):
    _, scene = rig
    sc = lc.scenes()[lc.CASES[name][0]]
    f = scene(lc.CASES[name][0])
    want = lc.statement(name)["gate"]
    serial = None
    for _ in range(2):
        f.search(sc.time, sc.min_age)
        f.gate_async()
        got = f.gate_wait()
        print(name, got)
        assert serial is None or got["serial"] == serial + 1
        serial = got["serial"]
        for k in ("match_id", "good_q", "keyframe_time", "count", "keyframes"):
            assert got[k] == want[k], k
        assert bits(got["dissimilarity"]) == bits(want["dissimilarity"])
        assert bits(got["overlap"]) == bits(want["overlap"]) or (np.isnan(got["overlap"]) and np.isnan(want["overlap"]))
        assert (got["match_id"] >= 0 and bool(got["overlap"] > f32(0.3))) == want["candidate"]
    with pytest.raises(Exception):
        f.gate_wait()   # nothing outstanding


@pytest.mark.parametrize("name", [n for n, c in lc.CASES.items() if c[2] is not None])
def test_closure_record_and_constraint_rows_are_the_statements(rig, name):
    _, scene = rig
    cl = lc.CASES[name][2]
    sc = lc.scenes()[cl["scene"]]
    f = scene(cl["scene"])
    rec, rows, _ = lc.statement(name)["closure"]
    est = sc.keyframes[cl["keyframe"]][1] if cl["est_pose"] is None else cl["est_pose"]
    for _ in range(2):
        got = f.constraints(cl["keyframe"], cl["curr_pose"], est, cl["icp_error"], cl["icp_count"], cl["lost"], cl["time"])
        print(name, got)
        for k in ("accepted", "n_constraints", "photo_sum", "photo_count", "keyframe_time"):
            assert got[k] == rec[k], k
        assert got["keyframe"] == cl["keyframe"]
        assert np.float64(got["photo_error"]).tobytes() == np.float64(rec["photo_error"]).tobytes()
        src, dst, tm = f.download_constraints(got["n_constraints"])
        assert src.tobytes() == rows[0].tobytes() and dst.tobytes() == rows[1].tobytes() and tm.tobytes() == rows[2].tobytes()


def test_a_keyframe_that_does_not_exist_is_not_accepted(rig):
    _, scene = rig
    f = scene("all_valid_64")
    got = f.constraints(3, lc.DRIFTED, lc.KF_POSE, f32(1e-4), f32(3000.0), 0, 1000)   # capacity 4, one keyframe
    assert got["keyframe"] == -1 and not got["accepted"] and got["n_constraints"] == 0
    with pytest.raises(Exception):
        f.constraints(4, lc.DRIFTED, lc.KF_POSE, f32(1e-4), f32(3000.0), 0, 1000)


def test_fern_counts_loop_closure_refuses(rig):
    from co_fusion_amd import ferns
    ctx, _ = rig
    assert [ferns.loop_samples(n) for n in (500, 2048, 127, 99, 64, 49)] == [50, 52, 64, None, 64, None]
    f = ferns.Ferns(ctx, n_ferns=99, capacity=2, max_depth_mm=lc.MAX_DEPTH_MM, table=lc.table(99))
    try:
        m = lc.base_frame(99)
        f.add(*(ctx.to_device(a) for a in m), lc.KF_POSE, 7, -1.0)
        f.encode(*(ctx.to_device(a) for a in m))
        with pytest.raises(Exception):
            f.constraints(0, lc.DRIFTED, lc.KF_POSE, f32(1e-4), f32(3000.0), 0, 1000)
        got = f.constraints(0, lc.DRIFTED, lc.KF_POSE, f32(1e-4), f32(3000.0), 1, 1000)   # a lost camera draws no samples
        assert got["accepted"] and got["n_constraints"] == 0 and got["photo_count"] == 99
    finally:
        f.close()


def test_weights_from_device_rows_equal_weights_from_host_rows():
    from co_fusion_amd import api, deform
    import torch
    ctx = api.Context(64, 48, 60.0, 60.0, 32.0, 24.0, max_models=1, max_surfels=1024)
    d = deform.Deform(ctx)
    try:
        s = dc.system(12, "small")
        n = len(s["tm"])
        d.set_nodes(s["nodes"])
        d.weights(s["src"], s["dst"], s["tm"])
        want = d.download()
        assert d.counts() == (12, n) and n > 0
        dev = [torch.from_numpy(np.ascontiguousarray(a, f32)).cuda() for a in (s["src"], s["dst"], s["tm"])]
        for _ in range(2):
            d.set_nodes(s["nodes"])
            d.weights_device(*dev, n)
            got = d.download()
            assert d.counts() == (12, n)
            assert got["ids"].tobytes() == want["ids"].tobytes() and got["weights"].tobytes() == want["weights"].tobytes()
        a, b = d.optimise(), None
        d.set_nodes(s["nodes"]); d.weights(s["src"], s["dst"], s["tm"])
        b = d.optimise()
        assert {k: np.asarray(v).tobytes() for k, v in a.items()} == {k: np.asarray(v).tobytes() for k, v in b.items()}   # (the targets arrived too)
    finally:
        d.close(); ctx.close()


def test_find_frame_equals_relocalise_on_the_same_state():
    """640x480 -> 80x60 on the scene of test_ferns_reloc_gpu.py: query 94 against keyframe 2"""
    from co_fusion_amd import api, ferns
    c = fs.CAM
    ctx = api.Context(fs.W, fs.H, c.fx, c.fy, c.cx, c.cy, max_models=1, max_surfels=1024)
    f = ferns.Ferns(ctx, n_ferns=500, capacity=8, max_depth_mm=5000, photo_threshold=115.0, seed=7)
    try:
        for i, t in enumerate(fs.KEYFRAME_TIMES):
            f.add(*(ctx.to_device(a) for a in fs.maps(t)), fs.view(t)[2], 1 + i, -1.0)
        f.encode(*(ctx.to_device(a) for a in fs.maps(fs.QUERY_TIME)))
        curr = fs.view(fs.QUERY_TIME)[2]
        want = f.relocalise(curr, 1000, 300, lost=False)
        f.search(1000, 300)
        f.gate_async()
        g = f.gate_wait()
        got, cl = f.find_frame(curr, 1000, 300, lost=False)
        print(want, got, cl, g)
        assert g["match_id"] == want["keyframe"] == fs.QUERY_KEYFRAME and bits(g["overlap"]) == bits(want["overlap"])
        assert want["icp_ran"] and want["photo_count"] > 0
        for k in ("accepted", "keyframe", "icp_ran", "photo_count"):
            assert got[k] == want[k], k
        for k in ("dissimilarity", "overlap", "icp_error", "icp_count", "pose"):
            assert bits(got[k]).tobytes() == bits(want[k]).tobytes(), k
        assert np.float64(got["photo_error"]).tobytes() == np.float64(want["photo_error"]).tobytes()
        assert cl["keyframe"] == want["keyframe"] and cl["accepted"] == want["accepted"]
        assert cl["n_constraints"] % 2 == 0 and cl["n_constraints"] <= 100 and (cl["n_constraints"] > 0) == want["accepted"]
    finally:
        f.close(); ctx.close()
