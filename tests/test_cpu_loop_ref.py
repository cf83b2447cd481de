"""CPU suite of the loop-closure seam: every case of tests/loop_cases.py reaches the branch it is named for, shown on the numpy statement
tests/loop_ref.py; the fern counts loop closure accepts; and the analytic model of a camera that returns with drift, held against
tests/deform_ref.py, which documents why the end-to-end scenario samples its graph at 10 000 and not at the reference's 25 000.  No GPU
call is made."""
import numpy as np
import pytest

import deform_ref
import loop_cases as lc
import loop_ref as lr

f32 = np.float32


@pytest.mark.parametrize("name", list(lc.CASES))
def test_case_reaches_its_branch(name):
    _, branch, cl, expect = lc.CASES[name]
    s = lc.statement(name)
    assert s["gate"]["branch"] == branch
    seen = dict(s["gate"])
    if cl is not None:
        rec, rows, trace = s["closure"]
        seen.update(trace); seen.update(rec)
        assert len(rows[0]) == len(rows[1]) == len(rows[2]) == rec["n_constraints"] <= 128
        # interleaved: row 2j is (raw -> model, now), row 2j + 1 pins the model point at the keyframe's time
        assert np.array_equal(rows[0][1::2], rows[1][1::2]) and np.array_equal(rows[1][0::2], rows[1][1::2])
        assert (rows[2][0::2] == f32(cl["time"])).all() and (rows[2][1::2] == f32(rec["keyframe_time"])).all()
        if rec["n_constraints"]:
            assert not np.array_equal(rows[0][0::2], rows[1][0::2])   # the drift
    for k, v in expect.items():
        assert seen[k] == v or (isinstance(v, float) and np.isnan(v) and np.isnan(seen[k])), (k, seen[k], v)


def test_compaction_keeps_the_order_of_the_samples():
    """the rows of the case with gaps are the rows of its valid samples in sample order"""
    sc = lc.scenes()["samples_gaps"]
    rec, rows, trace = lc.statement("valid_samples_with_gaps")["closure"]
    v4 = sc.query[0][4::8, 4::8]
    valid = [i for i in range(0, 100, 2) if lr.valid_sample(v4[i // lc.RW, i % lc.RW, 2], lc.MAX_DEPTH_MM)]
    assert 0 < len(valid) == trace["valid_samples"] < trace["samples"] == 50
    assert any(b - a > 2 for a, b in zip(valid, valid[1:])) and any(b - a == 2 for a, b in zip(valid, valid[1:]))
    for j, i in enumerate(valid):
        x, y, z = v4[i // lc.RW, i % lc.RW, :3]
        assert np.array_equal(rows[1][2 * j], np.array(lr._mul(lc.KF_POSE, x, y, z), f32))
    # 4.9999 m is inside (int(4999.9) == 4999), 5.0 and 5.0005 m are not
    assert lr.valid_sample(4.9999, 5000) and not lr.valid_sample(5.0, 5000) and not lr.valid_sample(5.0005, 5000)
    assert not lr.valid_sample(np.nan, 5000) and not lr.valid_sample(0.0, 5000) and lr.valid_sample(1e-30, 5000)


def test_fern_counts_loop_closure_accepts():
    assert [lr.loop_samples(n) for n in (500, 2048, 127, 99, 64, 50, 49)] == [50, 52, 64, None, 64, 50, None]
    for n in range(50, 2049):
        m = lr.loop_samples(n)
        assert m is None or (m == len(range(0, n, n // 50)) and 2 * m <= deform_ref.MAX_CONS)


def test_seam_entry_points_are_exported_with_the_documented_signatures():
    """include/cofusion_loop.h against co_fusion_amd/ferns.py and the built libraries; the argument checks that need no GPU"""
    import ctypes as C
    import os
    import re
    import subprocess
    import __graft_entry__ as g
    g.build()
    from co_fusion_amd import deform, ferns, lib as cflib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "cofusion_loop.h")).read(), flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(",")] for m in re.finditer(r"^int\s+(cf_ferns_[a-z_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.M | re.S)}
    assert set(protos) == set(ferns.LOOP_SIGNATURES) and len(protos) == 6
    ctype = lambda a: "ptr" if "*" in a or "[" in a else {"int": "int", "float": "float"}[re.sub(r"\s+", " ", a).rsplit(" ", 1)[0]]
    kind = lambda t: "ptr" if t is C.c_void_p or hasattr(t, "contents") else {C.c_int: "int", C.c_float: "float"}[t]
    for name, args in protos.items():
        assert [ctype(a) for a in args] == [kind(t) for t in ferns.LOOP_SIGNATURES[name][1]], name
    assert C.sizeof(ferns.FernsGate) == 32 and C.sizeof(ferns.FernsClosure) == 48
    assert '#include "cofusion_loop.h"' in open(os.path.join(root, "include", "cofusion_hip.h")).read()
    exported = set(re.findall(r" T (\w+)", subprocess.check_output(["nm", "-D", "--defined-only", cflib.LIB_PATH]).decode()))
    assert set(protos) | {"cf_deform_weights_device"} <= exported and set(protos) | {"cf_deform_weights_device"} <= set(cflib.SYMBOLS)
    assert "cf_deform_weights_device" in deform.SIGNATURES
    lib = deform.bind(ferns.bind(cflib.load()))
    assert lib.cf_ferns_gate_async(None) != 0 and lib.cf_ferns_gate_wait(None, None) != 0
    assert lib.cf_ferns_constraints(None, 0, None, None, 0.0, 0.0, 0, 0, None) != 0 and lib.cf_ferns_find_frame(None, None, 0, 0, 0, None, None) != 0
    assert lib.cf_ferns_constraint_buffers(None, None, None, None) != 0 and lib.cf_ferns_keyframe_buffers(None, None, None) != 0
    assert lib.cf_deform_weights_device(None, None, None, None, 0) != 0
    host = cflib.load_host()
    assert host.cofusion_set_loop_closure(None, 1, 0) != 0 and host.cofusion_loop_stats(None, None) != 0
    assert {"cofusion_set_loop_closure", "cofusion_loop_stats"} <= set(cflib.HOST_SYMBOLS)


# ------------------------------------------------------------------------------------------------ the modelled return
# An analytic box room of synth.Scene's dimensions, camera at (0, 0, 0.9) turning about the vertical axis by 3 degrees per frame at
# 640x480, fx = fy = 528.  Frame 1 contributes every pixel in raster order; every later frame the 37 leading columns (17 760 surfels),
# also on the second pass (the first pass is inactive by then).  Surfels are placed at poses whose yaw is 1.012 x the true yaw.  After
# 150 turns (450 degrees) the loop closes on the view of 90 degrees, the keyframe of tick 31: 50 constraints from the current view and
# their 50 pins, interleaved.
ROOM_MIN, ROOM_MAX = np.array([-1.8, -1.2, -0.8]), np.array([1.8, 1.0, 2.6])
EYE_AT = np.array([0.0, 0.0, 0.9])
CW, CH, FX, CX, CY = 640, 480, 528.0, 320.0, 240.0
FIRST, PER_FRAME, COLS = CW * CH, 37 * CH, 37
TURN, DRIFT, FRAMES, KEYFRAME = 3.0, 1.012, 150, 30


def yaw_pose(deg):
    a = np.radians(deg)
    p = np.eye(4)
    p[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    p[:3, 3] = EYE_AT
    return p


def camera_points(frame, u, v):
    """points of pixels (u, v) of the true view of `frame`, in its camera frame: the ray leaves the room through a wall"""
    d = np.stack([(u - CX) / FX, (v - CY) / FX, np.ones_like(u, float)], -1)
    dw = d @ yaw_pose(TURN * frame)[:3, :3].T
    with np.errstate(divide="ignore"):
        t = np.where(dw > 0, (ROOM_MAX - EYE_AT) / dw, np.where(dw < 0, (ROOM_MIN - EYE_AT) / dw, np.inf)).min(axis=-1)
    return d * t[..., None]


def surfel_nodes(stride):
    """(x, y, z, init_time) of the surfels at indices 0, stride, 2 stride, ... of the modelled map"""
    total = FIRST + FRAMES * PER_FRAME
    idx = np.arange(0, total, stride)
    late = idx >= FIRST
    frame = np.where(late, 1 + (idx - FIRST) // PER_FRAME, 0)
    k = np.where(late, (idx - FIRST) % PER_FRAME, idx)
    u = np.where(late, CW - COLS + k % COLS, k % CW).astype(float)
    v = np.where(late, k // COLS, k // CW).astype(float)
    nodes = np.zeros((len(idx), 4), f32)
    for f in np.unique(frame):
        m = frame == f
        p = camera_points(f, u[m], v[m])
        nodes[m, :3] = (p @ yaw_pose(DRIFT * TURN * f)[:3, :3].T + EYE_AT).astype(f32)
        nodes[m, 3] = f + 1
    return nodes, total


def modelled_constraints():
    rng = np.random.default_rng(31)
    u, v = rng.integers(0, 80, 50) * 8.0 + 4, rng.integers(0, 60, 50) * 8.0 + 4
    p = camera_points(FRAMES, u, v)
    src = p @ yaw_pose(DRIFT * TURN * FRAMES)[:3, :3].T + EYE_AT       # where the drifted camera puts them
    dst = p @ yaw_pose(DRIFT * TURN * KEYFRAME)[:3, :3].T + EYE_AT     # where the keyframe's pose puts them (450 = 90 mod 360)
    s = np.empty((100, 3)); d = np.empty((100, 3)); t = np.empty(100)
    s[0::2], d[0::2], t[0::2] = src, dst, FRAMES + 1
    s[1::2], d[1::2], t[1::2] = dst, dst, KEYFRAME + 1
    return s.astype(f32), d.astype(f32), t.astype(f32)


def test_modelled_return_is_accepted():
    src, dst, tm = modelled_constraints()
    drift = np.linalg.norm(src[0::2] - dst[0::2], axis=1).mean()
    print("mean drift of the non-pin constraints", drift)
    assert drift > 0.12   # the pins count in the mean constraint error: the 0.06 gate needs more than 0.12 m here
    out = {}
    for rate in (10000, 25000):
        nodes, total = surfel_nodes(deform_ref.stride_for(FIRST + FRAMES * PER_FRAME, rate))
        assert np.all(np.diff(nodes[:, 3]) >= 0)
        r = deform_ref.optimise(nodes, src, dst, tm)
        out[rate] = r
        print(rate, len(nodes), {k: r[k] for k in ("optimised", "accepted", "failed", "iterations", "error", "mean_cons_error_before", "mean_cons_error")})
    assert out[10000]["optimised"] and out[10000]["accepted"] and not out[10000]["failed"]
    assert out[10000]["mean_cons_error_before"] >= 0.06
    # 25 000 = 39 * 640 + 40: the first frame's nodes lie on one image diagonal of one flat wall, collinear, and the rotation about that
    # line is free: the normal equations are singular
    first = surfel_nodes(25000)[0][:13, :3].astype(np.float64)
    assert np.linalg.matrix_rank(first - first[0], tol=1e-5) == 1
    assert out[25000]["optimised"] and out[25000]["failed"] and not out[25000]["accepted"]
