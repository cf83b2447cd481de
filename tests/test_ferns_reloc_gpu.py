"""GPU suite of cf_ferns_relocalise (Ferns::findFrame) at 640x480 -> 80x60, the only size the small tracker runs at: a static
synthetic room, five keyframes at known poses along a smooth trajectory, a query view 3.5 cm and 0.58 degrees from keyframe 2
(chosen so that no correspondence coordinate of the photometric check lies within 1e-3 px of an integer: the nearest is 7e-3 px
away), and a view of the opposite wall.

The pose bound of test_pose_is_close_to_the_ground_truth is the CPU oracle's own error on this fixture (tests/orc.py's tracker on the
numpy-reduced maps, options rgb_only 0, icp_weight 100, pyramid 0, fast_odom 0, so3 0, started from the keyframe's pose): 1.257 mm
and 0.0329 degrees from the ground truth, times two for the choice of query -> 2.515 mm, 0.0657 degrees."""
import ctypes as C

import numpy as np
import pytest

import ferns_ref as fr
import ferns_scene as fs
import orc

pytestmark = pytest.mark.gpu

RW, RH = fs.W // 8, fs.H // 8
MAX_DEPTH_MM = 5000
f32 = np.float32


def reduced_cam():
    c = fs.CAM
    return f32(c.fx) / f32(8), f32(c.fy) / f32(8), f32(c.cx) / f32(8), f32(c.cy) / f32(8)


@pytest.fixture(scope="module")
def rig():
    from co_fusion_amd import api, ferns
    c = fs.CAM
    ctx = api.Context(fs.W, fs.H, c.fx, c.fy, c.cx, c.cy, max_models=1, max_surfels=1024)
    f = ferns.Ferns(ctx, n_ferns=500, capacity=8, max_depth_mm=MAX_DEPTH_MM, photo_threshold=115.0, seed=7)
    table = f.table()
    assert table.tobytes() == ferns.make_table(7, 500, RW, RH, MAX_DEPTH_MM).tobytes()
    db = fr.Database(table)
    for i, t in enumerate(fs.KEYFRAME_TIMES):
        m = fs.maps(t)
        f.add(*(ctx.to_device(a) for a in m), fs.view(t)[2], 1 + i, -1.0)
        db.add_frame(*m, fs.view(t)[2], 1 + i, -1.0)
    assert f.count() == (len(fs.KEYFRAME_TIMES), False)
    out = {"ctx": ctx, "f": f, "db": db, "table": table}
    for name, t in (("near", fs.QUERY_TIME), ("far", "far")):
        m = fs.maps(t)
        f.encode(*(ctx.to_device(a) for a in m))
        out[name] = f.relocalise(fs.view(t)[2], 1000, 300, lost=True)
        v4r, n4r, rgb = fr.reduce_maps(*m)
        codes, good = fr.codes_literal(table, v4r, rgb)
        out[name + "_ref"] = dict(v4r=v4r, n4r=n4r, rgb=rgb, codes=codes, good=good, planar=fr.planar(v4r, n4r), find=db.find(codes, good, 1000, 300))
    yield out
    f.close(); ctx.close()


def oracle_track(kf, vmap, nmap):
    """tests/orc.py's tracker the way Ferns.cpp:215-225 drives it: model side the keyframe's reduced maps at its pose, frame side the
    current reduced planar maps (written into the oracle's level-0 frame maps: its initICP builds them from a depth image, the
    reference's Ferns tracker copies them from the reduced textures)"""
    fx, fy, cx, cy = reduced_cam()
    od = orc.Odometry(RW, RH, cx, cy, fx, fy)
    v4 = np.zeros((RH, RW, 4), f32); n4 = np.zeros((RH, RW, 4), f32)
    ok = ~np.isnan(kf.vmap[2 * RH:])
    for c in range(3):
        v4[..., c] = np.where(ok, kf.vmap[c * RH:(c + 1) * RH], 0); n4[..., c] = np.where(ok, kf.nmap[c * RH:(c + 1) * RH], 0)
    od.init_icp_model(v4, n4, kf.pose)
    for which, arr in ((0, vmap), (1, nmap)):
        C.memmove(orc.lib.orc_odom_buffer(C.c_void_p(od.h_), which, 0), arr.ctypes.data, arr.nbytes)
    tr, rot, st = od.track(kf.pose[:3, 3], kf.pose[:3, :3], rgb_only=False, icp_weight=100.0, pyramid=False, fast_odom=False, so3=False)
    est = np.eye(4, dtype=f32)
    est[:3, :3] = rot; est[:3, 3] = tr
    return est, st


def test_the_match_is_the_nearby_keyframe(rig):
    got, ref = rig["near"], rig["near_ref"]
    m, mid, _ = ref["find"]
    assert got["keyframe"] == mid == fs.QUERY_KEYFRAME
    assert f32(got["dissimilarity"]).tobytes() == f32(m).tobytes()
    want = fr.block_hd_aware(ref["codes"], rig["db"].frames[mid].codes)
    assert f32(got["overlap"]).tobytes() == f32(want).tobytes() and want > 0.3 and got["icp_ran"]


def test_tracker_result_equals_the_oracle_bit_for_bit(rig):
    got, ref = rig["near"], rig["near_ref"]
    est, st = oracle_track(rig["db"].frames[got["keyframe"]], *ref["planar"])
    print("oracle", est, st.last_icp_error, st.last_icp_count, "gpu", got["pose"], got["icp_error"], got["icp_count"])
    assert got["pose"].tobytes() == est.tobytes()
    assert f32(got["icp_error"]).tobytes() == f32(st.last_icp_error).tobytes()
    assert f32(got["icp_count"]).tobytes() == f32(st.last_icp_count).tobytes()


def test_photometric_error_equals_the_numpy_value(rig):
    got, ref = rig["near"], rig["near_ref"]
    kf = rig["db"].frames[got["keyframe"]]
    err, cnt, margin = fr.photometric_check(rig["table"], ref["planar"][0], ref["rgb"], got["pose"], kf.pose, kf.rgb, *reduced_cam(), MAX_DEPTH_MM)
    print("photo", err, cnt, "margin", margin, "gpu", got["photo_error"], got["photo_count"])
    assert margin >= 1e-3, "a correspondence coordinate of this query lies within 1e-3 px of an integer: choose another query"
    assert cnt > 0 and got["photo_count"] == cnt and got["photo_error"] == err
    assert got["accepted"] == bool(np.float64(got["icp_error"]) < 0.0003 and got["icp_count"] > 1400 and err < 115.0)
    assert got["accepted"]


def test_pose_is_close_to_the_ground_truth(rig):
    got = rig["near"]
    gt = fs.view(fs.QUERY_TIME)[2]
    dt, dr = fs.pose_error(got["pose"], gt)
    start = fs.pose_error(fs.view(fs.KEYFRAME_TIMES[fs.QUERY_KEYFRAME])[2], gt)
    print("pose error", dt, dr, "from", start)
    assert dt < fs.POSE_BOUND_M and dr < fs.POSE_BOUND_DEG


def test_an_unrelated_view_is_not_accepted(rig):
    got = rig["far"]
    print("far", {k: v for k, v in got.items() if k != "pose"})
    assert not got["accepted"]
    assert got["keyframe"] < 0 or not (got["overlap"] > 0.3) or not (np.float64(got["icp_error"]) < 0.0003 and got["icp_count"] > 1400) \
        or not (got["photo_error"] < 115.0)
