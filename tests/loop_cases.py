"""Case table of the loop-closure seam of the fern database (csrc/ferns.hip: ferns_gate_kernel, ferns_close_kernel) at 128x64, reduced
to 16x8, with caller-supplied tables of 64 and 100 ferns: one named case per branch of the gate, the photometric check, the accept rule
and the constraint generation.  Keyframes and queries are hand-made full-size maps that go in through the ordinary encode / append
calls.  tests/test_cpu_loop_ref.py shows on the numpy statement (loop_ref.py) that every case reaches the branch it is named for;
tests/test_loop_kernels_gpu.py holds the kernels against the statement on the same table.

Geometry.  The reduced intrinsics are fx = fy = 8, cx = 8, cy = 4, so a point (X, Y, 1) projects to u = 8 X + 8, v = 8 Y + 4 exactly.
The base frame puts the vertex of reduced pixel (x, y) at ((x + 0.25 - 8) / 8 z, (y + 0.25 - 4) / 8 z, z): under an identity pose
difference it projects a quarter pixel inside its own pixel, far from every truncation boundary."""
from __future__ import annotations

import numpy as np

import ferns_ref as fr

f32 = np.float32
W, H, RW, RH = fr.W, fr.H, fr.RW, fr.RH
CAM = (64.0, 64.0, 64.0, 32.0)          # of the full frame; reduced: 8, 8, 8, 4
RCAM = (8.0, 8.0, 8.0, 4.0)
MAX_DEPTH_MM = 5000
PHOTO_THRESHOLD = 115.0


def table(n):
    """fern i sits at reduced pixel (i % 16, i // 16): every fern has a pixel of its own (n <= 128)"""
    t = np.zeros(n, fr.FERN)
    i = np.arange(n)
    t["x"], t["y"] = i % RW, i // RW
    t["r"] = t["g"] = t["b"] = 127
    t["d"] = 2000
    return t


def blank():
    v4 = np.zeros((H, W, 4), f32); n4 = np.zeros((H, W, 4), f32); rgba = np.zeros((H, W, 4), np.uint8)
    n4[..., 2] = 1
    rgba[..., 3] = 255
    return v4, n4, rgba


def put(maps, x, y, xyz, rgb):
    v4, _, rgba = maps
    v4[8 * y + 4, 8 * x + 4, :3] = np.asarray(xyz, f32)
    rgba[8 * y + 4, 8 * x + 4, :3] = rgb


def own_pixel(x, y, z):
    z = f32(z)
    return (f32((x + 0.25 - 8) / 8) * z, f32((y + 0.25 - 4) / 8) * z, z)


def colour(x, y):
    return (40 + 3 * x, 60 + 5 * y, 90 + x + y)   # all below the ferns' thresholds (127) and none black


def base_frame(n, z=lambda i: 1.0 + 0.01 * (i % 7), rgb=lambda i: colour(i % RW, i // RW)):
    """a frame with a vertex under each of the first n ferns; z(i) == None leaves the pixel empty (z = 0)"""
    m = blank()
    for i in range(n):
        zi = z(i)
        if zi is not None:
            put(m, i % RW, i // RW, own_pixel(i % RW, i // RW, zi), rgb(i))
    return m


def pose(rx, ry, rz, t):
    """a general rigid pose, f32"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    p = np.eye(4)
    p[:3, :3] = R; p[:3, 3] = t
    return p.astype(f32)


EYE = np.eye(4, dtype=f32)
KF_POSE = pose(0.11, -0.23, 0.07, (0.31, -0.12, 0.93))
DRIFTED = pose(0.13, -0.20, 0.05, (0.42, -0.10, 0.88))     # the camera's own (drifted) pose: source side of the constraints
GOOD_ICP = dict(icp_error=f32(1e-4), icp_count=f32(3000.0))
ERR_AT = f32(3e-4)                                          # as f64 it is 0.00030000001...: not < 0.0003


class Scene:
    """table + keyframes [(maps, pose, srcTime)] + the query maps + the search's (time, min_age)"""

    def __init__(self, n, keyframes, query, time=1000, min_age=300, photo_threshold=PHOTO_THRESHOLD):
        self.n, self.table, self.keyframes, self.query, self.time, self.min_age = n, table(n), keyframes, query, time, min_age
        self.photo_threshold = photo_threshold


def _recolour(n, changed, delta=(0, 0, 0), above=False):
    """the base colours, with ferns in `changed` moved by delta, or lifted above the ferns' thresholds (another code)"""
    def rgb(i):
        c = colour(i % RW, i // RW)
        if i in changed:
            return (200, 200, 200) if above else tuple(int(a) + int(b) for a, b in zip(c, delta))
        return c
    return rgb


def _scenes():
    S = {}
    same64, same100 = base_frame(64), base_frame(100)
    # --- gate
    S["young_keyframe"] = Scene(64, [(same64, KF_POSE, 800)], same64, time=1000, min_age=300)
    S["disjoint_good"] = Scene(64, [(base_frame(64, z=lambda i: 1.0 if i < 32 else None), KF_POSE, 5)],
                               base_frame(64, z=lambda i: 1.0 if i >= 32 else None))
    S["overlap_30"] = Scene(100, [(base_frame(100, rgb=_recolour(100, set(range(30, 100)), above=True)), KF_POSE, 5)], same100)
    S["overlap_31"] = Scene(100, [(base_frame(100, rgb=_recolour(100, set(range(31, 100)), above=True)), KF_POSE, 5)], same100)
    # --- closure
    S["all_valid_64"] = Scene(64, [(base_frame(64, rgb=_recolour(64, set(range(64)), (10, -7, 3))), KF_POSE, 7)], same64)
    S["second_keyframe"] = Scene(64, [(base_frame(64, rgb=_recolour(64, set(range(40, 64)), above=True)), EYE, 3),
                                      (base_frame(64, rgb=_recolour(64, set(range(64)), (1, 2, 3))), KF_POSE, 9)], same64)
    zs = [None, 0.0, 5.0, 5.0005, 6.0, -1.0]   # empty, 0 (NaN after the reduction), int(5000.0), int(5000.5) == 5000, over, negative
    S["samples_invalid"] = Scene(100, [(same100, KF_POSE, 7)], base_frame(100, z=lambda i: 1.0 + 0.01 * (i % 7) if i % 2 else zs[(i // 2) % 6]))
    gaps = lambda i: (4.9999 if i % 8 == 0 else 1.0 + 0.01 * (i % 7)) if i % 2 or (i // 2) % 3 != 1 else zs[(i // 6) % 6]
    S["samples_gaps"] = Scene(100, [(same100, KF_POSE, 7)], base_frame(100, z=gaps))
    # a keyframe whose colours differ by (40, 15, -60) under every fern, codes unchanged: the photometric error is 115 exactly
    S["photo_at_threshold"] = Scene(64, [(base_frame(64, rgb=_recolour(64, set(range(64)), (40, 15, -60))), KF_POSE, 7)], same64)
    S["photo_below_threshold"] = Scene(64, [(base_frame(64, rgb=_recolour(64, set(range(1, 64)), (40, 15, -60))), KF_POSE, 7)], same64)
    # --- projections, identity pose difference: the points of ferns 0..3 are moved by hand
    kf = base_frame(64)
    put(kf, 5, 2, own_pixel(5, 2, 1.0), (0, 0, 0))           # a black keyframe pixel
    def moved(points):
        q = base_frame(64, z=lambda i: 1.0 if i >= 4 else None)
        for i, xyz in enumerate(points):
            put(q, i, 0, xyz, colour(i, 0))
        return q
    S["trunc_left"] = Scene(64, [(kf, EYE, 7)], moved([(-1.0625, -0.5625, 1.0)]))                       # u = v = -0.5 -> pixel (0, 0)
    S["outside"] = Scene(64, [(kf, EYE, 7)], moved([(-1.1875, 0.0, 1.0), (1.0, 0.0, 1.0), (0.0, 0.5, 1.0), (0.0, -0.625, 1.0)]))   # u = -1.5, 16; v = 8, -1
    S["nonfinite"] = Scene(64, [(kf, EYE, 7)], moved([(np.inf, 0.0, 1.0), (1.0, 1.0, 1e-30), (0.0, np.nan, 1.0)]))
    S["black_pixel"] = Scene(64, [(kf, EYE, 7)], moved([own_pixel(5, 2, 1.5)]))
    none = blank()
    for i in range(64):
        put(none, i % RW, i // RW, (3.0 + i, 0.0, 1.0), colour(i % RW, i // RW))
    S["no_correspondence"] = Scene(64, [(kf, EYE, 7)], none)
    return S


_CACHE = {}


def scenes():
    if "s" not in _CACHE:
        _CACHE["s"] = _scenes()
    return _CACHE["s"]


def _cl(scene, keyframe=0, curr=DRIFTED, est=None, lost=0, time=1000, **icp):
    a = dict(GOOD_ICP)
    a.update(icp)
    return dict(scene=scene, keyframe=keyframe, curr_pose=curr, est_pose=est, lost=lost, time=time, **a)


# name -> (scene, expected gate branch, closure arguments or None, what the statement's record / trace must show)
# est_pose None: the keyframe's pose (an identity pose difference up to the rounding of R^T R)
CASES = {
    "no_match": ("young_keyframe", "no_match", None, {}),
    "none_good_in_both": ("disjoint_good", "nan_overlap", None, dict(count=0, match_id=0)),
    "overlap_exactly_0_3": ("overlap_30", "not_candidate", None, dict(count=100, overlap=f32(0.3))),
    "overlap_just_above": ("overlap_31", "candidate", None, dict(count=100, overlap=f32(0.31))),
    "every_sample_valid": ("all_valid_64", "candidate", _cl("all_valid_64"), dict(accepted=True, n_constraints=128, samples=64, photo_count=64, photo_sum=64 * 20)),
    "match_is_second_keyframe": ("second_keyframe", "candidate", _cl("second_keyframe", keyframe=1), dict(accepted=True, match_id=1, keyframe_time=9, n_constraints=128)),
    "no_sample_valid": ("samples_invalid", "candidate", _cl("samples_invalid"), dict(accepted=True, n_constraints=0, samples=50, valid_samples=0, photo_count=50)),
    "valid_samples_with_gaps": ("samples_gaps", "candidate", _cl("samples_gaps"), dict(accepted=True, samples=50, valid_samples=33, n_constraints=66)),
    "left_of_image_truncates_to_0": ("trunc_left", "candidate", _cl("trunc_left", est=EYE), dict(trunc_left=1, outside=0, photo_count=60)),
    "projection_outside": ("outside", "candidate", _cl("outside", est=EYE), dict(outside=4, photo_count=59)),
    "projection_not_finite": ("nonfinite", "candidate", _cl("nonfinite", est=EYE, lost=1), dict(nonfinite=3, photo_count=59, n_constraints=0)),
    "black_keyframe_pixel": ("black_pixel", "candidate", _cl("black_pixel", est=EYE), dict(black=2, photo_count=59)),
    "no_correspondence_at_all": ("no_correspondence", "candidate", _cl("no_correspondence", est=EYE), dict(accepted=False, photo_count=0, photo_error=float("inf"), n_constraints=0)),
    "icp_count_2400_not_lost": ("all_valid_64", "candidate", _cl("all_valid_64", icp_count=f32(2400.0)), dict(accepted=False, n_constraints=0)),
    "icp_count_2401_not_lost": ("all_valid_64", "candidate", _cl("all_valid_64", icp_count=f32(2401.0)), dict(accepted=True, n_constraints=128)),
    "icp_count_1400_lost": ("all_valid_64", "candidate", _cl("all_valid_64", icp_count=f32(1400.0), lost=1), dict(accepted=False, n_constraints=0)),
    "icp_count_2400_lost": ("all_valid_64", "candidate", _cl("all_valid_64", icp_count=f32(2400.0), lost=1), dict(accepted=True, n_constraints=0)),
    "icp_error_exactly_3e-4": ("all_valid_64", "candidate", _cl("all_valid_64", icp_error=ERR_AT), dict(accepted=False, n_constraints=0)),
    "icp_error_just_below_3e-4": ("all_valid_64", "candidate", _cl("all_valid_64", icp_error=np.nextafter(ERR_AT, f32(0))), dict(accepted=True, n_constraints=128)),
    "photo_error_at_threshold": ("photo_at_threshold", "candidate", _cl("photo_at_threshold"), dict(accepted=False, photo_error=115.0, photo_count=64, n_constraints=0)),
    "photo_error_below_threshold": ("photo_below_threshold", "candidate", _cl("photo_below_threshold"), dict(accepted=True, photo_sum=63 * 115, photo_count=64, n_constraints=128)),
    "lost_accepted_writes_no_constraints": ("all_valid_64", "candidate", _cl("all_valid_64", lost=1), dict(accepted=True, n_constraints=0, samples=0)),
}


def statement(name):
    """the numpy statement's answer to a case -> dict(gate=..., closure=(record, rows, trace) or None)"""
    import loop_ref as lr
    scene_name, _, cl, _ = CASES[name]
    sc = scenes()[scene_name]
    key = ("db", scene_name)
    if key not in _CACHE:
        db = fr.Database(sc.table)
        for maps, p, t in sc.keyframes:
            assert db.add_frame(*maps, p, t, -1.0)[0]
        v4r, n4r, rgb = fr.reduce_maps(*sc.query)
        codes, good = fr.codes_literal(sc.table, v4r, rgb)
        _CACHE[key] = (db, fr.planar(v4r, n4r)[0], rgb, codes, good)
    db, vmap, rgb, codes, good = _CACHE[key]
    out = dict(gate=lr.gate(codes, good, db.frames, sc.time, sc.min_age), closure=None)
    if cl is not None:
        frame = db.frames[cl["keyframe"]]
        est = frame.pose if cl["est_pose"] is None else cl["est_pose"]
        out["closure"] = lr.closure(sc.table, vmap, rgb, frame, cl["curr_pose"], est, cl["icp_error"], cl["icp_count"], cl["lost"], cl["time"], RCAM,
                                    MAX_DEPTH_MM, sc.photo_threshold)
    return out
