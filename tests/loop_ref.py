"""numpy statement of the loop-closure seam of the fern database (Ferns::findFrame for a camera that is not lost, Ferns.cpp:144-262),
written as literally as the reference: the gate (match + blockHDAware), the photometric check with its exact integer sum, the accept
rule and the surface-constraint rows in the interleaved layout of a pinned closure.  Test infrastructure only.

Conventions: the photometric check runs in f64 from the f32 inputs with the association written below and
truncates coordinates towards zero; a sample is valid when z > 0 and int(z * 1000.0f) < max_depth_mm (NaN z: invalid); constraint
coordinates are ((m0 x + m1 y) + m2 z) + m3 in f32; times are f32."""
from __future__ import annotations

import numpy as np

import ferns_ref as fr

f32 = np.float32
MAX_SAMPLES = 64


def loop_samples(n_ferns):
    """number of samples i = 0, s, 2s, ... < n with s = n // 50, or None where loop closure is refused"""
    if n_ferns < 50:
        return None
    s = n_ferns // 50
    m = -(-n_ferns // s)
    return m if m <= MAX_SAMPLES else None


def block_hd_aware(c1, c2):
    """Ferns.cpp:321-336 -> overlap (f32, NaN for 0 / 0), count of ferns good in both"""
    count = 0
    val = f32(0)
    for a, b in zip(c1, c2):
        if a != fr.BAD and b != fr.BAD:
            count += 1
            if a == b:
                val = f32(val + f32(1.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return f32(val / f32(count)), count


def gate(codes_q, good_q, frames, time, min_age):
    """the record ferns_gate_kernel writes, from the literal search (frames: ferns_ref.Frame list) + the candidate decision and the
    branch taken: 'no_match', 'nan_overlap', 'not_candidate' or 'candidate'"""
    K = len(frames)
    if K:
        _, _, m, mid = fr.search_vector(codes_q, good_q, np.stack([f.codes for f in frames]), np.array([f.good for f in frames]),
                                        np.array([f.time for f in frames]), time, min_age)
    else:
        m, mid = fr.FLT_MAX, -1
    rec = dict(match_id=int(mid), dissimilarity=f32(m), overlap=f32(0), good_q=int(good_q), keyframe_time=0, count=0, keyframes=K)
    if mid < 0:
        return dict(rec, candidate=False, branch="no_match")
    ov, count = block_hd_aware(codes_q, frames[mid].codes)
    rec.update(overlap=ov, count=count, keyframe_time=int(frames[mid].time))
    cand = bool(ov > f32(0.3))
    return dict(rec, candidate=cand, branch="nan_overlap" if np.isnan(ov) else "candidate" if cand else "not_candidate")


def valid_sample(z, max_depth_mm):
    z = f32(z)
    return bool(z > 0) and int(f32(z * f32(1000.0))) < max_depth_mm


def photometric(table, vmap_cur, rgb_cur, est_pose, fern_pose, fern_rgb, cam, max_depth_mm):
    """Ferns.cpp:264-307 -> sum, count, and how many ferns left by each way out (a trace for the case table)"""
    h, w = rgb_cur.shape[:2]
    E = np.asarray(est_pose, f32).reshape(4, 4).astype(np.float64)
    F = np.asarray(fern_pose, f32).reshape(4, 4).astype(np.float64)
    fx, fy, cx, cy = (float(f32(a)) for a in cam)
    Rd = [[0.0] * 3 for _ in range(3)]
    td = [0.0] * 3
    for i in range(3):
        for j in range(3):
            Rd[i][j] = (F[0, i] * E[0, j] + F[1, i] * E[1, j]) + F[2, i] * E[2, j]
        td[i] = (F[0, i] * (E[0, 3] - F[0, 3]) + F[1, i] * (E[1, 3] - F[1, 3])) + F[2, i] * (E[2, 3] - F[2, 3])
    total, count = 0, 0
    trace = dict(invalid=0, nonfinite=0, outside=0, trunc_left=0, black=0)
    for i in range(len(table)):
        f = table[i]
        z = f32(vmap_cur[2 * h + f["y"], f["x"]])
        if not valid_sample(z, max_depth_mm):
            trace["invalid"] += 1
            continue
        x, y, zz = np.float64(vmap_cur[f["y"], f["x"]]), np.float64(vmap_cur[h + f["y"], f["x"]]), np.float64(z)
        with np.errstate(all="ignore"):
            wx = ((Rd[0][0] * x + Rd[0][1] * y) + Rd[0][2] * zz) + td[0]
            wy = ((Rd[1][0] * x + Rd[1][1] * y) + Rd[1][2] * zz) + td[1]
            wz = ((Rd[2][0] * x + Rd[2][1] * y) + Rd[2][2] * zz) + td[2]
            u = float(np.float64(wx) * fx / np.float64(wz) + cx)
            v = float(np.float64(wy) * fy / np.float64(wz) + cy)
        if not (abs(u) < 1e9) or not (abs(v) < 1e9):
            trace["nonfinite"] += 1
            continue
        iu, iv = int(u), int(v)   # truncation towards zero
        if iu < 0 or iv < 0 or iu >= w or iv >= h:
            trace["outside"] += 1
            continue
        if u < 0 or v < 0:
            trace["trunc_left"] += 1   # (-1, 0) lands on pixel 0
        kp = fern_rgb[iv, iu]
        if not (kp[0] > 0 or kp[1] > 0 or kp[2] > 0):
            trace["black"] += 1
            continue
        cp = rgb_cur[f["y"], f["x"]]
        total += abs(int(kp[0]) - int(cp[0])) + abs(int(kp[1]) - int(cp[1])) + abs(int(kp[2]) - int(cp[2]))
        count += 1
    return total, count, trace


def accept(icp_error, icp_count, lost, photo_sum, photo_count, photo_threshold):
    """Ferns.cpp:233-237 -> accepted, photo error (f64; +inf with no correspondence)"""
    photo = float(photo_sum) / float(photo_count) if photo_count else float("inf")
    thresh = 1400 if lost else 2400
    ok = float(f32(icp_error)) < 0.0003 and f32(icp_count) > f32(thresh) and photo < float(f32(photo_threshold))
    return bool(ok), photo


def _mul(m, x, y, z):
    m = np.asarray(m, f32).reshape(4, 4)
    with np.errstate(all="ignore"):
        return [f32(f32(f32(f32(m[r, 0] * x) + f32(m[r, 1] * y)) + f32(m[r, 2] * z)) + m[r, 3]) for r in range(3)]


def constraint_rows(table, vmap_cur, curr_pose, est_pose, time, keyframe_time, max_depth_mm):
    """Ferns.cpp:240-255 + the pins -> src [2 m, 3], dst [2 m, 3], time [2 m] (f32), samples drawn"""
    h = vmap_cur.shape[0] // 3
    n = len(table)
    step = n // 50
    src, dst, tm = [], [], []
    samples = 0
    for i in range(0, n, step):
        samples += 1
        f = table[i]
        z = f32(vmap_cur[2 * h + f["y"], f["x"]])
        if not valid_sample(z, max_depth_mm):
            continue
        x, y = f32(vmap_cur[f["y"], f["x"]]), f32(vmap_cur[h + f["y"], f["x"]])
        raw, model = _mul(curr_pose, x, y, z), _mul(est_pose, x, y, z)
        src += [raw, model]; dst += [model, model]; tm += [f32(time), f32(keyframe_time)]
    return (np.array(src, f32).reshape(-1, 3), np.array(dst, f32).reshape(-1, 3), np.array(tm, f32)), samples


def closure(table, vmap_cur, rgb_cur, frame, curr_pose, est_pose, icp_error, icp_count, lost, time, cam, max_depth_mm, photo_threshold):
    """the record ferns_close_kernel writes against keyframe `frame` (a ferns_ref.Frame), the rows it leaves, and a trace"""
    s, c, trace = photometric(table, vmap_cur, rgb_cur, est_pose, frame.pose, frame.rgb, cam, max_depth_mm)
    ok, photo = accept(icp_error, icp_count, lost, s, c, photo_threshold)
    rows = (np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, f32))
    trace.update(samples=0, valid_samples=0)
    if ok and not lost:
        rows, trace["samples"] = constraint_rows(table, vmap_cur, curr_pose, est_pose, time, frame.time, max_depth_mm)
        trace["valid_samples"] = len(rows[2]) // 2
    rec = dict(accepted=ok, n_constraints=len(rows[2]), photo_sum=s, photo_count=c, photo_error=photo, keyframe_time=int(frame.time))
    return rec, rows, trace
