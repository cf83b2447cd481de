"""The re-detection search (DESIGN.md 4.13 "Search"; csrc/redetect_search.hip, CoFusion::searchModels) restated in numpy: per-element
arithmetic in f32, one operation per statement in the kernels' order; products formed exactly in f64 and rounded once to Python integers;
the registration loop in f64 with every operation spelled out (cf::redetect_register_solve).  Every device output is an integer that
does not depend on execution order, so the device is compared with this statement for EQUALITY (tests/test_redetect_search_gpu.py);
tests/test_cpu_redetect_search_ref.py checks the statement itself against cases known by construction (tests/redetect_search_cases.py)."""
import math

import numpy as np

import redetect_ref

F = np.float32
BINS = 512
POS_LIM = F(64.0)
POS_SCALE = F(65536.0)
ROW_LIM = F(4.0)
LAMBDA = 1e-3
EPS_T = 1e-5
EPS_R = 1e-5


def _pos_fix(x):
    """rint(clamp(x, +-64) * 2^16) as Python integers (fmax / fmin as the device's: a NaN becomes -64)"""
    c = np.fmax(np.asarray(x, F), -POS_LIM)
    c = np.fmin(c, POS_LIM)
    return [int(v) for v in np.rint((c * POS_SCALE).astype(np.float64))]


def _bins(r, g, b):
    r = np.asarray(r, np.int64); g = np.asarray(g, np.int64); b = np.asarray(b, np.int64)
    return ((r >> 5) << 6) | ((g >> 5) << 3) | (b >> 5)


def _hist(bins):
    return np.bincount(np.asarray(bins, np.int64), minlength=BINS).astype(np.uint32)


def pixel_vertex(px, py, d, cam):
    """createVMap: (d * (u - cx)) * (1 / fx), (d * (v - cy)) * (1 / fy), d"""
    fx, fy, cx, cy = (F(v) for v in cam)
    fx_inv = F(1.0) / fx
    fy_inv = F(1.0) / fy
    x = px.astype(F) - cx
    x = d * x
    x = x * fx_inv
    y = py.astype(F) - cy
    y = d * y
    y = y * fy_inv
    return x, y, d


def frame_moments(depth, label, rgba, new_label, cam, cutoff):
    """-> (moments [n, sx, sy, sz] as Python integers, hist uint32 [512])"""
    rows, cols = depth.shape
    d = depth.reshape(-1).astype(F)
    with np.errstate(all="ignore"):
        keep = (label.reshape(-1).astype(np.int64) == int(new_label)) & (d > 0) & ~(d > F(cutoff))
    i = np.nonzero(keep)[0]
    py = i // cols
    px = i - py * cols
    x, y, z = pixel_vertex(px, py, d[i], cam)
    c = rgba.reshape(-1, 4)[i]
    return [int(i.size), sum(_pos_fix(x)), sum(_pos_fix(y)), sum(_pos_fix(z))], _hist(_bins(c[:, 0], c[:, 1], c[:, 2]))


def _xform_dir(T, x, y, z):
    ox = T[0] * x
    ox = ox + T[1] * y
    ox = ox + T[2] * z
    oy = T[4] * x
    oy = oy + T[5] * y
    oy = oy + T[6] * z
    oz = T[8] * x
    oz = oz + T[9] * y
    oz = oz + T[10] * z
    return ox, oy, oz


def _xform_point(T, x, y, z):
    ox, oy, oz = _xform_dir(T, x, y, z)
    return ox + T[3], oy + T[7], oz + T[11]


def _dot(a, b):
    s = a[0] * b[0]
    s = s + a[1] * b[1]
    s = s + a[2] * b[2]
    return s


def model_moments(surfels, theta, pose, dhat):
    """one candidate; pose: the static hypothesis in the convention of the score (model <- camera; its f32 inverse is applied).
    -> (moments [n_front, sx, sy, sz] in the MODEL frame, hist uint32 [512] of all stable surfels)"""
    s = np.ascontiguousarray(surfels, F).reshape(-1, 12)
    T = redetect_ref.inv44f(pose)
    dh = [F(v) for v in np.asarray(dhat, F).reshape(3)]
    with np.errstate(all="ignore"):
        s = s[s[:, 3] >= F(theta)]
        ci = s[:, 4].astype(np.int32).astype(np.int64)
        hist = _hist(_bins((ci >> 16) & 255, (ci >> 8) & 255, ci & 255))
        n = _xform_dir(T, s[:, 8], s[:, 9], s[:, 10])
        front = _dot(n, dh) > 0          # (the maps' normals point away from the camera that saw them)
    s = s[front]
    return [int(s.shape[0]), sum(_pos_fix(s[:, 0])), sum(_pos_fix(s[:, 1])), sum(_pos_fix(s[:, 2]))], hist


def colour_similarity(hist_m, hist_f):
    """histogram intersection sum_b min(h_m / N_m, h_f / N_f) in f64, bins in order; 0 for an empty histogram"""
    nm = int(np.asarray(hist_m, np.int64).sum()); nf = int(np.asarray(hist_f, np.int64).sum())
    if not nm or not nf:
        return 0.0
    s = 0.0
    for a, b in zip(hist_m, hist_f):
        s += min(float(int(a)) / float(nm), float(int(b)) / float(nf))
    return s


def frame_centroid(moments):
    """f64 centroid of the label's vertices and the unit vector towards it; None for an empty label"""
    n = moments[0]
    if n <= 0:
        return None, None
    fbar = [math.ldexp(float(moments[1 + a]), -16) / float(n) for a in range(3)]
    norm = math.sqrt((fbar[0] * fbar[0] + fbar[1] * fbar[1]) + fbar[2] * fbar[2])
    if not norm > 0.0:
        return None, None
    return fbar, [fbar[a] / norm for a in range(3)]


def seed(T0, model_moments_k, fbar):
    """T(camera <- model) f32 [16] the registration starts from: the rotation of T0 (the static hypothesis, camera <- model), the
    front-facing centroid of the map on the label's centroid; None when no surfel faces the camera"""
    n = model_moments_k[0]
    if n <= 0:
        return None
    T0 = np.asarray(T0, F).reshape(16)
    mbar = [math.ldexp(float(model_moments_k[1 + a]), -16) / float(n) for a in range(3)]
    out = T0.copy()
    for i in range(3):
        s = float(T0[4 * i]) * mbar[0]
        s = s + float(T0[4 * i + 1]) * mbar[1]
        s = s + float(T0[4 * i + 2]) * mbar[2]
        out[4 * i + 3] = F(fbar[i] - s)
    return out


def register_step(surfels, theta, T, depth, label, new_label, cam, cutoff, tol, centre):
    """one step at T = T(camera <- model) f32 [16]: the 29 sums as Python integers in a list of 32"""
    s = np.ascontiguousarray(surfels, F).reshape(-1, 12)
    T = np.asarray(T, F).reshape(16)
    rows, cols = depth.shape
    fx, fy, cx, cy = (F(v) for v in cam)
    cutoff = F(cutoff); tol = F(tol)
    c = [F(v) for v in np.asarray(centre, F).reshape(3)]
    out = [0] * 32
    with np.errstate(all="ignore"):
        s = s[s[:, 3] >= F(theta)]
        px_, py_, pz_ = _xform_point(T, s[:, 0], s[:, 1], s[:, 2])
        keep = ~((pz_ > cutoff) | (pz_ < 0))
        u = fx * px_
        u = u / pz_
        u = u + cx
        v = fy * py_
        v = v / pz_
        v = v + cy
        keep &= (u >= 0) & (v >= 0) & (u < F(cols)) & (v < F(rows))
        keep &= pz_ < cutoff
        s = s[keep]; p = (px_[keep], py_[keep], pz_[keep]); u = u[keep]; v = v[keep]
        qy = np.floor(v).astype(np.int64)
        qx = np.floor(u).astype(np.int64)
        q = qy * cols + qx
        d = depth.reshape(-1).astype(F)[q]
        keep = (label.reshape(-1)[q].astype(np.int64) == int(new_label)) & (d > 0) & ~(d > cutoff)
        vx, vy, vz = pixel_vertex(qx, qy, d, cam)
        diff = (vx - p[0], vy - p[1], vz - p[2])
        dist = np.sqrt(_dot(diff, diff))
        keep &= dist <= tol
        n = _xform_dir(T, s[:, 8], s[:, 9], s[:, 10])
        keep &= _dot(n, p) > 0
        lever = (p[0] - c[0], p[1] - c[1], p[2] - c[2])
        cr = (lever[1] * n[2] - lever[2] * n[1], lever[2] * n[0] - lever[0] * n[2], lever[0] * n[1] - lever[1] * n[0])
        r = _dot(n, diff)
        row = [np.fmin(np.fmax(e, -ROW_LIM), ROW_LIM)[keep].astype(np.float64) for e in (n[0], n[1], n[2], cr[0], cr[1], cr[2], r)]
    w = 0
    for a in range(6):
        for b in range(a, 7):
            out[w] = sum(int(x) for x in np.rint(row[a] * row[b] * 4294967296.0))
            w += 1
    out[27] = sum(int(x) for x in np.rint(row[6] * row[6] * 4294967296.0))
    out[28] = int(row[0].size)
    return out


def _det_sincos(x):
    """cf_device.h: det_sincos, the same operations"""
    two_over_pi = 0.63661977236758134308
    pio2_1 = 1.57079632673412561417e+00
    pio2_1t = 6.07710050650619224932e-11
    fn = float(np.rint(x * two_over_pi))
    r = (x - fn * pio2_1) - fn * pio2_1t
    n = int(fn)
    r2 = r * r
    sp = -1.0 / 355687428096000.0
    sp = sp * r2 + 1.0 / 1307674368000.0
    sp = sp * r2 - 1.0 / 6227020800.0
    sp = sp * r2 + 1.0 / 39916800.0
    sp = sp * r2 - 1.0 / 362880.0
    sp = sp * r2 + 1.0 / 5040.0
    sp = sp * r2 - 1.0 / 120.0
    sp = sp * r2 + 1.0 / 6.0
    sr = r - r * r2 * sp
    cp = 1.0 / 20922789888000.0
    cp = cp * r2 - 1.0 / 87178291200.0
    cp = cp * r2 + 1.0 / 479001600.0
    cp = cp * r2 - 1.0 / 3628800.0
    cp = cp * r2 + 1.0 / 40320.0
    cp = cp * r2 - 1.0 / 720.0
    cp = cp * r2 + 1.0 / 24.0
    cp = cp * r2 - 1.0 / 2.0
    cr = 1.0 + r2 * cp
    return ((sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr))[n & 3]


def _norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def solve_step(sums, centre, R, t, lam=LAMBDA):
    """(A + lam tr(A) / 6 I) xi = b by Cholesky, xi = (tau, omega); R <- exp(omega) R, t <- exp(omega) (t - centre) + centre + tau.  All
    f64 (Python floats), R [9] and t [3] lists.  -> (R, t, |tau|, |omega|) or None when the damped matrix is not positive definite"""
    A = [[0.0] * 6 for _ in range(6)]
    b = [0.0] * 6
    w = 0
    for i in range(6):
        for j in range(i, 7):
            v = math.ldexp(float(sums[w]), -32)
            w += 1
            if j == 6:
                b[i] = v
            else:
                A[i][j] = v
                A[j][i] = v
    tr = A[0][0]
    for i in range(1, 6):
        tr = tr + A[i][i]
    mu = (lam * tr) / 6.0
    for i in range(6):
        A[i][i] = A[i][i] + mu
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            u = A[i][j]
            for k in range(j):
                u = u - L[i][k] * L[j][k]
            L[i][j] = u / L[j][j]
    y = [0.0] * 6
    x = [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    tau, om = x[:3], x[3:]
    theta = _norm3(om)
    E = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    if theta >= 2.2204460492503131e-16:
        sn, cs = _det_sincos(theta)
        c1 = 1.0 - cs
        it = 1.0 / theta
        rx, ry, rz = om[0] * it, om[1] * it, om[2] * it
        rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
        r_x = [0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0]
        I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        E = [(cs * I[k] + c1 * rrt[k]) + sn * r_x[k] for k in range(9)]
    Rn = [0.0] * 9
    for i in range(3):
        for j in range(3):
            s = E[i * 3] * R[j]
            s = s + E[i * 3 + 1] * R[3 + j]
            s = s + E[i * 3 + 2] * R[6 + j]
            Rn[i * 3 + j] = s
    u = [t[0] - centre[0], t[1] - centre[1], t[2] - centre[2]]
    tn = [0.0] * 3
    for i in range(3):
        s = E[i * 3] * u[0]
        s = s + E[i * 3 + 1] * u[1]
        s = s + E[i * 3 + 2] * u[2]
        s = s + centre[i]
        tn[i] = s + tau[i]
    return Rn, tn, _norm3(tau), theta


def _pose32(R, t):
    return np.array([R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0.0, 0.0, 0.0, 1.0], np.float64).astype(F)


def register(surfels, theta, seed_T, depth, label, new_label, cam, cutoff, tol, centre, iterations=10):
    """cf_redetect_register: dict(ok, iterations, first_inliers, last_inliers, rms (f32), cam_from_model f32 [4, 4])"""
    T = np.asarray(seed_T, F).reshape(16)
    R = [float(T[4 * i + j]) for i in range(3) for j in range(3)]
    t = [float(T[4 * i + 3]) for i in range(3)]
    c32 = np.asarray(centre, F).reshape(3)
    c = [float(v) for v in c32]
    res = dict(ok=True, iterations=0, first_inliers=0, last_inliers=0, rms=F(0))
    for it in range(iterations):
        sums = register_step(surfels, theta, _pose32(R, t), depth, label, new_label, cam, cutoff, tol, c32)
        n = sums[28]
        if it == 0:
            res["first_inliers"] = n
        res["last_inliers"] = n
        res["rms"] = F(math.sqrt(math.ldexp(float(sums[27]), -32) / float(n))) if n > 0 else F(0)
        if n < 6 or 2 * n < res["first_inliers"]:
            res["ok"] = False
            break
        step = solve_step(sums, c, R, t)
        if step is None:
            res["ok"] = False
            break
        R, t, tn, on = step
        res["iterations"] = it + 1
        if tn < EPS_T and on < EPS_R:
            break
    res["cam_from_model"] = _pose32(R, t).reshape(4, 4)
    return res
