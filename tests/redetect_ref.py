"""The re-detection score and decision (csrc/redetect.hip, CoFusion::redetectModels) restated in numpy f32, one operation
per statement in the kernel's order.  Every output is an integer count that does not depend on execution order, so the device is compared
with this statement for EQUALITY (tests/test_redetect_gpu.py); tests/test_cpu_redetect_cases.py checks the statement itself against
cases whose counts are known by construction (tests/redetect_cases.py)."""
import numpy as np

F = np.float32
COUNT_FIELDS = ("projected", "occluded", "seen_through", "agree", "agree_on_label", "covered")


def inv44f(pose):
    """pose.inverse() of a rigid transform, linear part by cofactors: inv44f of csrc/cf_kernels.h, f32 throughout"""
    a = np.asarray(pose, F).reshape(16)
    c00 = F(a[5] * a[10]) - F(a[6] * a[9])
    c01 = F(a[6] * a[8]) - F(a[4] * a[10])
    c02 = F(a[4] * a[9]) - F(a[5] * a[8])
    det = F(F(F(a[0] * c00) + F(a[1] * c01)) + F(a[2] * c02))
    inv = F(F(1.0) / det)
    Li = np.zeros(9, F)
    Li[0] = c00 * inv
    Li[1] = F(F(a[2] * a[9]) - F(a[1] * a[10])) * inv
    Li[2] = F(F(a[1] * a[6]) - F(a[2] * a[5])) * inv
    Li[3] = c01 * inv
    Li[4] = F(F(a[0] * a[10]) - F(a[2] * a[8])) * inv
    Li[5] = F(F(a[2] * a[4]) - F(a[0] * a[6])) * inv
    Li[6] = c02 * inv
    Li[7] = F(F(a[1] * a[8]) - F(a[0] * a[9])) * inv
    Li[8] = F(F(a[0] * a[5]) - F(a[1] * a[4])) * inv
    o = np.zeros(16, F)
    for i in range(3):
        o[i * 4 + 0] = Li[i * 3 + 0]
        o[i * 4 + 1] = Li[i * 3 + 1]
        o[i * 4 + 2] = Li[i * 3 + 2]
        s = F(Li[i * 3 + 0] * a[3])
        s = F(s + F(Li[i * 3 + 1] * a[7]))
        s = F(s + F(Li[i * 3 + 2] * a[11]))
        o[i * 4 + 3] = -s
    o[15] = 1
    return o


def score(surfels, theta, pose, depth, label, new_label, cam, cutoff, tol):
    """one candidate: surfels f32 [n, 12] (row 0 = x, y, z, confidence), its confidence threshold and hypothesis pose (4x4, model <-
    camera); depth f32 [H, W], label u8 [H, W]; cam = (fx, fy, cx, cy).  Returns the six counts as a dict."""
    s = np.ascontiguousarray(surfels, F).reshape(-1, 12)
    rows, cols = depth.shape
    fx, fy, cx, cy = (F(v) for v in cam)
    cutoff = F(cutoff)
    tol = F(tol)
    theta = F(theta)
    T = inv44f(pose)
    with np.errstate(all="ignore"):
        s = s[s[:, 3] >= theta]                       # a NaN confidence takes no part
        x = s[:, 0]
        y = s[:, 1]
        z = s[:, 2]
        # xform_point: ((T0 x + T1 y) + T2 z) + T3, row by row
        phx = T[0] * x
        phx = phx + T[1] * y
        phx = phx + T[2] * z
        phx = phx + T[3]
        phy = T[4] * x
        phy = phy + T[5] * y
        phy = phy + T[6] * z
        phy = phy + T[7]
        phz = T[8] * x
        phz = phz + T[9] * y
        phz = phz + T[10] * z
        phz = phz + T[11]
        keep = ~((phz > cutoff) | (phz < 0))
        u = fx * phx
        u = u / phz
        u = u + cx
        v = fy * phy
        v = v / phz
        v = v + cy
        keep &= (u >= 0) & (v >= 0) & (u < F(cols)) & (v < F(rows))
        keep &= phz < cutoff
        u = u[keep]
        v = v[keep]
        phz = phz[keep]
        q = np.floor(v).astype(np.int64) * cols + np.floor(u).astype(np.int64)
        projected = int(q.size)
        d = depth.reshape(-1).astype(F)[q]
        valid = (d > 0) & ~(d > cutoff)
        lo = phz - tol
        hi = phz + tol
        occluded = valid & (d < lo)
        seen_through = valid & ~occluded & (d > hi)
        agree = valid & ~occluded & ~seen_through
        on_label = agree & (label.reshape(-1)[q].astype(np.int64) == int(new_label))
    return dict(projected=projected, occluded=int(occluded.sum()), seen_through=int(seen_through.sum()), agree=int(agree.sum()),
                agree_on_label=int(on_label.sum()), covered=int(np.unique(q[on_label]).size))


def label_pixels(label, new_label):
    return int(np.count_nonzero(label.astype(np.int64) == int(new_label)))


def decide(counts, n_label_pixels, min_fit, min_cover):
    """The host's decision over the candidates of one attempt, in list order.  Returns (rows, winner): rows = dict(fit, cover, eligible)
    per candidate (f32 quotients, thresholds inclusive, a zero denominator is never eligible), winner = the position of the eligible
    candidate with the largest agree_on_label -- ties go to the earlier position -- or -1."""
    rows = []
    winner = -1
    for k, c in enumerate(counts):
        seen = c["agree"] + c["seen_through"]
        fit = F(c["agree_on_label"]) / F(seen) if seen else F(0)
        cover = F(c["covered"]) / F(n_label_pixels) if n_label_pixels else F(0)
        eligible = bool(seen != 0 and n_label_pixels != 0 and fit >= F(min_fit) and cover >= F(min_cover))
        if eligible and (winner < 0 or c["agree_on_label"] > counts[winner]["agree_on_label"]):
            winner = k
        rows.append(dict(fit=fit, cover=cover, eligible=eligible))
    return rows, winner
