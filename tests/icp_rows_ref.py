"""Independent reference of the ICP step's fixed-point sums (plain helper module, in the style of tests/render_ref.py).

The oracle (oracle/orc_track.c, oracle/orc_math.h) and the kernels (csrc/track_reduce.hip) share one specification,

    sums[k] += RNE(clamp(row_i) * clamp(row_j) * 2^32)      clamp at +-2^9, wrapping 64-bit integers,

and both implement it with the same floating-point trick, so a shared misconception would pass every parity test between the two.
Here the per-pixel row [n, vcurr x n, n . (vcurr - vprev)] (icp_row's n_cp . (s_cp - d_cp), source minus destination) and its gates are stated in numpy f32 in the operation order of
oracle/orc_track.c (icp_row), and the sums are then formed with Python's unbounded integers and exact rationals:
round(Fraction) is round-half-even by definition, nothing is scaled, split or wrapped.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import common
import orc

F32 = np.float32
LIM = F32(512.0)       # 2^((50 - 32) / 2)
FIX = 32


def _mul33(R, v):
    """orc_m33_mul: (m0*x + m1*y) + m2*z per component, f32"""
    R = np.asarray(R, F32).reshape(9)
    x, y, z = v
    return [R[3 * i] * x + R[3 * i + 1] * y + R[3 * i + 2] * z for i in range(3)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _f2i_rn(v):
    """__float2int_rn: round-half-even, saturating, NaN -> 0"""
    v = np.where(v != v, F32(0), v)
    v = np.clip(v, F32(-2147483648.0), F32(2147483520.0))
    return np.rint(v).astype(np.int64)


def rows_f32(Rcurr, tcurr, vc, nc, Rprev_inv, tprev, cam, vp, npv, dist_thres, angle_thres):
    """-> rows f32 [N, 7], found bool [N] (row major over the image); planar [3 * rows, cols] maps as the library's"""
    fx, fy, cx, cy = (F32(v) for v in cam)
    rows, cols = vc.shape[0] // 3, vc.shape[1]
    tcurr = [F32(v) for v in tcurr]; tprev = [F32(v) for v in tprev]
    P = lambda m: [np.ascontiguousarray(m[i * rows:(i + 1) * rows], F32).reshape(-1) for i in range(3)]
    with np.errstate(all="ignore"):
        vcurr, ncurr = P(vc), P(nc)
        g = _mul33(Rcurr, vcurr)
        vcurr_g = [g[i] + tcurr[i] for i in range(3)]
        cp = _mul33(Rprev_inv, [vcurr_g[i] - tprev[i] for i in range(3)])
        ux = _f2i_rn(cp[0] * fx / cp[2] + cx)
        uy = _f2i_rn(cp[1] * fy / cp[2] + cy)
        inside = (ux >= 0) & (uy >= 0) & (ux < cols) & (uy < rows) & ~(cp[2] < 0)
        at = np.where(inside, uy * cols + ux, 0)
        vprev_g = [p[at] for p in P(vp)]
        nprev_g = [p[at] for p in P(npv)]
        ncurr_g = _mul33(Rcurr, ncurr)
        d = [vprev_g[i] - vcurr_g[i] for i in range(3)]
        dist = np.sqrt(_dot(d, d))
        c = _cross(ncurr_g, nprev_g)
        sine = np.sqrt(_dot(c, c))
        found = inside & (sine < F32(angle_thres)) & (dist <= F32(dist_thres)) & ~np.isnan(ncurr[0]) & ~np.isnan(nprev_g[0])
        s_cp = cp
        d_cp = _mul33(Rprev_inv, [vprev_g[i] - tprev[i] for i in range(3)])
        n_cp = _mul33(Rprev_inv, nprev_g)
        cr = _cross(s_cp, n_cp)
        r6 = _dot(n_cp, [s_cp[i] - d_cp[i] for i in range(3)])
    out = np.stack(n_cp + cr + [r6], axis=1).astype(F32)
    out[~found] = 0
    return out, found


def exact_sums(rows, found):
    """the 29 sums in Python integers: 27 products i <= j over [row_0..5 | row_6], row_6^2, the count -- NOT wrapped"""
    sums = [0] * 29
    scale = 1 << FIX
    for r in rows[found]:
        q = [Fraction(float(min(max(v, -LIM), LIM))) for v in r]   # (a found row is finite: NaN fails both gates)
        k = 0
        for i in range(6):
            for j in range(i, 7):
                sums[k] += round(q[i] * q[j] * scale)   # round(Fraction): exact, half to even
                k += 1
        sums[27] += round(q[6] * q[6] * scale)
        sums[28] += 1
    return sums


def fits_int64(sums):
    return all(-(1 << 63) <= s < (1 << 63) for s in sums)


# ------------------------------------------------------------------------------------------------ inputs
COLS, ROWS = 80, 60
IDENT = np.eye(3, dtype=F32)
ZERO3 = np.zeros(3, F32)


def _planar(x, y, z):
    return np.concatenate([np.asarray(a, F32).reshape(ROWS, COLS) for a in (x, y, z)], axis=0)


def _self_projecting(fx, z):
    """vertices that project onto their own pixel exactly under identity poses: cx, cy, fx, z chosen as powers of two / small integers"""
    u, v = np.meshgrid(np.arange(COLS, dtype=F32), np.arange(ROWS, dtype=F32))
    cx, cy = F32(COLS // 2), F32(ROWS // 2)
    x = (u - cx) * F32(z) / F32(fx); y = (v - cy) * F32(z) / F32(fx)
    return x, y, np.full_like(x, F32(z)), (F32(fx), F32(fx), cx, cy)


def clamp_input():
    """vertices so far out that vcurr x n exceeds 512 for the pixels more than 12 columns from the centre: the clamp engages there"""
    x, y, z, cam = _self_projecting(64.0, 2560.0)        # x = (u - 40) * 40: up to +-1600
    n = (np.zeros_like(x), np.zeros_like(x), np.ones_like(x))
    off = F32(0.03125) * (1 + (np.arange(x.size, dtype=F32).reshape(x.shape) % 3))   # vprev = vcurr + off * n: dist <= 0.10
    vc, nc = _planar(x, y, z), _planar(*n)
    vp = _planar(x, y, z + off)
    return dict(Rcurr=IDENT, tcurr=ZERO3, vc=vc, nc=nc, Rprev_inv=IDENT, tprev=ZERO3, cam=cam, vp=vp, npv=nc.copy(), dist=0.10,
                angle=np.float32(np.sin(20.0 * 3.14159254 / 180.0)))


def ties_input():
    """rows from powers of two whose products land exactly half way between two grid points of 2^-32, with both signs: n = (k * 2^-17,
    -+2^-16, 1) with k odd gives n0 * n1 = -+k * 2^-33 = -+(k / 2) * 2^-32 -- k / 2 ends in .5 --, and n1 * n1 = 2^-32 exactly"""
    x, y, z, cam = _self_projecting(64.0, 2.0)
    idx = np.arange(x.size, dtype=np.int64).reshape(x.shape)
    k = (2 * (idx % 8) + 1).astype(F32)                        # 1, 3, ..., 15
    n0 = k * F32(2.0 ** -17)
    n1 = np.where(idx % 2 == 0, F32(-1), F32(1)) * F32(2.0 ** -16)
    n2 = np.ones_like(x)
    nc = _planar(n0, n1, n2)
    vc = _planar(x, y, z)
    vp = _planar(x, y, z + F32(2.0 ** -5) * np.where(idx % 3 == 0, F32(-1), F32(1)))
    return dict(Rcurr=IDENT, tcurr=ZERO3, vc=vc, nc=nc, Rprev_inv=IDENT, tprev=ZERO3, cam=cam, vp=vp, npv=nc.copy(), dist=0.10,
                angle=np.float32(np.sin(20.0 * 3.14159254 / 180.0)))


def count_ties(rows, found):
    """products of a found row that are exact ties (fraction exactly one half), by sign"""
    neg = pos = 0
    for r in rows[found]:
        q = [Fraction(float(v)) for v in r]
        for i in range(6):
            for j in range(i, 7):
                p = q[i] * q[j] * (1 << FIX)
                if p.denominator == 2:
                    neg += p < 0; pos += p > 0
    return neg, pos


POISON_LANES = (0, 63, 64)


def poison(inp):
    """NaN and +-Inf in vertices and normals of both maps at the wave boundaries (flat index % 128 in 0, 63, 64), a different poison from
    pixel to pixel -> (poisoned input, flat indices)"""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
    n = ROWS * COLS
    where = [i for i in range(n) if i % 128 in POISON_LANES]
    kinds = [("vc", 0, np.nan), ("vc", 2, np.inf), ("nc", 0, np.nan), ("nc", 1, -np.inf), ("vp", 0, np.nan), ("vp", 2, -np.inf),
             ("npv", 0, np.nan), ("npv", 2, np.inf), ("vc", 1, -np.inf), ("vp", 1, np.inf)]
    for j, i in enumerate(where):
        name, plane, val = kinds[j % len(kinds)]
        y, x = divmod(i, COLS)
        out[name][plane * ROWS + y, x] = val
    return out, where


def call_args(inp):
    """positional arguments of orc.icp_step / Context.icp_step up to the thresholds (the camera goes in between: see the callers)"""
    return inp["Rcurr"], inp["tcurr"], inp["vc"], inp["nc"], inp["Rprev_inv"], inp["tprev"]


def scene_input():
    """level 2 of the 320 x 240 synthetic frame pair, a perturbed pose on either side (the inputs of test_icp_step_exact, smaller)"""
    fp = common.frame_pair(320, 240)
    cam = fp["cam"]
    od = orc.Odometry(320, 240, cam.cx, cam.cy, cam.fx, cam.fy)
    pose = common.perturbed_pose(3)
    od.init_first_rgb(fp["rgba0"]); od.init_icp_model(fp["v4"], fp["n4"], pose); od.init_rgb_model(fp["img"])
    od.init_icp(orc.depth_pyramid(fp["d1"]), 20.0); od.init_rgb(fp["rgba1"])
    vc, nc, vp, npv = (od.buffer(k, 2) for k in range(4))
    assert vc.shape == (3 * ROWS, COLS)
    T2 = common.perturbed_pose(7, 0.004, 0.3) @ pose
    Rprev_inv = np.linalg.inv(pose[:3, :3].astype(np.float64)).astype(np.float32)
    return dict(Rcurr=T2[:3, :3].copy(), tcurr=T2[:3, 3].copy(), vc=vc, nc=nc, Rprev_inv=Rprev_inv, tprev=pose[:3, 3].copy(),
                cam=(np.float32(cam.fx / 4), np.float32(cam.fy / 4), np.float32(cam.cx / 4), np.float32(cam.cy / 4)), vp=vp, npv=npv, dist=0.10,
                angle=np.float32(np.sin(20.0 * 3.14159254 / 180.0)))


INPUTS = {"scene": scene_input, "clamp": clamp_input, "ties": ties_input}


def reference(inp):
    rows, found = rows_f32(inp["Rcurr"], inp["tcurr"], inp["vc"], inp["nc"], inp["Rprev_inv"], inp["tprev"], inp["cam"], inp["vp"],
                               inp["npv"], inp["dist"], inp["angle"])
    sums = exact_sums(rows, found)
    assert fits_int64(sums), "the true sums leave int64: the wrap engaged"
    return rows, found, sums


def check_preconditions(name, rows, found):
    """every input does what it is named after"""
    assert found.sum() >= 1000, f"{name}: {found.sum()} inliers"
    big = (np.abs(rows[found][:, 3:6]) > 512).any(axis=1)
    if name == "clamp":
        assert big.sum() >= 500 and (~big).sum() >= 500, "the clamp engages for a band of pixels, not for all"
    else:
        assert not big.any()
    if name == "ties":
        neg, pos = count_ties(rows, found)
        assert neg >= 1000 and pos >= 1000, (neg, pos)
