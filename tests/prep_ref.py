"""Plain numpy references of what the fused frame preparation leaves for the culling and the RGB residual pass.

zrange, occupancy and bounding_keys are written from the statement of the operation (include/cofusion_hip.h: cf_odom_buffer 14..16);
candidates is written from the oracle's residual pass (oracle/orc_track.c: orc_rgb_residual), not from the HIP body.  Test
infrastructure only.
"""
from __future__ import annotations

import numpy as np

RUN = 64          # pixels per depth run (flat index / 64)
MIN_GRAD = (5.0, 3.0, 1.0)
SOBEL_SCALE = 0.125


def min_scale(level):
    """the gradient gate of a level as the tracking call computes it: float32(minGrad^2 / sobelScale^2)"""
    return np.float32(MIN_GRAD[level] ** 2 / SOBEL_SCALE ** 2)


def zrange(depth_level, cutoff):
    """(min, max) of the valid depths (z != 0 and z < cutoff; NaN is invalid) of every run of 64 consecutive pixels, f32 [runs, 2];
    (+inf, -inf) for a run without one; the last run ends at N"""
    z = np.ascontiguousarray(depth_level, np.float32).reshape(-1)
    n = z.size
    out = np.empty(((n + RUN - 1) // RUN, 2), np.float32)
    with np.errstate(invalid="ignore"):
        ok = (z != 0) & (z < np.float32(cutoff))   # NaN < cutoff is False
    for r in range(out.shape[0]):
        v = z[r * RUN:min((r + 1) * RUN, n)][ok[r * RUN:min((r + 1) * RUN, n)]]
        out[r] = (v.min(), v.max()) if v.size else (np.inf, -np.inf)
    return out


def occupancy(v4):
    """u8 [H/4, W/4]: 1 where any z of the 4x4 block is not == 0 (a NaN z counts as occupied: the conservative direction)"""
    z = np.asarray(v4, np.float32)[..., 2]
    h, w = z.shape
    with np.errstate(invalid="ignore"):
        occupied = ~(z == 0)
    return occupied.reshape(h // 4, 4, w // 4, 4).any(axis=(1, 3)).astype(np.uint8)


def float_key(f):
    """order-preserving u32 key of a float32: of its bits u, u ^ (0xffffffff if u >> 31 else 0x80000000)"""
    u = int(np.float32(f).view(np.uint32))
    return u ^ (0xFFFFFFFF if u >> 31 else 0x80000000)


def key_float(key):
    """the inverse of float_key"""
    key = int(key) & 0xFFFFFFFF
    u = key ^ 0x80000000 if key >> 31 else key ^ 0xFFFFFFFF
    return float(np.uint32(u).view(np.float32))


def bounding_keys(v4):
    """six u32 keys of the pixel rectangle and the depth interval of the vertices with z != 0, x not NaN and z not NaN:
    ~key(xmin), ~key(ymin), ~key(zmin), key(xmax), key(ymax), key(zmax); all zero when there is no such vertex"""
    v4 = np.asarray(v4, np.float32)
    x, z = v4[..., 0], v4[..., 2]
    with np.errstate(invalid="ignore"):
        ok = (z != 0) & ~np.isnan(x) & ~np.isnan(z)
    if not ok.any():
        return np.zeros(6, np.uint32)
    ys, xs = np.nonzero(ok)
    zs = z[ok]
    lo = (xs.min(), ys.min(), zs.min())
    hi = (xs.max(), ys.max(), zs.max())
    return np.array([~float_key(v) & 0xFFFFFFFF for v in lo] + [float_key(v) for v in hi], np.uint32)


def describe_keys(keys):
    """the six keys as floats (x0, y0, z0, x1, y1, z1), or 'empty': for the message of a failed comparison"""
    keys = [int(k) for k in keys]
    if not any(keys):
        return "empty"
    return tuple(key_float(~k & 0xFFFFFFFF) for k in keys[:3]) + tuple(key_float(k) for k in keys[3:])


def candidate_terms(next_image, next_depth, dIdx, dIdy, min_scale):
    """the four conditions of a candidate pixel of the RGB residual pass, one bool array [rows, cols] each (orc_rgb_residual up to the
    NaN test of the depth):
      margin    x < cols - 5 and y < rows - 1
      window    every intensity of the clamped window [y-2, y+2) x [x-2, x+2) is > 0
      gradient  dIdx^2 + dIdy^2, in integer arithmetic cast to float32, >= min_scale
      depth     next_depth is not NaN"""
    img = np.asarray(next_image, np.uint8)
    rows, cols = img.shape
    yy, xx = np.mgrid[0:rows, 0:cols]
    margin = (xx < cols - 5) & (yy < rows - 1)
    pad = np.full((rows + 3, cols + 3), 255, np.uint8)   # 255 outside the image: the clamped part of a window does not decide
    pad[2:2 + rows, 2:2 + cols] = img
    wmin = np.full((rows, cols), 255, np.uint8)
    for dy in range(4):          # rows y-2 .. y+1
        for dx in range(4):      # cols x-2 .. x+1
            wmin = np.minimum(wmin, pad[dy:dy + rows, dx:dx + cols])
    gx = np.asarray(dIdx, np.int16).astype(np.int32)
    gy = np.asarray(dIdy, np.int16).astype(np.int32)
    gradient = (gx * gx + gy * gy).astype(np.float32) >= np.float32(min_scale)
    depth = ~np.isnan(np.asarray(next_depth, np.float32))
    return margin, wmin > 0, gradient, depth


def candidates(next_image, next_depth, dIdx, dIdy, min_scale):
    """u8 [rows, cols]: 1 where all four conditions of candidate_terms hold"""
    margin, window, gradient, depth = candidate_terms(next_image, next_depth, dIdx, dIdy, min_scale)
    return (margin & window & gradient & depth).astype(np.uint8)
