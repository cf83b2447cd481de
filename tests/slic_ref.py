"""SLIC as the oracle states it (oracle/orc_segment.c:12-30), restated in vectorised f32 numpy with a trace per assignment pass (plain
helper module, no tests in here).

Written from the statement, not from a kernel: centre k of grid cell (cx, cy) starts at pixel (16 cx + 8, 16 cy + 8) with that pixel's
colour; six assignment passes, an update of the centres before passes 2 to 6; a pixel looks at the centres of its own cell and the 3x3
cells around it, dy outer, dx inner, and takes the FIRST minimum (strict `<` against a start value of 999999.9999f) of

    d = sqrtf(dcolor * mc + (0.6f * dxy) * mx),   mc = (5.0f / (1.7321f * 255))^2,  mx = (1.0f / (1.4142f * 16))^2,
    dcolor = (dr dr + dg dg) + db db,  dxy = ex ex + ey ey,

every operation rounded to f32 on its own (no contraction); the cluster sums (x, y, r, g, b, count) are exact integers; a centre is
(float)sum / (float)count, or 0 in all five components for a cluster without a pixel.

numpy rounds every f32 operation on its own, converts int64 to f32 to nearest-even like the C cast, and its f32 sqrt and division are
correctly rounded: tests/test_cpu_slic_cases.py shows that the labels equal orc_slic's on every case of the table.
"""
from __future__ import annotations

import dataclasses

import numpy as np

SPIX = 16
PASSES = 6
F = np.float32
START = F(999999.9999)


@dataclasses.dataclass
class Pass:
    centres: np.ndarray    # f32 [K][5] (x y r g b): the centres this pass used
    sums: np.ndarray       # i64 [K][6] (x y r g b count): the sums this pass produced
    ties: int              # pixels whose minimum was met by a second centre with an equal distance
    empty: int             # clusters without a pixel behind this pass
    largest: int           # pixels of the largest cluster behind this pass


def normalisers():
    mc = F(5.0) / (F(1.7321) * F(255.0))
    mx = F(1.0) / (F(1.4142) * F(SPIX))
    return mc * mc, mx * mx, F(0.6)


def initial_centres(rgba):
    h, w = rgba.shape[:2]
    gx, gy = w // SPIX, h // SPIX
    px = (np.arange(gx) * SPIX + SPIX // 2)[None, :].repeat(gy, 0)
    py = (np.arange(gy) * SPIX + SPIX // 2)[:, None].repeat(gx, 1)
    c = np.empty((gy, gx, 5), F)
    c[..., 0], c[..., 1] = px, py
    c[..., 2:5] = rgba[py, px, :3]
    return c.reshape(gx * gy, 5)


SCAN = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))   # dy outer, dx inner: the scan order that decides ties


def assign(rgba, centres, order=SCAN, last=False):
    """one assignment pass -> (labels i32 [h][w], ties).  `order` and `last` are NOT part of the statement: another scan order, or the
    last minimum instead of the first (a `<=`), for the tests that show that a case's labels depend on them"""
    h, w = rgba.shape[:2]
    gx, gy = w // SPIX, h // SPIX
    mc, mx, weight = normalisers()
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    cx0, cy0 = np.minimum(x // SPIX, gx - 1), np.minimum(y // SPIX, gy - 1)
    xf, yf = x.astype(F), y.astype(F)
    r, g, b = (rgba[..., q].astype(F) for q in range(3))
    dist = np.full((9, h, w), np.inf, F)       # (an absent neighbour never competes)
    lab = np.zeros((9, h, w), np.int32)
    for n, (dy, dx) in enumerate(order):
        cx, cy = cx0 + dx, cy0 + dy
        ok = (cx >= 0) & (cy >= 0) & (cx < gx) & (cy < gy)
        k = np.where(ok, cy * gx + cx, 0)
        c = centres[k]
        dr, dg, db = r - c[..., 2], g - c[..., 3], b - c[..., 4]
        ex, ey = xf - c[..., 0], yf - c[..., 1]
        dcolor = (dr * dr + dg * dg) + db * db
        dxy = ex * ex + ey * ey
        d = np.sqrt(dcolor * mc + (weight * dxy) * mx)
        assert d.dtype == F
        dist[n] = np.where(ok, d, F(np.inf))
        lab[n] = k
    first = 8 - np.argmin(dist[::-1], 0) if last else np.argmin(dist, 0)   # the first minimum in scan order (`last`: the last)
    best = np.take_along_axis(dist, first[None], 0)[0]
    labels = np.take_along_axis(lab, first[None], 0)[0]
    won = best < START                         # (nothing under the start value: the pixel keeps its own cell)
    labels = np.where(won, labels, cy0 * gx + cx0).astype(np.int32)
    ties = int(np.count_nonzero(((dist == best[None]).sum(0) >= 2) & won))
    return labels, ties


def cluster_sums(rgba, labels):
    h, w = labels.shape
    K = (w // SPIX) * (h // SPIX)
    x, y = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
    lab = labels.ravel()
    cols = [x.ravel(), y.ravel()] + [rgba[..., q].astype(np.int64).ravel() for q in range(3)] + [np.ones(lab.size, np.int64)]
    out = np.zeros((K, 6), np.int64)
    for q, v in enumerate(cols):               # (integer accumulation: np.add.at, not the f64 weights of bincount)
        np.add.at(out[:, q], lab, v)
    return out


def update(sums):
    cnt = sums[:, 5]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = sums[:, :5].astype(F) / cnt.astype(F)[:, None]
    return np.where(cnt[:, None] > 0, c, F(0)).astype(F)


def slic(rgba, order=SCAN, last=False):
    """-> (labels i32 [h][w] of the sixth pass, [Pass] * 6)"""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    assert rgba.shape == (h, w, 4) and w % SPIX == 0 and h % SPIX == 0 and w and h
    centres = initial_centres(rgba)
    trace, labels = [], None
    for it in range(PASSES):
        if it:
            centres = update(trace[-1].sums)
        labels, ties = assign(rgba, centres, order, last)
        sums = cluster_sums(rgba, labels)
        trace.append(Pass(centres=centres, sums=sums, ties=ties, empty=int(np.count_nonzero(sums[:, 5] == 0)), largest=int(sums[:, 5].max())))
    return labels, trace
