"""An independent float64 statement of the scene renderer, written from DESIGN.md "Scene rendering" (§4.7) alone: every pixel is tested
against every surfel of every item.  No bounding box, no integer keys, no sorted lookup -- nothing of csrc/render.hip's or
tests/render_ref.py's structure is shared, so an error common to the kernels and their restatement (a box that is not conservative, a
wrong quad, a wrong colour formula) shows as a disagreement with this file.  Plain helper module, no tests in here.

    view, items as tests/render_ref.py takes them; modes: the colour modes wanted (ITEM_MODE = -1 is each item's own)
    render(view, items, modes, exempt=()) -> Result

The f32 kernels and this f64 statement may legitimately differ where a decision sits on a boundary.  `ambiguous` marks those pixels:
  * some surfel's hit lies within a relative RIM_TOL of its rim,
  * the two nearest hits are within a relative DEPTH_TOL in depth, unless they are exact duplicates (identical surfel rows under
    identical matrices: a tie here as well, the lowest draw index wins),
  * a hit's z, or a quad corner's z of the surfel hit, lies within a relative DEPTH_TOL of near or far;
a hit that lies behind the winner by more than DEPTH_TOL cannot change the pixel and marks nothing.  `ambiguous_capped` is the same mask
without the causes that involve a draw index in `exempt` (surfels a case puts on a boundary on purpose).  Separately `half_way(c)` is
true where c * 255 lies within HALF_TOL of k + 0.5: there alone a colour byte may differ by one.
"""
from __future__ import annotations

import dataclasses

import numpy as np

UNSTABLE, WINDOW, PHONG = 1, 2, 4
GREY, NORMALS, COLOUR, TIMES, LABEL, ITEM_MODE = 0, 1, 2, 3, 4, -1
RIM_TOL, DEPTH_TOL, HALF_TOL = 1e-4, 1e-5, 1e-3

PALETTE16 = np.array([
    (230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
    (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195)], float)


@dataclasses.dataclass
class Result:
    covered: np.ndarray            # bool (H, W)
    winner: np.ndarray             # int64 (H, W): draw index (surfels counted through the items in order), -1 where empty
    depth: np.ndarray              # f64 (H, W), 0 where empty
    colours: dict                  # mode -> f64 (H, W, 3) before clamping and rounding, 0 where empty
    label: np.ndarray              # int64 (H, W), 255 where empty
    ambiguous: np.ndarray          # bool (H, W)
    ambiguous_capped: np.ndarray   # bool (H, W): without the causes that involve an exempt draw index
    dim: np.ndarray                # bool (H, W): the winner is dimmed by the time window
    stable: np.ndarray             # bool (H, W): the winner lies above its item's threshold


def half_way(c):
    x = np.clip(c, 0.0, 1.0) * 255.0
    return np.abs(x - np.floor(x) - 0.5) <= HALF_TOL


def to_byte(c):
    return np.floor(np.clip(c, 0.0, 1.0) * 255.0 + 0.5).astype(np.int64)


def model_to_camera(view_pose, item_pose):
    """world -> camera [R^T | -R^T t] and V * Tp in f64, the product rounded once to f32 (as §4.7 states it)"""
    C = np.asarray(view_pose, np.float32).astype(float)
    V = np.eye(4)
    V[:3, :3] = C[:3, :3].T
    V[:3, 3] = -C[:3, :3].T @ C[:3, 3]
    return (V @ np.asarray(item_pose, np.float32).astype(float)).astype(np.float32).astype(float)


def _unit(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def quad_corners(c, n, r):
    """the reference's quad in the surfel's plane: x = unit(n.y - n.z, -n.x, n.x), y = n x x, corners c +- x r sqrt2, c +- y r sqrt2"""
    x = _unit(np.array([n[1] - n[2], -n[0], n[0]])) * (r * np.sqrt(2.0))
    y = np.cross(n, x)
    return np.array([c + x, c + y, c - y, c - x])


def times_ramp(init_time, tick):
    t = np.zeros_like(init_time, float)
    if tick > 1:
        t = (init_time - 1.0) / (tick - 1.0)
    t = np.clip(t, 0.0, 1.0)
    lo = t < 0.5
    return np.stack([np.where(lo, 0.0, 2 * t - 1), np.where(lo, 2 * t, 2 - 2 * t), np.where(lo, 1 - 2 * t, 0.0)], -1)


def render(view, items, modes=(), exempt=()):
    W, H = int(view["width"]), int(view["height"])
    near = float(np.float32(view.get("near", 0.1) or 0.1))
    far = float(np.float32(view.get("far", 1000.0) or 1000.0))
    flags, tick, tdelta = view.get("flags", 0), view.get("tick", 1), view.get("time_delta", 2 ** 30 - 1)
    fx, fy, cx, cy = (float(np.float32(view[k])) for k in ("fx", "fy", "cx", "cy"))
    exempt = set(int(e) for e in exempt)
    py, px = np.mgrid[0:H, 0:W]
    ray = np.stack([(px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, np.ones((H, W))], -1)     # z = 1: the hit's depth is the ray parameter

    inf = np.inf
    z1 = np.full((H, W), inf); z2 = np.full((H, W), inf)          # the two nearest hits
    win = np.full((H, W), -1, np.int64); second = np.full((H, W), -1, np.int64)
    c1 = np.full((H, W), -1, np.int64); c2 = np.full((H, W), -1, np.int64)          # their duplicate classes
    bz = np.full((H, W), inf); bz_cap = np.full((H, W), inf)      # nearest boundary hit (all causes / causes that count for the cap)
    classes = {}
    rows = []                                                     # per draw index: (surfel row f64, item number, camera normal)
    g = -1
    for k, it in enumerate(items):
        S = np.asarray(it["surfels"], np.float32).reshape(-1, 12)
        M = model_to_camera(view["pose"], it["pose"])
        thresh = float(np.float32(it["thresh"]))
        for i in range(len(S)):
            g += 1
            row = S[i].astype(float)
            rows.append((row, k, None))
            if not (row[3] > thresh or flags & UNSTABLE):
                continue
            p, nrm, r = row[0:3], row[8:11], abs(row[11])         # a negative radius draws the disc of |r|
            if not (np.isfinite(p).all() and np.isfinite(nrm).all() and np.isfinite(r)) or not nrm.any():
                continue
            c = M[:3, :3] @ p + M[:3, 3]
            n = _unit(M[:3, :3] @ nrm)
            corner_z = quad_corners(c, n, r)[:, 2]
            if not np.isfinite(corner_z).all() or not (corner_z > near).all():       # a corner at or behind the near plane: skipped
                continue
            rows[-1] = (row, k, n)
            corner_edge = bool((np.abs(corner_z - near) <= DEPTH_TOL * near).any())
            with np.errstate(all="ignore"):
                t = (c @ n) / (ray @ n)
                d = np.sqrt(np.sum((ray * t[..., None] - c) ** 2, -1))
                inz = (t > near) & (t < far)
                hit = (d <= r) & inz
                loose = (d <= r * (1 + RIM_TOL)) & (t > near * (1 - DEPTH_TOL)) & (t < far * (1 + DEPTH_TOL))
                edge = loose & ((np.abs(d - r) <= RIM_TOL * r) | (np.abs(t - near) <= DEPTH_TOL * near) | (np.abs(t - far) <= DEPTH_TOL * far)
                                | corner_edge)
            if edge.any():
                bz = np.where(edge, np.fmin(bz, t), bz)
                if g not in exempt:
                    bz_cap = np.where(edge, np.fmin(bz_cap, t), bz_cap)
            if not hit.any():
                continue
            cls = classes.setdefault((S[i].tobytes(), M.tobytes()), g)
            nearer = hit & (t < z1)
            dup = hit & (t == z1) & (c1 == cls)                   # an exact duplicate of the winner: loses the tie, and is no second hit
            z2 = np.where(nearer, z1, z2); second = np.where(nearer, win, second); c2 = np.where(nearer, c1, c2)
            z1 = np.where(nearer, t, z1); win = np.where(nearer, g, win); c1 = np.where(nearer, cls, c1)
            behind = hit & ~nearer & ~dup & (t < z2)
            z2 = np.where(behind, t, z2); second = np.where(behind, g, second); c2 = np.where(behind, cls, c2)

    covered = win >= 0
    with np.errstate(all="ignore"):
        close = covered & (second >= 0) & ((z2 - z1) <= DEPTH_TOL * z1)
        ambiguous = close | (np.isfinite(bz) & (bz <= np.where(covered, z1 * (1 + DEPTH_TOL), inf)))
        is_ex = np.isin(win, list(exempt)) | np.isin(second, list(exempt)) if exempt else np.zeros((H, W), bool)
        capped = (close & ~is_ex) | (np.isfinite(bz_cap) & (bz_cap <= np.where(covered, z1 * (1 + DEPTH_TOL), inf)))
    depth = np.where(covered, z1, 0.0)

    # colours of the winner
    q = np.nonzero(covered)
    w = win[q]
    n_it = max(len(items), 1)
    R = np.zeros((n_it, 3, 3)); th = np.zeros(n_it); mid = np.zeros(n_it, np.int64); imode = np.zeros(n_it, np.int64)
    for k, it in enumerate(items):
        R[k] = np.asarray(it["pose"], np.float32).astype(float)[:3, :3]
        th[k] = float(np.float32(it["thresh"])); mid[k] = it["model_id"]; imode[k] = it["mode"]
    row = np.array([rows[j][0] for j in w]).reshape(-1, 12)
    ki = np.array([rows[j][1] for j in w], np.int64)
    ncam = np.array([rows[j][2] for j in w], float).reshape(-1, 3)
    nw = _unit(np.einsum("pij,pj->pi", R[ki], row[:, 8:11]))
    s = np.abs(nw.sum(-1))[:, None]
    stable = row[:, 3] > th[ki]
    tcol = times_ramp(row[:, 6], tick) * (s + 0.1)
    bits = row[:, 4].astype(np.int64)
    col = np.stack([(bits >> 16) & 255, (bits >> 8) & 255, bits & 255], -1) / 255.0
    lab = PALETTE16[mid[ki] % 16] / 255.0 * s + 0.1
    grey = np.repeat(0.5 * s + 0.1, 3, -1)
    dim = bool(flags & WINDOW) & ((tick - row[:, 7]) > tdelta)
    if flags & PHONG:
        cp = ray[q] * z1[q][:, None]
        nn = np.where((np.sum(ncam * cp, -1) > 0)[:, None], -ncam, ncam)      # the normal faced towards the light at the camera centre
        L = _unit(-cp)
        nl = np.sum(nn * L, -1)
        refl = 2 * nl[:, None] * nn - L
        shade = (0.3 + np.maximum(nl, 0.0))[:, None]
        spec = (np.maximum(np.sum(refl * L, -1), 0.0) ** 32)[:, None]
    colours = {}
    for m in modes:
        mm = imode[ki] if m < 0 else np.full(len(w), m)
        v = np.select([(mm == GREY)[:, None], (mm == NORMALS)[:, None], (mm == COLOUR)[:, None], (mm == TIMES)[:, None]],
                      [grey, nw, col, tcol], lab)
        v = np.where(stable[:, None], v, tcol)
        if flags & PHONG:
            v = v * shade + spec
        v = np.where(dim[:, None], v * 0.25, v)
        img = np.zeros((H, W, 3)); img[q] = v
        colours[m] = img
    label = np.full((H, W), 255, np.int64); label[q] = mid[ki]
    dim_img = np.zeros((H, W), bool); dim_img[q] = dim
    st_img = np.zeros((H, W), bool); st_img[q] = stable
    return Result(covered, win, depth, colours, label, ambiguous, capped, dim_img, st_img)
