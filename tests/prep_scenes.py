"""Inputs of the frame-preparation parity tests (tests/test_track_prep_gpu.py): common.frame_pair(W, H, noise=True) with defects
injected at fixed and seeded places, so that every edge the fused preparation treats on its own is present at every shape.
tests/test_cpu_prep_ref.py checks, from the references alone, that they are.  Test infrastructure only.
"""
from __future__ import annotations

import functools

import numpy as np

import common
import orc
from co_fusion_amd import synth

# cf_create needs W % 16 == 0 and H % 4 == 0
SHAPES = [(16, 4), (48, 20), (80, 36), (176, 100)]   # every test that needs no tracking call
TRACKED = [(80, 36), (176, 100)]                     # the CPU oracle finds correspondences here (not at 48x20)
CUTOFF = 20.0                                        # depth cutoff of cf_odom_init_icp in these tests
QNAN = np.float32(np.nan)
# the 20x9 level 2 of 80x36 is small enough for the Gauss-Newton loop to run away when a defect lands badly (the divergence guard then
# restores the start pose): this seed keeps the oracle tracking on the full prediction (tests/test_cpu_prep_ref.py asserts it)
SEED_OFFSET = {(80, 36): 6}


def _block(W, H):
    """side of the big square defects: a 13x13 hole at level 0 is what makes one level-2 pixel of the Gaussian pyramids invalid"""
    return 16 if W >= 80 else (8 if W >= 48 else 4)


def _black(rgba, rng, corner, block_at, n_single):
    """black (intensity 0) pixels: a block in one corner (zeros in the border windows of every level), a block in the interior (zeros in
    interior windows of every level), and single pixels"""
    H, W = rgba.shape[:2]
    out = rgba.copy()
    ch, cw = min(7, H - 1), 7
    ys = slice(0, ch) if corner[0] == 0 else slice(H - ch, H)
    xs = slice(0, cw) if corner[1] == 0 else slice(W - cw, W)
    out[ys, xs, :3] = 0
    b = _block(W, H)
    if block_at is not None and W >= 48:
        y0, x0 = block_at
        out[y0:y0 + b, x0:x0 + b, :3] = 0
    for _ in range(n_single):
        out[rng.integers(0, H), rng.integers(0, W), :3] = 0
    return out


def _holes(v4, n4, rng, block_at):
    """defects of a prediction: zeroed 4x4 blocks (one big square of them and seeded single ones), single zeroed pixels inside valid
    blocks, a NaN x with a valid z, a NaN z"""
    H, W = v4.shape[:2]
    v4, n4 = v4.copy(), n4.copy()
    b = _block(W, H)
    y0, x0 = block_at
    v4[y0:y0 + b, x0:x0 + b] = 0; n4[y0:y0 + b, x0:x0 + b] = 0
    nb = (H // 4) * (W // 4)
    for _ in range(nb // 12):
        by, bx = rng.integers(0, H // 4), rng.integers(0, W // 4)
        v4[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = 0; n4[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = 0
    for _ in range(max(2, H * W // 100)):
        y, x = rng.integers(0, H), rng.integers(0, W)
        v4[y, x] = 0; n4[y, x] = 0
    ys, xs = np.nonzero(v4[..., 2] != 0)
    pick = rng.choice(ys.size, size=min(4, ys.size), replace=False)
    for k, i in enumerate(pick):
        v4[ys[i], xs[i], 0 if k % 2 == 0 else 2] = QNAN
    return v4, n4


def _depth_defects(pyr, rng):
    """per level: a whole 64-pixel run invalid (where the level has more than one), and seeded zeros, NaNs, values equal to and above the
    cutoff"""
    kinds = [np.float32(0), QNAN, np.float32(CUTOFF), np.float32(CUTOFF + 0.5)]
    out = []
    for lvl in pyr:
        d = np.array(lvl, np.float32)
        flat = d.reshape(-1)
        n = flat.size
        runs = (n + 63) // 64
        if runs >= 2:
            r = int(rng.integers(0, runs - 1))   # never the last run: the clipped one stays partly valid
            flat[64 * r:64 * r + 64] = [kinds[k % 4] for k in range(64)]
        for k in range(max(1, n // 16)):
            flat[rng.integers(0, n)] = kinds[k % 4]
        out.append(d)
    return out


def _rect(W, H):
    """(x0, x1, y0, y1), exclusive ends: a rectangle whose sides are not aligned to the 16 x 4 tiles of the model-map pass"""
    if (W, H) == (80, 36):
        return 11, 69, 3, 33   # (taller than the rule below gives: the Gauss-Newton loop of the oracle runs away on a 20-row rectangle)
    if H >= 16:
        x0, x1, y0, y1 = W // 8 + 1, 7 * W // 8 - 1, H // 8 + 1, 7 * H // 8 - 1
        return x0, x1 - (x1 % 16 == 0), y0, y1 - (y1 % 4 == 0)
    return W // 4 + 1, 3 * W // 4 - 1, 1, H - 1


@functools.lru_cache(maxsize=None)
def scene(W, H):
    fp = common.frame_pair(W, H, noise=True)
    cam = fp["cam"]
    rng = np.random.default_rng(1000 * W + H + SEED_OFFSET.get((W, H), 0))
    b = _block(W, H)
    s = dict(W=W, H=H, cam=cam, pose=common.perturbed_pose(2))
    # the big hole of the prediction on the left, the black block of the frame image on the right: a pixel rejected by the one is not
    # rejected by the other
    hole_at = (min(8, H - b) // 4 * 4, 8 if W >= 48 else 4)
    black_at = ((H - b) // 2, W - b - 12) if W >= 48 else None
    s["v4"], s["n4"] = _holes(fp["v4"], fp["n4"], rng, hole_at)
    s["img"] = _black(fp["img"], rng, (1, 0), (min(4, H - b), W // 2 - b // 2) if W >= 48 else None, 4)   # prediction image
    s["rgba0"] = _black(fp["rgba0"], rng, (0, 1), None, 4)                                                 # previous frame
    s["rgba1"] = _black(fp["rgba1"], rng, (0, 0), black_at, 4)                                             # current frame
    s["depth_pyr"] = _depth_defects(orc.depth_pyramid(fp["d1"]), rng)
    # every run of every level invalid (zeros, NaNs, at and above the cutoff): the only way a level of a single run has an empty one
    kinds = np.array([0, np.nan, CUTOFF, CUTOFF + 0.5], np.float32)
    s["blank_pyr"] = [kinds[np.arange((H >> l) * (W >> l)) % 4].reshape(H >> l, W >> l) for l in range(3)]
    # the prediction cut down to a rectangle, plus one vertex with a NaN x and one with a NaN z outside of it: occupied blocks that
    # must not extend the box
    x0, x1, y0, y1 = _rect(W, H)
    keep = np.zeros((H, W), bool); keep[y0:y1, x0:x1] = True
    v4r, n4r = s["v4"].copy(), s["n4"].copy()
    v4r[~keep] = 0; n4r[~keep] = 0
    v4r[y0 - 1, x0 - 3] = (QNAN, 0.1, 1.5, 20.0)
    v4r[y1, x1 + 2] = (0.1, 0.1, QNAN, 20.0)
    s["v4_rect"], s["n4_rect"], s["rect"] = v4r, n4r, (x0, x1, y0, y1)
    # the alternative (fill-in) images of the batched initialisers: other content (the second frame's ideal prediction) and other holes
    av4, an4, aimg = synth.ideal_prediction(cam, fp["d1"], fp["rgb1"])
    arng = np.random.default_rng(1000 * W + H + 7)
    s["alt_v4"], s["alt_n4"] = _holes(av4, an4, arng, (0, W - b - 4))
    s["alt_img"] = _black(aimg, arng, (1, 1), None, 6)
    # a second frame image, for trackers of several sequences
    s["rgba2"] = _black(fp["rgba0"][::-1, ::-1].copy(), arng, (1, 1), None, 4)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    for lvl in s["depth_pyr"] + s["blank_pyr"]:
        lvl.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def oracle_prepared(W, H, pred="full"):
    """an orc.Odometry after the five initialisers on the scene (pred: 'full' or 'rect'); shared, do not track with it"""
    return _oracle(W, H, pred)


def _oracle(W, H, pred="full", v4=None, n4=None, img=None, frame=None):
    s = scene(W, H)
    cam = s["cam"]
    od = orc.Odometry(W, H, cam.cx, cam.cy, cam.fx, cam.fy)
    od.init_first_rgb(s["rgba0"])
    sfx = "_rect" if pred == "rect" else ""
    od.init_icp_model(s["v4" + sfx] if v4 is None else v4, s["n4" + sfx] if n4 is None else n4, s["pose"])
    od.init_rgb_model(s["img"] if img is None else img)
    od.init_icp(s["depth_pyr"], CUTOFF)
    od.init_rgb(s["rgba1"] if frame is None else frame)
    return od


@functools.lru_cache(maxsize=None)
def oracle_tracked(W, H, pred="full"):
    """the oracle after its own tracking call with default options from the preparation's pose -> dict of its buffers 4..7 (before the
    call) and 9, 10, 11 (after it) per level, and the tracking result"""
    s = scene(W, H)
    od = _oracle(W, H, pred)
    out = {w: [od.buffer(w, l) for l in range(3)] for w in (4, 5, 6, 7)}   # (a tracking call with the SO3 step swaps nextImage away)
    out["cam"] = s["cam"]
    tr, rot, st = od.track(s["pose"][:3, 3], s["pose"][:3, :3])
    out.update({w: [od.buffer(w, l) for l in range(3)] for w in (9, 10, 11)})
    out["trans"], out["rot"], out["icp_count"], out["rgb_count"] = tr, rot, st.last_icp_count, st.last_rgb_count
    return out


def oracle_with(W, H, v4, n4, img, frame):
    """a fresh prepared oracle tracker on other images than the scene's own (the batched initialisers' cases)"""
    return _oracle(W, H, v4=v4, n4=n4, img=img, frame=frame)
