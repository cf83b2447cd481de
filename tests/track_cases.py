"""The case table of the batched, culled Gauss-Newton launch (plain helper module, no tests in here).

Every case is a small, seeded description of two or three tracking STEPS on consecutive frames of the synthetic scene.  Step s
tracks frame s + 1 against the ideal prediction of frame s, cut down to one rectangle per tracker ("mask"), from the pose the
prediction was prepared with.  The GPU side (tests/test_track_batch_gpu.py) re-prepares the SAME tracker object step after step,
so from step 1 on the launcher sizes the tracker's workgroups from the screen box of the step before (the "hint") and the ICP
reduction runs on the culled-slot mapping; the CPU side (tests/test_cpu_track_cases.py and `oracle_step` below) uses a fresh
oracle tracker per step, which knows nothing of batches, slots, boxes or hints.

Each case aims at ONE branch of the mapping (`aims`), so that a mapping error fails with the case's name.  This table is the
contract a re-mapping of the ICP launch must keep.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import common
import orc
from co_fusion_amd import synth

TIMES = (0, 3, 6, 9)          # frames of the scene a case steps through (common.frame_pair uses 0 and 3)
EMPTY = "empty"               # a mask: the prediction is empty at this step
FULL = None                   # a mask: the whole prediction
CUTOFF = 20.0
SLIVER_V_WIDTH, SLIVER_H_HEIGHT = 5, 8   # the narrowest slivers the oracle still tracks (see CASES)


@dataclasses.dataclass(frozen=True)
class Tracker:
    masks: tuple               # per step: (x0, x1, y0, y1) half open | FULL | EMPTY
    seed: int                  # common.perturbed_pose(seed): model pose = start pose
    cull: bool = True          # cf_odom_set_culling
    neg_zero: bool = False     # translation x is +0.0 in the model pose and -0.0 in the start pose


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    aims: str
    size: tuple                # (W, H); intrinsics are synth.Camera.scaled(W, H)
    trackers: tuple
    steps: int = 2
    opts: tuple = ()           # keyword options of the tracking call, as sorted items
    err: bool = False          # request the ICP error surface of every tracker
    occluder: tuple = ()       # (y0, y1, depth): rows of every CURRENT frame replaced by a near band (depth_split)
    batched: bool = False      # one Context.track_batch call per step instead of Odometry.track per tracker


def _r(x0, x1, y0, y1):
    return (x0, x1, y0, y1)


# sixteen pairwise different object-sized trackers at 256 x 192 (every level a multiple of 64 wide: the rectangle-of-runs form) and one
# full-image tracker that is not culled, the shape of a frame with a background and several object models
_B = (256, 192)
_BG = Tracker((FULL, FULL, FULL), seed=40, cull=False)
_OBJ = tuple(Tracker((_r(x, x + w, y, y + h),) * 3, seed=41 + i)
             for i, (x, y, w, h) in enumerate([(10, 8, 110, 85), (136, 6, 110, 88), (30, 100, 100, 88), (128, 98, 118, 86),
                                               (90, 60, 60, 50), (0, 0, 50, 40), (200, 140, 56, 52), (60, 10, 50, 90),
                                               (10, 60, 100, 40), (180, 50, 70, 100), (100, 120, 90, 60), (40, 40, 64, 64),
                                               (120, 0, 64, 48), (0, 120, 60, 72), (190, 0, 66, 60)]))
_MIXED5 = (_BG,) + _OBJ[:4]


def _opts(**kw):
    return tuple(sorted(kw.items()))


CASES = [
    Case("interior_320", "a rectangle in the image interior with a live hint: the baseline of the culled-slot branch",
         (320, 240), (Tracker((_r(120, 200, 60, 150),) * 2, seed=2),), err=True),
    Case("narrow_208x156", "levels 208 / 104 / 52 wide: no level is a multiple of 64 (nrx == 0, runs straddle rows); level 2 has 2028 pixels, the last run is partial",
         (208, 156), (Tracker((_r(70, 150, 40, 110),) * 2, seed=3),), err=True),
    Case("odd_336x252", "levels 336x252, 168x126, 84x63: N % 64 != 0 at levels 1 and 2, the last run is partial",
         (336, 252), (Tracker((_r(200, 336, 150, 252),) * 2, seed=4),)),
    Case("corner_tl", "mask touching (0, 0): the box clamps at -1", (320, 240), (Tracker((_r(0, 90, 0, 70),) * 2, seed=5),)),
    Case("corner_br", "mask touching (W-1, H-1): the box clamps past cols - 1 / rows - 1, and the final run of the image",
         (208, 156), (Tracker((_r(120, 208, 90, 156),) * 2, seed=6),)),
    # slivers: meant to be 2 pixels wide / high, widened until the oracle finds >= 100 ICP inliers and an RGB correspondence at both steps
    # (tests/test_cpu_track_cases.py).  Oracle inliers per step by width -- vertical: 2 -> 19 / 0, 3 -> 58 / 0, 4 -> 110 / 103,
    # 5 -> 146 / 150; horizontal: 2 ... 6 -> 0 / 0, 8 -> 155 / 138
    Case("sliver_v", f"a mask {SLIVER_V_WIDTH} pixels wide over the full height", (320, 240),
         (Tracker((_r(156, 156 + SLIVER_V_WIDTH, 0, 240),) * 2, seed=7),)),
    Case("sliver_h", f"a mask {SLIVER_H_HEIGHT} pixels high over the full width, crossing every 64-pixel run boundary of its rows",
         (320, 240), (Tracker((_r(0, 320, 116, 116 + SLIVER_H_HEIGHT),) * 2, seed=8),)),
    Case("whole_image", "culling on with the full prediction: box_blocks capped at the full grid", (320, 240),
         (Tracker((FULL, FULL), seed=9),)),
    Case("grown", "step 1's mask has >= 6x the area of step 0's: the launch is sized from the small hint, the waves walk on (r += stride)",
         (320, 240), (Tracker((_r(140, 184, 100, 140), _r(40, 290, 20, 220)), seed=10),)),
    Case("moved", "step 1's mask is disjoint from step 0's: the hint points at the wrong place, the kernel reads the live box",
         (320, 240), (Tracker((_r(20, 100, 20, 90), _r(200, 300, 140, 230)), seed=11),)),
    # (the SO(3) pre-alignment works on the images alone and turns the pose whatever the prediction holds -- in the oracle as in the library --,
    # so "pose unchanged" is asserted without it; vanished_so3 keeps it on: translation unchanged, rotation the oracle's)
    Case("vanished", "step 1's prediction is empty after a non-empty step 0: exact zeros, pose unchanged, empty box",
         (320, 240), (Tracker((_r(120, 200, 60, 150), EMPTY), seed=12),), opts=_opts(so3=False)),
    Case("vanished_so3", "the same with the SO(3) pre-alignment on: exact zeros, translation unchanged, empty box",
         (320, 240), (Tracker((_r(120, 200, 60, 150), EMPTY), seed=12),)),
    Case("depth_split", "a near occluder band across the object's box in the current frame: runs inside the box fail the depth-interval test",
         (320, 240), (Tracker((_r(100, 230, 50, 170),) * 2, seed=13),), occluder=(90, 120, 0.5)),
    Case("neg_zero_pose", "the start pose has -0.0f where the model pose has +0.0f: the same pose, culled all the same",
         (320, 240), (Tracker((_r(120, 200, 60, 150),) * 2, seed=14, neg_zero=True),)),
    # ---- batched
    Case("batch_mixed_5", "one unculled full-image tracker + four culled object-sized ones in one grid, hints live", _B, _MIXED5,
         err=True, batched=True),
    Case("batch_orders", "the same five trackers in three orders: a tracker's result does not depend on its position in the batch", _B, _MIXED5,
         batched=True),
    Case("batch_9", "nine trackers: slots_used > 12, the second half of the slot table is decoded", _B, (_BG,) + _OBJ[:8], batched=True),
    Case("batch_16", "kMaxBatch trackers in one call", _B, (_BG,) + _OBJ[:15], batched=True),
    Case("batch_17_rejected", "n = 17 is refused on the host (CF_EINVAL) with nothing enqueued; the valid call behind it is unaffected", _B,
         (_BG,) + _OBJ[:15], batched=True),
    Case("batch_partial_fetch", "only some trackers of a batch are fetched before the next call (the result_pending drain)", _B, _MIXED5,
         steps=3, batched=True),
    Case("batch_opts_so3_off", "so3=False on batch_mixed_5", _B, _MIXED5, opts=_opts(so3=False), batched=True),
    Case("batch_opts_no_pyramid", "pyramid=False on batch_mixed_5 (level 0 only)", _B, _MIXED5, opts=_opts(pyramid=False), batched=True),
    Case("batch_opts_fast_odom", "fast_odom=True on batch_mixed_5", _B, _MIXED5, opts=_opts(fast_odom=True), batched=True),
    Case("batch_opts_icp_only", "icp_weight=100 on batch_mixed_5 (no RGB slots)", _B, _MIXED5, opts=_opts(icp_weight=100.0), batched=True),
    Case("batch_opts_rgb_only", "rgb_only=True on batch_mixed_5 (no ICP slots)", _B, _MIXED5, opts=_opts(rgb_only=True), batched=True),
]
BY_NAME = {c.name: c for c in CASES}
SINGLE = [c.name for c in CASES if not c.batched]
BATCH_ORDERS = {"culled_first": (1, 2, 3, 4, 0), "culled_last": (0, 1, 2, 3, 4), "interleaved": (1, 0, 2, 3, 4)}
PARTIAL_FETCH = (0, 2)        # the trackers batch_partial_fetch fetches at step 1


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=32)
def _frame(size, t, occluder=()):
    cam = synth.Camera.scaled(*size)
    d, rgb, _, _ = _scene().render(cam, t, noise=True)
    if occluder:
        y0, y1, z = occluder
        d = d.copy(); d[y0:y1, :] = np.float32(z)
    return d, rgb, synth.rgb_to_rgba(rgb)


@functools.lru_cache(maxsize=1)
def _scene():
    return synth.Scene(n_obj=0, seed=1234)


@functools.lru_cache(maxsize=32)
def _prediction(size, t):
    d, rgb, _ = _frame(size, t)
    return synth.ideal_prediction(synth.Camera.scaled(*size), d, rgb)


def camera(case):
    return synth.Camera.scaled(*case.size)


def keep_mask(case, k, s):
    """the pixels of step s's prediction tracker k keeps"""
    W, H = case.size
    m = case.trackers[k].masks[s]
    keep = np.zeros((H, W), bool)
    if m is FULL:
        keep[:] = True
    elif m != EMPTY:
        x0, x1, y0, y1 = m
        keep[y0:y1, x0:x1] = True
    return keep


def frame_inputs(case, s):
    """what every tracker of step s shares: the previous frame's image, the current frame's depth and image"""
    _, _, rgba_prev = _frame(case.size, TIMES[s])
    d_cur, _, rgba_cur = _frame(case.size, TIMES[s + 1], case.occluder)
    return dict(rgba_prev=rgba_prev, d_cur=d_cur, rgba_cur=rgba_cur)


def tracker_inputs(case, k, s):
    """tracker k at step s: the cut-down prediction, the pose it is prepared with and the pose the tracking call starts from"""
    tr = case.trackers[k]
    v4, n4, img = _prediction(case.size, TIMES[s])
    keep = keep_mask(case, k, s)
    v4 = v4.copy(); n4 = n4.copy()
    v4[~keep] = 0; n4[~keep] = 0
    pose = common.perturbed_pose(tr.seed)
    start = pose.copy()
    if tr.neg_zero:
        pose[0, 3] = np.float32(0.0)
        start[0, 3] = np.float32(-0.0)
    valid = keep & (v4[..., 2] > 0)
    ys, xs = np.nonzero(valid)
    rect = (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())) if len(xs) else None   # inclusive, of the valid vertices
    return dict(v4=v4, n4=n4, img=img, pose=pose, start=start, rect=rect, n_valid=int(valid.sum()), valid=valid)


def projected_rect(case, k, s, trans, rot):
    """the rectangle of tracker k's valid predicted vertices seen from the camera at (trans, rot), f64, inclusive pixel bounds rounded
    outwards: the screen box of a tracking call lives in the CURRENT camera, which has moved away from the prediction's by the end"""
    ti = tracker_inputs(case, k, s)
    cam = camera(case)
    v = ti["v4"][ti["valid"]][:, :3].astype(np.float64)
    P = ti["pose"].astype(np.float64)
    g = v @ P[:3, :3].T + P[:3, 3]
    c = (g - np.asarray(trans, np.float64)) @ np.asarray(rot, np.float64)      # R^T (g - t)
    u = c[:, 0] * cam.fx / c[:, 2] + cam.cx
    w = c[:, 1] * cam.fy / c[:, 2] + cam.cy
    return int(np.ceil(u.min())), int(np.ceil(w.min())), int(np.floor(u.max())), int(np.floor(w.max()))


def track_opts(case):
    return dict(case.opts)


def uses_icp(case):
    o = track_opts(case)
    return not o.get("rgb_only", False) and o.get("icp_weight", 10.0) > 0


def uses_rgb(case):
    o = track_opts(case)
    return bool(o.get("rgb_only", False)) or o.get("icp_weight", 10.0) < 100


# ------------------------------------------------------------------------------------------------ the oracle
_oracle_cache = {}


def oracle_step(case, k, s):
    """the CPU oracle's plain Odometry.track for tracker k at step s (a fresh tracker), cached by content: cases that share trackers
    (batch_mixed_5, batch_orders, batch_9, ...) share the results"""
    tr = case.trackers[k]
    key = (case.size, s, case.occluder, tr.masks[s], tr.seed, tr.neg_zero, case.opts, case.err)
    if key in _oracle_cache:
        return _oracle_cache[key]
    W, H = case.size
    cam = camera(case)
    fi, ti = frame_inputs(case, s), tracker_inputs(case, k, s)
    od = orc.Odometry(W, H, cam.cx, cam.cy, cam.fx, cam.fy)
    od.init_first_rgb(fi["rgba_prev"])
    od.init_icp_model(ti["v4"], ti["n4"], ti["pose"])
    od.init_rgb_model(ti["img"])
    od.init_icp(orc.depth_pyramid(fi["d_cur"]), CUTOFF)
    od.init_rgb(fi["rgba_cur"])
    err = np.zeros((H, W), np.float32) if case.err else None
    t, r, st = od.track(ti["start"][:3, 3], ti["start"][:3, :3], err_surface=err, **track_opts(case))
    out = dict(trans=np.asarray(t, np.float32).copy(), rot=np.asarray(r, np.float32).copy(), icp_count=float(st.last_icp_count),
               rgb_count=float(st.last_rgb_count), icp_error=float(st.last_icp_error), so3_iterations=int(st.so3_iterations),
               so3_error=np.float32(st.last_so3_error), so3_count=np.float32(st.last_so3_count),
               lastA=np.array(st.lastA, np.float64), lastb=np.array(st.lastb, np.float64), err=err)
    _oracle_cache[key] = out
    return out


# ------------------------------------------------------------------------------------------------ the documented run table
def cull_runs_total(box, L, cols, rows):
    """CullRuns::total of csrc/cf_kernels.h, from its documented formula: the 64-pixel runs of level L inside a level-0 screen box --
    the rectangle in units of runs where the level's width is a multiple of 64, the flat runs that hold the box's rows otherwise"""
    bx0, by0, bx1, by1 = (box[0] >> L) - 1, (box[1] >> L) - 1, (box[2] >> L) + 1, (box[3] >> L) + 1
    bx0, by0, bx1, by1 = max(bx0, 0), max(by0, 0), min(bx1, cols - 1), min(by1, rows - 1)
    if bx0 > bx1 or by0 > by1:
        return 0
    if cols % 64 == 0:
        return ((bx1 >> 6) - (bx0 >> 6) + 1) * (by1 - by0 + 1)
    return (((by1 + 1) * cols - 1) >> 6) - ((by0 * cols) >> 6) + 1
