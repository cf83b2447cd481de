"""The case table of the surfel chain's parity tests (tests/test_surfel_chain_gpu.py): maps, frames and the items of one or more consecutive
cf_models_frame_passes calls, with the CPU oracle's results for them (tests/orc_pipeline.py, in the reference's order: predictIndices,
fuse, predictIndices, clean, combinedPredict).  The maps are mostly crafted so that the branches a rendered scene barely visits are
taken by many surfels; tests/test_cpu_surfel_cases.py asserts from the oracle alone (its traced fuse and clean) that they are.
Test infrastructure only.

cf_create accepts widths that are multiples of 16 and heights that are multiples of 4, so the second shape is 80x44: 80 is a multiple of
neither 32 nor 64, and 80 * 44 = 3520 pixels are a multiple of neither the 256-thread workgroups nor the 2048-element scan blocks.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

import common
import orc
import orc_pipeline as op
from orc import P, f32, u8
from co_fusion_amd import synth

K_SURF_BATCH = 16          # kSurfBatch, csrc/cf_kernels.h
SCAN_ITEMS = 2048          # kScanItems, csrc/surf_scan_dev.h
DEPTH_CUTOFF = 20.0        # maxDepthProcessed: the cutoff of both index passes and of the prediction
FILTER_CUTOFF = 5.0
CONF = 10.0
OUTLIER = 3.0
TIME_DELTA = 2 ** 31 // 2 - 1
SURFEL = 12
A, B = (64, 48), (80, 44)


@dataclass
class Frame:
    rgba: np.ndarray
    depth: np.ndarray
    depth_filt: np.ndarray
    mask: np.ndarray


@dataclass
class Item:
    model: int                      # index into Case.maps
    frame: str                      # key into Case.frames
    pose: np.ndarray
    time: int
    do_fuse: int = 1
    fuse_max_depth: float = DEPTH_CUTOFF
    weighting: float = 1.0
    mask_id: int = 0
    conf: float = CONF


@dataclass
class Case:
    name: str
    shape: Tuple[int, int]
    cam: synth.Camera
    maps: List[np.ndarray]
    frames: Dict[str, Frame]
    calls: List[List[Item]]
    time_delta: int = TIME_DELTA
    outlier: float = OUTLIER
    between: Dict[int, list] = field(default_factory=dict)   # before call k: [("initialise", model, frame, time)]
    max_surfels: int = 1 << 14
    note: dict = field(default_factory=dict)                 # what the builder wants the CPU test to look at (ids, regions)


@dataclass
class Result:
    """the oracle's chain for one item of one call"""
    map: np.ndarray
    index: tuple = None        # (index, vertConf, colorTime, normRad) of the SECOND index pass (what buffers 0..3 hold after the chain)
    fresh: np.ndarray = None   # the new unstable surfels the fuse appended
    splat: tuple = None        # (image, vertexConf, normalRad, time)
    index_first: tuple = None
    pix_trace: np.ndarray = None    # [H, W, 4], orc_fuse_trace
    upd_trace: np.ndarray = None    # [count, 2]
    clean_trace: np.ndarray = None  # [count + fresh, 8], orc_clean_trace
    map_fused: np.ndarray = None    # the map between fuse and clean


def ocam(cam):
    return orc.Cam(cam.fx, cam.fy, cam.cx, cam.cy)


# ------------------------------------------------------------------------------------------------------------------ oracle chain
def _fuse_traced(surf, idx, vc, nr, fr, pose, cam, time, weighting, mask_id, max_depth):
    h, w = fr.depth.shape
    s = f32(surf).reshape(-1, SURFEL)
    out = np.zeros((max(s.shape[0], 1), SURFEL), np.float32)
    new = np.zeros((h * w // 4 + 16, SURFEL), np.float32)
    pix = np.zeros((h, w, 4), np.int32); upd = np.zeros((max(s.shape[0], 1), 2), np.int32)
    n_new = C.c_int()
    orc.lib.orc_fuse_trace(P(s), s.shape[0], P(idx), P(f32(vc)), P(f32(nr)), P(u8(fr.rgba)), P(f32(fr.depth)), P(f32(fr.depth_filt)),
                           P(u8(fr.mask)), P(f32(pose).reshape(16)), cam, w, h, time, C.c_float(weighting), mask_id, C.c_float(max_depth),
                           P(out), P(new), C.byref(n_new), P(pix), P(upd))
    return out[:s.shape[0]].copy(), new[:n_new.value].copy(), pix, upd[:s.shape[0]]


def _clean_traced(surf, new, idx, vc, ct, fr, pose, cam, time, conf, outlier, time_delta, mask_id):
    h, w = fr.depth.shape
    s = f32(surf).reshape(-1, SURFEL); nw = f32(new).reshape(-1, SURFEL)
    out = np.zeros((s.shape[0] + nw.shape[0] + 1, SURFEL), np.float32)
    tr = np.zeros((s.shape[0] + nw.shape[0] + 1, 8), np.int32)
    orc.lib.orc_clean_trace.restype = C.c_int
    n = orc.lib.orc_clean_trace(P(s), s.shape[0], P(nw), nw.shape[0], P(idx), P(f32(vc)), P(f32(ct)), P(f32(fr.depth_filt)), P(u8(fr.mask)),
                                P(f32(pose).reshape(16)), cam, w, h, time, C.c_float(conf), C.c_float(outlier), time_delta, mask_id, P(out),
                                P(tr))
    return out[:n].copy(), tr[:s.shape[0] + nw.shape[0]]


def oracle_item(case: Case, it: Item, surf):
    w, h = case.shape
    cam = ocam(case.cam)
    fr = case.frames[it.frame]
    r = Result(map=surf)
    if it.do_fuse:
        r.index_first = op.predict_indices(surf, it.pose, cam, w, h, DEPTH_CUTOFF, it.time, case.time_delta)
        idx, vc, ct, nr = r.index_first
        r.map_fused, r.fresh, r.pix_trace, r.upd_trace = _fuse_traced(surf, idx, vc, nr, fr, it.pose, cam, it.time, it.weighting, it.mask_id,
                                                                      it.fuse_max_depth)
        r.index = op.predict_indices(r.map_fused, it.pose, cam, w, h, DEPTH_CUTOFF, it.time, case.time_delta)
        idx, vc, ct, nr = r.index
        r.map, r.clean_trace = _clean_traced(r.map_fused, r.fresh, idx, vc, ct, fr, it.pose, cam, it.time, it.conf, case.outlier,
                                             case.time_delta, it.mask_id)
    r.splat = op.combined_predict(r.map, it.pose, cam, w, h, DEPTH_CUTOFF, it.conf, it.time, it.time, case.time_delta)
    return r


def bootstrap(fr: Frame, cam, time):
    """computeFeedbackBuffers + Model::initialise on the oracle: the surfels of a frame in its camera's coordinates"""
    raw, n_raw = op.vertex_feedback(fr.rgba, fr.depth, ocam(cam), time, DEPTH_CUTOFF)
    filt, _ = op.vertex_feedback(fr.rgba, fr.depth_filt, ocam(cam), time, DEPTH_CUTOFF)
    return op.model_initialise(raw, n_raw, filt)


@functools.lru_cache(maxsize=None)
def oracle(name) -> List[Dict[int, Result]]:
    """per call: item position -> Result.  Shared by the CPU and the GPU test; do not modify"""
    case = get(name)
    maps = [m.copy() for m in case.maps]
    out = []
    for k, call in enumerate(case.calls):
        for act in case.between.get(k, []):
            assert act[0] == "initialise"
            maps[act[1]] = bootstrap(case.frames[act[2]], case.cam, act[3])
        res = {}
        for q, it in enumerate(call):
            res[q] = oracle_item(case, it, maps[it.model])
            maps[it.model] = res[q].map
        out.append(res)
    return out


# ------------------------------------------------------------------------------------------------------------------ building blocks
def rendered(shape, t, n_obj, seed=1234):
    cam = synth.Camera.scaled(*shape)
    d, rgb, label, _ = synth.Scene(n_obj=n_obj, seed=seed).render(cam, t, noise=True)
    return cam, Frame(synth.rgb_to_rgba(rgb), d, op.bilateral(d, FILTER_CUTOFF), label.astype(np.uint8))


def confident(surf, every=3, conf=20.0):
    """bootstrap confidences are below 1: lift all but every `every`-th surfel over the threshold (the prediction shows them, clean counts them)"""
    s = surf.copy()
    keep = np.arange(s.shape[0]) % every != 0
    s[keep, 3] += np.float32(conf)
    return s


def to_world(surf, pose):
    """camera-frame surfels -> the model frame of `pose` (T model <- camera)"""
    s = surf.copy()
    R = np.asarray(pose, np.float64)[:3, :3]; t = np.asarray(pose, np.float64)[:3, 3]
    s[:, 0:3] = (surf[:, 0:3].astype(np.float64) @ R.T + t).astype(np.float32)
    s[:, 8:11] = (surf[:, 8:11].astype(np.float64) @ R.T).astype(np.float32)
    return s


def at_pixel(cam, u, v, z):
    """camera-frame point that projects to the continuous image position (u, v) at depth z"""
    return np.array([(u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z], np.float64)


def plane_frame(shape, cam, seed):
    """a hand-made frame: a slanted plane (4 mm per column, 3 mm per row) with a seeded colour image and an all-zero mask"""
    w, h = shape
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    d = np.round((1.5 + 0.004 * (x - w // 2) + 0.003 * (y - h // 2)) * 1000.0).astype(np.float32) * np.float32(0.001)
    rng = np.random.default_rng(seed)
    rgba = rng.integers(1, 255, size=(h, w, 4), dtype=np.uint8); rgba[..., 3] = 255
    return Frame(rgba, d, op.bilateral(d, FILTER_CUTOFF), np.zeros((h, w), np.uint8))


def refilter(fr: Frame):
    fr.depth_filt = op.bilateral(fr.depth, FILTER_CUTOFF)
    return fr


# ------------------------------------------------------------------------------------------------------------------ the cases
def _one_model():
    cam, f0 = rendered(B, 0, 2)
    _, f1 = rendered(B, 3, 2)
    f1.mask[:] = 0
    return Case("one_model", B, cam, [confident(bootstrap(f0, cam, 1))], {"f": f1}, [[Item(0, "f", common.perturbed_pose(1), 2)]])


def _five_models():
    cam, f0 = rendered(A, 0, 4)
    _, f1 = rendered(A, 3, 4)
    maps = []
    for lab in range(5):
        part = Frame(f0.rgba, np.where(f0.mask == lab, f0.depth, np.float32(0)), None, f0.mask)
        maps.append(confident(bootstrap(refilter(part), cam, 1), every=2 + lab))
    maps[2] = np.zeros((0, SURFEL), np.float32)              # an empty map that fuses: it only appends
    poses = [common.perturbed_pose(10 + k, 0.004, 0.4) for k in range(5)]
    call = [Item(0, "f", poses[0], 2, mask_id=0),
            Item(1, "f", poses[1], 3, mask_id=1, weighting=0.7),               # the other parity in the same launch
            Item(2, "f", poses[2], 2, mask_id=2),
            Item(3, "f", poses[3], 3, mask_id=3, do_fuse=0),                   # prediction only
            Item(4, "f", poses[4], 5, mask_id=4, fuse_max_depth=1.3, conf=0.5)]
    return Case("five_models", A, cam, maps, {"f": f1}, [call])


def _many_models(n):
    cam, f0 = rendered(A, 0, 1)
    _, f1 = rendered(A, 3, 1)
    f1.mask = ((np.arange(A[0])[None, :] * n // A[0]) * np.ones((A[1], 1), np.int64)).astype(np.uint8)   # vertical stripes: model k fuses stripe k
    base = confident(bootstrap(f0, cam, 1), every=4)
    stripe = np.floor(cam.fx * base[:, 0] / base[:, 2] + cam.cx).astype(np.int64) * n // A[0]
    maps = [base[stripe == k][7 * k:7 * k + 24 + 5 * k].copy() for k in range(n)]                          # tiny maps of different sizes, each under its own stripe
    call = [Item(k, "f", common.perturbed_pose(20 + k, 0.003, 0.3), 2 + k % 2, mask_id=k, weighting=1.0 - 0.02 * k) for k in range(n)]
    return Case("sixteen_models" if n == 16 else "seventeen_models", A, cam, maps, {"f": f1}, [call])


def _two_frames(reinit):
    cam, f0 = rendered(B, 0, 2)
    _, f1 = rendered(B, 3, 2)
    _, f2 = rendered(B, 6, 2)
    maps = []
    for lab in range(3):
        part = Frame(f0.rgba, np.where(f0.mask == lab, f0.depth, np.float32(0)), None, f0.mask)
        maps.append(confident(bootstrap(refilter(part), cam, 1), every=3))
    p1 = [common.perturbed_pose(30 + k, 0.004, 0.4) for k in range(3)]
    p2 = [common.perturbed_pose(40 + k, 0.006, 0.6) for k in range(3)]
    calls = [[Item(k, "f1", p1[k], 2, mask_id=k) for k in range(3)], [Item(k, "f2", p2[k], 3, mask_id=k) for k in range(3)]]
    between = {1: [("initialise", 1, "f1", 2)]} if reinit else {}
    return Case("two_frames_reinit" if reinit else "two_frames", B, cam, maps, {"f1": f1, "f2": f2}, calls, between=between)


def _plane_base(cam, fr, conf=30.0, time=41):
    """the bootstrap of the plane frame: surfel id = column * rows + row, at its pixel's centre"""
    s = bootstrap(fr, cam, 1)
    assert s.shape[0] == fr.depth.size
    s[:, 3] = conf; s[:, 6] = 1; s[:, 7] = time
    return s


def _crafted(cam, base, h, i, j, du, dv, dz, **attr):
    """a copy of the base surfel of pixel (i, j) moved to the image position (i + du, j + dv) and dz nearer / farther"""
    s = base[i * h + j].copy()
    s[0:3] = at_pixel(cam, i + du, j + dv, float(base[i * h + j][2]) + dz)
    for k, v in attr.items():
        s[{"conf": 3, "init": 6, "time": 7, "radius": 11}[k]] = v
    return s


# ------------------------------------------------------------------------------------------------------------------ clean thresholds
def window_samples(px, py, w, h):
    """the 4x4 half-pixel window of clean() around a surfel at the centre of pixel (px, py): per sample the texels its bilinear fetch
    weighs (clamped to the edge as the fetch clamps) and whether the sample lies outside the image"""
    out = []
    for kx in range(4):
        for ky in range(4):
            a, b = px + 0.5 + 0.5 * (kx - 2), py + 0.5 + 0.5 * (ky - 2)
            fu, fv = a - 0.5, b - 0.5
            x0, y0 = int(np.floor(fu)), int(np.floor(fv))
            wx, wy = fu - x0, fv - y0
            tex = {}
            outside = not (0 <= np.floor(a) < w and 0 <= np.floor(b) < h)
            for xx, wxx in ((x0, 1 - wx), (x0 + 1, wx)):
                for yy, wyy in ((y0, 1 - wy), (y0 + 1, wy)):
                    t = (min(max(xx, 0), w - 1), min(max(yy, 0), h - 1))
                    if wxx * wyy > 0:
                        tex[t] = tex.get(t, 0.0) + wxx * wyy
                        outside |= t != (xx, yy)
            out.append(dict(tex=tex, outside=bool(outside)))
    return out


PATCH_CONF, SEMI_CONF = 11.5, 6.0   # over the threshold of 10; a texel that sinks a sample it weighs by a half, not one it weighs by a quarter


def window_count(px, py, w, h, conf, kind):
    """how many samples qualify for the texel confidences `conf` (missing: PATCH_CONF): kind 'count' wants a sample that is not the surfel's
    own texel alone, kind 'z_count' one that does not touch it at all, both a confidence over the threshold; -> (count, how many of them
    lie outside the image), or None when a sample's confidence is within what the fuse may add (1) below the threshold"""
    n = n_out = 0
    for s in window_samples(px, py, w, h):
        own = s["tex"].get((px, py), 0.0)
        if own >= 1.0 if kind == "count" else own > 0.0:
            continue
        c = sum(v * conf.get(t, PATCH_CONF) for t, v in s["tex"].items())
        if 9.0 <= c <= CONF:
            return None
        if c > CONF:
            n += 1; n_out += int(s["outside"])
    return n, n_out


def design_conf(px, py, w, h, kind, target):
    """the fewest neighbouring texels to make unconfident (0) or half confident so that exactly `target` samples qualify -- at a border with
    at least one qualifying sample outside the image, so that the outcome hangs on what the clamped fetch returns"""
    import itertools
    nb = [(x, y) for x in range(px - 1, px + 2) for y in range(py - 1, py + 2) if (x, y) != (px, py) and 0 <= x < w and 0 <= y < h]
    border = px in (0, w - 1) or py in (0, h - 1)
    for k in range(len(nb) + 1):
        for which in itertools.combinations(nb, k):
            for vals in itertools.product((0.0, SEMI_CONF), repeat=k):
                conf = dict(zip(which, vals))
                got = window_count(px, py, w, h, conf, kind)
                if got is not None and got[0] == target and (got[1] > 0 or not border):
                    return conf, got[1]
    raise AssertionError((px, py, kind, target))


def _threshold_model(cam, fr, T):
    """a second map for clean_branches: surfels whose count / zCount lands exactly on either side of the thresholds (9 and 8, 5 and 4),
    in the interior and on every border.  Each site is a flat 3x3 patch of texels (confidence just over the threshold, or none for the
    texels design_conf picks) with the tested surfel in front of its centre"""
    w, h = A
    base = _plane_base(cam, fr, conf=PATCH_CONF, time=T - 1)
    ids = np.arange(w * h).reshape(w, h)
    extra, sites = [], {}

    def site(group, px, py, kind, target):
        conf, n_out = design_conf(px, py, w, h, kind, target)
        z0 = float(base[ids[px, py], 2])
        for x in range(max(px - 1, 0), min(px + 2, w)):
            for y in range(max(py - 1, 0), min(py + 2, h)):
                s = base[ids[x, y]]
                s[0:3] = at_pixel(cam, x + 0.5, y + 0.5, z0)
                s[3] = conf.get((x, y), PATCH_CONF)
                if kind == "z_count":
                    s[7] = T                                   # counts as updated in this very frame
        s = base[ids[px, py]].copy()
        s[0:3] = at_pixel(cam, px + 0.5, py + 0.5, z0 - (0.004 if kind == "count" else 0.1))
        s[3] = PATCH_CONF; s[7] = T - 1
        if kind == "count":
            s[6] = 5; s[11] = 0.06                              # initialised later than the surface behind it; a radius that covers the window
        sites.setdefault(group, []).append(dict(id=w * h + len(extra), px=px, py=py, kind=kind, target=target, outside=n_out))
        extra.append(s)
    interior = (("count_9", "count", 9), ("count_8", "count", 8), ("z_count_5", "z_count", 5), ("z_count_4", "z_count", 4))
    for r_ in range(10):
        for c_ in range(11):
            g = interior[(0, 2, 3, 1, 2, 3, 0, 2, 3, 1)[(r_ * 11 + c_) % 10]]     # (the zCount sites need a bilinear fetch that returns T exactly: fewer of them survive)
            site(g[0], 4 + 5 * c_, 4 + 4 * r_, g[1], g[2])
    for k in range(14):                                         # removed at 9: one sample less, as when a clamped fetch went wrong, keeps them
        site("left", 0, 3 + 3 * k, "count", 9); site("right", w - 1, 3 + 3 * k, "count", 9)
        site("top", 8 + 4 * k, 0, "count", 9); site("bottom", 8 + 4 * k, h - 1, "count", 9)
    return np.concatenate([base, np.array(extra, np.float32)]), sites


def _clean_branches():
    w, h = A
    cam = synth.Camera.scaled(w, h)
    T, delta = 42, 25
    fr = plane_frame(A, cam, 5)
    fr.mask[30:44, 4:21] = 7                                   # a foreign label
    base = _plane_base(cam, fr, time=T - 1)
    ids = np.arange(w * h).reshape(w, h)                       # [column, row]
    base[ids[40:56, 8:41].reshape(-1), 7] = T                  # region R: texels that count as updated in this very frame
    extra, groups = [], {}

    def add(name, s):
        groups.setdefault(name, []).append(w * h + len(extra)); extra.append(s)
    for k in range(12):
        # old and unconfident (22 frames, below the threshold): half of them hidden behind the surface, half outside the image
        if k < 6:
            add("old_unconfident", _crafted(cam, base, h, 6 + 5 * k, 6, 0.5, 0.5, 0.3, conf=1.0, time=T - 22))
        else:
            add("old_unconfident", _crafted(cam, base, h, 3, 4 * k - 20, -20.0, 0.5, 0.0, conf=1.0, time=T - 22))
        # older than timeDelta: kept whatever else holds
        add("outdated", _crafted(cam, base, h, 5 + 4 * k, 12, 0.5, 0.5, 0.2 if k % 2 else -0.2, conf=1.0, time=T - 30))
        # stacked: 4 mm in front of an older, confident surface, initialised later than it
        add("stacked", _crafted(cam, base, h, 5 + 3 * k, 17 + (k % 3) * 3, 0.5, 0.5, -0.004, init=5, radius=0.05))
        # free-space violation against texels updated in this frame (region R), normal towards the camera
        add("z_count", _crafted(cam, base, h, 42 + 3 * (k % 4), 11 + 9 * (k // 4), 0.5, 0.5, -0.1))
        # 6 cm in front of the measured depth, own label
        add("violation", _crafted(cam, base, h, 24 + 3 * (k % 4), 28 + 4 * (k // 4), 0.5, 0.5, -0.06))
        # 4 cm in front of it under a foreign label
        add("violation_foreign", _crafted(cam, base, h, 6 + 3 * (k % 4), 32 + 4 * (k // 4), 0.5, 0.5, -0.04))
        # behind the camera / outside the image
        s = base[k].copy(); s[0:3] = (0.05 * k - 0.3, 0.1, -1.0 - 0.1 * k); add("behind", s)
        add("outside", _crafted(cam, base, h, 0 if k % 2 else w - 1, 3 + 3 * k, -4.0 if k % 2 else 5.0, 0.5, 0.0))
        # within one pixel of every border (some in front of the surface, some hidden behind it)
        dz = -0.002 if k % 2 else 0.02
        add("left", _crafted(cam, base, h, 0, 2 + 4 * (k % 11), 0.3 + 0.05 * k, 0.5, dz))
        add("right", _crafted(cam, base, h, w - 1, 3 + 4 * (k % 11), 0.2 + 0.06 * k, 0.4, dz))
        add("top", _crafted(cam, base, h, 3 + 5 * k, 0, 0.5, 0.25 + 0.05 * k, dz))
        add("bottom", _crafted(cam, base, h, 4 + 5 * k, h - 1, 0.6, 0.15 + 0.07 * k, dz))
    for (i, j, du, dv) in ((0, 0, 0.4, 0.4), (w - 1, 0, 0.6, 0.3), (0, h - 1, 0.2, 0.7), (w - 1, h - 1, 0.7, 0.8)):
        add("corner", _crafted(cam, base, h, i, j, du, dv, -0.002))
    pose = common.perturbed_pose(3)
    m = to_world(np.concatenate([base, np.array(extra, np.float32)]), pose)
    plain = plane_frame(A, cam, 5)                             # (the second model fuses the whole frame: its own label everywhere)
    m1, sites = _threshold_model(cam, plain, T)
    pose1 = common.perturbed_pose(4)
    call = [Item(0, "f", pose, T), Item(1, "plain", pose1, T)]
    case = Case("clean_branches", A, cam, [m, to_world(m1, pose1)], {"f": fr, "plain": plain}, [call], time_delta=delta,
                note=dict(groups=groups))
    # the f32 loop counters of the window take a fifth step at some image positions, which the design above does not model: keep as
    # threshold sites those where the oracle counts exactly what was designed (the others stay in the map as they are)
    tr = oracle_item(case, call[1], case.maps[1]).clean_trace
    col = {"count": 1, "z_count": 2}
    case.note["sites"] = {g: [s for s in ss if tr[s["id"], col[s["kind"]]] == s["target"] and tr[s["id"], 3 - col[s["kind"]]] == 0]
                          for g, ss in sites.items()}
    return case


def _fuse_branches():
    """two models on one frame.  Model 0 (a perturbed pose): radius-rejecting merges, surfels claimed by two pixels, duplicated surfels (equal
    z in the index pass), and every rejection of the association.  Model 1 (the identity pose, so that the index map holds the crafted
    coordinates exactly): along the column through the principal point two window samples of different outer iterations are at
    bit-equal distance and the earlier one must be kept"""
    w, h = A
    cam = synth.Camera(w, h, 52.8, 52.8, 32.5, 24.5)          # x - cx == 0 exactly for column 32
    T = 42
    fr = plane_frame(A, cam, 6)
    for k, (x, y) in enumerate([(21, 6), (23, 12), (25, 18), (27, 24), (21, 30), (23, 36), (25, 2)]):
        fr.depth[y, x] = 0                                     # odd column, even row: both horizontal neighbours are pixels of this frame's parity
    full = plane_frame(A, cam, 6)                              # the map comes from the frame without the holes
    fr = refilter(fr)
    fr.mask[40:48, 16:31] = 9
    base = _plane_base(cam, full)
    ids = np.arange(w * h).reshape(w, h)
    # ---- model 0
    m0 = base.copy()
    m0[ids[4:16, :].reshape(-1), 11] *= np.float32(0.3)        # radii a third of the measurement's: update.vert rejects the averaging
    for i in range(40, 56, 4):                                 # [hidden | near its left edge | near its right edge | hidden]: pixel i and pixel i + 2 both pick texel i + 1
        for j in range(h):
            m0[ids[i - 1, j], 0:3] = at_pixel(cam, i - 0.5, j + 0.5, float(base[ids[i - 1, j], 2]) + 0.5)
            m0[ids[i, j], 0:3] = at_pixel(cam, i + 0.005, j + 0.5, float(base[ids[i, j], 2]))
            m0[ids[i + 1, j], 0:3] = at_pixel(cam, i + 1.95, j + 0.5, float(base[ids[i + 1, j], 2]))
            m0[ids[i + 2, j], 0:3] = at_pixel(cam, i + 2.5, j + 0.5, float(base[ids[i + 2, j], 2]) + 0.5)
    dup_of = [int(ids[18 + (k % 6) * 2, 4 + (k // 6) * 8 + 2 * (k % 3)]) for k in range(18)]
    dups = m0[dup_of].copy()
    dups[:, 3] = 3.0; dups[:, 4] = 255.0                       # same position, other confidence and colour: the wrong winner changes the merge
    pose0 = common.perturbed_pose(5)
    m0 = to_world(np.concatenate([m0, dups]), pose0)
    assert all(np.array_equal(m0[a, 0:3], m0[w * h + k, 0:3]) for k, a in enumerate(dup_of))
    # ---- model 1
    m1 = base.copy()
    inv_fx = np.float32(1.0 / cam.fx)
    for j in range(h):
        a, b, c = ids[31, j], ids[32, j], ids[33, j]
        assert m1[b, 0] == 0.0
        e = np.float32(m1[b, 2] * inv_fx)                      # one pixel at this depth
        m1[a, 0:3] = (-e, m1[b, 1], m1[b, 2]); m1[c, 0:3] = (e, m1[b, 1], m1[b, 2])
        m1[b, 8:11] = -m1[b, 8:11]                             # alone it fails the normal gate; averaged with its neighbours it passes
        m1[a, 8:11] = (0, 1, 0); m1[c, 8:11] = (0, 1, 0)
    call = [Item(0, "f", pose0, T, fuse_max_depth=1.58), Item(1, "f", np.eye(4, dtype=np.float32), T)]
    return Case("fuse_branches", A, cam, [m0, m1], {"f": fr}, [call], note=dict(dup_of=dup_of, tie_column=32))


def _long_map():
    w, h = A
    cam, f0 = rendered(A, 0, 1)
    _, f1 = rendered(A, 3, 1)
    f1.mask[:] = 0
    T = 40
    n = SCAN_ITEMS * 257 + 5
    base = bootstrap(f0, cam, 1)
    layers = -(-n // base.shape[0])
    rng = np.random.default_rng(77)
    s = np.tile(base, (layers, 1))
    lay = np.repeat(np.arange(layers), base.shape[0]).astype(np.float32)
    s[:, 0:3] *= (np.float32(1) + np.float32(0.0015) * lay)[:, None]          # along the ray: many surfels per pixel
    s = s[rng.permutation(s.shape[0])[:n]]                                     # (the nearest surfel of a pixel is not its lowest id)
    s[:, 3] = np.where(rng.random(n) < 0.3, 2.0, 25.0)
    s[:, 7] = np.where(rng.random(n) < 0.2, T - 30, T - 1)
    return Case("long_map", A, cam, [s], {"f": f1}, [[Item(0, "f", common.perturbed_pose(7, 0.004, 0.4), T)]], max_surfels=n + 4096)


_BUILDERS = {
    "one_model": _one_model, "five_models": _five_models, "sixteen_models": lambda: _many_models(16),
    "seventeen_models": lambda: _many_models(17), "two_frames": lambda: _two_frames(False), "two_frames_reinit": lambda: _two_frames(True),
    "clean_branches": _clean_branches, "fuse_branches": _fuse_branches, "long_map": _long_map,
}
NAMES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def get(name) -> Case:
    c = _BUILDERS[name]()
    for m in c.maps:
        m.setflags(write=False)
    for fr in c.frames.values():
        for a in (fr.rgba, fr.depth, fr.depth_filt, fr.mask):
            a.setflags(write=False)
    return c
