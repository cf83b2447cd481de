"""GPU parity of the fused frame preparation the tracker object runs (csrc/track_prep.hip, track_prep_dev.h: frame_maps_kernel,
model_maps_tiled_kernel / prep_fused_kernel, rgbd_base_kernel, rgbd_pyrdown_kernel, rgb_prep_body), stage by stage and bit for bit:
against the CPU oracle's chain of single operations, against the plain references of tests/prep_ref.py for what only the culling
reads (zrange, occ, aabb, cand), and -- for the batched initialisers -- against a fresh tracker prepared by the three single calls.

No tolerances: both sides claim the same IEEE operation order; NaN equals NaN.  Buffers 0..3 go through _planar_valid_only because the
reference writes only the x plane of an invalid pixel.  The scenes (tests/prep_scenes.py) carry the defects that send the kernels down
their side branches; tests/test_cpu_prep_ref.py holds them to that.

cf_create admits only widths that are multiples of 16 and heights that are multiples of 4, so the tiled pass is the only one: the untiled
fallback kernel and the W % 4 || H % 4 branches of the initialisers, which no context could reach, are gone.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import pytest

import orc
import prep_ref as pr
import prep_scenes as ps
from test_track_gpu import _planar_valid_only

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts():
    from co_fusion_amd import api
    made = {}

    def get(shape):
        if shape not in made:
            cam = ps.scene(*shape)["cam"]
            made[shape] = api.Context(shape[0], shape[1], cam.fx, cam.fy, cam.cx, cam.cy, max_models=16)
        return made[shape]
    yield get
    for c in made.values():
        c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, what):
    """bit for bit; NaN equals NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} != {want.dtype}{want.shape}"
    same = _bits(got) == _bits(want)
    if got.dtype.kind == "f":
        same |= np.isnan(got) & np.isnan(want)
    if not same.all():
        bad = np.argwhere(~same)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {same.size} differ, first at {i}: {got[i]!r} != {want[i]!r}")


def _same_buffer(which, a, b, what):
    if which <= 3:
        a, b = _planar_valid_only(a), _planar_valid_only(b)
    _same(a, b, what)


def _dev(ctx, a):
    return ctx.to_device(np.array(a))   # (a writable copy: the scenes are read-only)


def _prepare(ctx, s, pred="full", cull=False, pyr="depth_pyr"):
    """the five single calls on the scene"""
    from co_fusion_amd import api
    sfx = "_rect" if pred == "rect" else ""
    g = api.Odometry(ctx)
    g.set_culling(cull)
    g.init_first_rgb(_dev(ctx, s["rgba0"]))
    g.init_icp_model(_dev(ctx, s["v4" + sfx]), _dev(ctx, s["n4" + sfx]), s["pose"])
    g.init_rgb_model(_dev(ctx, s["img"]))
    g.init_icp([_dev(ctx, l) for l in s[pyr]], ps.CUTOFF)
    g.init_rgb(_dev(ctx, s["rgba1"]))
    return g


# ------------------------------------------------------------------------------------- the single-call path
@pytest.mark.parametrize("shape", ps.SHAPES)
def test_single_calls_buffers_0_to_8(contexts, shape):
    ctx, s = contexts(shape), ps.scene(*shape)
    for pred in ("full", "rect"):
        g = _prepare(ctx, s, pred)
        od = ps.oracle_prepared(*shape, pred)
        for which in (1, 2, 3, 4, 5, 6, 7, 8, 0):   # (0 last: reading it drops the depth intervals)
            for lvl in range(3):
                _same_buffer(which, g.buffer(which, lvl), od.buffer(which, lvl), f"{shape} {pred} buffer {which} L{lvl}")
        g.close()


@pytest.mark.parametrize("shape", ps.SHAPES)
def test_zrange(contexts, shape):
    ctx, s = contexts(shape), ps.scene(*shape)
    cam = s["cam"]
    for pyr in ("depth_pyr", "blank_pyr"):
        g = _prepare(ctx, s, pyr=pyr)
        for lvl in range(3):
            got = g.buffer(14, lvl)
            want = pr.zrange(s[pyr][lvl], ps.CUTOFF)
            assert got.shape == want.shape == (((shape[0] >> lvl) * (shape[1] >> lvl) + 63) // 64, 2)
            _same(got, want, f"{shape} {pyr} zrange L{lvl}")
        if pyr == "blank_pyr":
            # a pyramid without one valid depth (the empty run of the levels that are a single run): all runs (+inf, -inf), all maps NaN
            assert all(np.isinf(g.buffer(14, lvl)).all() for lvl in range(3))
            ocam = orc.Cam(cam.fx, cam.fy, cam.cx, cam.cy)
            for lvl in range(3):
                ov = orc.create_vmap(s[pyr][lvl], ocam.level(lvl), ps.CUTOFF)
                _same_buffer(1, g.buffer(1, lvl), orc.create_nmap(ov), f"{shape} blank nmap L{lvl}")
                _same_buffer(0, g.buffer(0, lvl), ov, f"{shape} blank vmap L{lvl}")
        g.close()


@pytest.mark.parametrize("shape", ps.SHAPES)
def test_occupancy_and_bounding_keys(contexts, shape):
    from co_fusion_amd import api
    ctx, s = contexts(shape), ps.scene(*shape)
    zero = np.zeros_like(s["v4"])
    cases = [("full", s["v4"], s["n4"], True), ("rect", s["v4_rect"], s["n4_rect"], True), ("empty", zero, zero, True),
             ("full, culling off", s["v4"], s["n4"], False), ("rect, culling off", s["v4_rect"], s["n4_rect"], False)]
    for name, v4, n4, cull in cases:
        g = api.Odometry(ctx)
        g.set_culling(cull)
        g.init_icp_model(_dev(ctx, v4), _dev(ctx, n4), s["pose"])
        occ, keys = g.buffer(15, 0), g.buffer(16, 0)
        _same(occ, pr.occupancy(v4), f"{shape} {name}: occ")
        want = pr.bounding_keys(v4) if cull else np.zeros(6, np.uint32)
        assert keys.dtype == np.uint32 and keys.shape == (6,)
        assert np.array_equal(keys, want), f"{shape} {name}: box {pr.describe_keys(keys)} != {pr.describe_keys(want)}"
        if name == "empty":
            assert not keys.any() and not occ.any()
        # reading them changed nothing: the same bytes again
        assert np.array_equal(g.buffer(15, 0), occ) and np.array_equal(g.buffer(16, 0), keys)
        with pytest.raises(api.CofusionError):
            g.buffer(15, 1)
        with pytest.raises(api.CofusionError):
            g.buffer(16, 2)
        g.close()


# ------------------------------------------------------------------------------------- the RGB preparation
@pytest.mark.parametrize("shape", ps.TRACKED)
@pytest.mark.parametrize("pred,cull", [("full", False), ("rect", True)])
def test_rgb_preparation_after_one_tracking_call(contexts, shape, pred, cull):
    """dIdx, dIdy, cloud and cand are written by the first launch of the Gauss-Newton loop.  Culling on + the rectangle prediction takes
    the res_range / __syncthreads_or branch of rgb_prep_body, which must leave the same four buffers."""
    ctx, s = contexts(shape), ps.scene(*shape)
    W, H = shape
    o = ps.oracle_tracked(*shape, pred)
    g = _prepare(ctx, s, pred, cull)
    tr, rot, st = g.track(s["pose"][:3, 3], s["pose"][:3, :3])
    box = list(st.cull_box)
    if cull:
        # (the scenes keep the loop converging: a pose that runs away makes the screen box fall back to the whole image)
        assert box != [0, 0, W - 1, H - 1] and box[0] <= box[2], f"the tracker was not culled: {box}"
    else:
        assert box == [0, 0, W - 1, H - 1]
    assert (st.last_icp_count, st.last_rgb_count) == (o["icp_count"], o["rgb_count"]) and o["icp_count"] > 0
    for lvl in range(3):
        for which in (9, 10, 11):
            _same(g.buffer(which, lvl), o[which][lvl], f"{shape} {pred} buffer {which} L{lvl}")
        want = pr.candidates(o[7][lvl], o[5][lvl], o[9][lvl], o[10][lvl], pr.min_scale(lvl))
        got = g.buffer(13, lvl)
        assert want.any() and not want.all()
        _same(got, want, f"{shape} {pred} cand L{lvl}")
    g.close()


# ------------------------------------------------------------------------------------- the batched initialisers
@dataclass(frozen=True)
class T:
    """one tracker of a batch"""
    frame: str = "rgba1"                       # scene key of its frame image: equal keys share one device image
    pred: str = "full"                         # its prediction: 'full' or 'rect'
    cull: bool = False
    counts: Optional[Tuple[int, int]] = None   # device-resident (covered, total); None: a NULL fill_counts entry


RATIO = 0.5
BELOW, EQUAL = (1, 4), (1, 2)                  # 0.25 < 0.5: the alternative images; 0.5 < 0.5 is false: the prediction

BATCHES = {
    "n1": [T()],
    "n3_one_frame": [T(), T(pred="rect", cull=True), T(cull=True)],
    "n3_three_frames": [T("rgba1"), T("rgba2", "rect", True), T("rgba0")],
    "n8_two_frames_interleaved": [T("rgba1" if k % 2 == 0 else "rgba2", "rect" if k % 3 == 0 else "full", k % 2 == 1) for k in range(8)],
    # crosses kPrepBatch = 8: the ninth tracker is a launch of its own and shares its frame image with the first
    "n9_crosses_the_batch": [T("rgba1")] + [T("rgba2", "rect" if k % 2 else "full", k % 2 == 0) for k in range(7)] + [T("rgba1", "rect", True)],
    "choice_below_takes_the_alternative": [T(counts=BELOW), T(pred="rect", cull=True, counts=BELOW)],
    "choice_equal_takes_the_prediction": [T(counts=EQUAL), T(pred="rect", cull=True, counts=EQUAL)],
    "choice_zero_total": [T(counts=(0, 0)), T(counts=(3, 0), cull=True)],
    "choice_null_amid_counts": [T(counts=BELOW, cull=True), T(counts=None), T("rgba2", counts=BELOW), T(counts=EQUAL), T(counts=None, cull=True)],
}
# which trackers of the choice cases end up on the alternative images, written out
TAKES_ALT = {"choice_below_takes_the_alternative": [True, True], "choice_equal_takes_the_prediction": [False, False],
             "choice_zero_total": [False, False], "choice_null_amid_counts": [True, False, True, False, False]}


def _takes_alt(t):
    if t.counts is None:
        return False
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(np.float32(t.counts[0]) / np.float32(t.counts[1]) < np.float32(RATIO))


def _run_batch(ctx, shape, trackers, entry="select"):
    """prepare the trackers with one batched call and compare each with (a) a fresh tracker prepared by the three single calls on the
    images the choice should have selected, (b) the oracle and the references"""
    from co_fusion_amd import api
    s = ps.scene(*shape)
    n = len(trackers)
    frames = {k: _dev(ctx, s[k]) for k in sorted({t.frame for t in trackers})}
    rgba0 = _dev(ctx, s["rgba0"])
    poses = [ps.common.perturbed_pose(2 + k) for k in range(n)]
    ods, pv, pn, pi, av, an, ai, fc = [], [], [], [], [], [], [], []
    for k, t in enumerate(trackers):
        sfx = "_rect" if t.pred == "rect" else ""
        g = api.Odometry(ctx)
        g.set_culling(t.cull)
        g.init_first_rgb(rgba0)
        ods.append(g)
        pv.append(_dev(ctx, s["v4" + sfx])); pn.append(_dev(ctx, s["n4" + sfx])); pi.append(_dev(ctx, s["img"]))
        has = t.counts is not None
        av.append(_dev(ctx, s["alt_v4"]) if has else None); an.append(_dev(ctx, s["alt_n4"]) if has else None)
        ai.append(_dev(ctx, s["alt_img"]) if has else None)
        fc.append(_dev(ctx, np.array(t.counts, np.uint32).view(np.int32)) if has else None)
    fr = [frames[t.frame] for t in trackers]
    if entry == "select":
        choose = any(c is not None for c in fc)
        ctx.init_models_batch_select(ods, pv, pn, pi, poses, fr, av if choose else None, an if choose else None, ai if choose else None,
                                     fc if choose else None, RATIO)
    elif entry == "frames":
        ctx.init_models_batch_frames(ods, pv, pn, pi, poses, fr)
    else:
        ctx.init_models_batch(ods, pv, pn, pi, poses, fr[0])
    for k, t in enumerate(trackers):
        what = f"{shape} tracker {k} of {n} {t}"
        sfx = "_rect" if t.pred == "rect" else ""
        alt = _takes_alt(t)
        v4, n4, img = (s["alt_v4"], s["alt_n4"], s["alt_img"]) if alt else (s["v4" + sfx], s["n4" + sfx], s["img"])
        single = api.Odometry(ctx)
        single.set_culling(t.cull)
        single.init_first_rgb(rgba0)
        single.init_icp_model(_dev(ctx, v4), _dev(ctx, n4), poses[k])
        single.init_rgb_model(_dev(ctx, img))
        single.init_rgb(frames[t.frame])
        od = orc.Odometry(shape[0], shape[1], s["cam"].cx, s["cam"].cy, s["cam"].fx, s["cam"].fy)
        od.init_first_rgb(s["rgba0"]); od.init_icp_model(v4, n4, poses[k]); od.init_rgb_model(img); od.init_rgb(s[t.frame])
        for which in range(2, 9):
            for lvl in range(3):
                got = ods[k].buffer(which, lvl)
                _same_buffer(which, got, single.buffer(which, lvl), f"{what}: buffer {which} L{lvl} vs the single calls")
                _same_buffer(which, got, od.buffer(which, lvl), f"{what}: buffer {which} L{lvl} vs the oracle")
        occ, keys = ods[k].buffer(15, 0), ods[k].buffer(16, 0)
        _same(occ, single.buffer(15, 0), f"{what}: occ vs the single calls")
        _same(occ, pr.occupancy(v4), f"{what}: occ vs the reference")
        want = pr.bounding_keys(v4) if t.cull else np.zeros(6, np.uint32)
        assert np.array_equal(keys, want), f"{what}: box {pr.describe_keys(keys)} != {pr.describe_keys(want)}"
        assert np.array_equal(keys, single.buffer(16, 0)), f"{what}: box vs the single calls"
        single.close()
    return ods


@pytest.mark.parametrize("name", list(BATCHES))
def test_batched_initialisers(contexts, name):
    shape = (48, 20)
    trackers = BATCHES[name]
    if name in TAKES_ALT:
        assert [_takes_alt(t) for t in trackers] == TAKES_ALT[name]
    ods = _run_batch(contexts(shape), shape, trackers)
    if name == "n3_one_frame":
        # one chain fanned out to three pyramids: equal contents, each tracker's own allocation
        for lvl in range(3):
            imgs = [g.buffer(7, lvl) for g in ods]
            assert np.array_equal(imgs[0], imgs[1]) and np.array_equal(imgs[0], imgs[2]) and imgs[0].any()
            assert len({g.buffer_address(7, lvl) for g in ods}) == 3
    for g in ods:
        g.close()


def test_batched_initialisers_mixed_176x100(contexts):
    shape = (176, 100)
    trackers = [T("rgba1", "rect", True, BELOW), T("rgba2", "full", False, EQUAL), T("rgba1", "full", True, None),
                T("rgba2", "rect", True, (0, 0)), T("rgba1", "full", False, BELOW)]
    for g in _run_batch(contexts(shape), shape, trackers):
        g.close()


@pytest.mark.parametrize("entry", ["batch", "frames"])
def test_batched_initialisers_forwarding(contexts, entry):
    """cf_odom_init_models_batch (one frame image) and _frames (one per tracker) forward to _select without a choice"""
    shape = (48, 20)
    second = "rgba1" if entry == "batch" else "rgba2"
    for g in _run_batch(contexts(shape), shape, [T("rgba1", "rect", True), T(second), T("rgba1", cull=True)], entry=entry):
        g.close()
