"""GPU parity of the pyramids the batched initialiser builds inside its one launch (csrc/track_prep.hip: prep_fused_kernel ->
rgbd_tile_body, a workgroup per 16 x 8 rectangle of level-2 pixels that evaluates all three levels through LDS) against fresh trackers
prepared by the single calls (rgbd_base_kernel + two rgbd_pyrdown_kernel launches) and against the CPU oracle: every level of
lastDepth, lastImage and nextImage of every tracker, bit for bit, NaN equal to NaN.

The scenes are built here from seeds.  Their invalid pixels (z = 0, z beyond the tracker's 6 m cutoff, zero intensity) sit on every
border of the image and across the level-0 lines where one workgroup's rectangle ends and the next begins (x = 64 k, y = 32 k), so
that a tap taken from the wrong side of a tile, a border decided by the tile instead of the image, or a pixel stored by two or by no
workgroup shows.  The level-2 images are 4x1, 12x5, 20x9 and 44x25: the last tile of a row and of a column lies partly outside the image.
"""
import functools

import numpy as np
import pytest

import common
import orc
import prep_scenes as ps
from co_fusion_amd import synth

pytestmark = pytest.mark.gpu

TILE_W0, TILE_H0 = 64, 32    # level-0 extent of a workgroup's rectangle (kT2W * 4, kT2H * 4)
RGB_CUTOFF = 6.0             # maxDepthRGB of a tracker: the cutoff of the depth chain
RATIO = 0.75
BELOW, ABOVE = (1, 4), (7, 8)   # 0.25 < 0.75: the fill-in images; 0.875: the prediction


def _mask(H, W, rng):
    """pixels to invalidate: about half of each border line (both ends of each always), a band of four across every tile line, singles"""
    m = rng.random((H, W)) < 0.03
    for sl in (np.s_[0, :], np.s_[H - 1, :], np.s_[:, 0], np.s_[:, W - 1]):
        line = rng.random(m[sl].shape) < 0.5
        line[0] = line[-1] = True
        m[sl] |= line
    for x in range(TILE_W0, W, TILE_W0):
        m[:, x - 2:x + 2] |= rng.random((H, 4)) < 0.5
    for y in range(TILE_H0, H, TILE_H0):
        m[y - 2:y + 2, :] |= rng.random((4, W)) < 0.5
    if W > TILE_W0 and H > TILE_H0:
        # a 16 x 16 hole on the corner where four rectangles meet: wide enough to leave invalid pixels at levels 1 and 2 on all four
        m[TILE_H0 - 8:TILE_H0 + 8, TILE_W0 - 8:TILE_W0 + 8] = True
    return m


def _break_vertices(v4, rng):
    v4 = v4.copy()
    m = _mask(v4.shape[0], v4.shape[1], rng)
    far = rng.random(m.shape) < 0.5
    v4[m & far, 2] = np.float32(RGB_CUTOFF + 1.0)
    v4[m & ~far, 2] = 0
    return v4


def _break_image(rgba, rng):
    rgba = rgba.copy()
    rgba[_mask(rgba.shape[0], rgba.shape[1], rng), :3] = 0
    return rgba


@functools.lru_cache(maxsize=None)
def pyramid_scene(W, H):
    fp = common.frame_pair(W, H, noise=True)
    rng = np.random.default_rng(77000 + 1000 * W + H)
    av4, an4, aimg = synth.ideal_prediction(fp["cam"], fp["d1"], fp["rgb1"])
    s = dict(cam=fp["cam"], rgba0=fp["rgba0"], n4=fp["n4"], alt_n4=an4,
             v4=_break_vertices(fp["v4"], rng), img=_break_image(fp["img"], rng),
             alt_v4=_break_vertices(av4, rng), alt_img=_break_image(aimg, rng),
             frame_a=_break_image(fp["rgba1"], rng), frame_b=_break_image(fp["rgba0"][::-1, ::-1].copy(), rng))
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def _oracle(s, W, H, v4, n4, img, frame, pose):
    cam = s["cam"]
    od = orc.Odometry(W, H, cam.cx, cam.cy, cam.fx, cam.fy)
    od.init_first_rgb(s["rgba0"]); od.init_icp_model(v4, n4, pose); od.init_rgb_model(img); od.init_rgb(frame)
    return od


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} != {want.dtype}{want.shape}"
    same = _bits(got) == _bits(want)
    if got.dtype.kind == "f":
        same |= np.isnan(got) & np.isnan(want)
    if not same.all():
        bad = np.argwhere(~same)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {same.size} differ, first at {i}: {got[i]!r} != {want[i]!r}")


def _borders(a):
    a = np.asarray(a)
    return a[0, :], a[-1, :], a[:, 0], a[:, -1]


@pytest.mark.parametrize("shape", ps.SHAPES)
def test_batched_pyramids_match_the_single_calls(shape):
    from co_fusion_amd import api
    W, H = shape
    s = pyramid_scene(W, H)
    ctx = api.Context(W, H, s["cam"].fx, s["cam"].fy, s["cam"].cx, s["cam"].cy, max_models=8)
    dev = lambda a: ctx.to_device(np.array(a))
    try:
        # two trackers share a frame image (one chain fanned out to both), the third has its own; the choice goes both ways
        frames = {"frame_a": dev(s["frame_a"]), "frame_b": dev(s["frame_b"])}
        trackers = [("frame_a", BELOW), ("frame_a", ABOVE), ("frame_b", BELOW)]
        poses = [common.perturbed_pose(2 + k) for k in range(3)]
        rgba0 = dev(s["rgba0"])
        ods = []
        for _ in trackers:
            g = api.Odometry(ctx)
            g.init_first_rgb(rgba0)
            ods.append(g)
        n = len(trackers)
        ctx.init_models_batch_select(ods, [dev(s["v4"]) for _ in range(n)], [dev(s["n4"]) for _ in range(n)], [dev(s["img"]) for _ in range(n)],
                                     poses, [frames[f] for f, _ in trackers], [dev(s["alt_v4"]) for _ in range(n)],
                                     [dev(s["alt_n4"]) for _ in range(n)], [dev(s["alt_img"]) for _ in range(n)],
                                     [dev(np.array(c, np.uint32).view(np.int32)) for _, c in trackers], RATIO)
        for k, (frame, counts) in enumerate(trackers):
            alt = np.float32(counts[0]) / np.float32(counts[1]) < np.float32(RATIO)
            assert alt == (counts == BELOW)
            v4, n4, img = (s["alt_v4"], s["alt_n4"], s["alt_img"]) if alt else (s["v4"], s["n4"], s["img"])
            single = api.Odometry(ctx)
            single.init_first_rgb(rgba0)
            single.init_icp_model(dev(v4), dev(n4), poses[k])
            single.init_rgb_model(dev(img))
            single.init_rgb(frames[frame])
            od = _oracle(s, W, H, v4, n4, img, s[frame], poses[k])
            # the scene does what it is for: invalid pixels in the first and last row and column of level 0 of all three images
            for which, invalid in ((4, np.isnan), (6, lambda a: a == 0), (7, lambda a: a == 0)):
                base = od.buffer(which, 0)
                assert base.shape == (H, W)
                assert all(invalid(line).any() for line in _borders(base)), f"{shape} tracker {k}: buffer {which} has a border without an invalid pixel"
                assert not invalid(base).all()
            for which in (4, 6, 7):
                for lvl in range(3):
                    got = ods[k].buffer(which, lvl)
                    assert got.shape == (H >> lvl, W >> lvl)
                    _same(got, single.buffer(which, lvl), f"{shape} tracker {k}: buffer {which} L{lvl} vs the single calls")
                    _same(got, od.buffer(which, lvl), f"{shape} tracker {k}: buffer {which} L{lvl} vs the oracle")
            single.close()
        # the fanned-out pyramid: equal contents in each tracker's own allocation
        for lvl in range(3):
            assert np.array_equal(ods[0].buffer(7, lvl), ods[1].buffer(7, lvl))
            assert ods[0].buffer_address(7, lvl) != ods[1].buffer_address(7, lvl)
        for g in ods:
            g.close()
    finally:
        ctx.close()
