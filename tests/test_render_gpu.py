"""GPU tests of the scene renderer (csrc/render.hip through cf_render): crafted surfel maps against the numpy restatement
tests/render_ref.py, byte for byte, and the depth-test / footprint rules of DESIGN.md "Scene rendering"."""
import warnings

import numpy as np
import pytest

import render_ref as rr

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

W, H = 320, 240
FX, FY, CX, CY = 277.0, 277.0, 160.0, 120.0
TICK, TDELTA = 30, 10


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _pose(ax, ay, az, t):
    T = np.eye(4); T[:3, :3] = _rot(ax, ay, az); T[:3, 3] = t
    return T.astype(np.float32)


def _surfels(rng, n, big=0, spread=1.0):
    S = np.zeros((n, 12), np.float32)
    S[:, 0] = rng.uniform(-1.6, 1.6, n) * spread
    S[:, 1] = rng.uniform(-1.3, 1.3, n) * spread
    S[:, 2] = rng.uniform(-0.5, 4.0, n)                      # some behind the camera, some straddling the near plane
    S[:, 3] = rng.uniform(0.0, 20.0, n)                      # confidences on both sides of the thresholds
    S[:, 4] = rng.integers(0, 1 << 24, n).astype(np.float32)
    S[:, 6] = rng.integers(1, TICK + 1, n)
    S[:, 7] = rng.integers(1, TICK + 1, n)
    nrm = rng.normal(size=(n, 3)) * 0.5 + np.array([0, 0, -1.0])
    S[:, 8:11] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    S[:, 11] = rng.uniform(0.004, 0.04, n)
    if big:
        S[:big, 11] = rng.uniform(0.15, 0.5, big)            # footprints far above the overflow threshold
    return S


@pytest.fixture(scope="module")
def env():
    from co_fusion_amd import api, model as M, render as R
    ctx = api.Context(W, H, FX, FY, CX, CY)
    rnd = R.Renderer(ctx, 400, 300)
    rng = np.random.default_rng(5)
    maps = [(_surfels(rng, 3000, big=6), np.eye(4, dtype=np.float32), 10.0, 0, R.COLOUR),
            (_surfels(rng, 1200, big=3, spread=0.6), _pose(0.1, -0.2, 0.05, [0.2, -0.1, 0.3]), 0.5, 3, R.LABEL),
            (_surfels(rng, 800, spread=0.5), _pose(-0.3, 0.25, 0.4, [-0.3, 0.2, 0.6]), 1.0, 17, R.LABEL)]
    models = []
    for S, *_ in maps:
        m = M.Model(ctx, 1 << 14)
        m.upload_map(S)
        models.append(m)
    yield dict(ctx=ctx, R=R, rnd=rnd, maps=maps, models=models)
    for m in models:
        m.close()
    rnd.close()
    ctx.close()


def _items(env, maps=None, models=None):
    R = env["R"]
    out = []
    for (S, Tp, thr, mid, mode), m in zip(maps or env["maps"], models or env["models"]):
        ptr, nbytes = m.tensor(11)
        assert nbytes == S.nbytes
        out.append(R.make_item(ptr, len(S), Tp, thr, mid, mode))
    return out


def _ref_items(maps):
    return [dict(surfels=S, pose=Tp, thresh=thr, model_id=mid, mode=mode) for S, Tp, thr, mid, mode in maps]


def _views():
    return [dict(pose=np.eye(4, dtype=np.float32), fx=FX, fy=FY, cx=CX, cy=CY, width=W, height=H),
            dict(pose=_pose(0.15, 0.35, -0.1, [-0.6, 0.1, -0.4]), fx=205.0, fy=199.0, cx=131.5, cy=93.0, width=272, height=184,
                 near=0.3, far=3.5)]


def _gpu_view(R, v, flags):
    return R.make_view(v["pose"], v["fx"], v["fy"], v["cx"], v["cy"], v["width"], v["height"], v.get("near", 0.0), v.get("far", 0.0),
                       flags, TICK, TDELTA)


def _check(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint8) != want.view(np.uint8)
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {bad.size} bytes differ"


@pytest.mark.parametrize("flags", [0, rr.UNSTABLE, rr.WINDOW, rr.PHONG, rr.UNSTABLE | rr.WINDOW | rr.PHONG])
def test_crafted_scenes_match_the_restatement(env, flags):
    R = env["R"]
    modes = (R.ITEM_MODE, R.GREY, R.NORMALS, R.COLOUR, R.TIMES, R.LABEL)
    for vi, v in enumerate(_views()):
        got = env["rnd"].render(_gpu_view(R, v, flags), _items(env), modes, depth=True, labels=True)
        got = [t.cpu().numpy() for t in got]
        want = rr.render(dict(v, flags=flags, tick=TICK, time_delta=TDELTA), _ref_items(env["maps"]),
                         [("rgba", m) for m in modes] + [("depth",), ("labels",)])
        covered = np.count_nonzero(want[-1] != 255)
        assert covered > 0.2 * v["width"] * v["height"], f"view {vi}: the scene covers too little ({covered} pixels)"
        assert len(np.unique(want[-1])) >= 3, "the objects are visible beside the background"
        for k, name in enumerate([f"rgba mode {m}" for m in modes] + ["depth", "labels"]):
            _check(got[k], want[k], f"view {vi} flags {flags} {name}")


def test_empty_call_and_the_key_buffer_is_left_clear(env):
    """no items: every output empty; a following render is unaffected by the keys of the one before (resolve clears them)"""
    R = env["R"]
    v = _views()[0]
    rgba, depth, lab = env["rnd"].render(_gpu_view(R, v, 0), [], (R.COLOUR,), depth=True, labels=True)
    assert not rgba.cpu().numpy().any() and not depth.cpu().numpy().any() and (lab.cpu().numpy() == 255).all()
    items = _items(env)
    a = env["rnd"].render(_gpu_view(R, v, 0), items[1:2], (R.COLOUR,), labels=True)
    want = rr.render(dict(v, tick=TICK, time_delta=TDELTA), _ref_items(env["maps"][1:2]), [("rgba", R.COLOUR), ("labels",)])
    _check(a[0].cpu().numpy(), want[0], "one item after a full scene")
    _check(a[1].cpu().numpy(), want[1], "labels")


def _one(x, y, z, n, r, conf=5.0, colour=0, t=1):
    s = np.zeros(12, np.float32)
    s[:3] = (x, y, z); s[3] = conf; s[4] = colour; s[6] = t; s[7] = t
    s[8:11] = np.asarray(n, np.float32) / np.linalg.norm(n); s[11] = r
    return s


def _upload(env, S, cap=64):
    from co_fusion_amd import model as M
    m = M.Model(env["ctx"], cap)
    m.upload_map(np.asarray(S, np.float32))
    return m


def test_depth_test_rules(env):
    R = env["R"]
    v = _views()[0]
    I = np.eye(4, dtype=np.float32)
    red, green, blue = float(0xFF0000), float(0x00FF00), float(0x0000FF)
    # model 1: a far surfel at index 0, an exact duplicate (same depth) at index 1; model 2: the same surfel again, and a nearer one
    a = [_one(0.0, 0.0, 2.0, (0, 0, -1), 0.3, colour=red), _one(0.0, 0.0, 2.0, (0, 0, -1), 0.3, colour=blue)]
    b = [_one(0.0, 0.0, 2.0, (0, 0, -1), 0.3, colour=green), _one(0.1, 0.0, 1.5, (0, 0, -1), 0.05, colour=blue)]
    ma, mb = _upload(env, a), _upload(env, b)
    try:
        maps = [(np.array(a), I, 1.0, 1, R.COLOUR), (np.array(b), I, 1.0, 2, R.COLOUR)]
        items = _items(env, maps, [ma, mb])
        rgba, lab = [t.cpu().numpy() for t in env["rnd"].render(_gpu_view(R, v, 0), items, (R.COLOUR,), labels=True)]
        want = rr.render(dict(v, tick=TICK), _ref_items(maps), [("rgba", R.COLOUR), ("labels",)])
        _check(rgba, want[0], "rgba"); _check(lab, want[1], "labels")
        # the nearer surfel of the LATER model wins its pixels; elsewhere the tie goes to model 1, and within it to index 0 (red)
        u = int(FX * 0.1 / 1.5 + CX); vv = int(CY)
        assert lab[vv, u] == 2 and tuple(rgba[vv, u, :3]) == (0, 0, 255)
        ctr = lab[int(CY) + 20, int(CX)]
        assert ctr == 1 and tuple(rgba[int(CY) + 20, int(CX), :3]) == (255, 0, 0)
        # reversed draw order: the tie now goes to model 2 (green), the nearer surfel still wins
        rgba2, lab2 = [t.cpu().numpy() for t in env["rnd"].render(_gpu_view(R, v, 0), items[::-1], (R.COLOUR,), labels=True)]
        assert lab2[int(CY) + 20, int(CX)] == 2 and tuple(rgba2[int(CY) + 20, int(CX), :3]) == (0, 255, 0)
        assert lab2[vv, u] == 2 and tuple(rgba2[vv, u, :3]) == (0, 0, 255)
    finally:
        ma.close(); mb.close()


def test_large_footprint_is_the_analytic_disc_and_near_plane_corners_skip(env):
    R = env["R"]
    v = _views()[0]
    I = np.eye(4, dtype=np.float32)
    z = 1.0
    # analytic: the ray through the pixel centre meets z = 1 at ((px + .5 - cx) / fx, (py + .5 - cy) / fy); a radius whose rim passes
    # no pixel centre closer than 1e-6 (the f32 arithmetic is exact to a few 1e-8 there)
    py, px = np.mgrid[0:H, 0:W]
    d = np.hypot((px + 0.5 - CX) / FX - 0.03, (py + 0.5 - CY) / FY + 0.02)
    r = next(float(np.float32(c)) for c in np.arange(0.41, 0.415, 0.0001) if np.abs(d - float(np.float32(c))).min() > 1e-6)
    s = _one(0.03, -0.02, z, (0, 0, -1), r, colour=float(0x808080))
    m = _upload(env, [s])
    try:
        maps = [(np.array([s]), I, 1.0, 0, R.COLOUR)]
        rgba, depth = [t.cpu().numpy() for t in env["rnd"].render(_gpu_view(R, v, 0), _items(env, maps, [m]), (R.COLOUR,), depth=True)]
        disc = d <= r
        assert disc.sum() > 0.5 * W * H
        assert np.array_equal(rgba[..., 3] == 255, disc)
        assert np.allclose(depth[disc], z, atol=1e-6) and (depth[~disc] == 0).all()
        want = rr.render(dict(v), _ref_items(maps), [("rgba", R.COLOUR), ("depth",)])
        _check(rgba, want[0], "large splat"); _check(depth, want[1], "large splat depth")
    finally:
        m.close()
    # a surfel seen edge-on close to the camera has quad corners at z <= near: skipped; the same surfel further away is drawn
    near_s = _one(0.0, 0.0, 0.15, (1, 0, 0.2), 0.1)
    far_s = _one(0.0, 0.0, 0.6, (1, 0, 0.2), 0.1)
    for s, drawn in ((near_s, False), (far_s, True)):
        m = _upload(env, [s])
        try:
            maps = [(np.array([s]), I, 1.0, 0, R.GREY)]
            (lab,) = [t.cpu().numpy() for t in env["rnd"].render(_gpu_view(R, v, 0), _items(env, maps, [m]), (), labels=True)]
            assert (lab != 255).any() == drawn
            _check(lab, rr.render(dict(v), _ref_items(maps), [("labels",)])[0], "near-plane labels")
        finally:
            m.close()


def test_refusals(env):
    """more than 2^32 - 1 surfels in one call, a view larger than the render object, an unknown mode: errors, nothing enqueued"""
    from co_fusion_amd import api
    R = env["R"]
    v = _views()[0]
    big = [R.make_item(1 << 20, 1 << 31, np.eye(4), 1.0, 0, R.COLOUR), R.make_item(1 << 20, 1 << 31, np.eye(4), 1.0, 1, R.COLOUR)]
    with pytest.raises(api.CofusionError, match="2\\^32"):
        env["rnd"].render(_gpu_view(R, v, 0), big, (R.COLOUR,))
    with pytest.raises(api.CofusionError, match="maximum"):
        env["rnd"].render(R.make_view(np.eye(4), FX, FY, CX, CY, 640, 480), [], (R.COLOUR,))
    with pytest.raises(api.CofusionError, match="colour mode"):
        env["rnd"].render(_gpu_view(R, v, 0), _items(env)[:1], (7,))
    env["ctx"].synchronize()


def test_palette_is_the_documented_one():
    from co_fusion_amd import render as R
    assert np.array_equal(R.palette(), rr.palette())
    assert tuple(R.palette()[255]) == (0, 0, 0)
