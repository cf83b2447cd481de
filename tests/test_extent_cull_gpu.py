"""Extent culling of the batched index passes (cf_set_extent_culling; csrc/surf_index_dev.h, EXTENTS): the index-map resolve launches of
cf_models_preindex / cf_models_frame_passes skip the 64-texel runs outside the rectangle a model's maps were rasterised into in this pass
and in the one before it.  The promise is that every buffer holds the same bytes as without it after every launch.

Every scenario plays one sequence of calls twice in one process, on two sets of models in one context: set A with the switch as the
scenario sets it (on, unless it turns it off), set B with the switch off.  After EVERY call and for EVERY model of the scenario, bit for bit:
the index-map buffers 0-3, the clean stage's packed texel records (13), the prediction 4-7, the fill-in maps 8-10 where the model has
them, the surfel map and its count -- A against B, and both against the CPU oracle's chain where tests/surfel_cases.py has one (the
batched calls and the per-model calls); and the z-keys (buffer 14) of both are all ones.

Shapes: 128x32 (two 64-texel runs per row) and 80x24 (a run straddles two rows).  The maps are a few hundred surfels cut out of a flat wall
1.5 m in front of the camera; a translation of the pose moves their footprint by whole pixels, so a scenario says where the footprint goes
in pixels and asserts from the oracle's maps that it went there (moved away, touching a border, gone, back).
"""
import numpy as np
import pytest

import surfel_cases as sc
from test_surfel_chain_gpu import _compare, _dev, _item, _per_model, contexts  # noqa: F401  (contexts: the module-scoped fixture)
from test_surfel_gpu import _same

pytestmark = pytest.mark.gpu

SHAPES = [(128, 32), (80, 24)]
Z = 1.5
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
NOBODY = 7          # a mask id no pixel carries: the model fuses nothing of the frame, its footprint is its map's


def _wall(shape, seed, labels=None):
    """a flat wall at Z with a seeded colour image; labels: [(value, x0, x1, y0, y1)] rectangles of the mask (0 elsewhere)"""
    w, h = shape
    d = np.full((h, w), Z, np.float32)
    rng = np.random.default_rng(seed)
    rgba = rng.integers(1, 255, size=(h, w, 4), dtype=np.uint8); rgba[..., 3] = 255
    mask = np.zeros((h, w), np.uint8)
    for v, x0, x1, y0, y1 in labels or []:
        mask[y0:y1, x0:x1] = v
    return sc.Frame(rgba, d, sc.op.bilateral(d, sc.FILTER_CUTOFF), mask)


def _blob(cam, shape, x0, x1, y0, y1, time=1):
    """the wall's surfels under the pixels [x0, x1) x [y0, y1): confident, last seen at `time`"""
    w, h = shape
    base = sc._plane_base(cam, _wall(shape, 1), conf=30.0, time=time)
    ids = np.arange(w * h).reshape(w, h)
    return base[ids[x0:x1, y0:y1].reshape(-1)].copy()


def _moved(cam, du, dv):
    """the pose under which the footprint of a map at depth Z appears du pixels to the right and dv pixels down"""
    p = np.eye(4, dtype=np.float32)
    p[0, 3] = -du * Z / cam.fx; p[1, 3] = -dv * Z / cam.fy
    return p


def _box(a):
    """bounding box (x0, x1, y0, y1; inclusive) of the non-zero texels of a map, or None"""
    ys, xs = np.nonzero(a.reshape(a.shape[0], a.shape[1], -1).any(axis=2))
    return None if xs.size == 0 else (int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max()))


class Play:
    """two sets of models in one context and the oracle's maps beside them"""

    def __init__(self, ctx, cam, shape, maps, frames, time_delta=sc.TIME_DELTA, fill=()):
        from co_fusion_amd import model as M
        self.M, self.ctx, self.cam, self.shape, self.time_delta, self.fill = M, ctx, cam, shape, time_delta, set(fill)
        self.case = sc.Case("extent", shape, cam, [np.array(m) for m in maps], frames, [], time_delta=time_delta)
        self.frames = {k: dict(rgba=_dev(ctx, f.rgba), mask=_dev(ctx, f.mask), depth=_dev(ctx, f.depth), depth_filt=_dev(ctx, f.depth_filt))
                       for k, f in frames.items()}
        self.a = [M.Model(ctx, 1 << 13) for _ in maps]
        self.b = [M.Model(ctx, 1 << 13) for _ in maps]
        self.maps = [np.array(m) for m in maps]
        self.filled = set()      # models whose fill-in maps have been written
        self.on = True
        self.step = 0
        for ms in (self.a, self.b):
            for m, s in zip(ms, maps):
                m.upload_map(s)

    def close(self):
        self.M.set_extent_culling(self.ctx, True)
        for m in self.a + self.b:
            m.close()

    def switch(self, on):
        self.on = on

    def _both(self, fn):
        self.M.set_extent_culling(self.ctx, self.on)
        fn(self.a)
        self.M.set_extent_culling(self.ctx, False)
        fn(self.b)
        self.M.set_extent_culling(self.ctx, True)

    def _items(self, ms, call):
        out = []
        for it in call:
            d = _item(ms[it.model], it, self.frames[it.frame])
            if it.model in self.fill:
                d.update(fill_in=1, passthrough_geom=0, passthrough_rgb=0)
            out.append(d)
        return out

    def same(self, what):
        """A against B, every model, every buffer; the z-keys of both all empty"""
        for k, (ma, mb) in enumerate(zip(self.a, self.b)):
            assert ma.count() == mb.count(), f"{what}: model {k}: count"
            _same(ma.download_map(), mb.download_map(), f"{what}: model {k}: map")
            for which in (0, 1, 2, 3, 13, 4, 5, 6, 7) + ((8, 9, 10) if k in self.filled else ()):
                _same(ma.buffer(which), mb.buffer(which), f"{what}: model {k}: buffer {which}, culled against unculled")
            for m, tag in ((ma, "culled"), (mb, "unculled")):
                assert (m.buffer(14) == EMPTY_KEY).all(), f"{what}: model {k}: z-keys left behind ({tag})"

    def chain(self, call, preindexed=False):
        """one cf_models_frame_passes on both sets; -> the oracle's Results by position"""
        self.step += 1
        what = f"step {self.step} (chain)"
        self._both(lambda ms: self.M.frame_passes(self.ctx, self._items(ms, call), sc.DEPTH_CUTOFF, sc.OUTLIER, self.time_delta))
        res = []
        for q, it in enumerate(call):
            r = sc.oracle_item(self.case, it, self.maps[it.model])
            self.maps[it.model] = r.map
            res.append(r)
            if it.model in self.fill:
                self.filled.add(it.model)
        self.same(what)
        for q, it in enumerate(call):
            fr = self.case.frames[it.frame]
            for ms, tag in ((self.a, "culled"), (self.b, "unculled")):
                _compare(ms[it.model], res[q], fr, f"{what} item {q}, {tag}", True)
                if it.model in self.fill:
                    img, vc, nr, _ = res[q].splat
                    want = sc.op.fill_in(vc, nr, img, fr.depth_filt, fr.rgba, sc.ocam(self.cam))
                    for j in range(3):
                        _same(ms[it.model].buffer(8 + j), want[j], f"{what} item {q}, {tag}: fill-in map {8 + j}")
        return res

    def per_model(self, it, which="all"):
        """an unculled per-model call on both sets: the whole chain of one model, or its index pass / its prediction alone"""
        self.step += 1
        what = f"step {self.step} (per-model {which})"
        fr = self.frames[it.frame]
        if which == "all":
            self._both(lambda ms: _per_model(ms[it.model], it, fr, self.case))
            r = sc.oracle_item(self.case, it, self.maps[it.model])
            self.maps[it.model] = r.map
            for ms in (self.a, self.b):
                _compare(ms[it.model], r, self.case.frames[it.frame], what, False)
        elif which == "index":
            self._both(lambda ms: ms[it.model].predict_indices(it.pose, it.time, sc.DEPTH_CUTOFF, self.time_delta))
            w, h = self.shape
            want = sc.op.predict_indices(self.maps[it.model], it.pose, sc.ocam(self.cam), w, h, sc.DEPTH_CUTOFF, it.time, self.time_delta)
            for ms in (self.a, self.b):
                for j in range(4):
                    _same(ms[it.model].buffer(j), want[j], f"{what}: buffer {j}")
        else:
            self._both(lambda ms: ms[it.model].combined_predict(it.pose, sc.DEPTH_CUTOFF, it.conf, it.time, it.time, self.time_delta))
            w, h = self.shape
            want = sc.op.combined_predict(self.maps[it.model], it.pose, sc.ocam(self.cam), w, h, sc.DEPTH_CUTOFF, it.conf, it.time, it.time,
                                          self.time_delta)
            for ms in (self.a, self.b):
                for j in range(4):
                    _same(ms[it.model].buffer(4 + j), want[j], f"{what}: buffer {4 + j}")
        self.same(what)

    def upload(self, model, surfels):
        self.step += 1
        self.maps[model] = np.array(surfels)
        for ms in (self.a, self.b):
            ms[model].upload_map(surfels)


@pytest.fixture
def play(contexts):
    made = []

    def make(shape, maps, frames, **kw):
        cam = sc.synth.Camera.scaled(*shape)
        p = Play(contexts(shape, cam), cam, shape, maps, frames, **kw)
        made.append(p)
        return p
    yield make
    for p in made:
        p.close()


def _centre(shape):
    w, h = shape
    return w // 2 - 10, w // 2 + 10, h // 2 - 6, h // 2 + 6     # 20 x 12 pixels = 240 surfels


@pytest.mark.parametrize("shape", SHAPES)
def test_moving_footprint_borders_and_ring(play, shape):
    """eight chains in a row (sixteen index passes: the ring wraps five times): the footprint moves away from where
    it was -- the texels it leaves must be put back to empty --, then over each border and a corner of the image, then home"""
    w, h = shape
    cam = sc.synth.Camera.scaled(*shape)
    x0, x1, y0, y1 = _centre(shape)
    p = play(shape, [_blob(cam, shape, x0, x1, y0, y1)], {"f": _wall(shape, 2)})
    moves = [(0, 0, None), (25, 0, None), (-x0 - 8, 0, "left"), (w - x1 + 8, 0, "right"), (0, -y0 - 4, "top"), (0, h - y1 + 4, "bottom"),
             (-x0 - 8, -y0 - 4, "corner"), (0, 0, None)]
    last = None
    for t, (du, dv, border) in enumerate(moves):
        r = p.chain([sc.Item(0, "f", _moved(cam, du, dv), 2 + t, mask_id=NOBODY)])[0]
        for name, a in (("index map", r.index[0]), ("prediction", r.splat[0])):
            b = _box(a)
            assert b is not None, f"move {t}: the {name} is empty"
            if border in ("left", "corner"):
                assert b[0] == 0 and b[1] < x0
            if border == "right":
                assert b[1] == w - 1 and b[0] > x1
            if border in ("top", "corner"):
                assert b[2] == 0
            if border == "bottom":
                assert b[3] == h - 1
        if t == 1:   # disjoint from where it was: nothing of the first footprint may survive
            assert _box(r.index[0])[0] > _box(last.index[0])[1] - 3
        last = r
    assert _box(last.index[0])[0] in (x0 - 1, x0, x0 + 1)


@pytest.mark.parametrize("shape", SHAPES)
def test_footprint_vanishes_and_returns(play, shape):
    """every surfel time-gated (a frame far in the future of a closed loop): empty maps, empty extents; then the same map again.  Beside it
    a model without surfels from the start: its second and every later pass is culled against an empty rectangle"""
    cam = sc.synth.Camera.scaled(*shape)
    x0, x1, y0, y1 = _centre(shape)
    blob = _blob(cam, shape, x0, x1, y0, y1)
    p = play(shape, [blob, np.zeros((0, sc.SURFEL), np.float32)], {"f": _wall(shape, 3)}, time_delta=25)
    pose = _moved(cam, 3, 1)

    def call(t):
        return p.chain([sc.Item(0, "f", pose, t, mask_id=NOBODY), sc.Item(1, "f", pose, t, mask_id=NOBODY)])
    r = call(2)
    assert _box(r[0].index[0]) is not None and _box(r[0].splat[0]) is not None and _box(r[1].index[0]) is None
    r = call(3)
    assert _box(r[0].index[0]) is not None and r[1].map.shape[0] == 0
    r = call(1000)      # 1000 - 3 > 25: gated in both rasterisers
    assert _box(r[0].index[0]) is None and _box(r[0].index_first[0]) is None and _box(r[0].splat[0]) is None
    assert r[0].map.shape[0] == blob.shape[0]      # (confident surfels: the clean stage keeps them)
    r = call(1001)
    assert _box(r[0].index[0]) is None
    r = call(4)         # back
    assert _box(r[0].index[0]) is not None and _box(r[0].splat[0]) is not None
    call(5)
    # count 0 through an upload, and the map back the same way (an upload leaves the extents unknown)
    p.upload(0, np.zeros((0, sc.SURFEL), np.float32))
    r = call(6)
    assert _box(r[0].index[0]) is None and _box(r[0].splat[0]) is None
    call(7)
    p.upload(0, blob)
    r = call(8)
    assert _box(r[0].index[0]) is not None


@pytest.mark.parametrize("shape", SHAPES)
def test_two_models_one_with_fill_in(play, shape):
    """two models with different footprints in one batch.  Model 0 carries the fill-in and fuses the wall left of the middle -- it grows
    past the size up to which a model has extents at all --; model 1 fuses its own label and moves"""
    w, h = shape
    cam = sc.synth.Camera.scaled(*shape)
    fr = _wall(shape, 4, labels=[(9, w // 2, w, 0, h), (1, w - 30, w - 6, 4, h - 4)])
    maps = [_blob(cam, shape, 6, 30, 3, h - 6), _blob(cam, shape, w - 28, w - 8, 6, h - 6)]
    p = play(shape, maps, {"f": fr}, fill=(0,))
    for t, (du, dv) in enumerate([(0, 0), (2, 1), (-9, -2), (0, 0)]):
        r = p.chain([sc.Item(0, "f", _moved(cam, du // 2, 0), 2 + t, mask_id=0), sc.Item(1, "f", _moved(cam, du, dv), 2 + t, mask_id=1)])
        b0, b1 = _box(r[0].index[0]), _box(r[1].index[0])
        assert b0[0] < b1[0] - 20 and b0[1] < b1[1] - 20, f"call {t}: two different footprints"
        assert r[0].fresh.shape[0] > 0 or t > 0      # (model 0 grows: the wall it has not mapped yet)


@pytest.mark.parametrize("shape", SHAPES)
def test_unculled_calls_between_culled_chains(play, shape):
    """the per-model entry points run today's launches and know nothing of the rings: each of them -- an index pass alone, a prediction
    alone, the whole per-model chain -- puts a footprint where no rectangle of the ring is, and the chain behind it must not trust the ring"""
    cam = sc.synth.Camera.scaled(*shape)
    x0, x1, y0, y1 = _centre(shape)
    p = play(shape, [_blob(cam, shape, x0, x1, y0, y1)], {"f": _wall(shape, 5)})

    def item(t, du, dv):
        return sc.Item(0, "f", _moved(cam, du, dv), t, mask_id=NOBODY)
    p.chain([item(2, 0, 0)])
    p.chain([item(3, 1, 0)])
    p.per_model(item(4, -x0 + 2, -3), "index")
    p.chain([item(4, 1, 1)])
    p.chain([item(5, 1, 1)])
    p.per_model(item(6, x0 - 4, 3), "predict")
    p.chain([item(6, 0, 1)])
    p.per_model(item(7, -x0 + 4, 2), "all")
    p.chain([item(8, 2, 0)])
    p.chain([item(9, 2, 0)])


@pytest.mark.parametrize("shape", SHAPES)
def test_switch_off_and_on_again(play, shape):
    cam = sc.synth.Camera.scaled(*shape)
    x0, x1, y0, y1 = _centre(shape)
    p = play(shape, [_blob(cam, shape, x0, x1, y0, y1)], {"f": _wall(shape, 6)})

    def call(t, du, dv):
        return p.chain([sc.Item(0, "f", _moved(cam, du, dv), t, mask_id=NOBODY)])
    call(2, 0, 0)
    call(3, 4, 0)
    p.switch(False)
    call(4, -x0 + 3, 2)     # unculled: the footprint goes where the ring does not know it
    p.switch(True)
    call(5, x0 - 5, -2)
    call(6, 0, 0)
    p.switch(False)
    call(7, 5, 5)
    p.switch(True)
    call(8, 5, 5)


@pytest.mark.parametrize("shape", SHAPES)
def test_preindex_shares_the_ring(play, shape):
    """cf_models_preindex is a pass of the index maps' ring.  The chain that is handed the tracker's pose skips its first index pass (the
    ring does not advance for it); a pose that differs in one bit rasterises again"""
    from co_fusion_amd import api
    import prep_scenes as ps
    s = ps.scene(*shape)
    cam = s["cam"]
    x0, x1, y0, y1 = _centre(shape)
    start = sc.to_world(_blob(cam, shape, x0, x1, y0, y1), s["pose"])
    p = play(shape, [start], {"f": _wall(shape, 7)})
    ctx = p.ctx
    g = api.Odometry(ctx)
    try:
        g.init_first_rgb(_dev(ctx, s["rgba0"]))
        g.init_icp_model(_dev(ctx, s["v4"]), _dev(ctx, s["n4"]), s["pose"])
        g.init_rgb_model(_dev(ctx, s["img"]))
        g.init_icp([_dev(ctx, l) for l in s["depth_pyr"]], ps.CUTOFF)
        g.init_rgb(_dev(ctx, s["rgba1"]))
        p.chain([sc.Item(0, "f", s["pose"] @ _moved(cam, 12, 2), 2, mask_id=NOBODY)])      # a known state, elsewhere
        ctx.track_batch([g], [s["pose"]])
        p._both(lambda ms: p.M.preindex(ctx, [(ms[0], g, 3)], sc.DEPTH_CUTOFF))
        tr, rot, _ = g.fetch()
        pose = np.eye(4, dtype=np.float32); pose[:3, :3] = rot; pose[:3, 3] = tr
        w, h = shape
        first = sc.op.predict_indices(p.maps[0], pose, sc.ocam(cam), w, h, sc.DEPTH_CUTOFF, 3, sc.TIME_DELTA)
        assert _box(first[0]) is not None
        for ms in (p.a, p.b):
            for k in range(4):
                _same(ms[0].buffer(k), first[k], f"preindex: buffer {k}")
        p.same("preindex")
        p.chain([sc.Item(0, "f", pose, 3, mask_id=NOBODY)])          # skips its first index pass
        p._both(lambda ms: p.M.preindex(ctx, [(ms[0], g, 4)], sc.DEPTH_CUTOFF))
        p.same("second preindex")
        other = pose.copy()
        other[0, 3] = np.nextafter(other[0, 3], np.float32(np.inf))
        p.chain([sc.Item(0, "f", other, 4, mask_id=NOBODY)])         # rasterises again
        p.chain([sc.Item(0, "f", other @ _moved(cam, -6, 1), 5, mask_id=NOBODY)])
    finally:
        g.close()
