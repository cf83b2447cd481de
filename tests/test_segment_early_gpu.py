"""GPU parity of the split segmentation chain: cf_seg_early (the half that needs no tracking: the frame's and the confidences' sums,
their statistics, the appearance kernel) followed by cf_seg_sums + cf_seg_infer (the ICP-error half) against the oracle and against
the plain chain -- on the adversarial scenarios of test_segment_gpu.py, through the segmenter's state handling (an early half nobody
finishes, early halves that do not match the inference), at a ragged superpixel count, with superpixels that own no pixel, and
through the facade's switch on a free run with a spawn."""
import copy
import ctypes as C
import warnings

import numpy as np
import pytest

import test_segment_gpu as base
from test_segment_gpu import SegResult, _compare, _ref

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)


class _Run:
    """One scenario's device inputs on one segmenter; the calls of the chain one by one"""

    def __init__(self, ctx, seg, sc):
        self.ctx, self.seg, self.lib = ctx, seg, ctx.lib
        self.name, self.params, rgba, depth, self.ids, icp, vc, self.next_id, self.allow_new = sc
        self.n = len(self.ids)
        self.keep = [ctx.to_device(rgba), ctx.to_device(depth)] + [ctx.to_device(a) for a in icp] + [ctx.to_device(a) for a in vc]
        self.rgba, self.depth = self.keep[0], self.keep[1]
        self.icp, self.vc = self.keep[2:2 + self.n], self.keep[2 + self.n:]
        self.full = ctx.to_device(np.zeros((base.H, base.W), np.uint8))

    def _ptrs(self, ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def slic(self):
        self.ctx._check(self.lib.cf_seg_slic(self.seg, C.c_void_p(self.rgba.data_ptr())))

    def early(self, params=None, n=None):
        n = self.n if n is None else n
        p = self.params if params is None else params
        p = p.__class__.from_buffer_copy(p)
        self.ctx._check(self.lib.cf_seg_early(self.seg, C.c_void_p(self.depth.data_ptr()), C.c_void_p(self.rgba.data_ptr()), n,
                                              self._ptrs(self.vc[:n]), C.byref(p)))

    def sums(self, n=None):
        n = self.n if n is None else n
        s = C.c_void_p(); w = C.c_uint64()
        self.ctx._check(self.lib.cf_seg_sums(self.seg, C.c_void_p(self.depth.data_ptr()), n, self._ptrs(self.icp[:n]), self._ptrs(self.vc[:n]),
                                             C.byref(s), C.byref(w)))

    def infer(self):
        p = self.params.__class__.from_buffer_copy(self.params)
        ids = (C.c_uint32 * self.n)(*self.ids)
        self.ctx._check(self.lib.cf_seg_infer(self.seg, C.byref(p), C.c_void_p(self.rgba.data_ptr()), self.n, ids, C.c_uint32(self.next_id),
                                              int(self.allow_new), C.c_void_p(self.full.data_ptr())))
        res = SegResult()
        low = np.zeros(base.GX * base.GY, np.uint8)
        self.ctx._check(self.lib.cf_seg_fetch(self.seg, C.byref(res), low.ctypes.data_as(C.c_void_p)))
        return res, low.reshape(base.GY, base.GX), self.full.cpu().numpy()

    def split_chain(self):
        self.slic(); self.early(); self.sums()
        return self.infer()

    def plain_chain(self):
        self.slic(); self.sums()
        return self.infer()


def _context(w, h):
    from co_fusion_amd import api, synth
    cam = synth.Camera.scaled(w, h)
    ctx = api.Context(w, h, cam.fx, cam.fy, cam.cx, cam.cy, max_models=48)
    seg = C.c_void_p()
    ctx._check(ctx.lib.cf_seg_create(ctx.h, C.byref(seg)))
    return ctx, seg


def _close(ctx, seg):
    ctx.lib.cf_seg_destroy(seg)
    ctx.close()


def test_early_then_late_chain_matches_the_oracle():
    """cf_seg_slic -> cf_seg_early -> cf_seg_sums -> cf_seg_infer -> cf_seg_fetch on every scenario of test_segment_gpu.py (depth holes
    and their replay, a zero-confidence model, 24 and 40 models, a new label allowed and not), twice each: the accumulators are clean."""
    ctx, seg = _context(base.W, base.H)
    for sc in base._scenarios():
        run, ref = _Run(ctx, seg, sc), _ref(sc)
        for rep in range(2):
            _compare(f"early chain, {sc[0]} (pass {rep})", *run.split_chain(), ref)
    _close(ctx, seg)


def test_early_halves_that_are_dropped_or_do_not_match():
    """The segmenter's state: an early half no inference follows, one formed with other feature scales, one with another model count --
    every result is the oracle's for what cf_seg_infer was given, and the plain chain still works behind all of them."""
    ctx, seg = _context(base.W, base.H)
    scs = base._scenarios()
    five, three = scs[3], scs[4]   # default CRF on five models (+ new label); depth holes on three
    run5, run3 = _Run(ctx, seg, five), _Run(ctx, seg, three)
    # an inference that never came: early (another frame's), early, sums, infer
    run3.slic(); run3.early()
    run5.slic(); run5.early(); run5.sums()
    _compare("early, early, sums, infer", *run5.infer(), _ref(five))
    # an early half that got as far as its ICP sums, and no further
    run3.slic(); run3.early(); run3.sums()
    _compare("early, sums, early, sums, infer", *run5.split_chain(), _ref(five))
    # other feature scales than the inference's
    other = five[1].__class__.from_buffer_copy(five[1])
    other.scaleFeaturesRGB *= 0.5; other.scaleFeaturesDepth *= 2.0; other.scaleFeaturesPos *= 1.5
    run5.slic(); run5.early(params=other); run5.sums()
    _compare("early with other feature scales", *run5.infer(), _ref(five))
    # ... and the other way round: the inference's own parameters differ from the early half's defaults
    sc_other = (five[0] + ", other scales", other) + five[2:]
    run5o = _Run(ctx, seg, sc_other)
    run5o.slic(); run5o.early(params=five[1]); run5o.sums()
    _compare("inference with other feature scales", *run5o.infer(), _ref(sc_other))
    # an early half with n models, the sums and the inference with n - 1
    sc4 = (five[0] + ", four models",) + five[1:4] + (five[4][:4], five[5][:4], five[6][:4]) + five[7:]
    run4 = copy.copy(run5)   # (the same device images: only the count differs)
    run4.n, run4.ids, run4.icp, run4.vc = 4, sc4[4], run5.icp[:4], run5.vc[:4]
    run5.slic(); run5.early(); run4.sums()
    _compare("early with one model more", *run4.infer(), _ref(sc4))
    # the plain chain after all of these, then the split one again
    _compare("plain chain afterwards", *run3.plain_chain(), _ref(three))
    _compare("plain chain afterwards, five models", *run5.plain_chain(), _ref(five))
    _compare("split chain afterwards", *run3.split_chain(), _ref(three))
    _close(ctx, seg)


def test_early_chain_with_a_ragged_superpixel_count(monkeypatch):
    """176 x 144: K = 11 x 9 = 99 superpixels -- not a multiple of sixteen (the strided average-confidence sums), gx != gy (the k / gy
    row of the resample coordinates), one wave's worth of superpixels: the split chain and the plain one against the oracle."""
    w, h = 176, 144
    for k, v in (("W", w), ("H", h), ("GX", w // 16), ("GY", h // 16)):
        monkeypatch.setattr(base, k, v)
    monkeypatch.setattr(base, "_REFS", {})
    ctx, seg = _context(w, h)
    for sc in base._scenarios()[:6]:
        run, ref = _Run(ctx, seg, sc), _ref(sc)
        _compare(f"early chain, {sc[0]} at {w}x{h}", *run.split_chain(), ref)
        _compare(f"plain chain, {sc[0]} at {w}x{h}", *run.plain_chain(), ref)
        _compare(f"early chain again, {sc[0]} at {w}x{h}", *run.split_chain(), ref)
    assert (base.GX * base.GY) % 16 != 0
    _close(ctx, seg)


def test_superpixels_without_a_pixel():
    """SLIC's own labels are overwritten on the device so that a few superpixels own no pixel -- their rows are replayed from the
    resample label, already divided when it is smaller than the superpixel's index and still raw when larger -- and the split chain must
    equal the plain chain bit for bit (the list of these superpixels is formed by the early half and replayed for the ICP rows by the
    late one).  The new labels keep the precondition of seg_accumulate_kernel (a pixel's label is one of the 3x3 cells around the pixel's
    own cell), and both chains must equal the oracle's staged entry on the same label image as well."""
    import torch
    import orc_multi as om
    import seg_cases
    ctx, seg = _context(base.W, base.H)
    gx, gy, K = base.GX, base.GY, base.GX * base.GY
    empty_natural = []
    for sc in (base._scenarios()[3], base._scenarios()[4]):
        run = _Run(ctx, seg, sc)
        run.slic()
        dptr = C.c_void_p(); nbytes = C.c_uint64()
        ctx._check(ctx.lib.cf_seg_labels(seg, C.byref(dptr), C.byref(nbytes)))
        labels = torch.empty((base.H, base.W), dtype=torch.int32, device=ctx.device)
        assert nbytes.value == labels.numel() * 4
        ctx._check(ctx.lib.cf_memcpy_d2d_async(ctx.h, C.c_void_p(labels.data_ptr()), dptr, C.c_uint64(nbytes.value)))
        ctx.synchronize()
        lab = labels.cpu().numpy().copy()
        empty_natural.append(int(np.count_nonzero(np.bincount(lab.ravel(), minlength=K) == 0)))
        assert seg_cases.invariant_3x3(lab)
        # superpixel k gives its pixels to its left or right neighbour -- those in a cell that does not touch the neighbour's, to the cell's own
        cell = seg_cases.grid_labels(base.W, base.H)
        for k, to in ((5, 6), (300, 299), (302, 303), (777, 776), (K - 1, K - 2), (0, 1)):   # (no two of them neighbours: the cell between keeps its own)
            near = (np.abs(cell % gx - to % gx) <= 1) & (np.abs(cell // gx - to // gx) <= 1)
            lab[:] = np.where(lab == k, np.where(near, to, cell), lab)
        assert seg_cases.invariant_3x3(lab)
        counts = np.bincount(lab.ravel(), minlength=K)
        empties = np.flatnonzero(counts == 0)
        ks = np.arange(K)
        xs = np.minimum((ks % gx) * 16 + 8, base.W - 1); ys = np.minimum((ks // gy) * 16 + 8, base.H - 1)   # (k / gy: the reference's)
        read = lab[ys, xs]
        assert len(empties) >= 6 and np.any(read[empties] < empties) and np.any(read[empties] > empties), (empties, read[empties])
        crafted = torch.from_numpy(lab).to(ctx.device)

        def chain(split):
            run.slic()
            ctx._check(ctx.lib.cf_memcpy_d2d_async(ctx.h, dptr, C.c_void_p(crafted.data_ptr()), C.c_uint64(nbytes.value)))
            if split:
                run.early()
            run.sums()
            return run.infer()

        ref = om.segment_crf_stages(*sc[1:], labels_in=lab, stages=False)
        plain = chain(False)
        _compare(f"{sc[0]}, superpixels without a pixel: plain chain against the oracle", *plain, ref)
        for rep in range(2):
            res, low, full = chain(True)
            _compare(f"{sc[0]}, superpixels without a pixel: split chain against the oracle (pass {rep})", res, low, full, ref)
            assert np.array_equal(low, plain[1]) and np.array_equal(full, plain[2]), f"{sc[0]}: label maps (pass {rep})"
            assert bytes(res)[:12 + 36 * res.n_models] == bytes(plain[0])[:12 + 36 * plain[0].n_models], f"{sc[0]}: decisions (pass {rep})"
        again = chain(False)
        assert np.array_equal(again[2], plain[2]) and bytes(again[0])[:12 + 36 * again[0].n_models] == bytes(plain[0])[:12 + 36 * plain[0].n_models]
    print(f"pixel-empty superpixels SLIC itself left in these scenarios: {empty_natural}")
    _close(ctx, seg)


def test_facade_switch_changes_nothing():
    """cofusion_set_seg_early on / off on a free run of the two-object CRF scene of the frame-loop pin (160 x 128, a spawn on the way):
    ids, counts, poses, surfel buffers and label masks digested after every frame."""
    import cfpin
    from co_fusion_amd import facade
    _, _, conf_global, spawn, _, _ = cfpin.SCENARIOS["crf_two_objects"]
    cam, frames = cfpin.frames_of("crf_two_objects")
    runs = []
    for on in (True, False):
        cf = facade.CoFusion(cfpin.W, cfpin.H, cam.fx, cam.fy, cam.cx, cam.cy, max_surfels=1 << 17, conf_global_init=conf_global,
                             model_spawn_offset=spawn, enable_multiple_models=1)
        cf.set_seg_early(on)
        rows = []
        for t, (d, rgb, _, _) in enumerate(frames):
            cf.process_frame(d, rgb, timestamp=t)
            infos = [cf.model_info(i) for i in range(cf.num_models)]
            rows.append(([m["id"] for m in infos], [m["count"] for m in infos], [cfpin._sha(m["pose"]) for m in infos],
                         [cfpin._sha(cf.model_download(i)) for i in range(cf.num_models)], cfpin._sha(cf.mask())))
        cf.close()
        runs.append(rows)
    assert max(len(r[0]) for r in runs[0]) >= 2, "no object model was spawned"
    for t, (a, b) in enumerate(zip(*runs)):
        assert a == b, f"frame {t}: early half on {a} vs off {b}"
