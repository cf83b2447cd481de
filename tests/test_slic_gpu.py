"""GPU parity of the SLIC superpixel passes on the crafted images of tests/slic_cases.py: cf_seg_slic -- slic_init_kernel, six
slic_assign_kernel, five slic_update_kernel -- on its own, its labels against orc_slic and what it leaves behind (cf_seg_buffer 12:
the centres of the fifth update, 13: the sums of the sixth pass) against the last pass of tests/slic_ref.py's trace, bit for bit, no
tolerance anywhere.  Behind it the handoff to the chain: cf_seg_sums with one model over SLIC's own labels -- the pixel counts against
the labels' bincount and column 5 of buffer 13, the Q32 depth counts and sums against numpy, the resample labels (buffer 14) against
seg_cases.resample_labels -- and cf_seg_infer, which must leave the accumulators zero.  One context and one segmenter per shape serve
all cases of the shape, one after the other: every case also meets the state its predecessor left.  Stale state has a test of its
own (capture, flat, capture on one segmenter against fresh ones), and so has the launch of seg_resample_kernel for gy > 256 (32x4112,
with 32x4096 on the other side of the branch): crafted labels whose empty superpixels lie around k = 257, the sums and buffer 14 against
numpy, the means (buffer 5) against the oracle's staged entry, which accepts these shapes (tests/test_cpu_slic_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import orc_multi as om
import seg_cases as sc
import slic_cases as sl
from test_seg_stages_gpu import ACCUMULATORS, DCNT, DSUM, LOW_MEAN, SPC, _grab, _host, _same_bits
from test_segment_gpu import SegResult

pytestmark = pytest.mark.gpu

CENTRES, SLIC_SUMS, RESAMPLE = 12, 13, 14   # cf_seg_buffer (include/cofusion_hip.h)
IDS, NEXT_ID = [0], 3
_CTX = {}


def _context(w, h):
    """one context and one segmenter on it per image size for the whole module"""
    if (w, h) not in _CTX:
        from co_fusion_amd import api, synth
        cam = synth.Camera.scaled(w, h)
        ctx = api.Context(w, h, cam.fx, cam.fy, cam.cx, cam.cy)
        _CTX[w, h] = (ctx, _segmenter(ctx))
    return _CTX[w, h]


def _segmenter(ctx):
    seg = C.c_void_p()
    ctx._check(ctx.lib.cf_seg_create(ctx.h, C.byref(seg)))
    return seg


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for ctx, seg in _CTX.values():
        ctx.lib.cf_seg_destroy(seg)
        ctx.close()
    _CTX.clear()


def _dev(ctx, a):
    """a device copy of a (possibly read-only, shared) host array"""
    return ctx.to_device(np.array(a))


def _labels_view(ctx, seg, n_pixels):
    ptr = C.c_void_p(); nbytes = C.c_uint64()
    ctx._check(ctx.lib.cf_seg_labels(seg, C.byref(ptr), C.byref(nbytes)))
    assert ptr.value and nbytes.value == n_pixels * 4
    return ptr, nbytes


def _slic(ctx, seg, rgba):
    """cf_seg_slic on an image -> labels i32 [h][w], centres f32 [K][5], sums i64 [K][6] (one host wait)"""
    import torch
    h, w = rgba.shape[:2]
    K = (w // 16) * (h // 16)
    t = _dev(ctx, rgba)
    ctx._check(ctx.lib.cf_seg_slic(seg, C.c_void_p(t.data_ptr())))
    ptr, nbytes = _labels_view(ctx, seg, w * h)
    lab = torch.empty((h, w), dtype=torch.int32, device=ctx.device)
    ctx._check(ctx.lib.cf_memcpy_d2d_async(ctx.h, C.c_void_p(lab.data_ptr()), ptr, nbytes))
    centres, sums = _grab(ctx, seg, CENTRES, np.float32), _grab(ctx, seg, SLIC_SUMS, np.int64)
    ctx.synchronize()
    return dict(labels=lab.cpu().numpy(), centres=_host(centres).reshape(K, 5), sums=_host(sums).reshape(K, 6), rgba=t)


def _check_slic(name, got, what):
    want, _, trace = sl.reference(name)
    _same_bits(got["labels"], want, f"{name} [{what}]: labels against orc_slic")
    _same_bits(got["centres"], trace[-1].centres, f"{name} [{what}]: the centres of the fifth update (buffer 12)")
    _same_bits(got["sums"], trace[-1].sums, f"{name} [{what}]: the sums of the sixth pass (buffer 13)")


class _Chain:
    """the handoff's one model on the device, bound to a segmenter: cf_seg_sums -> the accumulators and buffer 14 -> cf_seg_infer"""

    def __init__(self, ctx, seg, w, h, rgba_dev):
        self.ctx, self.seg, self.lib, self.w, self.h, self.K = ctx, seg, ctx.lib, w, h, (w // 16) * (h // 16)
        depth, icp, conf = sl.handoff(w, h)
        self.rgba = rgba_dev
        self.depth, self.icp, self.vc = _dev(ctx, depth), _dev(ctx, icp), _dev(ctx, sl.vertconf(conf))
        self.full = ctx.to_device(np.zeros((h, w), np.uint8))
        self.icp_arr, self.vc_arr = (C.c_void_p * 1)(self.icp.data_ptr()), (C.c_void_p * 1)(self.vc.data_ptr())
        self.id_arr = (C.c_uint32 * 1)(*IDS)
        self.params = om.SegParams.defaults()

    def run(self):
        """-> the buffers between the sums and the inference, and behind the inference"""
        ctx, lib = self.ctx, self.lib
        s = C.c_void_p(); words = C.c_uint64()
        ctx._check(lib.cf_seg_sums(self.seg, C.c_void_p(self.depth.data_ptr()), 1, self.icp_arr, self.vc_arr, C.byref(s), C.byref(words)))
        between = {w: _grab(ctx, self.seg, w, dt) for w, dt in ACCUMULATORS + ((RESAMPLE, np.int32), (SLIC_SUMS, np.int64))}
        ctx._check(lib.cf_seg_infer(self.seg, C.byref(self.params), C.c_void_p(self.rgba.data_ptr()), 1, self.id_arr, C.c_uint32(NEXT_ID), 1,
                                    C.c_void_p(self.full.data_ptr())))
        res = SegResult()
        low = np.zeros(self.K, np.uint8)
        ctx._check(lib.cf_seg_fetch(self.seg, C.byref(res), low.ctypes.data_as(C.c_void_p)))
        behind = {w: _grab(ctx, self.seg, w, dt) for w, dt in ACCUMULATORS + ((LOW_MEAN, np.float32),)}
        ctx.synchronize()
        return {w: _host(g) for w, g in between.items()}, {w: _host(g) for w, g in behind.items()}


def _check_handoff(name, labels, depth, between, behind):
    """the sums over a label image against numpy, the resample labels, and clean accumulators behind the inference"""
    K = between[SPC].size
    spc, dcnt, dsum = sl.handoff_sums(labels, depth)
    _same_bits(between[SPC], spc, f"{name}: pixel counts against the labels' bincount")
    _same_bits(between[SLIC_SUMS].reshape(K, 6)[:, 5].astype(np.uint32), between[SPC], f"{name}: pixel counts against column 5 of buffer 13")
    _same_bits(between[DCNT], dcnt, f"{name}: depth counts")
    _same_bits(between[DSUM], dsum, f"{name}: Q32 depth sums")
    _same_bits(between[RESAMPLE], sc.resample_labels(labels)[0].astype(np.int32), f"{name}: resample labels (buffer 14)")
    for w, _ in ACCUMULATORS:
        assert not behind[w].any(), f"{name}: accumulator {w} is not clean behind the inference"


@pytest.mark.parametrize("name", sl.names())
def test_slic_and_its_handoff_on_a_crafted_image(name):
    c = sl.case(name)
    ctx, seg = _context(c.w, c.h)
    got = _slic(ctx, seg, sl.image(name))
    _check_slic(name, got, "the shape's segmenter")
    between, behind = _Chain(ctx, seg, c.w, c.h, got["rgba"]).run()
    _check_handoff(name, sl.reference(name)[0], sl.handoff(c.w, c.h)[0], between, behind)
    assert np.array_equal(between[SPC], np.bincount(got["labels"].ravel(), minlength=c.K))


def test_slic_does_not_see_the_previous_call():
    """capture, flat, capture on ONE segmenter: the sum buffer (which cf_seg_slic leaves filled) and the centres of the call before --
    among them capture's one-pixel clusters and its 2296-pixel one -- reach nothing; every result is that of a fresh segmenter"""
    ctx, _ = _context(48, 48)
    used = _segmenter(ctx)
    for step, name in enumerate(("capture-48x48", "flat-48x48", "capture-48x48")):
        fresh = _segmenter(ctx)
        a, b = _slic(ctx, used, sl.image(name)), _slic(ctx, fresh, sl.image(name))
        for k in ("labels", "centres", "sums"):
            _same_bits(a[k], b[k], f"step {step} ({name}): {k} of the used segmenter against a fresh one")
        _check_slic(name, a, f"step {step} on a used segmenter")
        ctx.lib.cf_seg_destroy(fresh)
    ctx.lib.cf_seg_destroy(used)


@pytest.mark.parametrize("shape", (sl.TALL, sl.TALL_TWIN), ids=lambda s: f"{s[0]}x{s[1]}")
def test_resample_labels_on_either_side_of_gy_256(shape):
    """gy = 257: enqueue_accumulate cannot carry the resample labels in its extra grid row and launches seg_resample_kernel; gy = 256: it
    still can.  Crafted labels over SLIC's own (superpixels in front of and behind k = 257 own no pixel, so their rows are replayed from
    buffer 14): the sums and buffer 14 against numpy, the means against the oracle's staged entry, twice on the shape's segmenter"""
    w, h = shape
    gx, gy, K = sc.grid_of(w, h)
    assert (gy > 256) == (shape == sl.TALL)
    ctx, seg = _context(w, h)
    name = f"noise-{w}x{h}"
    labels, depth = sl.crafted_labels(w, h), sl.handoff(w, h)[0]
    st = sl.crafted_reference(w, h)["stages"]
    lab_dev = _dev(ctx, labels)
    for rep in range(2):
        got = _slic(ctx, seg, sl.image(name))
        _check_slic(name, got, f"pass {rep}")
        ptr, nbytes = _labels_view(ctx, seg, w * h)
        ctx._check(ctx.lib.cf_memcpy_d2d_async(ctx.h, ptr, C.c_void_p(lab_dev.data_ptr()), nbytes))
        between, behind = _Chain(ctx, seg, w, h, got["rgba"]).run()
        what = f"crafted labels at {w}x{h}, pass {rep}"
        spc, dcnt, dsum = sl.handoff_sums(labels, depth)
        _same_bits(between[SPC], spc, f"{what}: pixel counts")
        _same_bits(between[DCNT], dcnt, f"{what}: depth counts")
        _same_bits(between[DSUM], dsum, f"{what}: Q32 depth sums")
        _same_bits(between[SPC], st["spc"], f"{what}: pixel counts against the oracle")
        _same_bits(between[DSUM], st["dsum"], f"{what}: Q32 depth sums against the oracle")
        assert sorted(np.flatnonzero(between[SPC] == 0).tolist()) == sl.crafted_empty(w, h)
        _same_bits(between[RESAMPLE], sc.resample_labels(labels)[0].astype(np.int32), f"{what}: resample labels (buffer 14)")
        low = behind[LOW_MEAN].reshape(3, K)
        _same_bits(low[0], st["lowDepth"], f"{what}: mean depths (empty superpixels replayed from buffer 14)")
        _same_bits(low[1:2], st["lowICP"], f"{what}: mean errors behind the weak-confidence substitution")
        _same_bits(low[2:3], st["lowConf"], f"{what}: mean confidences")
        for a, _ in ACCUMULATORS:
            assert not behind[a].any(), f"{what}: accumulator {a} is not clean behind the inference"
