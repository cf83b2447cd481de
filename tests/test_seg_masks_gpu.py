"""GPU parity of the label-mask branch as kernels (cf_seg_masks -> cf_seg_fetch -> cf_seg_new_mask_value, csrc/segment_masks.hip)
against the oracle's orc_segment_gt on the case table of tests/mask_cases.py: the label image byte for byte, the spawn decision, every
row's id, superPixelCount and the BIT PATTERNS of avgConfidence, depthMean and depthStd (sequential f32 sums in raster order: the order
cases of the table cannot be met by a kernel that re-associates them), and the mask value that was bound to the new label."""
import ctypes as C

import numpy as np
import pytest

import mask_cases as mc
import orc_multi as om

pytestmark = pytest.mark.gpu

CASES = mc.build()
CF_EINVAL, CF_ESTATE = -1, -4


class SegModel(C.Structure):
    _fields_ = [("id", C.c_uint32), ("superPixelCount", C.c_uint32), ("avgConfidence", C.c_float), ("depthMean", C.c_float),
                ("depthStd", C.c_float), ("top", C.c_int32), ("right", C.c_int32), ("bottom", C.c_int32), ("left", C.c_int32)]


class SegResult(C.Structure):
    _fields_ = [("has_new_label", C.c_int32), ("n_models", C.c_int32), ("depth_range", C.c_float), ("model", SegModel * 256)]


class MaskJob(C.Structure):
    _fields_ = [("seg", C.c_void_p), ("mask_dev", C.c_void_p), ("depth_dev", C.c_void_p), ("n_models", C.c_int32), ("model_ids", C.c_void_p),
                ("next_model_id", C.c_uint32), ("allow_new", C.c_int32), ("mapping", C.c_void_p), ("full_dev", C.c_void_p)]


_REFS = {}


def ref(case):  # the oracle's result of a case, computed once and shared by the tests of this module
    if case["name"] not in _REFS:
        mapping = case["mapping"].copy()
        r = om.segment_gt(case["mask"], case["depth"], case["ids"], case["next_id"], case["allow_new"], mapping)
        new = np.flatnonzero(mapping != case["mapping"])
        r["new_value"] = int(new[0]) if len(new) else -1
        r["rows"] = mc.parse_expected_rows(r)
        _REFS[case["name"]] = r
    return _REFS[case["name"]]


class Box:
    """a context of one image size with its segmenters (created on demand, destroyed with the module)"""

    def __init__(self, w, h):
        from co_fusion_amd import api, synth
        cam = synth.Camera.scaled(w, h)
        self.w, self.h = w, h
        self.ctx = api.Context(w, h, cam.fx, cam.fy, cam.cx, cam.cy, max_models=8)
        self.lib = self.ctx.lib
        self.lib.cf_seg_masks.argtypes = [C.c_void_p]
        self.lib.cf_seg_masks_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self.lib.cf_seg_new_mask_value.argtypes = [C.c_void_p, C.c_void_p]
        self.segs = []

    def segmenter(self, k):
        while len(self.segs) <= k:
            seg = C.c_void_p()
            # a height that is no multiple of 16 has no superpixel grid: the segmenter of the mask branch alone
            create = self.lib.cf_seg_create if self.h % 16 == 0 else self.lib.cf_seg_create_masks
            self.ctx._check(create(self.ctx.h, C.byref(seg)))
            self.segs.append(seg)
        return self.segs[k]

    def job(self, seg, case):
        """(MaskJob, what must stay alive, the label image tensor)"""
        d = self.ctx.to_device
        t_mask, t_depth = d(case["mask"]), d(case["depth"])
        t_full = d(np.full((self.h, self.w), 0xAB, np.uint8))   # (every byte must be written)
        ids = (C.c_uint32 * len(case["ids"]))(*case["ids"])
        mapping = case["mapping"].copy()
        j = MaskJob(seg.value, t_mask.data_ptr(), t_depth.data_ptr(), len(case["ids"]), C.cast(ids, C.c_void_p).value, case["next_id"],
                    case["allow_new"], mapping.ctypes.data, t_full.data_ptr())
        return j, (t_mask, t_depth, ids, mapping), t_full

    def fetch(self, seg):
        res = SegResult()
        self.ctx._check(self.lib.cf_seg_fetch(seg, C.byref(res), None))
        value = C.c_int(-7)
        self.ctx._check(self.lib.cf_seg_new_mask_value(seg, C.byref(value)))
        return res, value.value

    def close(self):
        for s in self.segs:
            self.lib.cf_seg_destroy(s)
        self.ctx.close()


@pytest.fixture(scope="module")
def boxes():
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = Box(w, h)
        return made[(w, h)]
    yield get
    for b in made.values():
        b.close()


def compare(what, case, res, value, full):
    r = ref(case)
    assert np.array_equal(full, r["full"]), f"{what}: label image differs at {np.argwhere(full != r['full'])[:4].tolist()}"
    assert bool(res.has_new_label) == r["hasNewLabel"], what
    assert res.n_models == len(r["rows"]), what
    assert res.depth_range == 0, what
    bits = lambda x: int(np.float32(x).view(np.uint32))
    for i, want in enumerate(r["rows"]):
        m = res.model[i]
        got = (m.id, m.superPixelCount, bits(m.avgConfidence), bits(m.depthMean), bits(m.depthStd))
        assert got == want, f"{what}: row {i}: {got} != {want} (depthMean {m.depthMean!r} / {r['modelData'][i]['depthMean']!r})"
        assert (m.top, m.right, m.bottom, m.left) == (0, 0, 0, 0), what
    assert value == r["new_value"], what


def run_single(box, seg, case):
    j, keep, t_full = box.job(seg, case)
    box.ctx._check(box.lib.cf_seg_masks(C.byref(j)))
    res, value = box.fetch(seg)
    return res, value, t_full.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_mask_case_matches_the_oracle(boxes, case):
    box = boxes(case["w"], case["h"])
    res, value, full = run_single(box, box.segmenter(0), case)
    compare(case["name"], case, res, value, full)


def test_one_segmenter_keeps_no_state_between_jobs(boxes):
    """different cases back to back on ONE segmenter, twice round: a spawn followed by none, many rows followed by few, and each of
    the segmenter's two work blocks meets every case"""
    for w, h in mc.SIZES:
        box = boxes(w, h)
        seg = box.segmenter(0)
        cases = [c for c in CASES if (c["w"], c["h"]) == (w, h)]
        for c in cases + cases[::-1] + cases[:1]:
            res, value, full = run_single(box, seg, c)
            compare(f"{c['name']} (in sequence)", c, res, value, full)


def _batch(box, cases):
    jobs, keep, fulls = (MaskJob * len(cases))(), [], []
    for k, c in enumerate(cases):
        j, alive, t_full = box.job(box.segmenter(k), c)
        jobs[k] = j; keep.append(alive); fulls.append(t_full)
    box.ctx._check(box.lib.cf_seg_masks_batch(box.ctx.h, jobs, len(cases)))
    for k, c in enumerate(cases):
        res, value = box.fetch(box.segmenter(k))
        compare(f"{c['name']} (job {k} of {len(cases)})", c, res, value, fulls[k].cpu().numpy())


def test_batched_jobs_equal_the_single_calls(boxes):
    """cf_seg_masks_batch with 8 (one chunk) and 9 (two chunks) mixed cases -- spawning and not, 1 to 4 rows -- and, at 80 x 36, a batch
    that holds a job with more ids than a batched launch carries (one chain per job)"""
    w, h = mc.SIZES[0]
    small = [c for c in CASES if (c["w"], c["h"]) == (w, h)]
    assert len(small) >= 9 and {c["allow_new"] for c in small[:8]} == {0, 1}
    _batch(boxes(w, h), small[:8])
    _batch(boxes(w, h), small[-9:])
    w, h = mc.SIZES[1]
    ragged = [c for c in CASES if (c["w"], c["h"]) == (w, h)]
    assert any(len(c["ids"]) > 17 for c in ragged)
    _batch(boxes(w, h), ragged)
    _batch(boxes(w, h), [c for c in ragged if len(c["ids"]) <= 17])


def test_error_returns(boxes):
    w, h = mc.SIZES[0]
    box = boxes(w, h)
    lib = box.lib
    case = CASES[0]
    fresh = C.c_void_p()
    box.ctx._check(lib.cf_seg_create(box.ctx.h, C.byref(fresh)))
    value = C.c_int(0)
    try:
        assert lib.cf_seg_new_mask_value(fresh, C.byref(value)) == CF_ESTATE          # nothing fetched yet
        assert lib.cf_seg_new_mask_value(None, C.byref(value)) == CF_EINVAL and lib.cf_seg_new_mask_value(fresh, None) == CF_EINVAL
        assert lib.cf_seg_masks(None) == CF_EINVAL
        assert lib.cf_seg_masks_batch(box.ctx.h, None, 1) == CF_EINVAL and lib.cf_seg_masks_batch(None, None, 0) == CF_EINVAL
        good, keep, _ = box.job(fresh, case)
        assert lib.cf_seg_masks_batch(box.ctx.h, C.byref(good), 0) == CF_EINVAL
        for field, bad in (("seg", None), ("mask_dev", None), ("depth_dev", None), ("model_ids", None), ("mapping", None), ("full_dev", None),
                           ("n_models", 0), ("n_models", 256), ("mask_dev", good.mask_dev + 1), ("depth_dev", good.depth_dev + 4),
                           ("full_dev", good.full_dev + 8), ("full_dev", good.mask_dev)):
            j = MaskJob.from_buffer_copy(good)
            setattr(j, field, bad)
            assert lib.cf_seg_masks(C.byref(j)) == CF_EINVAL, (field, bad)
            if field != "seg":
                assert lib.cf_seg_masks_batch(box.ctx.h, C.byref(j), 1) == CF_EINVAL, (field, bad)
        two = (MaskJob * 2)(good, good)                                                # one segmenter twice in a batch
        assert lib.cf_seg_masks_batch(box.ctx.h, two, 2) == CF_EINVAL
        assert lib.cf_seg_new_mask_value(fresh, C.byref(value)) == CF_ESTATE          # the refused calls enqueued nothing
        box.ctx._check(lib.cf_seg_masks(C.byref(good)))
        assert lib.cf_seg_new_mask_value(fresh, C.byref(value)) == CF_ESTATE          # enqueued, not fetched
        res, v = box.fetch(fresh)
        assert v == ref(case)["new_value"] and res.n_models == len(ref(case)["rows"])
    finally:
        lib.cf_seg_destroy(fresh)
    if h % 16 == 0:   # the segmenter of the mask branch alone refuses the motion branch
        only = C.c_void_p()
        box.ctx._check(lib.cf_seg_create_masks(box.ctx.h, C.byref(only)))
        try:
            rgba = box.ctx.to_device(np.zeros((h, w, 4), np.uint8))
            assert lib.cf_seg_slic(only, C.c_void_p(rgba.data_ptr())) == CF_EINVAL
            res, value, full = run_single(box, only, CASES[0])
            compare("mask-only segmenter", CASES[0], res, value, full)
        finally:
            lib.cf_seg_destroy(only)
