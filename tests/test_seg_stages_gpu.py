"""GPU parity of the CRF segmentation chain STAGE BY STAGE, on the crafted label images and values of tests/seg_cases.py: every buffer the
chain holds between its stages (cf_seg_buffer: the Q32 sums and counts, the means after the weak-confidence substitution, the depth
range, the average confidences, the unaries, the appearance features, the marginals, the label map) against the oracle's staged entry
(orc_segment_crf_stages with the same labels), bit for bit -- the chain's own contract ("same arithmetic, same summation order"), no
tolerance --, and behind them the arg-max, the low-resolution map, the full mask and the decision rows.  Every case runs through the
plain chain (cf_seg_sums + cf_seg_infer), the split chain (cf_seg_early, then the late half) and cf_seg_run_batch beside other cases
of its shape whose label counts differ; every path twice on the same segmenter (the accumulators must be clean again).  Cases whose
unaries are not finite (a depth range of 0) are compared through the unary stage only, NaN equal to NaN.  The mean field has a table of
its own: cf_seg_crf against orc_crf_meanfield."""
import ctypes as C
import warnings

import numpy as np
import pytest

import seg_cases as sc
from test_segment_gpu import SegJob, SegResult, _compare

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

# cf_seg_buffer (include/cofusion_hip.h)
SPC, DCNT, DSUM, ICP_SUM, CONF_SUM, LOW_MEAN, UNARY, FEAT2, AVG_CONF, DEPTH_RANGE, LOW_MAP, MARGINALS = range(12)
ACCUMULATORS = ((SPC, np.uint32), (DCNT, np.uint32), (DSUM, np.int64), (ICP_SUM, np.int64), (CONF_SUM, np.int64))
_CTX = {}


def _context(w, h):
    """one context per image size for the whole module"""
    if (w, h) not in _CTX:
        from co_fusion_amd import api, synth
        cam = synth.Camera.scaled(w, h)
        _CTX[w, h] = api.Context(w, h, cam.fx, cam.fy, cam.cx, cam.cy, max_models=48)
    return _CTX[w, h]


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for ctx in _CTX.values():
        ctx.close()
    _CTX.clear()


def _segmenter(ctx):
    seg = C.c_void_p()
    ctx._check(ctx.lib.cf_seg_create(ctx.h, C.byref(seg)))
    return seg


def _grab(ctx, seg, which, dtype):
    """a copy of one of the segmenter's buffers, enqueued on the context's stream (valid after ctx.synchronize())"""
    import torch
    ptr = C.c_void_p(); nbytes = C.c_uint64()
    ctx._check(ctx.lib.cf_seg_buffer(seg, which, C.byref(ptr), C.byref(nbytes)))
    assert ptr.value and nbytes.value % np.dtype(dtype).itemsize == 0, (which, nbytes.value)
    out = torch.empty(nbytes.value, dtype=torch.uint8, device=ctx.device)
    ctx._check(ctx.lib.cf_memcpy_d2d_async(ctx.h, C.c_void_p(out.data_ptr()), ptr, C.c_uint64(nbytes.value)))
    return out, dtype


def _host(grabbed):
    t, dtype = grabbed
    return t.cpu().numpy().view(dtype)


class _Dev:
    """a case's inputs on the device, bound to one segmenter"""

    def __init__(self, ctx, case, seg):
        self.ctx, self.case, self.seg, self.lib = ctx, case, seg, ctx.lib
        n = case.n
        self.rgba, self.depth = ctx.to_device(case.rgba), ctx.to_device(case.depth)
        self.icp = [ctx.to_device(a) for a in case.icp]
        self.vc = [ctx.to_device(a) for a in case.vertconf()]
        self.labels = ctx.to_device(case.labels)
        self.full = ctx.to_device(np.zeros((case.h, case.w), np.uint8))
        self.icp_arr = (C.c_void_p * n)(*[t.data_ptr() for t in self.icp])
        self.vc_arr = (C.c_void_p * n)(*[t.data_ptr() for t in self.vc])
        self.id_arr = (C.c_uint32 * n)(*case.ids)
        self.params = case.params.__class__.from_buffer_copy(case.params)

    def labels_in(self):
        """SLIC, then the crafted labels over its own (the chain's entry for labels that SLIC did not make)"""
        ctx = self.ctx
        ctx._check(self.lib.cf_seg_slic(self.seg, C.c_void_p(self.rgba.data_ptr())))
        ptr = C.c_void_p(); nbytes = C.c_uint64()
        ctx._check(self.lib.cf_seg_labels(self.seg, C.byref(ptr), C.byref(nbytes)))
        assert nbytes.value == self.labels.numel() * 4
        ctx._check(self.lib.cf_memcpy_d2d_async(ctx.h, ptr, C.c_void_p(self.labels.data_ptr()), nbytes))

    def early(self):
        self.ctx._check(self.lib.cf_seg_early(self.seg, C.c_void_p(self.depth.data_ptr()), C.c_void_p(self.rgba.data_ptr()), self.case.n, self.vc_arr,
                                              C.byref(self.params)))

    def sums(self):
        s = C.c_void_p(); w = C.c_uint64()
        self.ctx._check(self.lib.cf_seg_sums(self.seg, C.c_void_p(self.depth.data_ptr()), self.case.n, self.icp_arr, self.vc_arr, C.byref(s), C.byref(w)))

    def infer(self):
        c = self.case
        self.ctx._check(self.lib.cf_seg_infer(self.seg, C.byref(self.params), C.c_void_p(self.rgba.data_ptr()), c.n, self.id_arr, C.c_uint32(c.next_id),
                                              int(c.allow_new), C.c_void_p(self.full.data_ptr())))

    def job(self):
        c = self.case
        return SegJob(self.seg.value, self.depth.data_ptr(), c.n, C.cast(self.icp_arr, C.c_void_p).value, C.cast(self.vc_arr, C.c_void_p).value,
                      self.rgba.data_ptr(), C.cast(self.id_arr, C.c_void_p).value, c.next_id, int(c.allow_new), self.full.data_ptr())

    def grab(self, whiches):
        return {w: _grab(self.ctx, self.seg, w, dt) for w, dt in whiches}

    def collect(self, sums):
        """behind the inference: the decisions, the stage buffers, and the accumulators as the chain left them"""
        res = SegResult()
        low = np.zeros(self.case.K, np.uint8)
        self.ctx._check(self.lib.cf_seg_fetch(self.seg, C.byref(res), low.ctypes.data_as(C.c_void_p)))
        late = self.grab(((LOW_MEAN, np.float32), (UNARY, np.float32), (FEAT2, np.float32), (AVG_CONF, np.float32), (DEPTH_RANGE, np.float32),
                          (LOW_MAP, np.uint8), (MARGINALS, np.float32)))
        after = self.grab(ACCUMULATORS)
        self.ctx.synchronize()
        return dict(res=res, low=low, full=self.full.cpu().numpy(), sums={w: _host(g) for w, g in sums.items()},
                    late={w: _host(g) for w, g in late.items()}, after={w: _host(g) for w, g in after.items()})


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    if got.dtype == np.float32:
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got != want
    if bad.any():
        at = np.argwhere(bad)[0]
        assert False, f"{what}: {np.count_nonzero(bad)} of {bad.size} entries differ, first at {tuple(at)}: {got[tuple(at)]!r} against {want[tuple(at)]!r}"


def _check(case, got, path):
    ref = sc.reference(case.name)
    st, K, n, L = ref["stages"], case.K, case.n, case.L
    s = got["sums"]
    if SPC in s:
        _same_bits(s[SPC], st["spc"], f"{case.name} [{path}]: pixel counts")
    if DCNT in s:
        _same_bits(s[DCNT], st["dcnt"], f"{case.name} [{path}]: depth counts")
        _same_bits(s[DSUM], st["dsum"], f"{case.name} [{path}]: depth sums")
    if ICP_SUM in s:
        rows = s[ICP_SUM].reshape(-1, K)
        _same_bits(rows[:n], st["icp_sum"], f"{case.name} [{path}]: ICP-error sums")
        assert not rows[n:].any(), f"{case.name} [{path}]: ICP-error sums behind the last model"
    if CONF_SUM in s:
        rows = s[CONF_SUM].reshape(-1, K)
        _same_bits(rows[:n], st["conf_sum"], f"{case.name} [{path}]: confidence sums")
        assert not rows[n:].any(), f"{case.name} [{path}]: confidence sums behind the last model"
    for w, a in got["after"].items():
        assert not a.any(), f"{case.name} [{path}]: accumulator {w} is not clean behind the inference"
    late = got["late"]
    low = late[LOW_MEAN].reshape(1 + 2 * n, K)
    _same_bits(low[0], st["lowDepth"], f"{case.name} [{path}]: mean depths")
    _same_bits(low[1 + n:], st["lowConf"], f"{case.name} [{path}]: mean confidences (non-finite entries zeroed)")
    _same_bits(late[DEPTH_RANGE], st["depthRange"], f"{case.name} [{path}]: depth range")
    _same_bits(late[AVG_CONF], st["avgConfidence"], f"{case.name} [{path}]: average confidences")
    _same_bits(low[1:1 + n], st["lowICP"], f"{case.name} [{path}]: mean errors behind the weak-confidence substitution")
    _same_bits(late[FEAT2].reshape(K, 6), st["feat2"], f"{case.name} [{path}]: appearance features")
    _same_bits(late[UNARY].reshape(K, L), st["unary"], f"{case.name} [{path}]: unaries")
    if case.nonfinite:
        return
    Q = late[MARGINALS].reshape(K, L)
    _same_bits(Q, st["Q"], f"{case.name} [{path}]: marginals")
    ids = np.array(case.ids + ([case.next_id] if case.allow_new else []), np.uint8)
    _same_bits(ids[np.argmax(Q, 1)], st["argmax"], f"{case.name} [{path}]: arg-max (first maximum)")
    _same_bits(late[LOW_MAP], ref["low"].ravel(), f"{case.name} [{path}]: low-resolution map on the device")
    gy = case.h // 16
    _compare(f"{case.name} [{path}]", got["res"], got["low"].reshape(gy, K // gy), got["full"], ref)


@pytest.mark.parametrize("name", sc.names())
def test_plain_and_split_chain_stage_by_stage(name):
    case = sc.case(name)
    ctx = _context(case.w, case.h)
    seg = _segmenter(ctx)
    dev = _Dev(ctx, case, seg)
    for rep in range(2):
        dev.labels_in(); dev.sums()
        sums = dev.grab(ACCUMULATORS)
        dev.infer()
        _check(case, dev.collect(sums), f"plain chain, pass {rep}")
    for rep in range(2):
        dev.labels_in(); dev.early(); dev.sums()
        sums = dev.grab(((SPC, np.uint32), (ICP_SUM, np.int64)))   # (the early half consumed the others)
        dev.infer()
        _check(case, dev.collect(sums), f"split chain, pass {rep}")
    dev.labels_in(); dev.sums()
    sums = dev.grab(ACCUMULATORS)
    dev.infer()
    _check(case, dev.collect(sums), "plain chain behind the split one")
    ctx.lib.cf_seg_destroy(seg)


@pytest.mark.parametrize("batch", sc.batches(), ids=lambda b: f"{b[0]}+{len(b) - 1}")
def test_batched_chain_stage_by_stage(batch):
    cases = [sc.case(x) for x in batch]
    assert len({c.L for c in cases}) >= 2 and len({c.group() for c in cases}) == 1
    ctx = _context(cases[0].w, cases[0].h)
    ctx.lib.cf_seg_run_batch.restype = C.c_int
    ctx.lib.cf_seg_run_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    devs = [_Dev(ctx, c, _segmenter(ctx)) for c in cases]
    jobs = (SegJob * len(devs))(*[d.job() for d in devs])
    for rep in range(2):
        for d in devs:
            d.labels_in()
        ctx._check(ctx.lib.cf_seg_run_batch(ctx.h, C.byref(devs[0].params), C.cast(jobs, C.c_void_p), len(devs)))
        for d in devs:
            _check(d.case, d.collect({}), f"batch of {len(devs)}, pass {rep}")
    for d in devs:
        ctx.lib.cf_seg_destroy(d.seg)


@pytest.mark.parametrize("mf", sc.MF_CASES, ids=lambda m: m.name)
def test_mean_field_against_the_oracle(mf):
    """cf_seg_crf on its own: the marginals it returns, and the buffer cf_seg_buffer names as the last inference's (Q0 or Q1 by the
    parity of the steps), against orc_crf_meanfield"""
    w, h = sc.SHAPES[mf.K]
    ctx = _context(w, h)
    seg = _segmenter(ctx)
    unary, f1, f2 = mf.inputs()
    want = sc.mf_reference(mf)
    for rep in range(2):
        Q = np.full((mf.K, mf.L), -1.0, np.float32)
        ctx._check(ctx.lib.cf_seg_crf(seg, unary.ctypes.data_as(C.c_void_p), mf.L, f1.ctypes.data_as(C.c_void_p), f2.ctypes.data_as(C.c_void_p),
                                      C.c_float(mf.w_smooth), C.c_float(mf.w_app), mf.iterations, Q.ctypes.data_as(C.c_void_p)))
        _same_bits(Q, want, f"{mf.name}: marginals (pass {rep})")
        g = _grab(ctx, seg, MARGINALS, np.float32)
        ctx.synchronize()
        _same_bits(_host(g).reshape(mf.K, mf.L), want, f"{mf.name}: the marginals' buffer (pass {rep})")
    ctx.lib.cf_seg_destroy(seg)
