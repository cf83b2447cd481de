"""The case table of the CRF segmentation chain (plain helper module, no tests in here).

Every case is one frame's worth of inputs of Segmentation::performSegmentationCRF -- colour, depth, the models' ICP error surfaces and
confidence projections -- TOGETHER WITH ITS LABEL IMAGE: SLIC is skipped on both sides (the oracle's staged entry takes `labels_in`,
the device gets a copy over the cf_seg_labels pointer behind cf_seg_slic), so that every sum, mean, unary and marginal between the
inputs and the decisions has a known place and, where the images are constant over each superpixel, a known value.  The CPU side
(tests/test_cpu_seg_cases.py) shows with the oracle alone that each case reaches what it `aims` at; the GPU side
(tests/test_seg_stages_gpu.py) compares every stage buffer of the device chain (cf_seg_buffer) with the oracle's, bit for bit.

Three families:
  values      the regular 16x16 grid as labels; the VALUES are crafted (thresholds of the confidence rules, non-finite pixels, the sign and
              the clamp of the Q32 sums, their rounding, the floors of the unaries, the depth range, the label counts)
  labels      label images built from the regular grid under the precondition of seg_accumulate_kernel -- a pixel's label is one of the
              3x3 cells around the pixel's own cell (`invariant_3x3`) --: superpixels without a pixel, without a depth sample, with
              nine cells, ragged borders
  mean field  cf_seg_crf against orc_crf_meanfield on its own (`MF_CASES`): node counts below / off the sixteen chunks, label counts
              on both sides of the sixteen-label kernels, the Q0 / Q1 parity of 0, 1, 2 and 10 steps, each weight zero in turn

Exactness.  A block-constant value v enters a superpixel's Q32 sum as 256 * round(v * 2^32); every crafted value below is a float with
no bit under 2^-32 (v >= 2^-9, or a multiple of 2^-32), so the sum is 256 * v * 2^32 exactly, its f32 image 256 v and the mean v: the
`sp_*` arrays of a case ARE the expected means, bit for bit.

The replay of the empty superpixels.  A superpixel without a pixel (or, for the depth row, without a depth sample) takes the entry of
the label at its resample pixel, divided by that label's pixel count: already a mean when the label lies in front of it in index
order, still a raw sum when behind.  A label that is read owns the pixel it was read at, so its count is never zero, and a pixel-empty
superpixel never reads itself.  A depth-empty one can (the regular grid on a square image): its entry is then the raw sum 0 on either
side of the comparison, so `read < k` and `read <= k` are the same function -- the cases pin the order through reads in front of and
behind the superpixel, not through that tie.

Non-finite unaries.  With a depth range of 0 the unaries divide by zero; the order in which max / compare steps meet a NaN is not part
of the chain's statement, so such cases (`Case.nonfinite`, at most a quarter of the table) are compared through the unary stage only,
NaN equal to NaN.  Every other case is compared to the end.

Shapes: 48x48 (K = 9: fewer nodes than CRF chunks, every cell touches a border), 48x80 (K = 15, portrait: gx < gy), 176x144 (K = 99, no
multiple of 16), 320x240 (K = 300, gx > gy: the resample row (k / gy) * 16 + 8 runs past the image and is clamped) and, for the second
half of the unary kernel's lanes alone, 640x480 (K = 1200 > 1024).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np

import orc
import orc_multi as om

SEED = 4711
SPIX = 16
F = np.float32
SHAPES = {9: (48, 48), 15: (48, 80), 99: (176, 144), 300: (320, 240), 1200: (640, 480)}


def prev32(x):
    return np.nextafter(F(x), F(-np.inf), dtype=F)


def next32(x):
    return np.nextafter(F(x), F(np.inf), dtype=F)


def grid_of(w, h):
    return w // SPIX, h // SPIX, (w // SPIX) * (h // SPIX)


def grid_labels(w, h):
    gx, _, _ = grid_of(w, h)
    return ((np.arange(h)[:, None] // SPIX) * gx + np.arange(w)[None, :] // SPIX).astype(np.int32)


def block(values, w, h):
    """[K] per-superpixel values -> [h, w] image constant over each 16x16 cell"""
    gx, gy, _ = grid_of(w, h)
    return np.ascontiguousarray(np.repeat(np.repeat(np.asarray(values, F).reshape(gy, gx), SPIX, 0), SPIX, 1))


def invariant_3x3(labels):
    """the precondition of seg_accumulate_kernel: every pixel's label is one of the 3x3 cells around the pixel's own cell"""
    h, w = labels.shape
    gx, gy, K = grid_of(w, h)
    if labels.min() < 0 or labels.max() >= K:
        return False
    cx, cy = np.arange(w)[None, :] // SPIX, np.arange(h)[:, None] // SPIX
    return bool(np.all(np.abs(labels % gx - cx) <= 1) and np.all(np.abs(labels // gx - cy) <= 1))


def resample_labels(labels):
    """the label an empty superpixel k reads (Slic.h:192-206, k / gy sic); also whether k's row was clamped"""
    h, w = labels.shape
    gx, gy, K = grid_of(w, h)
    ks = np.arange(K)
    xs, ys = (ks % gx) * SPIX + SPIX // 2, (ks // gy) * SPIX + SPIX // 2
    return labels[np.minimum(ys, h - 1), np.minimum(xs, w - 1)], ys >= h


@dataclasses.dataclass
class Case:
    name: str
    family: str
    aims: str
    w: int
    h: int
    ids: list
    next_id: int
    allow_new: bool
    rgba: np.ndarray
    depth: np.ndarray
    icp: list
    conf: list
    labels: np.ndarray
    params: om.SegParams
    nonfinite: bool = False          # a non-finite value reaches the unaries: compared through the unary stage only
    sp_depth: np.ndarray = None      # [K] the crafted per-superpixel values where the image is block-constant and exact (else None)
    sp_icp: list = None              # [n][K]
    sp_conf: list = None             # [n][K]
    expect: dict = dataclasses.field(default_factory=dict)   # what the CPU test looks for (see tests/test_cpu_seg_cases.py)

    @property
    def n(self):
        return len(self.ids)

    @property
    def L(self):
        return self.n + (1 if self.allow_new else 0)

    @property
    def K(self):
        return grid_of(self.w, self.h)[2]

    def vertconf(self):
        """the splat vertexConf textures: channel 3 is the confidence, the others are never read by the segmentation"""
        out = []
        for c in self.conf:
            v = np.zeros((self.h, self.w, 4), F)
            v[..., 0] = 7.0; v[..., 1] = -3.0; v[..., 2] = 2.0; v[..., 3] = c
            out.append(v)
        return out

    def group(self):
        """cases of one group can share a cf_seg_run_batch call: one shape, one parameter set"""
        return (self.w, self.h, bytes(self.params))


def _base(name, aims, K, n=2, allow_new=True, family="values", seed=0):
    """The plain scene every case starts from: regular labels, noise colours, depths 1 .. 1.109 in steps of 1/64, every model owning a
    share of the superpixels (error 2^-8 there, 1/8 + m/64 elsewhere), every seventh superpixel explained by nobody (error 1/4: the new
    label's), confidences 1."""
    w, h = SHAPES[K]
    rng = np.random.default_rng([SEED, seed, K])
    rgba = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8); rgba[..., 3] = 255
    ks = np.arange(K)
    sp_depth = (1.0 + (ks * 5 % 8) / 64.0).astype(F)
    owner = (ks * 7 // 3) % n
    nobody = ks % 7 == 3
    sp_icp = [np.where(nobody, 0.25, np.where(owner == m, 2.0 ** -8, 0.125 + (m % 8) / 64.0)).astype(F) for m in range(n)]
    sp_conf = [np.ones(K, F) for _ in range(n)]
    ids = [0] + list(range(3, 3 + n - 1))
    return Case(name=name, family=family, aims=aims, w=w, h=h, ids=ids, next_id=3 + n - 1, allow_new=allow_new, rgba=rgba,
                depth=block(sp_depth, w, h), icp=[block(e, w, h) for e in sp_icp], conf=[block(c, w, h) for c in sp_conf],
                labels=grid_labels(w, h), params=om.SegParams.defaults(), sp_depth=sp_depth, sp_icp=sp_icp, sp_conf=sp_conf)


def _set_sp(c, what, m, values):
    """replace a block-constant image of the case by other per-superpixel values"""
    values = np.asarray(values, F)
    if what == "depth":
        c.sp_depth = values; c.depth = block(values, c.w, c.h)
    else:
        getattr(c, "sp_" + what)[m] = values
        getattr(c, what)[m] = block(values, c.w, c.h)


def _cell(c, k):
    """the pixel slices of grid cell k"""
    gx = grid_of(c.w, c.h)[0]
    return slice((k // gx) * SPIX, (k // gx + 1) * SPIX), slice((k % gx) * SPIX, (k % gx + 1) * SPIX)


# ---------------------------------------------------------------------------------------------------------------- family "values"
def _values_cases():
    out = []
    nan, inf = F(np.nan), F(np.inf)

    # -- confidence thresholds: (double)conf < 0.3 for model 0, (double)conf <= 0.4 for the others; 0.3f and 0.4f lie ABOVE 0.3 and 0.4
    for K, n in ((9, 2), (15, 3)):
        c = _base(f"conf-thresholds-K{K}", "block-constant confidences at prev(t), t, next(t) of both rules' thresholds: only prev(t) is weak "
                  "(a comparison with 0.4f in f32 would also take 0.4f itself)", K, n=n, seed=1)
        t0 = np.array([prev32(0.3), F(0.3), next32(0.3)], F)
        t1 = np.array([prev32(0.4), F(0.4), next32(0.4)], F)
        ks = np.arange(K)
        _set_sp(c, "conf", 0, t0[ks % 3])
        for m in range(1, n):
            _set_sp(c, "conf", m, t1[(ks + m) % 3])
        c.expect["weak"] = [ks % 3 == 0] + [(ks + m) % 3 == 0 for m in range(1, n)]
        out.append(c)

    # -- non-finite pixels inside ICP surfaces and confidence images: nothing to the sum, one to the divisor
    c = _base("nonfinite-pixels", "NaN, +inf and -inf pixels in ICP surfaces and confidence images add nothing to the Q32 sums and count "
              "in the divisor", 9, n=2, seed=2)
    rng = np.random.default_rng([SEED, 2])
    bad = {}
    for what, imgs in (("icp", c.icp), ("conf", c.conf)):
        for m in range(c.n):
            at = rng.random((c.h, c.w)) < 0.1
            imgs[m][at] = rng.choice(np.array([nan, inf, -inf], F), size=int(at.sum()))
            bad[what, m] = at
    c.expect["bad_pixels"] = bad     # sums = (256 - bad pixels of the cell) * q32(value); the sp_* arrays are the GOOD pixels' values
    out.append(c)

    c = _base("conf-all-nan", "a superpixel whose confidences are all NaN: sum 0, mean 0, weak for both rules", 9, n=2, seed=3)
    for m in range(c.n):
        c.conf[m][_cell(c, 4 + m)] = nan
        c.sp_conf[m][4 + m] = 0.0
    c.expect["weak"] = [np.arange(9) == 4, np.arange(9) == 5]
    out.append(c)

    c = _base("depth-nonfinite-and-threshold", "depth NaN (not counted), +inf (counted, adds 0), exactly 0.02f (not counted: the test is >) "
              "and next(0.02f) (counted)", 9, n=2, seed=4)
    c.sp_depth = None
    c.depth[_cell(c, 0)][::2, :] = nan            # half the cell: 128 samples left
    c.depth[_cell(c, 1)][:, ::4] = inf            # a quarter of the cell adds nothing and counts
    c.depth[_cell(c, 2)] = F(0.02)                # not one valid sample: depth-empty
    c.depth[_cell(c, 3)] = next32(0.02)           # all valid
    c.depth[_cell(c, 5)][3:9, 2:7] = F(0.02)      # 30 samples out
    c.expect["dcnt"] = {0: 128, 1: 256, 2: 0, 3: 256, 5: 226}
    out.append(c)

    # -- sign and clamp of the Q32 sums
    c = _base("icp-negative", "negative ICP errors: the 64-bit sums go negative (two's complement through the unsigned atomics), the "
              "unaries fall under the 1e-5 floor", 9, n=2, seed=5)
    _set_sp(c, "icp", 0, -c.sp_icp[0])
    _set_sp(c, "icp", 1, np.where(np.arange(9) % 2 == 0, -c.sp_icp[1], c.sp_icp[1]))
    c.expect["negative_sums"] = True
    out.append(c)

    c = _base("icp-clamped", "ICP errors beyond +-2^20 are clamped: 256 pixels of +-2^20 * 2^32 per superpixel, |sum| = 2^60 < 2^62", 9, n=2, seed=6)
    big = np.array([2.0 ** 21, -2.0 ** 21, 1e30, -1e30, 2.0 ** 20, 3.0e38, -3.0e38, 2.0 ** 20 + 0.125, -(2.0 ** 20)], F)
    _set_sp(c, "icp", 0, big)
    c.sp_icp[0] = np.clip(big, F(-2.0 ** 20), F(2.0 ** 20))
    _set_sp(c, "conf", 1, np.where(np.arange(9) % 2 == 0, 2.0 ** 25, 1.0))
    c.sp_conf[1] = np.minimum(c.sp_conf[1], F(2.0 ** 20))
    c.expect["clamped"] = True
    out.append(c)

    # -- rounding of q32
    c = _base("q32-random", "per-pixel random values over 1e-7 .. 1e3 in ICP surfaces, confidences and depth: the rounding to Q32 of "
              "every magnitude, sums of 256 different terms", 99, n=3, seed=7)
    rng = np.random.default_rng([SEED, 7])
    for m in range(c.n):
        c.icp[m] = np.exp(rng.uniform(np.log(1e-7), np.log(1e3), size=(c.h, c.w))).astype(F)
        c.conf[m] = np.exp(rng.uniform(np.log(1e-7), np.log(1e3), size=(c.h, c.w))).astype(F)
    c.depth = np.exp(rng.uniform(np.log(1e-3), np.log(90.0), size=(c.h, c.w))).astype(F)
    c.sp_depth = c.sp_icp = c.sp_conf = None
    out.append(c)

    c = _base("q32-ties", "2^-33 (0.5 in Q32: a tie, to even = 0), 3 * 2^-34 (0.75: up), 3 * 2^-33 (1.5: a tie, to even = 2), 5 * 2^-33 "
              "(2.5: a tie, to even = 2)", 9, n=2, seed=8)
    tie = np.array([2.0 ** -33, 3 * 2.0 ** -34, 3 * 2.0 ** -33, 5 * 2.0 ** -33], F)
    q = np.array([0, 1, 2, 2], np.int64)
    pat = (np.arange(c.h)[:, None] * 3 + np.arange(c.w)[None, :]) % 4
    c.icp[0] = tie[pat]
    c.conf[1] = tie[(pat + 1) % 4]
    c.sp_icp = c.sp_conf = None
    lab = c.labels.ravel()
    c.expect["sums"] = {("icp", 0): np.bincount(lab, q[pat].ravel(), 9).astype(np.int64),
                        ("conf", 1): np.bincount(lab, q[(pat + 1) % 4].ravel(), 9).astype(np.int64)}
    out.append(c)

    # -- floors of the unaries
    c = _base("floor-1e-5", "zero ICP error: the unary 0 is raised to 1e-5", 9, n=2, seed=9)
    _set_sp(c, "icp", 0, np.where(np.arange(9) % 2 == 0, 0.0, c.sp_icp[0]))
    _set_sp(c, "icp", 1, np.where(np.arange(9) % 3 == 0, 0.0, c.sp_icp[1]))
    c.expect["floor_1e-5"] = True
    out.append(c)

    c = _base("floor-0.01", "every model's error high: unaryThresholdNew - w * lowest < 0.01, the new label's unary sits on the 0.01 floor "
              "(and above it elsewhere)", 9, n=2, seed=10)
    c.expect["floor_0.01"] = True     # (the base scene's `nobody` superpixels: error 1/4 over a range of 7/64)
    out.append(c)

    # -- depth range
    c = _base("depth-above-100", "mean depths above MAX_DEPTH = 100 are left out of the range; the depth feature is clamped at 100", 9, n=2, seed=11)
    d = c.sp_depth.copy(); d[2] = 150.0; d[6] = 100.5; d[7] = 100.0
    _set_sp(c, "depth", 0, d)
    c.expect["range"] = float(F(100.0) - F(1.0))   # (100 itself is inside: the test is >)
    out.append(c)

    c = _base("depth-range-zero", "all depths equal: the range is 0, every error is divided by zero", 9, n=2, seed=12)
    _set_sp(c, "depth", 0, np.full(9, 1.5, F))
    c.nonfinite = True
    c.expect["range"] = 0.0
    out.append(c)

    c = _base("depth-all-invalid", "no valid depth sample at all: every superpixel is depth-empty, every mean depth 0, the range 0", 15, n=2, seed=13)
    _set_sp(c, "depth", 0, np.zeros(15, F))
    c.nonfinite = True
    c.expect["range"] = 0.0
    out.append(c)

    # -- label counts
    for n, new, why in ((1, False, "L = 1: one model, no new label"), (1, True, "L = 2: one model and the new label"),
                        (16, False, "L = 16: the last count of the sixteen-label kernels and of a batch"),
                        (16, True, "L = 17: sixteen models in ONE accumulation tile, the large-table post-processing"),
                        (17, False, "n = 17: two accumulation tiles, the device pointer table")):
        c = _base(f"labels-n{n}-{'new' if new else 'nonew'}", why, 9, n=n, allow_new=new, seed=20 + n)
        rng = np.random.default_rng([SEED, 20, n])
        for m in range(n):   # distinct confidences per model and superpixel, so that a row or tile mix-up shows in the means
            _set_sp(c, "conf", m, (0.5 + rng.integers(0, 256, 9) / 512.0).astype(F))
        out.append(c)

    # -- K = 1200 > the unary kernel's 1024 lanes: superpixels 1024 .. 1199 are the k0 + T half
    c = _base("wide-new-label", "K = 1200: the second half of the unary kernel's lanes (k >= 1024) with weak confidences and the new "
              "label's unary, distinct per superpixel", 1200, n=2, allow_new=True, seed=30)
    ks = np.arange(1200)
    _set_sp(c, "icp", 0, (2.0 ** -8 * (1 + ks % 61)).astype(F))
    _set_sp(c, "icp", 1, (2.0 ** -8 * (1 + ks % 53)).astype(F))
    _set_sp(c, "conf", 0, np.where(ks % 5 == 0, prev32(0.3), next32(0.3)))
    _set_sp(c, "conf", 1, np.where(ks % 3 == 0, prev32(0.4), F(0.4)))
    c.expect["weak"] = [ks % 5 == 0, ks % 3 == 0]
    out.append(c)
    c = _base("wide-four-models", "K = 1200 without a new label (L = 4): the batch partner of the case above", 1200, n=4, allow_new=False, seed=31)
    out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------- family "labels"
def _give(labels, k, to):
    """superpixel k gives all pixels it still owns to superpixel `to`"""
    labels[labels == k] = to


def _vary(c, seed):
    """per-pixel varying values in every image (exact means are not known any more; the sums are exact integers on both sides)"""
    rng = np.random.default_rng([SEED, seed])
    c.depth = rng.uniform(0.5, 4.0, size=(c.h, c.w)).astype(F)
    for m in range(c.n):
        c.icp[m] = rng.uniform(0.0, 0.3, size=(c.h, c.w)).astype(F)
        c.conf[m] = rng.uniform(0.2, 1.0, size=(c.h, c.w)).astype(F)
    c.sp_depth = c.sp_icp = c.sp_conf = None


def _labels_cases():
    out = []

    def start(name, aims, K, seed, n=2):
        c = _base(name, aims, K, n=n, family="labels", seed=seed)
        _vary(c, seed)
        return c

    c = start("empty-read-smaller-K9", "square grid: superpixels give their cell to the LEFT neighbour, so the resample label k - 1 < k is "
              "already divided when it is read", 9, 40)
    for k in (1, 5, 8):
        _give(c.labels, k, k - 1)
    c.expect["pixel_empty"] = [1, 5, 8]; c.expect["read"] = "smaller"
    out.append(c)

    c = start("empty-read-smaller-K15", "portrait (gx < gy): the resample row k / gy lies ABOVE the superpixel's own, the label read there "
              "is smaller than k; no row is clamped", 15, 41)
    for k, to in ((7, 8), (11, 10), (14, 13)):
        _give(c.labels, k, to)
    c.expect["pixel_empty"] = [7, 11, 14]; c.expect["read"] = "smaller"; c.expect["row_clamped"] = False
    out.append(c)

    c = start("empty-read-larger-K9", "square grid: superpixels give their cell to the RIGHT or LOWER neighbour, the resample label > k is "
              "still a raw sum when it is read", 9, 42)
    for k, to in ((0, 1), (3, 6), (7, 8)):
        _give(c.labels, k, to)
    c.expect["pixel_empty"] = [0, 3, 7]; c.expect["read"] = "larger"
    out.append(c)

    c = start("empty-read-larger-K300", "gx > gy: the resample row (k / gy) * 16 + 8 lies BELOW the superpixel's own (label read > k) and, "
              "from k = 225 on, past the image: clamped to the last row", 300, 43, n=3)
    for k, to in ((21, 22), (130, 110), (226, 227), (250, 249), (285, 286), (299, 298)):
        _give(c.labels, k, to)
    c.expect["pixel_empty"] = [21, 130, 226, 250, 285, 299]; c.expect["read"] = "both"; c.expect["row_clamped"] = True
    out.append(c)

    c = start("empty-chain-K99", "depth-empty superpixels whose resample label is itself depth-empty and larger (gx > gy: the row read lies "
              "below), some of them pixel-empty as well", 99, 44)
    for k, to in ((12, 13), (40, 39), (70, 81)):
        _give(c.labels, k, to)
    holes = [12, 13, 14, 23, 24, 25, 34, 35, 36, 39, 40, 41, 50, 51, 52, 70, 81, 92]
    for k in holes:
        c.depth[_cell(c, k)] = 0.0
    c.expect["pixel_empty"] = [12, 40, 70]; c.expect["depth_chain"] = "larger"; c.expect["both_empty"] = [12, 40, 70]
    out.append(c)

    c = start("both-empty-K15", "superpixels that own neither a pixel nor a depth sample, next to depth holes; a depth-empty superpixel whose "
              "resample label is itself depth-empty and smaller (gx < gy: the row read lies above)", 15, 45)
    for k, to in ((4, 3), (9, 12)):
        _give(c.labels, k, to)
    for k in (3, 4, 9, 10):
        c.depth[_cell(c, k)] = 0.0
    c.expect["pixel_empty"] = [4, 9]; c.expect["both_empty"] = [4, 9]; c.expect["depth_chain"] = "smaller"
    out.append(c)

    c = start("owns-nine-K9", "the centre superpixel owns all nine cells: 2304 pixels through all nine LDS slots, eight pixel-empty "
              "superpixels that all read it", 9, 46)
    c.labels[:] = 4
    c.expect["pixel_empty"] = [0, 1, 2, 3, 5, 6, 7, 8]; c.expect["owner_pixels"] = 2304; c.expect["read"] = "both"
    out.append(c)

    c = start("owns-nine-K99", "an inner superpixel owns its 3x3 cells at a ragged superpixel count", 99, 47)
    gx = 11
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            c.labels[_cell(c, 49 + dy * gx + dx)] = 49
    c.expect["pixel_empty"] = sorted(49 + dy * gx + dx for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    c.expect["owner_pixels"] = 2304; c.expect["read"] = "both"
    out.append(c)

    for K, seed in ((99, 48), (300, 49)):
        c = start(f"ragged-borders-K{K}", "every pixel within four pixels of a cell border picks one of the 3x3 cells around its own at random: "
                  "all nine slots of every workgroup, sums of many small shares", K, seed, n=3 if K == 99 else 2)
        rng = np.random.default_rng([SEED, seed, 1])
        gx, gy, _ = grid_of(c.w, c.h)
        yy, xx = np.mgrid[0:c.h, 0:c.w]
        near = (np.minimum(xx % SPIX, SPIX - 1 - xx % SPIX) < 4) | (np.minimum(yy % SPIX, SPIX - 1 - yy % SPIX) < 4)
        cx = np.clip(xx // SPIX + rng.integers(-1, 2, size=xx.shape), 0, gx - 1)
        cy = np.clip(yy // SPIX + rng.integers(-1, 2, size=xx.shape), 0, gy - 1)
        c.labels = np.where(near, cy * gx + cx, c.labels).astype(np.int32)
        c.expect["ragged"] = True
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _values_cases() + _labels_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def names(family=None):
    return [c.name for c in cases() if family is None or c.family == family]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's result and stages of a case (computed once, shared by the tests; treat as read-only)"""
    c = case(name)
    ref = om.segment_crf_stages(c.params, c.rgba, c.depth, c.ids, c.icp, c.vertconf(), c.next_id, c.allow_new, labels_in=c.labels)
    for a in ref["stages"].values():
        a.setflags(write=False)
    return ref


def batches():
    """the cf_seg_run_batch calls of the GPU test: per shape and parameter set ONE call with all its cases of up to sixteen labels (the
    batched launches, eight segmenters each; their label counts differ) and, where the group has cases with more, one call with those
    and one of the others (the per-segmenter fallback)"""
    groups = {}
    for c in cases():
        groups.setdefault(c.group(), []).append(c)
    out = []
    for g in groups.values():
        small, big = [c.name for c in g if c.L <= 16], [c.name for c in g if c.L > 16]
        if len(small) > 1:
            out.append(tuple(small))
        if big:
            out.append(tuple(big + small[:1]))
    return out


# ------------------------------------------------------------------------------------------------------------ family "mean field"
@dataclasses.dataclass(frozen=True)
class MFCase:
    K: int
    L: int
    iterations: int
    w_smooth: float
    w_app: float
    aims: str

    @property
    def name(self):
        return f"mf-K{self.K}-L{self.L}-it{self.iterations}-w{self.w_smooth:g}-{self.w_app:g}"

    def inputs(self):
        """unaries as the chain forms them (>= 1e-5, a few on the floor), the grid's smoothness features, appearance features in the
        ranges of the chain's (positions / 1.8, colours / 10, depths / 0.9)"""
        w, h = SHAPES[self.K]
        gx = w // SPIX
        rng = np.random.default_rng([SEED, 60, self.K, self.L, self.iterations])
        unary = rng.uniform(0.0, 6.0, size=(self.K, self.L)).astype(F)
        unary[rng.random(unary.shape) < 0.1] = F(1e-5)
        ks = np.arange(self.K)
        f1 = np.stack([(ks % gx).astype(F) / F(2.0), (ks // gx).astype(F) / F(2.0)], -1).astype(F)
        f2 = np.concatenate([np.stack([(ks % gx).astype(F), (ks // gx).astype(F)], -1) / F(1.8), rng.integers(0, 256, size=(self.K, 3)).astype(F) * F(0.1),
                             rng.uniform(0.5, 4.0, size=(self.K, 1)).astype(F)], -1).astype(F)
        return np.ascontiguousarray(unary), np.ascontiguousarray(f1), np.ascontiguousarray(f2)


# every K, L, iteration count and weight setting at least once; 0 and 1 iterations (marginals in Q0 / in Q1) with small and with large L
MF_CASES = (
    MFCase(9, 1, 0, 2.0, 7.0, "fewer nodes than chunks, one label, no step: the first marginals (all 1) in Q0"),
    MFCase(9, 17, 1, 2.0, 7.0, "fewer nodes than chunks, L > 16, one step: the marginals are in Q1"),
    MFCase(9, 16, 10, 2.0, 7.0, "fewer nodes than chunks, the last label count of the sixteen-label update"),
    MFCase(15, 2, 1, 2.0, 7.0, "K = 15 (one empty chunk), one step with small L: Q1"),
    MFCase(15, 40, 0, 2.0, 7.0, "no step with large L: Q0"),
    MFCase(99, 16, 2, 0.0, 7.0, "K no multiple of 16, the smoothness weight zero"),
    MFCase(99, 17, 10, 2.0, 0.0, "K no multiple of 16, L = 17 (the 32-slot update), the appearance weight zero"),
    MFCase(99, 1, 1, 2.0, 7.0, "one label, one step"),
    MFCase(300, 2, 10, 2.0, 7.0, "K = 300 (chunks of 19, the 5-wide and 1-wide tails of the message loop)"),
    MFCase(300, 40, 2, 2.0, 7.0, "K = 300, L = 40 (the 64-slot update), two steps: back in Q0"),
)


@functools.lru_cache(maxsize=None)
def mf_reference(mf):
    unary, f1, f2 = mf.inputs()
    Q = np.zeros((mf.K, mf.L), F)
    orc.lib.orc_crf_meanfield(orc.P(unary), mf.L, mf.K, orc.P(f1), orc.P(f2), C.c_float(mf.w_smooth), C.c_float(mf.w_app), mf.iterations, orc.P(Q))
    Q.setflags(write=False)
    return Q
