"""The case table of the SLIC superpixel passes (plain helper module, no tests in here).

Every case is one RGBA image generated from a formula and a seed -- no files -- at one of the shapes below.  The GPU side
(tests/test_slic_gpu.py) sends it through cf_seg_slic, the production launches on their own (slic_init_kernel, six slic_assign_kernel,
five slic_update_kernel), and compares the labels with orc_slic and the centres and sums SLIC leaves behind (cf_seg_buffer 12, 13) with
the last pass of tests/slic_ref.py's trace, bit for bit; the CPU side (tests/test_cpu_slic_cases.py) shows from the two references
alone that slic_ref equals orc_slic label for label and that every case reaches what it `aims` at, read from the trace.

Shapes, width x height (K superpixels):
  16x16 (1)                 no neighbour exists: eight of the nine candidates are off the grid
  48x16, 16x48 (3)          one row, one column of cells: six candidates are off the grid for the end cells
  48x48 (9)                 every cell touches a border
  80x48 (15), 64x48 (12), 96x48 (18)
  80x80 (25)                one interior cell
  176x48 (33), 48x176 (33)
  4112x16 (257)             one lane in the second workgroup of the init and update grids (K % 256 == 1)
  32x4112 (514)             gy = 257: the superpixel sums cannot carry the resample labels in the accumulation launch's extra grid row
                            and launch seg_resample_kernel (the only shape in the suite that does); 32x4096 (gy = 256) is its twin on
                            the other side of the branch

The cases, and what the trace shows for them (the figures are slic_ref's; the CPU test asserts the PROPERTY, e.g. `> 0`):
 * flat: a constant colour, at every shape with K > 1.  Pass 1 is decided by position alone and the pixels of column / row 16 c are as
   far from centre c - 1 as from centre c: 32 ties at 48x16, 188 at 48x48, 344 at 80x48, 812 at 176x48, 4096 at 4112x16.  The strict `<`
   gives them to the first centre in the scan; a `<=` gives other labels (asserted with slic_ref's `last` switch).  A dx-major scan does
   NOT: two centres of one row or column and the four around a cell corner come in the same order in both scans.  Only a tie between
   a centre above and one beside it separates them, and that needs colour: capture-80x80, extreme-80x80 and both mirror cases have one
   (asserted with the `order` switch).  At 32x4112 the ties stay in every pass.
 * stripes8: vertical 0 / 255 stripes of period 16 (the centre pixels are white).  At 80x48 three clusters, at 80x80 five are empty from
   the third pass on and stay at the reset centre (0, 0), colour 0, from where they go on competing (the reset value is in buffer 12).
   At 176x48 and 4112x16 none is empty; the first pass ties like flat's and clusters grow to 408 / 384 pixels.
 * hstripes8: the transpose, at 48x176.
 * capture: grey 90 with every centre pixel but the middle cell's at 255.  At 48x48 the middle cluster holds 2296 of the 2304 pixels in
   every pass -- all nine cells, the most the 3x3 search allows, through all nine LDS slots of every workgroup -- and the eight others
   their own centre pixel, with the centre exactly on it.  At 80x80 the middle cluster cannot reach the outer ring, which ties 345 times
   in pass 1 and 10 times in pass 2: a tie behind an update (blocks8-48x48 and flat-32x4112 have the others of the table).
 * centre_dots: the 80x80 image inverted (grey 165, every centre pixel 0): every initial centre colour is an outlier of its cell; the
   centres agree with each other, so pass 1 ties like flat's.
 * checker16: cells alternate 0 and 255.  Ties at the cell corners only (the diagonal neighbour has the cell's colour), and every cluster
   ends with exactly its own 256 pixels.
 * extreme: random 0 / 255 per channel in 4x4 blocks: the largest colour residuals (3 * 255^2) and colour sums 8 bits can give.
 * noise: uniform noise, the baseline, from 16x16 to the two tall shapes.
 * blocks8: random 0 / 255 greys in 8x8 blocks, at the seeds `search_empty` found (48x48: 8, 80x48: 18, 80x80: 43).  Clusters lose all
   their pixels in pass 2, are reset to centre (0, 0), colour 0 -- and one of them WINS PIXELS AGAIN from there in a later pass (cluster
   0 at 48x48, cluster 5 at the other two, which is not the corner's own), while others stay empty to the end: the reset value decides
   labels here, not only buffer 12.  At 48x48 the ties go on through pass 3 (80, 25, 3).
 * mirror: left-right symmetric noise of four levels per channel at 64x48 and 96x48: equal colours at different centres (ties in
   pass 1, some of them between a centre above and one beside the pixel) under content whose symmetry the grid does not share (the
   centres sit at 16 c + 8, their mirror images at 16 c + 7).

Every label image obeys seg_cases.invariant_3x3 and every sum stays below 2^24 (exact in f32, oracle/orc_segment.c:23-25).

The handoff to the chain (`handoff`): one model, a depth that is constant over each 16x16 cell (1 + (k * 5 % 8) / 64, every fifth cell a
hole of zeros), constant error 1/8 and confidence 1/2 -- the pixel counts, the Q32 depth counts and sums over SLIC's labels have a plain
numpy statement (`handoff_sums`).  `crafted_labels`: the regular grid at the tall shapes with superpixels in front of and behind
k = 257 (250, 255, 256, 258, 261, 400 and the last one) given to a neighbour, so that their rows are replayed from buffer 14.

NOT COVERED, so that nobody takes the table for complete: a pixel with no candidate under the start value 999999.9999f (it would keep
its own cell: the distances of 8-bit colours on a grid this size stay below a few hundred); image sizes that are no multiple of 16
(cf_seg_create refuses them; the oracle clamps the cell); a cluster larger than 2296 pixels (all nine cells less the eight centre
pixels that keep the other clusters alive).
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import orc_multi as om
import seg_cases as sc
import slic_ref

SEED = 16180
SPIX = 16
F = np.float32
TALL, TALL_TWIN = (32, 4112), (32, 4096)

FLAT_SHAPES = ((48, 16), (16, 48), (48, 48), (80, 48), (80, 80), (176, 48), (4112, 16), TALL)
TABLE = (
    ("flat", FLAT_SHAPES, "ties in pass 1 that the scan order alone decides"),
    ("stripes8", ((80, 48), (80, 80)), "clusters without a pixel from the third pass on, left at the reset centre"),
    ("stripes8", ((176, 48), (4112, 16)), "first-pass ties and growing clusters, no empty cluster"),
    ("hstripes8", ((48, 176),), "the transpose of stripes8: ties along rows"),
    ("capture", ((48, 48),), "one cluster of 2296 pixels over all nine cells, eight clusters of one pixel"),
    ("capture", ((80, 80),), "ties in pass 1 AND in pass 2 (behind an update)"),
    ("centre_dots", ((80, 80),), "every centre pixel an outlier of its cell; ties like flat"),
    ("checker16", ((48, 48), (80, 80), (176, 48)), "ties at cell corners only; every cluster keeps exactly its 256 pixels"),
    ("extreme", ((80, 80), (176, 48)), "the largest colour residuals and colour sums"),
    ("noise", ((16, 16), (48, 16), (16, 48), (80, 48), (176, 48), (4112, 16), TALL, TALL_TWIN), "the baseline; K = 1, 257, 514 and gy = 256 / 257"),
    ("blocks8", ((48, 48), (80, 48), (80, 80)), "clusters emptied in pass 2, one revived from the reset centre, others empty to the end"),
    ("mirror", ((64, 48), (96, 48)), "equal colours at different centres under symmetric content"),
)


@dataclasses.dataclass(frozen=True)
class Case:
    content: str
    w: int
    h: int
    aims: str

    @property
    def name(self):
        return f"{self.content}-{self.w}x{self.h}"

    @property
    def K(self):
        return (self.w // SPIX) * (self.h // SPIX)


def _rgba(rgb):
    rgb = np.asarray(rgb)
    if rgb.ndim == 2:
        rgb = np.repeat(rgb[..., None], 3, -1)
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = rgb
    return out


def _capture(w, h):
    g = np.full((h, w), 90, np.uint8)
    gx, gy = w // SPIX, h // SPIX
    for cy in range(gy):
        for cx in range(gx):
            if (cx, cy) != (gx // 2, gy // 2):
                g[cy * SPIX + 8, cx * SPIX + 8] = 255
    return g


BLOCK_SEEDS = {(48, 48): 8, (80, 48): 18, (80, 80): 43}   # found by search_empty


def _block_image(w, h, bw, bh, seed):
    rng = np.random.default_rng([SEED, 99, w, h, bw, bh, seed])
    b = rng.integers(0, 2, size=(h // bh, w // bw)) * 255
    return _rgba(np.repeat(np.repeat(b, bh, 0), bw, 1))


def make_image(content, w, h):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    gx, gy = w // SPIX, h // SPIX
    rng = np.random.default_rng([SEED, sorted(c for c, _, _ in TABLE).index(content), w, h])
    if content == "flat":
        img = np.empty((h, w, 3), np.uint8); img[:] = (100, 150, 200)
        return _rgba(img)
    if content == "stripes8":
        return _rgba(((x // 8) % 2) * 255)
    if content == "hstripes8":
        return _rgba(((y // 8) % 2) * 255)
    if content == "capture":
        return _rgba(_capture(w, h))
    if content == "centre_dots":
        g = 255 - _capture(w, h)
        g[(gy // 2) * SPIX + 8, (gx // 2) * SPIX + 8] = 0
        return _rgba(g)
    if content == "checker16":
        return _rgba(((x // SPIX + y // SPIX) % 2) * 255)
    if content == "extreme":
        b = rng.integers(0, 2, size=(h // 4, w // 4, 3)) * 255
        return _rgba(np.repeat(np.repeat(b, 4, 0), 4, 1))
    if content == "blocks8":
        return _block_image(w, h, 8, 8, BLOCK_SEEDS[w, h])
    if content == "noise":
        return _rgba(rng.integers(0, 256, size=(h, w, 3)))
    if content == "mirror":
        half = rng.integers(0, 4, size=(h, w // 2, 3)) * 85
        return _rgba(np.concatenate([half, half[:, ::-1]], 1))
    raise KeyError(content)


@functools.lru_cache(maxsize=None)
def cases():
    out = tuple(Case(content, w, h, aims) for content, shapes, aims in TABLE for w, h in shapes)
    assert len({c.name for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


def names():
    return [c.name for c in cases()]


@functools.lru_cache(maxsize=None)
def image(name):
    c = case(name)
    img = np.ascontiguousarray(make_image(c.content, c.w, c.h))
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(name):
    """(orc_slic's labels, slic_ref's labels, slic_ref's trace) of a case: computed once, shared by the tests, read-only"""
    img = image(name)
    orc_labels = om.slic(img)
    labels, trace = slic_ref.slic(img)
    for a in [orc_labels, labels] + [p.centres for p in trace] + [p.sums for p in trace]:
        a.setflags(write=False)
    return orc_labels, labels, tuple(trace)


# ------------------------------------------------------------------------------------------------------------ the handoff to the chain
@functools.lru_cache(maxsize=None)
def handoff(w, h):
    """(depth, icp error, confidence) images [h][w] f32 of the one model the handoff runs with; read-only"""
    K = (w // SPIX) * (h // SPIX)
    ks = np.arange(K)
    sp_depth = np.where(ks % 5 == 2, 0.0, 1.0 + (ks * 5 % 8) / 64.0).astype(F)
    depth = sc.block(sp_depth, w, h)
    icp, conf = np.full((h, w), 0.125, F), np.full((h, w), 0.5, F)
    for a in (depth, icp, conf):
        a.setflags(write=False)
    return depth, icp, conf


def vertconf(conf):
    v = np.zeros(conf.shape + (4,), F)
    v[..., 0] = 7.0; v[..., 1] = -3.0; v[..., 2] = 2.0; v[..., 3] = conf
    return v


def handoff_sums(labels, depth):
    """pixel counts u32 [K], depth counts u32 [K] and Q32 depth sums i64 [K] over a label image (the depths have no bit under 2^-32)"""
    h, w = labels.shape
    K = (w // SPIX) * (h // SPIX)
    lab = labels.ravel()
    q = depth.astype(np.float64).ravel() * 4294967296.0
    assert np.all(q == np.rint(q)) and np.all(np.isfinite(q))
    valid = depth.ravel() > F(0.02)
    spc = np.bincount(lab, minlength=K).astype(np.uint32)
    dcnt = np.bincount(lab[valid], minlength=K).astype(np.uint32)
    dsum = np.zeros(K, np.int64)
    np.add.at(dsum, lab[valid], q.astype(np.int64)[valid])
    return spc, dcnt, dsum


GIVEN = ((250, 251), (255, 253), (256, 254), (258, 260), (261, 263), (400, 401))


@functools.lru_cache(maxsize=None)
def crafted_labels(w, h):
    """the regular grid at a tall shape, with superpixels in front of and behind k = 257 (and the last one) given to a 3x3 neighbour"""
    K = (w // SPIX) * (h // SPIX)
    labels = sc.grid_labels(w, h)
    for k, to in GIVEN + ((K - 1, K - 3),):
        labels[labels == k] = to
    labels.setflags(write=False)
    return labels


def crafted_empty(w, h):
    K = (w // SPIX) * (h // SPIX)
    return sorted([k for k, _ in GIVEN] + [K - 1])


@functools.lru_cache(maxsize=None)
def crafted_reference(w, h):
    """the oracle's staged entry on the noise image of the shape with the crafted labels and the handoff's model"""
    depth, icp, conf = handoff(w, h)
    ref = om.segment_crf_stages(om.SegParams.defaults(), image(f"noise-{w}x{h}"), depth, [0], [icp], [vertconf(conf)], 3, True,
                                labels_in=crafted_labels(w, h))
    for a in ref["stages"].values():
        a.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------- the search for another empty cluster
def search_empty(seeds=120, shapes=((48, 48), (80, 48), (80, 80)), blocks=((8, 8), (4, 4))):
    """The seed search behind blocks8: [(shape, block, seed, empty clusters per pass, revived)] of the random 0 / 255 block images that
    leave a cluster without a pixel; revived: a cluster that was empty behind one pass owns pixels behind the next"""
    found = []
    for w, h in shapes:
        for bw, bh in blocks:
            for seed in range(seeds):
                img = _block_image(w, h, bw, bh, seed)
                if np.unique(om.slic(img)).size == (w // SPIX) * (h // SPIX):
                    continue
                gone = [set(np.flatnonzero(p.sums[:, 5] == 0).tolist()) for p in slic_ref.slic(img)[1]]
                found.append(((w, h), (bw, bh), seed, [len(g) for g in gone], any(a - b for a, b in zip(gone, gone[1:]))))
    return found
