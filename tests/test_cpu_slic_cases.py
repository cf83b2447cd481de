"""The case table of the SLIC passes (tests/slic_cases.py) on the references alone: tests/slic_ref.py, the numpy restatement with a
trace, equals orc_slic label for label on every case; every case reaches what it aims at, read from the trace -- first-pass ties that
the scan order decides, ties behind an update, clusters without a pixel at the reset centre, the 2296-pixel cluster over nine cells,
K = 257 and 514 --; every label image obeys the 3x3 precondition of the accumulation kernel; and the oracle's staged entry accepts the
tall shapes with the crafted labels whose empty superpixels lie on both sides of k = 257."""
import numpy as np
import pytest

import seg_cases as sc
import slic_cases as sl
import slic_ref

F = np.float32
DX_MAJOR = tuple((dy, dx) for dx in (-1, 0, 1) for dy in (-1, 0, 1))


def test_the_table_has_the_shapes_and_contents_it_names():
    by = {}
    for c in sl.cases():
        by.setdefault(c.content, set()).add((c.w, c.h))
        assert c.aims and c.w % 16 == 0 and c.h % 16 == 0
    assert by["flat"] == set(sl.FLAT_SHAPES) and all(w * h > 256 for w, h in by["flat"])
    assert {(80, 48), (80, 80), (176, 48), (4112, 16)} <= by["stripes8"] and by["hstripes8"] == {(48, 176)}
    assert by["capture"] == {(48, 48), (80, 80)} and by["mirror"] == {(64, 48), (96, 48)}
    assert {(16, 16), (4112, 16), sl.TALL, sl.TALL_TWIN} <= by["noise"]
    Ks = {c.K for c in sl.cases()}
    assert {1, 3, 9, 15, 25, 33, 257, 514} <= Ks
    assert 257 % 256 == 1 and (257 + 255) // 256 == 2                       # one lane in the second workgroup of the init / update grids
    assert sl.TALL[1] // 16 == 257 and sl.TALL_TWIN[1] // 16 == 256           # gy on either side of the resample launch's branch


@pytest.mark.parametrize("name", sl.names())
def test_case_reaches_what_it_aims_at(name):
    c = sl.case(name)
    img = sl.image(name)
    want, labels, tr = sl.reference(name)
    K, gx, gy = c.K, c.w // 16, c.h // 16
    assert img.shape == (c.h, c.w, 4) and img.dtype == np.uint8
    assert np.array_equal(labels, want), f"slic_ref differs from orc_slic in {np.count_nonzero(labels != want)} pixels"
    assert sc.invariant_3x3(want), "a pixel's label lies outside the 3x3 cells around its own"
    assert len(tr) == 6
    for it, p in enumerate(tr):
        assert p.centres.shape == (K, 5) and p.centres.dtype == F and p.sums.shape == (K, 6) and p.sums.dtype == np.int64
        assert p.sums[:, 5].sum() == c.w * c.h and p.sums.max() < 2 ** 24 and p.sums.min() >= 0, "a sum leaves what f32 holds exactly"
        assert p.largest <= 9 * 256 and p.largest == p.sums[:, 5].max() and p.empty == np.count_nonzero(p.sums[:, 5] == 0)
        if it:   # the update: (float)sum / (float)count, zeros for a cluster without a pixel
            prev = tr[it - 1].sums
            has = prev[:, 5] > 0
            assert np.array_equal(p.centres[has], (prev[has, :5].astype(F) / prev[has, 5].astype(F)[:, None])) and not p.centres[~has].any()
    assert np.array_equal(tr[0].centres, slic_ref.initial_centres(img))
    assert np.array_equal(tr[-1].sums[:, 5], np.bincount(want.ravel(), minlength=K))
    ties, empty, largest = [p.ties for p in tr], [p.empty for p in tr], [p.largest for p in tr]
    last = tr[-1]

    def order_matters(dx_major=False):
        """the labels under a `<=` (the last minimum) differ from the statement's; with dx_major, those of a dx-major scan do too.  (Two
        centres in one row or one column, and the four around a cell corner, come in the same order in both scans: only a tie between a
        centre above and one to the side of it -- which needs colour -- tells the scans apart.)"""
        assert not np.array_equal(slic_ref.slic(img, last=True)[0], want), "a `<=` in the assignment gives the same labels"
        if dx_major:
            assert not np.array_equal(slic_ref.slic(img, order=DX_MAJOR)[0], want), "a dx-major scan gives the same labels"

    if c.content == "flat":
        assert len(np.unique(img.reshape(-1, 4), axis=0)) == 1
        assert ties[0] > 0 and empty == [0] * 6
        if gx > 1:   # the pixels of column 16 c are as far from centre c - 1 as from centre c: a tie in every row at least
            assert ties[0] >= (gx - 1) * c.h
        order_matters()
    elif c.content in ("stripes8", "hstripes8"):
        assert set(np.unique(img[..., :3])) == {0, 255} and np.all(tr[0].centres[:, 2:] == 255)
        assert ties[0] > 0 and max(largest) > 256
        if (c.w, c.h) in ((80, 48), (80, 80)):
            assert empty[:2] == [0, 0] and all(e > 0 for e in empty[2:]), empty
            gone = tr[2].sums[:, 5] == 0
            for p in tr[3:]:   # left at the reset centre, from where they compete and win nothing
                assert not p.centres[gone].any() and not p.sums[gone].any()
            assert K - np.unique(want).size == empty[-1]
        else:
            assert empty == [0] * 6
        order_matters()
    elif c.content == "capture":
        mid = (gy // 2) * gx + gx // 2
        outer = np.arange(K) != mid
        assert np.all(tr[0].centres[outer, 2:] == 255) and np.all(tr[0].centres[mid, 2:] == 90)
        if (c.w, c.h) == (48, 48):
            assert all(x >= 2296 for x in largest) and 2296 == 9 * 256 - 8
            for p in tr:
                assert p.sums[mid, 5] >= 2296 and np.all(p.sums[outer, 5] == 1)
                assert np.array_equal(p.centres[outer], tr[0].centres[outer]), "a one-pixel cluster's centre left its pixel"
            assert np.all(want[img[..., 0] == 90] == mid)
        else:
            assert ties[0] > 0 and ties[1] > 0, ties
            order_matters(dx_major=True)
    elif c.content == "centre_dots":
        assert np.all(tr[0].centres[:, 2:] == 0) and np.count_nonzero(img[..., 0] == 0) == K and np.count_nonzero(img[..., 0] == 165) == c.w * c.h - K
        assert ties[0] > 0
        order_matters()
    elif c.content == "checker16":
        assert ties[0] > 0 and ties[0] <= 4 * (gx - 1) * (gy - 1), "ties away from the cell corners"
        assert np.all(last.sums[:, 5] == 256) and np.array_equal(want, sc.grid_labels(c.w, c.h))
    elif c.content == "extreme":
        assert set(np.unique(img[..., :3])) == {0, 255}
        rgb = img[..., :3].reshape(-1, 3)
        assert np.any(np.all(rgb == 0, 1)) and np.any(np.all(rgb == 255, 1))     # a residual of 3 * 255^2 against a centre of the other
        assert {0.0, 255.0} <= set(tr[0].centres[:, 2:].ravel().tolist())
        assert max(p.sums[:, 2:5].max() for p in tr) > 255 * 256, "no colour sum above a full cell of 255"
        assert ties[0] > 0
        order_matters(dx_major=(c.w, c.h) == (80, 80))
    elif c.content == "blocks8":
        gone = [set(np.flatnonzero(p.sums[:, 5] == 0).tolist()) for p in tr]
        assert not gone[0] and gone[1] and gone[-1], empty
        revived = set().union(*[a - b for a, b in zip(gone, gone[1:])])
        assert revived, "no empty cluster wins pixels again"
        for it in range(1, 6):   # the centre a revived cluster won its pixels from is the reset value
            for k in gone[it - 1]:
                assert not tr[it].centres[k].any()
        assert revived & set(np.unique(want).tolist()), "the revived cluster owns no pixel of the final labels"
        order_matters()
    elif c.content == "noise":
        assert empty == [0] * 6
        if K > 1:
            assert len(set(largest)) > 1, "the clusters do not move"
        else:
            assert not want.any() and largest == [256] * 6
    elif c.content == "mirror":
        assert np.array_equal(img, img[:, ::-1]) and set(np.unique(img[..., :3])) == {0, 85, 170, 255}
        assert ties[0] > 0
        order_matters(dx_major=True)
    else:
        raise AssertionError(f"no aim is checked for {c.content}")


def test_the_seed_search_finds_the_block_cases():
    """slic_cases.search_empty is how the seeds of blocks8 were found: it still reports them, with a revived cluster"""
    for (w, h), seed in sl.BLOCK_SEEDS.items():
        found = sl.search_empty(seeds=seed + 1, shapes=((w, h),), blocks=((8, 8),))
        assert any(f[2] == seed and f[4] and f[3][-1] > 0 for f in found), (w, h, found)


@pytest.mark.parametrize("shape", (sl.TALL, sl.TALL_TWIN))
def test_oracle_staged_entry_accepts_the_tall_shapes(shape):
    """orc_segment_crf_stages with labels_in at 32x4112 and 32x4096: the crafted labels keep the 3x3 precondition, their empty
    superpixels lie in front of and behind k = 257, the resample labels depend on the k / gy (sic) of the statement, and the oracle's
    sums are the plain numpy ones"""
    w, h = shape
    gx, gy, K = sc.grid_of(w, h)
    labels = sl.crafted_labels(w, h)
    assert sc.invariant_3x3(labels)
    empty = sl.crafted_empty(w, h)
    spc = np.bincount(labels.ravel(), minlength=K)
    assert sorted(np.flatnonzero(spc == 0).tolist()) == empty and min(empty) < 257 < max(empty) and 257 not in empty
    read, clamped = sc.resample_labels(labels)
    assert not clamped.any() and set(read.tolist()) <= {0, 1, 2, 3}          # k / gy is 0 or 1: every superpixel reads the first two rows
    ks = np.arange(K)
    wrong = labels[np.minimum((ks // gx) * 16 + 8, h - 1), (ks % gx) * 16 + 8]   # k / gx: every superpixel would read its own cell
    assert np.count_nonzero(wrong != read) > K - 8
    depth, _, _ = sl.handoff(w, h)
    st = sl.crafted_reference(w, h)["stages"]
    want = sl.handoff_sums(labels, depth)
    assert np.array_equal(st["spc"], want[0]) and np.array_equal(st["dcnt"], want[1]) and np.array_equal(st["dsum"], want[2])
    assert np.isfinite(st["lowDepth"]).all() and np.isfinite(st["unary"]).all()
    for k in empty:   # a pixel-empty superpixel's rows are its resample label's, raw or divided by the side it lies on
        r = int(read[k])
        assert r < k and st["lowConf"][0][k] == st["lowConf"][0][r] / F(spc[r])
