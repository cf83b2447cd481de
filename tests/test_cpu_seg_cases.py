"""The case table of the segmentation chain (tests/seg_cases.py) on the oracle alone: every case reaches what it aims at -- the means
are the crafted floats, the weak-confidence rules fall on the expected side of 0.3 and 0.4, the lists of empty superpixels hold a
label read in front of and behind the superpixel and a depth-empty read, the resample row is clamped at 320x240 and not at 48x80, the
floors are reached, no sum leaves 2^62, the label images obey the 3x3 precondition of the accumulation kernel -- and the oracle's
staged entry is the plain one."""
import ctypes as C
import warnings

import numpy as np
import pytest

import orc_multi as om
import seg_cases as sc

warnings.filterwarnings("ignore", category=RuntimeWarning)
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _q32(v):
    """round(v * 2^32) of values that have no bit under 2^-32 (exact in f64)"""
    q = np.asarray(v, np.float64) * 4294967296.0
    assert np.all(q == np.rint(q))
    return q.astype(np.int64)


def _weak(m, conf):
    """the two rules of Segmentation.cpp:240-249 in f64, as the reference's text has them"""
    c = np.asarray(conf, F).astype(np.float64)
    return c < 0.3 if m == 0 else c <= 0.4


@pytest.mark.parametrize("name", sc.names())
def test_case_reaches_what_it_aims_at(name):
    c, ref = sc.case(name), sc.reference(name)
    st, e, K, n = ref["stages"], c.expect, c.K, c.n
    assert c.aims and (c.w, c.h) == sc.SHAPES[K]
    assert sc.invariant_3x3(c.labels), "a pixel's label lies outside the 3x3 cells around its own"
    if c.family == "values":
        assert np.array_equal(c.labels, sc.grid_labels(c.w, c.h))
    assert np.array_equal(st["spc"], np.bincount(c.labels.ravel(), minlength=K))
    for k in ("dsum", "icp_sum", "conf_sum"):
        assert np.abs(st[k].astype(np.float64)).max() < 2.0 ** 62, f"{k} beyond 2^62"
    assert (not np.isfinite(st["unary"]).all()) == c.nonfinite, "non-finite unaries: the case's flag is wrong"
    rng_ = st["depthRange"][0]
    fill = [F(np.float64(rng_) * 0.01)] + [F(rng_) * F(c.params.unaryKError)] * (n - 1)

    # the means are the crafted floats, bit for bit; the substitution falls where the rules say
    if c.sp_depth is not None:
        assert np.array_equal(_bits(st["lowDepth"]), _bits(c.sp_depth)), "mean depths"
    if c.sp_conf is not None and "bad_pixels" not in e:
        for m in range(n):
            assert np.array_equal(_bits(st["lowConf"][m]), _bits(c.sp_conf[m])), f"mean confidences of model {m}"
            weak = _weak(m, c.sp_conf[m])
            if "weak" in e:
                assert np.array_equal(weak, e["weak"][m]), f"model {m}: the case expects other weak superpixels than the rules give"
            assert np.array_equal(_bits(st["lowICP"][m]), _bits(np.where(weak, fill[m], c.sp_icp[m]))), f"mean errors of model {m}"
            assert not np.any(c.sp_icp[m] == fill[m]), "an error equal to the fill value would hide the substitution"
    if "weak" in e:
        assert all(w.any() and not w.all() for w in e["weak"])
    if name.startswith("conf-thresholds"):
        t = np.concatenate(c.sp_conf)
        assert {sc.prev32(0.3), F(0.3), sc.next32(0.3), sc.prev32(0.4), F(0.4), sc.next32(0.4)} <= set(t.tolist())
        # 0.3f and 0.4f are NOT weak (they lie above 0.3 and 0.4); a rule evaluated against 0.4f in f32 would take 0.4f
        assert not _weak(0, F(0.3)) and not _weak(1, F(0.4)) and F(0.4) <= F(0.4) and np.float64(F(0.4)) > 0.4
        for m in range(1, n):
            assert np.any(c.sp_conf[m] == F(0.4)) and not np.any(e["weak"][m] & (c.sp_conf[m] == F(0.4)))

    if "bad_pixels" in e:   # non-finite pixels: nothing to the sum, one to the divisor
        lab = c.labels.ravel()
        for (what, m), at in e["bad_pixels"].items():
            img = (c.icp if what == "icp" else c.conf)[m]
            assert np.array_equal(~np.isfinite(img), at) and {"nan", "inf", "-inf"} <= {str(v) for v in img[at]}
            good = 256 - np.bincount(lab, at.ravel(), K).astype(np.int64)
            assert good.min() < 256
            values = (c.sp_icp if what == "icp" else c.sp_conf)[m]
            assert np.array_equal(st[what + "_sum"][m], good * _q32(values)), f"{what} sums of model {m}"
        assert np.all(st["spc"] == 256)
    if name == "conf-all-nan":
        assert st["conf_sum"][0][4] == 0 and st["conf_sum"][1][5] == 0 and np.all(st["spc"] == 256)
    if "dcnt" in e:
        for k, cnt in e["dcnt"].items():
            assert st["dcnt"][k] == cnt, f"superpixel {k}: {st['dcnt'][k]} depth samples"
        assert st["dsum"][2] == 0 and st["dsum"][3] == 256 * int(np.rint(np.float64(sc.next32(0.02)) * 2.0 ** 32))
        assert np.isnan(c.depth).any() and np.isposinf(c.depth).any()
    if e.get("negative_sums"):
        assert (st["icp_sum"] < 0).any() and (st["lowICP"] < 0).any() and (st["unary"] == F(1e-5)).any()
    if e.get("clamped"):
        assert np.all(np.abs(st["icp_sum"][0]) == 256 * 2 ** 52) and (st["icp_sum"][0] < 0).any() and st["conf_sum"][1].max() == 256 * 2 ** 52
        assert np.abs(c.icp[0]).min() >= 2.0 ** 20 and np.abs(c.icp[0]).max() > 1e38
    if "sums" in e:
        for (what, m), want in e["sums"].items():
            assert np.array_equal(st[what + "_sum"][m], want), f"{what} sums of model {m}: the ties of the rounding to Q32"
            assert want.min() > 0
    if name == "q32-random":
        v = np.concatenate([a.ravel() for a in c.icp + c.conf])
        assert v.min() < 2e-7 and v.max() > 500 and np.unique(c.icp[0]).size > c.icp[0].size // 2
    if e.get("floor_1e-5"):
        zero = np.stack([s == 0 for s in c.sp_icp], 1)
        assert zero.any() and np.all(st["unary"][:, :n][zero] == F(1e-5)) and not np.all(st["unary"] == F(1e-5))
    if e.get("floor_0.01"):
        new = st["unary"][:, n]
        assert (new == F(0.01)).any() and (new > F(0.01)).any()
        lowest = np.min(np.stack(st["lowICP"]), 0) / rng_
        assert np.array_equal(new == F(0.01), c.params.unaryThresholdNew - c.params.unaryWeightError * lowest < 0.01)
    if "range" in e:
        assert rng_ == F(e["range"]), f"depth range {rng_}"
    if name == "depth-above-100":
        assert np.all(st["feat2"][[2, 6, 7], 5] == F(100.0)) and np.all(st["feat2"][[0, 1, 3], 5] < 100) and st["lowDepth"].max() == 150
    if name == "depth-all-invalid":
        assert np.all(st["dcnt"] == 0) and np.all(st["lowDepth"] == 0)

    # the lists of empty superpixels
    read, clamped = sc.resample_labels(c.labels)
    pix_empty, depth_empty = np.flatnonzero(st["spc"] == 0), np.flatnonzero(st["dcnt"] == 0)
    if c.family == "labels":
        assert pix_empty.tolist() == sorted(e.get("pixel_empty", [])), pix_empty
    else:
        assert pix_empty.size == 0
    assert np.all(st["spc"][read] > 0)    # a label that was read at a pixel owns that pixel: no division by a zero count
    if "read" in e:
        r = read[pix_empty]
        assert not np.any(r == pix_empty)
        assert {"smaller": np.all(r < pix_empty), "larger": np.all(r > pix_empty), "both": np.any(r < pix_empty) and np.any(r > pix_empty)}[e["read"]], (pix_empty, r)
        if c.sp_icp is None:   # read < k: divided twice (the reference's in-place order); read > k: once
            for m in range(n):
                raw = (st["icp_sum"][m].astype(np.float64) * 2.0 ** -32).astype(F)
                for k, rd in zip(pix_empty, r):
                    once = raw[rd] / F(st["spc"][rd])
                    want = once / F(st["spc"][rd]) if rd < k else once
                    got = st["lowICP"][m][k]
                    assert _bits(got) == _bits(want) or got == fill[m], (k, rd, got, want)
    if "row_clamped" in e:
        empties = np.union1d(pix_empty, depth_empty)
        assert bool(clamped[empties].any()) == e["row_clamped"] and (e["row_clamped"] or not clamped.any())
    if "both_empty" in e:
        assert set(e["both_empty"]) <= set(pix_empty.tolist()) & set(depth_empty.tolist())
    if "depth_chain" in e:
        rd = read[depth_empty]
        chain = np.isin(rd, depth_empty) & (rd < depth_empty if e["depth_chain"] == "smaller" else rd > depth_empty)
        assert np.any(chain), "no depth-empty superpixel reads another one"
    # Slic::downsampleThresholded's in-place normalisation, replayed here in index order: an empty superpixel reads an entry that is
    # already a mean when it lies in front of it and still a raw sum when behind
    low = (st["dsum"].astype(np.float64) * 2.0 ** -32).astype(F)
    for k in range(K):
        rd = k if st["dcnt"][k] else read[k]
        low[k] = low[rd] / F(st["dcnt"][k] if st["dcnt"][k] else st["spc"][rd])
    assert np.array_equal(_bits(low), _bits(st["lowDepth"])), "mean depths against the in-order replay"
    if "owner_pixels" in e:
        assert st["spc"].max() == e["owner_pixels"]
    if e.get("ragged"):
        gx = c.w // 16
        cell = sc.grid_labels(c.w, c.h)
        slots = (c.labels // gx - cell // gx + 1) * 3 + (c.labels % gx - cell % gx + 1)
        inner = cell == (c.h // 32) * gx + gx // 2   # a cell with all eight neighbours
        assert set(np.unique(slots[inner]).tolist()) == set(range(9)) and pix_empty.size == 0


def test_the_table_covers_what_it_promises():
    cs = sc.cases()
    assert {c.K for c in cs} == {9, 15, 99, 300, 1200} and sum(c.K == 1200 for c in cs) <= 3
    assert sum(c.nonfinite for c in cs) * 4 <= len(cs)
    assert {(c.n, c.allow_new) for c in cs} >= {(1, False), (1, True), (16, False), (16, True), (17, False)}
    # label families: a read in front of the superpixel, one behind it, a depth-empty read, both kinds of empty, the clamp at 320x240 only
    lab = [c for c in cs if c.family == "labels"]
    assert {c.expect.get("read") for c in lab} >= {"smaller", "larger", "both"}
    assert {c.expect.get("depth_chain") for c in lab} >= {"smaller", "larger"} and any(c.expect.get("both_empty") for c in lab)
    assert [c.expect["row_clamped"] for c in lab if (c.w, c.h) == (320, 240) and "row_clamped" in c.expect] == [True]
    assert [c.expect["row_clamped"] for c in lab if (c.w, c.h) == (48, 80) and "row_clamped" in c.expect] == [False]
    # every batch call has segmenters whose label counts differ
    for b in sc.batches():
        assert len(b) >= 2 and len({sc.case(x).L for x in b}) >= 2 and len({sc.case(x).group() for x in b}) == 1, b
    assert {x for b in sc.batches() for x in b} == set(sc.names())
    mf = sc.MF_CASES
    assert {m.K for m in mf} == {9, 15, 99, 300} and {m.L for m in mf} == {1, 2, 16, 17, 40} and {m.iterations for m in mf} == {0, 1, 2, 10}
    assert {(m.w_smooth, m.w_app) for m in mf} == {(2.0, 7.0), (0.0, 7.0), (2.0, 0.0)}
    for it in (0, 1):   # the marginals in Q0 and in Q1, with small and with large L
        assert {m.L <= 16 for m in mf if m.iterations == it} == {True, False}
    assert len({m.name for m in mf}) == len(mf)
    for m in mf:
        Q = sc.mf_reference(m)
        assert np.isfinite(Q).all() and np.allclose(Q.sum(1), 1.0, atol=1e-5)
        if m.iterations:   # the steps do something: the marginals are not the first ones
            first = sc.mf_reference(sc.MFCase(m.K, m.L, 0, m.w_smooth, m.w_app, m.aims)) if m.L > 1 else None
            assert first is None or not np.array_equal(first, Q)


def _same_result(a, b, what):
    for k in ("full", "low", "labels"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k}"
    assert a["hasNewLabel"] == b["hasNewLabel"] and _bits(a["depthRange"]) == _bits(b["depthRange"]), what
    assert len(a["modelData"]) == len(b["modelData"])
    for x, y in zip(a["modelData"], b["modelData"]):
        for k in x:
            assert x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]), f"{what}: {k}"


def test_staged_entry_without_labels_and_stages_is_the_plain_entry():
    """orc_segment_crf_stages(labels_in = NULL, out = NULL) against orc_segment_crf on the scenarios of test_segment_gpu.py; with the
    stages asked for, and with SLIC's own labels handed back in, the results stay the same"""
    import test_segment_gpu as base
    for i, s in enumerate(base._scenarios()):
        plain = base._ref(s)   # (om.segment_crf of the scenario, shared with that module's tests)
        _same_result(om.segment_crf_stages(*s[1:], stages=False), plain, s[0])
        if i in (3, 4):
            staged = om.segment_crf_stages(*s[1:], labels_in=plain["labels"])
            _same_result(staged, plain, s[0] + ", labels handed in")
            L = len(s[4]) + (1 if s[8] else 0)
            assert staged["stages"]["Q"].shape == (base.GX * base.GY, L) and np.allclose(staged["stages"]["Q"].sum(1), 1.0, atol=1e-5)
            assert staged["stages"]["depthRange"][0] == F(plain["depthRange"])
