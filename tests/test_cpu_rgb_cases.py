"""CPU suite: the case table of the photometric record-slot path (tests/rgb_cases.py) and its independent reference
(tests/rgb_rows_ref.py).

  * the reference equals the oracle -- orc_rgb_residual's correspondences on the pixels of the oracle's own candidate rule, orc_rgb_step's
    sums fed the reference's correspondences and sigma, orc_rgb_fix_bits, orc_se3_sums_to_host -- on every case: the two share no code;
  * every case reaches its aim, computed by the reference itself: a case that does not fails by name;
  * the domain conditions of the reference hold for every case and every planted stale slot.
All comparisons are integer or bit equality."""
import numpy as np
import pytest

import orc
import rgb_cases as rc
import rgb_rows_ref as rr

THREADS = [t for t, _ in rc.SHAPES]


def _img(c, a):
    return np.asarray(a).reshape(c.rows, c.cols)


@pytest.mark.parametrize("name", rc.NAMES)
def test_reference_equals_the_oracle(name):
    c = rc.case(name)
    r = rr.residual(c)
    ocor, osig, ocnt = orc.rgb_residual(0.0, _img(c, c.dIdx), _img(c, c.dIdy), _img(c, c.last_depth), _img(c, c.next_depth), _img(c, c.last_image),
                                        _img(c, c.next_image), float(c.max_dd), c.kt, c.krk)
    rule = rc.cand_rule(c, 0.0) != 0           # what the oracle tests in front of the pose-dependent half
    want = r["ok"] & rule
    assert np.array_equal(ocor["valid"] != 0, want), np.flatnonzero((ocor["valid"] != 0) != want)[:8]
    k = np.flatnonzero(want)
    assert np.array_equal(ocor["zero_y"][k].astype(np.int64) * c.cols + ocor["zero_x"][k], r["g"][k])
    assert np.array_equal(ocor["one_y"][k].astype(np.int64) * c.cols + ocor["one_x"][k], k)
    assert np.array_equal(ocor["diff"][k], r["diff"][k].astype(np.float32))
    assert (ocnt, osig) == (len(k), rr.wrap32(int((r["diff"][k] ** 2).sum())))
    for threads in (THREADS if c.res_range is not None else THREADS[:1]):
        ref = rc.reference(name, threads)
        cor = np.zeros(c.n, orc.DATATERM)
        kv = np.flatnonzero(ref["valid"])
        cor["valid"][kv] = 1; cor["diff"][kv] = r["diff"][kv]
        cor["one_x"][kv] = kv % c.cols; cor["one_y"][kv] = kv // c.cols
        cor["zero_x"][kv] = r["g"][kv] % c.cols; cor["zero_y"][kv] = r["g"][kv] // c.cols
        osums = orc.rgb_step(cor, float(ref["sigma"]), c.cloud.reshape(c.rows, c.cols, 3), float(c.fx), float(c.fy), _img(c, c.dIdx), _img(c, c.dIdy), float(c.sobel))
        assert orc.rgb_fix_bits(float(ref["sigma"])) == ref["F"]
        assert np.array_equal(osums[:29], ref["sums64"][:29]), (name, threads, np.flatnonzero(osums[:29] != ref["sums64"][:29]))
        A, b, _ = orc.se3_to_host(ref["sums64"], ref["F"])
        q = [np.float32(np.ldexp(np.float64(int(v)), -ref["F"])) for v in ref["sums64"][:27]]
        kk = 0
        for i in range(6):
            for j in range(i, 7):
                got = b[i] if j == 6 else A[i, j]
                assert got.tobytes() == q[kk].tobytes() and (j == 6 or A[j, i].tobytes() == q[kk].tobytes()), (i, j)
                kk += 1


def _slot_counts(ref):
    return {s: len(v) for s, v in ref["slots"].items()}


def _half_ties(q, rounded):
    """(ties rounded down, ties rounded up) among the finite quotients q"""
    fin = np.isfinite(q)
    tie = fin & (np.where(fin, q, 0) - np.floor(np.where(fin, q, 0)) == 0.5)
    return int((tie & (rounded < q)).sum()), int((tie & (rounded > q)).sum())


def _check_aim(name, c):
    refs = {t: rc.reference(name, t) for t in THREADS}
    ref = refs[64]
    r, valid, rows = ref["res"], ref["valid"], ref["rows"]
    cand = c.cand != 0
    n = c.n
    lim = 2.0 ** ((50 - ref["F"]) // 2)
    beyond = np.abs(rows[:, :6]) > lim if len(rows) else np.zeros((0, 6), bool)
    if not name.startswith("clamp"):
        assert not beyond.any(), "the clamp engages in a case that does not aim at it"
    if name == "scene":
        assert 300 <= ref["count"] < c.cand.sum() - 100 and ref["sigma"] == ref["count"] and ref["sigma_total"] > 0
    elif name == "project_ties":
        from icp_rows_ref import _f2i_rn
        for q, size in ((r["uq"], c.cols), (r["vq"], c.rows)):
            down, up = _half_ties(q, _f2i_rn(q))
            assert down >= 100 and up >= 100, (down, up)
            assert (valid & (q == -0.5)).any(), "-0.5 rounds to 0 and is valid"
            assert ((q == size - 0.5) & cand & ~r["inb"]).any(), "size - 0.5 rounds out of the image"
    elif name == "project_degenerate":
        uq, vq = r["uq"], r["vq"]
        assert (cand & (uq == np.inf)).any() and (cand & (uq == -np.inf)).any()
        nan00 = cand & np.isnan(uq) & np.isnan(vq)
        assert nan00.any() and r["inb"][nan00].all() and not r["ok"][nan00].any(), "0 / 0 lands on (0, 0) and the depth gate rejects it"
        assert (cand & (r["td1"] < 0) & r["inb"] & ~r["ok"]).any() and (cand & (c.next_depth == 0) & r["inb"] & ~r["ok"]).any()
        assert ref["count"] >= 100
    elif name == "depth_gate":
        dd = np.abs(r["td1"] - r["d0"])
        assert (valid & (dd == c.max_dd)).sum() >= 100, "a difference exactly at the gate passes"
        above = dd == np.nextafter(c.max_dd, np.float32(1))
        assert (cand & above).sum() >= 100 and not valid[above].any(), "one ulp above the gate fails"
        for sel in (r["d0"] == 0, r["d0"] < 0, np.isnan(r["d0"]), (r["li"] == 0) & (dd <= c.max_dd) & (r["d0"] > 0)):
            assert (cand & sel).sum() >= 100 and not valid[sel].any()
    elif name == "diff_extremes":
        kv = np.flatnonzero(valid)
        assert {1, 256, 510} <= set((r["diff"][kv] + 256).tolist())
        assert valid[0] and r["g"][0] == 0 and valid[n - 1] and r["g"][n - 1] == n - 1
        assert len(set(r["g"][kv].tolist())) < len(kv), "two pixels share a g"
    elif name.startswith("full_slot_"):
        t = int(name.rsplit("_", 1)[1])
        counts = _slot_counts(refs[t])
        full = [s for s, v in counts.items() if v == 4 * t]
        assert len(full) == 1 and sum(counts.values()) == 4 * t, counts
    elif name == "full_last_64x48":
        for t in (64, 256):
            counts = _slot_counts(refs[t])
            assert n % (4 * t) == 0 and counts[refs[t]["n_slots"] - 1] == 4 * t
    elif name == "stride_walk":
        assert sorted(v for v in _slot_counts(refs[256]).values() if v) == [129, 257]
    elif name == "sparse":
        assert ref["count"] == 1 and valid[4095] and all(4096 % (4 * t) == 0 for t in THREADS)
    elif name == "empty":
        assert ref["count"] == 0 and cand.sum() > 1000 and ref["sums"] == [0] * 29
    elif name == "tail":
        for t in THREADS:
            assert np.flatnonzero(valid).min() >= (refs[t]["n_slots"] - 1) * 4 * t and n % (4 * t) != 0
        assert valid[n - 1]
    elif name.startswith("ranged"):
        for t in THREADS:
            f = refs[t]
            planted, _ = rc.plant(c, t)
            outside = [s for s in range(f["n_slots"]) if s < f["first"] or s > f["last"]]
            assert outside and all(planted[s] > 0 for s in outside), "stale slots planted outside the range"
            slot = np.arange(n) // (4 * t)
            assert (r["ok"] & cand & np.isin(slot, outside)).any(), "candidates outside the range that must not be counted"
            if name == "ranged_empty":
                assert f["last"] < f["first"] and f["count"] == 0
            else:
                assert f["count"] > 0 and f["last"] >= f["first"]
        in64 = refs[64]["last"] - refs[64]["first"] + 1
        assert {"ranged_b1": c.res_blocks == 1, "ranged_b2": c.res_blocks == 2, "ranged_b100": c.res_blocks > in64, "ranged_empty": True}[name]
    elif name.startswith("sigma_"):
        want_F = dict(rgbonly=8, zero_diffs=8, count3=10, hundreds=24, wrap=18, neg=18, w0=8, zero_zero=8, no_counts=24)
        want_F["4096"] = 32
        assert ref["F"] == want_F[name[6:]], ref["F"]
        if name == "sigma_rgbonly":
            assert ref["sigma"] == -1
        if name == "sigma_zero_diffs":
            assert ref["sigma"] == 1 and ref["count"] > 0 and ref["sigma_total"] == 0
        if name == "sigma_4096":
            assert ref["count"] >= 4096
        if name == "sigma_wrap":
            assert sum(int(v) for v in c.count_seed) == (1 << 32) + 5 and (c.count_seed != 0).sum() >= 5 and ref["sigma"] == 45
        if name == "sigma_neg":
            assert rr.wrap32(ref["sigma_total"]) < 0 and ref["sigma"] == ref["count"]
        if name == "sigma_w0":
            assert ref["sigma"] == 0 and ref["sigma_total"] != 0 and (ref["mid"]["w"] == 1).all() and not r["diff"][valid].any()
        if name == "sigma_zero_zero":
            assert (ref["count_total"], ref["sigma_total"], ref["sigma"]) == (0, 0, 0) and ref["count"] == 40
            assert (ref["mid"]["w"] != 1).sum() >= 30 and (r["diff"][valid] != 0).sum() >= 30
        if name == "sigma_no_counts":
            assert (ref["count_total"], ref["sigma_total"], ref["sigma"]) == (500, 12345, 500) and ref["count"] == 40
    elif name.startswith("clamp"):
        assert ref["F"] == (8 if name == "clamp_f8" else 32)
        assert (rows[:, :6] > lim).any() and (rows[:, :6] < -lim).any() and (~beyond.any(axis=1)).sum() >= 100
    elif name == "sum_ties":
        neg, pos = rr.count_sum_ties(rows, ref["F"])
        assert neg >= 1000 and pos >= 1000, (neg, pos)
    else:
        raise AssertionError("no precondition written for case %s" % name)


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_reaches_its_aim(name):
    c = rc.case(name)
    assert c.aims and c.cols % 4 == 0
    _check_aim(name, c)


@pytest.mark.parametrize("name", rc.NAMES)
def test_domain(name):
    c = rc.case(name)
    tiny = np.finfo(np.float32).tiny
    r = rr.residual(c)
    can_point = r["g"][r["ok"] & (c.cand != 0)]
    z = c.cloud[can_point, 2]
    assert np.isfinite(z).all() and (z > 0).all(), "cloud z where a record can point"
    for t in (THREADS if c.res_range is not None else THREADS[:1]):
        ref = rc.reference(name, t)
        for a in [ref["rows"]] + list(ref["mid"].values()):
            assert np.isfinite(a).all() and not ((a != 0) & (np.abs(a) < tiny)).any(), "rows and their intermediates: finite, no subnormal"
        assert all(-(1 << 63) <= v < (1 << 63) for v in ref["sums"]), "the true sums leave int64"
    for t in THREADS:
        counts, recs = rc.plant(c, t)
        cap = np.minimum(4 * t, c.n - np.arange(len(counts)) * 4 * t)
        assert len(counts) == (c.n + 4 * t - 1) // (4 * t) and (counts <= cap).all() and (counts > 0).all()
        k, g, d = rr.unpack(recs)
        assert (k < c.n).all() and (g < c.n).all() and (d >= -255).all() and (d <= 255).all() and len(recs) == c.n


def test_table_covers_the_issue_and_batches_share_a_launch():
    families = ("scene", "project_ties", "project_degenerate", "depth_gate", "diff_extremes", "full_slot", "sparse", "empty", "tail", "ranged", "sigma",
                "clamp", "sum_ties")
    for f in families:
        assert any(n.startswith(f) for n in rc.NAMES), f
    assert len(rc.BATCHES["batch_3"]) == 3 and len(rc.BATCHES["batch_9"]) == 9
    for members in rc.BATCHES.values():
        assert len(set(members)) == len(members)
        cs = [rc.case(m) for m in members]
        assert len({(c.cols, c.rows, float(c.max_dd), float(c.sobel), float(c.fx), float(c.fy)) for c in cs}) == 1
    assert set(rc.MODE0) <= set(rc.NAMES) and all(rc.case(m).min_scale is not None for m in rc.MODE0)
    assert rr.pack(3, 5, -255) == 3 | ((5 | (1 << 22)) << 32) and rr.pack(0, 0, 255) >> 32 == 511 << 22
