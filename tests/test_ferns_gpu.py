"""GPU suite of the fern keyframe database (csrc/ferns.hip) at 128x64 -> 16x8: a named case table, every case compared BIT FOR BIT with
the literal numpy reference (tests/ferns_ref.py): reduced maps, codes, good count, co[], both minima as f32 bits, the chosen keyframe
and the appended-or-not decision of every add."""
import numpy as np
import pytest

import ferns_ref as fr

pytestmark = pytest.mark.gpu

W, H = fr.W, fr.H


@pytest.fixture(scope="module")
def ctx():
    from co_fusion_amd import api
    c = api.Context(W, H, 100.0, 100.0, 64.0, 32.0, max_models=1, max_surfels=1024)
    yield c
    c.close()


def _bits(x):
    return np.float32(x).tobytes()


def _dev(ctx, maps):
    return tuple(ctx.to_device(a) for a in maps)


def _same(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def run_case(ctx, table, adds, query, qtime, min_age, capacity=None, check_each=True):
    """adds: [(maps, time, threshold)].  Runs the GPU object and the literal reference side by side and compares everything; returns
    (reference database, GPU last_search of the query, reference decisions)."""
    from co_fusion_amd import ferns
    cap = capacity if capacity is not None else max(1, len(adds))
    f = ferns.Ferns(ctx, n_ferns=len(table), capacity=cap, max_depth_mm=fr.MAX_DEPTH_MM, table=table)
    try:
        assert f.table().tobytes() == np.ascontiguousarray(table, ferns.FERN).tobytes()
        db = fr.Database(table, capacity=cap)
        decisions = []
        # every input is on the device before the first add (and stays alive): with check_each off the adds below are enqueued back to
        # back, no copy, getter or other host wait between them, so a scan reads the count while the append before it is in flight
        dev = [_dev(ctx, maps) for maps, _, _ in adds]
        ctx.synchronize()
        if not check_each:
            for i, (maps, time, thr) in enumerate(adds):
                f.add(*dev[i], fr.pose_of(i), time, thr)
        for i, (maps, time, thr) in enumerate(adds):
            if check_each:
                f.add(*dev[i], fr.pose_of(i), time, thr)
            ok, minimum, co = db.add_frame(*maps, fr.pose_of(i), time, thr)
            decisions.append(ok)
            if check_each:
                ls = f.last_search()
                assert ls["appended"] == ok, f"add {i}: appended"
                assert _bits(ls["min_all"]) == _bits(minimum), f"add {i}: minimum {ls['min_all']} != {minimum}"
                _same(ls["co"], co, f"add {i}: co")
        count, full = f.count()
        assert count == len(db.frames) and full == db.full
        for k, want in enumerate(db.frames):
            got = f.download(k)
            _same(got["codes"], want.codes, f"keyframe {k}: codes")
            assert got["good"] == want.good and got["time"] == want.time
            _same(got["pose"], want.pose, f"keyframe {k}: pose")
            _same(got["vmap"], want.vmap, f"keyframe {k}: vertex map"); _same(got["nmap"], want.nmap, f"keyframe {k}: normal map")
            _same(got["rgb"], want.rgb, f"keyframe {k}: rgb")
        # the query
        f.encode(*_dev(ctx, query))
        v4r, n4r, rgb = fr.reduce_maps(*query)
        codes, good = fr.codes_literal(table, v4r, rgb)
        vm, nm = fr.planar(v4r, n4r)
        cur = f.download(-1)
        _same(cur["vmap"], vm, "reduced vertex map"); _same(cur["nmap"], nm, "reduced normal map"); _same(cur["rgb"], rgb, "reduced rgb")
        _same(cur["codes"], codes, "codes")
        assert cur["good"] == good
        f.search(qtime, min_age)
        ls = f.last_search()
        min_add, co_add = db.add_minimum(codes, good)
        m, mid, co = db.find(codes, good, qtime, min_age)
        assert ls["searched"] == len(db.frames)
        _same(ls["co"], co, "co")
        assert _bits(ls["min_all"]) == _bits(min_add), (ls["min_all"], min_add)
        assert _bits(ls["min_match"]) == _bits(m), (ls["min_match"], m)
        assert ls["match_id"] == mid
        # a second scan of the same slot gives the same answer (the accumulators re-arm themselves)
        f.search(qtime, min_age)
        ls2 = f.last_search()
        assert ls2["match_id"] == mid and _bits(ls2["min_match"]) == _bits(m) and _bits(ls2["min_all"]) == _bits(min_add)
        return db, ls, decisions
    finally:
        f.close()


def _table(n, seed=None):
    t = fr.random_table(np.random.default_rng(n if seed is None else seed), n)
    if n == 1:
        ys, xs = np.nonzero(fr.reduce_maps(*fr.base_maps())[0][..., 2] > 0)
        t["x"], t["y"] = xs[0], ys[0]
    return t


@pytest.mark.parametrize("n,K", [(1, 1), (7, 5), (63, 63), (64, 64), (65, 65), (500, 257), (2048, 9)])
def test_fern_counts_and_database_sizes(ctx, n, K):
    """row padding (n not a multiple of 16), lanes per keyframe (1 .. 64, two pieces per lane at 2048), wave tails of the scan"""
    adds = [(fr.variant(i), 10 + i, -1.0) for i in range(K)]
    db, ls, dec = run_case(ctx, _table(n), adds, fr.variant(K // 2, 0.3), 10 + K + 400, 300, check_each=K <= 9)
    assert len(db.frames) == K and ls["min_match"] == 0
    if n >= 63:   # (with a handful of ferns an earlier keyframe can agree in every code as well, and wins the tie)
        assert ls["match_id"] == K // 2


def test_edge_codes_and_corner_ferns(ctx):
    """ferns at (0,0) and (15,7); z = 0, z < 0, tiny z; int(z*1000) equal to, below and above the threshold; colour equal to it"""
    t = fr.edge_case_table()
    db, ls, _ = run_case(ctx, t, [(fr.edge_case_maps(), 1, -1.0)], fr.edge_case_maps(), 100, 10)
    assert list(db.frames[0].codes) == [0, 0b1001, 0, 0b1000, 0b0011, 255, 255, 0b1110, 0, 0, 0b1111, 0]
    assert ls["match_id"] == 0 and ls["co"][0] == 10


def test_all_codes_bad(ctx):
    v4, n4, rgba = (a.copy() for a in fr.base_maps())
    v4[..., 2] = 0
    bad = (v4, n4, rgba)
    db, ls, dec = run_case(ctx, _table(40), [(fr.variant(0), 1, -1.0), (bad, 2, -1.0)], bad, 1000, 0, capacity=4)
    assert dec == [True, False] and ls["match_id"] == -1 and ls["min_all"] == fr.FLT_MAX
    # ... and into an empty database
    db, ls, dec = run_case(ctx, _table(40), [(bad, 2, -1.0)], bad, 1000, 0)
    assert dec == [False] and len(db.frames) == 0


def test_empty_database(ctx):
    db, ls, _ = run_case(ctx, _table(100), [], fr.variant(1), 1000, 0)
    assert ls["searched"] == 0 and ls["match_id"] == -1 and ls["min_all"] == fr.FLT_MAX and ls["min_match"] == fr.FLT_MAX
    # the first frame is appended whatever the threshold (Ferns.cpp:127: frames.size() == 0)
    db, ls, dec = run_case(ctx, _table(100), [(fr.variant(1), 5, 10.0), (fr.variant(2), 6, 10.0)], fr.variant(1), 1000, 0)
    assert dec == [True, False]


def test_identical_keyframes_lowest_index_wins(ctx):
    ids = [1, 2, 3, 7, 4, 7, 5, 7]
    adds = [(fr.variant(i), 10, -1.0) for i in ids]
    db, ls, _ = run_case(ctx, _table(200), adds, fr.variant(7), 1000, 0)
    assert ls["match_id"] == 3 and ls["co"][3] == ls["co"][5] == ls["co"][7]


def test_min_age_excludes_the_best_keyframe(ctx):
    adds = [(fr.variant(1), 10, -1.0), (fr.variant(2, 0.1), 11, -1.0), (fr.variant(0), 95, -1.0), (fr.variant(3), 12, -1.0)]
    db, ls, _ = run_case(ctx, _table(300), adds, fr.variant(0), 100, 20)
    assert ls["min_all"] == 0 and ls["match_id"] == 1 and ls["min_match"] > 0   # the runner-up: variant 2 differs least from the base
    db, ls, _ = run_case(ctx, _table(300), adds, fr.variant(0), 100, 5)            # 100 - 95 > 5 is false, 100 - 95 > 4 is true
    assert ls["match_id"] == 1
    db, ls, _ = run_case(ctx, _table(300), adds, fr.variant(0), 100, 4)
    assert ls["match_id"] == 2 and ls["min_match"] == 0


def test_every_keyframe_excluded(ctx):
    adds = [(fr.variant(i), 50 + i, -1.0) for i in range(5)]
    db, ls, _ = run_case(ctx, _table(300), adds, fr.variant(2), 60, 300)
    assert ls["match_id"] == -1 and ls["min_match"] == fr.FLT_MAX and ls["min_all"] == 0


def test_threshold_equal_to_the_minimum_is_not_greater(ctx):
    t = _table(500)
    first, second = fr.variant(0), fr.variant(9, 0.5)
    ref = fr.Database(t)
    ref.add_frame(*first, fr.pose_of(0), 1, -1.0)
    minimum = ref.add_frame(*second, fr.pose_of(1), 2, -1.0)[1]
    assert 0 < minimum < 1
    _, _, dec = run_case(ctx, t, [(first, 1, -1.0), (second, 2, float(minimum))], first, 100, 0, capacity=2)
    assert dec == [True, False]
    _, _, dec = run_case(ctx, t, [(first, 1, -1.0), (second, 2, float(np.nextafter(minimum, np.float32(0))))], first, 100, 0, capacity=2)
    assert dec == [True, True]


def test_capacity_reached(ctx):
    adds = [(fr.variant(i), i, -1.0) for i in range(5)]
    db, ls, dec = run_case(ctx, _table(64), adds, fr.variant(4), 100, 0, capacity=3)
    assert dec == [True, True, True, False, False] and db.full and ls["searched"] == 3


def test_appends_back_to_back_without_a_host_wait(ctx):
    adds = [(fr.variant(i), i, 0.05) for i in (0, 0, 1, 1, 2)]
    db, ls, dec = run_case(ctx, _table(500), adds, fr.variant(1), 100, 0, check_each=False)
    assert dec == [True, False, True, False, True]


def test_create_refuses_what_the_header_says(ctx):
    from co_fusion_amd import api, ferns
    with pytest.raises(api.CofusionError):
        ferns.Ferns(ctx, n_ferns=0)
    with pytest.raises(api.CofusionError):
        ferns.Ferns(ctx, n_ferns=2049)
    bad = _table(8); bad["x"][3] = 16
    with pytest.raises(api.CofusionError):
        ferns.Ferns(ctx, n_ferns=8, table=bad)
    small = api.Context(64, 32, 50.0, 50.0, 32.0, 16.0, max_models=1, max_surfels=1024)   # 64 is not a multiple of 128
    try:
        with pytest.raises(api.CofusionError):
            ferns.Ferns(small, n_ferns=8)
    finally:
        small.close()
