"""The case table of the scene renderer, on the CPU alone: the restatement tests/render_ref.py (f32, the kernels' order, boxes and keys)
against the independent f64 statement tests/render_oracle.py (every pixel against every surfel), and every case of
tests/render_cases.py against what it `aims` at.  Nothing in here touches the GPU."""
import warnings

import numpy as np
import pytest

import render_cases as rc
import render_oracle as ro
import render_ref as rr

warnings.filterwarnings("ignore", category=RuntimeWarning)
f32 = np.float32
CAP = 0.02          # ambiguous pixels per call, of the covered ones (a condition of the table, not a measurement)


def _calls(name):
    return list(zip(rc.case(name).calls, rc.reference(name)))


def _boxes(call, indices):
    return [rc.box(call, g) for g in indices]


def _paths(call, indices):
    """'lanes' / 'list' per surfel: which of the two raster paths its box takes"""
    return ["list" if w * h > rc.K_BIG_AREA else "lanes" for ok, w, h, *_ in _boxes(call, indices) if ok]


@pytest.mark.parametrize("name", rc.NAMES)
def test_restatement_agrees_with_the_oracle(name):
    for k, (call, (want, gid, orc)) in enumerate(_calls(name)):
        what = f"{name} call {k} {call.note}"
        sure = ~orc.ambiguous
        assert np.array_equal((gid >= 0)[sure], orc.covered[sure]), f"{what}: coverage"
        bad = (gid != orc.winner) & sure
        assert not bad.any(), f"{what}: {np.count_nonzero(bad)} winners differ, first at {np.argwhere(bad)[0][::-1]}"
        rc.against_oracle(call, want, orc, what)
        covered = int(np.count_nonzero(orc.covered))
        amb = int(np.count_nonzero(orc.ambiguous_capped))
        assert amb <= CAP * covered, f"{what}: {amb} ambiguous pixels of {covered} covered"


@pytest.mark.parametrize("name", rc.NAMES)
def test_hand_stated_expectations(name):
    """what a case states by hand holds in the restatement: drawn / not drawn, the label at a probe"""
    for k, (call, (want, gid, orc)) in enumerate(_calls(name)):
        winners = set(np.unique(gid).tolist())
        for g in call.drawn:
            assert g in winners, f"{name} call {k}: draw index {g} wins no pixel"
        for g in call.not_drawn:
            assert g not in winners, f"{name} call {k}: draw index {g} is drawn"
        lab = want[len(call.modes) + int(call.depth)]
        for px, py, label in call.probes:
            assert lab[py, px] == label, f"{name} call {k}: label {lab[py, px]} at ({px}, {py}), not {label}"


def test_depth_bound_is_the_measured_one():
    """DEPTH_MEASURED is what this table gives (to its three printed digits), DEPTH_BOUND four times that"""
    worst, where = 0.0, None
    for name in rc.NAMES:
        for k, (call, (want, gid, orc)) in enumerate(_calls(name)):
            w = rc.against_oracle(call, want, orc, name, bound=np.inf)
            if w > worst:
                worst, where = w, (name, k)
    print(f"largest relative depth difference restatement / oracle: {worst:.4g} in {where}")
    assert worst <= rc.DEPTH_MEASURED <= worst * 1.01, (worst, where)
    assert rc.DEPTH_BOUND == 4 * rc.DEPTH_MEASURED


def test_every_case_has_a_name_an_aim_and_calls():
    assert len(set(rc.NAMES)) == len(rc.NAMES)
    for name in rc.NAMES:
        c = rc.case(name)
        assert c.aims and c.calls
        for call in c.calls:
            assert call.view["width"] <= c.size[0] and call.view["height"] <= c.size[1]
            assert len(call.items) <= 256 and len(call.modes) <= 8
    assert rc.__doc__.rstrip().split("NOT COVERED")[1]


# ---- the aims, case by case

def test_aim_conf_at_threshold():
    (c0, (w0, g0, o0)), (c1, (w1, g1, o1)) = _calls("conf_at_threshold")
    S = c0.items[0]["surfels"]
    t = f32(c0.items[0]["thresh"])
    assert S[1, 3] == t and S[0, 3] == np.nextafter(t, f32(-np.inf)) and S[2, 3] == np.nextafter(t, f32(np.inf))
    assert set(np.unique(g0)) == {-1, 2} and set(np.unique(g1)) == {-1, 0, 1, 2}
    assert not o1.stable[g1 == 0].any() and not o1.stable[g1 == 1].any() and o1.stable[g1 == 2].all()
    times = w1[rc.ALL_MODES.index(rc.TIMES)]
    for m in range(5):                                  # below the threshold: the times colour in every mode
        for g in (0, 1):
            assert np.array_equal(w1[m][g1 == g], times[g1 == g])
    assert not np.array_equal(w1[2][g1 == 2], times[g1 == 2])


def test_aim_window_boundary():
    (c0, (w0, g0, o0)), (c1, (w1, g1, o1)) = _calls("window_boundary")
    v = c0.view
    assert [v["tick"] - int(s[7]) - v["time_delta"] for s in c0.items[0]["surfels"]] == [0, -1, 1]
    assert o0.dim[g0 == 2].all() and not o0.dim[g0 == 0].any() and not o0.dim[g0 == 1].any() and not o1.dim.any()
    assert tuple(w0[0][g0 == 0][0][:3]) == (200, 200, 200) and tuple(w0[0][g0 == 2][0][:3]) == (50, 50, 50)
    assert tuple(w1[0][g1 == 2][0][:3]) == (200, 200, 200)


def test_aim_times_ramp():
    calls = _calls("times_ramp")
    assert [c.view["tick"] for c, _ in calls] == [0, 1, 3]
    for c, (w, g, o) in calls[:2]:                     # tick <= 1: ratio 0, blue times (s + 0.1) for every init_time
        assert all(w[0][g == k][0][0] == 0 and w[0][g == k][0][1] == 0 and w[0][g == k][0][2] > 0 for k in range(6))
    c, (w, g, o) = calls[2]
    rgb = [tuple(int(x) for x in w[0][g == k][0][:3]) for k in range(6)]
    blue, half, below, red, over, one = rgb
    assert blue[0] == 0 and blue[1] == 0 and blue[2] > 0 and one == blue          # init 0 clamps to the ratio of init 1
    assert half[0] == 0 and half[2] == 0 and half[1] > 0                           # t == 0.5: green alone
    assert red[1] == 0 and red[2] == 0 and red[0] > 0 and over == red              # init > tick clamps to 1
    S = c.items[0]["surfels"]
    t = (S[:, 6] - f32(1)) / f32(2)
    assert t[1] == f32(0.5) and f32(0.5) - f32(1e-7) < t[2] < f32(0.5)


def test_aim_palette_ids():
    ((c, (w, g, o)),) = _calls("palette_ids")
    lab = w[-1]
    assert set(np.unique(lab)) == {0, 15, 16, 17, 254, 255}
    colour = {i: tuple(w[1][lab == i][0][:3]) for i in (0, 15, 16, 17, 254)}
    assert colour[16] == colour[0] and colour[17] != colour[16] and colour[254] != colour[0] and colour[15] != colour[0]
    s = abs(float(np.sum(c.items[0]["surfels"][0, 8:11])))
    assert colour[254] == tuple(int(np.floor(min(p / 255 * s + 0.1, 1.0) * 255 + 0.5)) for p in ro.PALETTE16[254 % 16])


def test_aim_item_mode_and_eight_outputs():
    for c, (w, g, o) in _calls("item_mode_and_eight_outputs"):
        assert len(c.modes) == 8 and c.modes[0] == rc.ITEM_MODE and c.depth and c.labels
        assert sorted(it["mode"] for it in c.items) == [0, 1, 2, 3, 4]
        lab = w[-1]
        assert set(np.unique(lab)) == {1, 2, 3, 4, 5, 255}                         # every item is visible
        for it in c.items:                                                         # ITEM_MODE is each item's own fixed-mode image
            sel = lab == it["model_id"]
            assert np.array_equal(w[0][sel], w[1 + it["mode"]][sel])
        assert not np.array_equal(w[0], w[1]) and not np.array_equal(w[0], w[3])
    assert _calls("item_mode_and_eight_outputs")[1][1][2].dim.any()


def test_aim_colour_bytes():
    (c0, (w0, g0, o0)), (c1, (w1, g1, o1)) = _calls("colour_bytes")
    for ch in range(3):
        assert set(np.unique(w0[0][..., ch][g0 >= 0])) == set(range(256))
    for b in range(256):
        assert tuple(w0[0][g0 == b][0][:3]) == (b, (b + 85) & 255, (b + 170) & 255)
    assert o1.dim[g1 >= 0].all()
    half = ro.half_way(o1.colours[rc.COLOUR]) & o1.covered[..., None]
    assert half.any()
    for b in range(256):                                                           # b / 4 rounded half up: 0.5 goes up
        assert w1[0][g1 == b][0][0] == (b + 2) // 4
    assert all(ro.half_way(o1.colours[rc.COLOUR][g1 == b][0][0]) == (b % 4 == 2) for b in range(256))


def test_aim_phong_facing():
    (c, (w, g, o)), (c_off, (w_off, g_off, o_off)) = _calls("phong_facing")
    S = c.items[0]["surfels"]
    facing = [float(np.dot(s[8:11], s[0:3])) for s in S]                           # > 0: the normal points away from the camera
    assert facing[0] < 0 and facing[1] > 0 and facing[4] > 0
    assert abs(facing[2]) < 0.15 * np.linalg.norm(S[2, 0:3])                        # grazing
    axis = w[0][32, 48]
    assert g[32, 48] == 0 and tuple(axis[:3]) == (255, 255, 255) and tuple(w_off[0][32, 48][:3]) == (64, 64, 64)     # saturated specular
    assert o.colours[rc.COLOUR][32, 48, 0] > 1.0
    for k in (1, 4):                                                               # flipped normals are lit, not black
        assert w[1][g == k][..., :3].min() > 0.3 * 0.1 * 255 - 1 and (w[1][g == k][..., :3] > w_off[1][g == k][..., :3] * 0.3 + 1).any()


def test_aim_item_table_edges():
    for c, (w, g, o) in _calls("item_table_edges"):
        counts = [len(it["surfels"]) for it in c.items]
        assert counts == [0, 1, 63, 0, 0, 64, 65, 0]
        bases = np.concatenate([[0], np.cumsum(counts)[:-1]])
        blocks = np.concatenate([[0], np.cumsum([(4 * n + 255) // 256 for n in counts])[:-1]])
        for k in (0, 3, 4):                                                        # an empty item shares base and first workgroup
            assert bases[k] == bases[k + 1] and blocks[k] == blocks[k + 1]
        assert bases[7] == sum(counts) and list(blocks) == [0, 0, 1, 2, 2, 2, 3, 5]
        ids = {it["model_id"] for it in c.items if len(it["surfels"])}
        assert ids <= set(np.unique(w[-1])), "every non-empty item is visible"
        assert len({(it["thresh"], it["model_id"], it["pose"].tobytes()) for it in c.items}) == 8
        # the first and the last surfel of the neighbours of the empty items win pixels: a lookup off by one item shows
        firsts = {bases[k] for k in (1, 2, 5, 6)}; lasts = {bases[k] + counts[k] - 1 for k in (1, 2, 5, 6)}
        assert firsts | lasts <= set(np.unique(g))
    assert not _calls("item_table_edges")[1][1][2].stable[_calls("item_table_edges")[1][1][1] >= 0].all()


def test_aim_max_items():
    ((c, (w, g, o)),) = _calls("max_items")
    assert len(c.items) == 256 and len(c.items[101]["surfels"]) == 0
    assert all(1 <= len(it["surfels"]) <= 3 for k, it in enumerate(c.items) if k != 101)
    a, b, d = (c.items[k] for k in (100, 102, 103))
    assert a["surfels"].tobytes() == b["surfels"].tobytes() == d["surfels"].tobytes() and a["pose"].tobytes() == b["pose"].tobytes()
    base = sum(len(it["surfels"]) for it in c.items[:100])
    assert g[40, 20] == base and o.winner[40, 20] == base and not o.ambiguous[40, 20]          # the tie is exact in the oracle too
    assert len(np.unique(w[-1])) > 100


def test_aim_all_empty_after_full():
    (c0, r0), (c1, (w1, g1, o1)), (c2, r2) = _calls("all_empty_after_full")
    assert (r0[1] >= 0).any() and all(len(it["surfels"]) == 0 for it in c1.items) and len(c1.items) == 3
    assert not w1[0].any() and not w1[1].any() and not w1[2].any() and (w1[3] == 255).all()
    assert np.array_equal(r0[0][0], r2[0][0])


def test_aim_narrow_boxes():
    ((c, (w, g, o)),) = _calls("narrow_boxes")
    boxes = _boxes(c, range(len(rc.NARROW)))
    assert [(bw, bh) for ok, bw, bh, *_ in boxes] == list(rc.NARROW) and all(b[0] for b in boxes)
    assert len(set(np.unique(g)) - {-1}) >= 6, "most narrow boxes cover a pixel"


def test_aim_path_switch():
    calls = _calls("path_switch")
    boxes = [rc.box(c, 0) for c, _ in calls]
    assert [(w, h) for ok, w, h, *_ in boxes] == list(rc.PATH_SWITCH)
    assert [_paths(c, [0])[0] for c, _ in calls] == ["lanes", "list", "list"]
    assert len({c.items[0]["surfels"][0, 11].tobytes() for c, _ in calls}) == 1, "the same surfel, nudged"


def test_aim_tile_seams():
    (c0, _), (c1, _) = _calls("tile_seam")
    assert rc.box(c0, 0)[:3] == (True, 64, 64) and rc.box(c1, 0)[:3] == (True, 82, 50)
    assert 64 * 64 == rc.K_TILE and 82 * 50 == 4100 and rc.K_TILE % 82 != 0
    # no box of 4097 .. 4099 pixels exists in a 96 x 64 view
    assert not [(w, a // w) for a in (4097, 4098, 4099) for w in range(1, 97) if a % w == 0 and a // w <= 64]
    for (c, (w, g, o)), (W, H) in zip(_calls("tile_seam_whole_views"), rc.SEAM_VIEWS):
        assert rc.box(c, 0)[:3] == (True, W, H) and W * H in (4097, 8193) and rc.K_TILE % W != 0
        assert (g >= 0).all() and (g == 1).any()


def test_aim_clipped():
    for c, (w, g, o) in _calls("clipped"):
        W, H = c.view["width"], c.view["height"]
        for first, path in ((0, "lanes"), (8, "list")):
            boxes = _boxes(c, range(first, first + 8))
            assert all(p == path for p in _paths(c, range(first, first + 8))) and all(b[0] for b in boxes)
            left = [b[3] == 0 for b in boxes]; top = [b[4] == 0 for b in boxes]
            right = [b[3] + b[1] == W for b in boxes]; bottom = [b[4] + b[2] == H for b in boxes]
            #          corner         edge            corner
            assert left == [True, False, False, True, False, True, False, False]
            assert right == [False, False, True, False, True, False, False, True]
            assert top == [True, True, True, False, False, False, False, False]
            assert bottom == [False, False, False, False, False, True, True, True]
            full = max(b[1] for b in boxes)
            assert all(b[1] < full for b, l, r in zip(boxes, left, right) if l or r), "a clipped box is narrower"


def test_aim_outside_or_barely_inside():
    ((c, (w, g, o)),) = _calls("outside_or_barely_inside")
    boxes = _boxes(c, range(7))
    assert [b[0] for b in boxes] == [False, False, False, False, False, True, True]
    assert boxes[5][1] == 1 and boxes[5][3] == 0, "the box of one column"
    assert set(np.unique(g)) == {-1, 6}


def test_aim_full_view():
    ((c, (w, g, o)),) = _calls("full_view")
    assert rc.box(c, 0)[:3] == (True, 96, 64) and (g == 0).all() and o.covered.all()


def test_aim_near_far():
    calls = _calls("near_far")
    (c0, (w0, g0, o0)), (c1, (w1, g1, o1)) = calls[:2]
    assert np.nextafter(f32(c1.view["near"]), f32(np.inf)) == f32(c0.view["near"])
    assert not rc.box(c0, 0)[0] and rc.box(c1, 0)[0]
    assert not (g0 == 0).any() and (g1 == 0).any()
    (c2, (w2, g2, o2)), (c3, (w3, g3, o3)) = calls[2:4]
    assert c2.items[0]["surfels"][0, 2] == f32(c2.view["far"]) and c3.items[0]["surfels"][0, 2] == np.nextafter(f32(c3.view["far"]), f32(0))
    assert g2[32, 48] == -1 and g3[32, 48] == 0 and w3[1][32, 48] == c3.items[0]["surfels"][0, 2]
    c4, (w4, g4, o4) = calls[4]
    assert c4.view["near"] == 0 and c4.view["far"] == 0 and set(np.unique(g4)) == {-1, 0, 2}
    # the boundary surfels alone are exempt from the cap
    assert [c.exempt for c, _ in calls] == [(0,), (0,), (0,), (0,), ()]


def test_aim_degenerate():
    ((c, (w, g, o)),) = _calls("degenerate")
    n = len(rc.DEGENERATE)
    S = c.items[0]["surfels"]
    assert not S[0, 8:11].any() and np.isnan(S[1, 0]) and np.isnan(S[2, 9]) and np.isnan(S[3, 11]) and np.isinf(S[4, 2]) and np.isinf(S[5, 0])
    assert S[6, 11] == 0 and S[7, 11] < 0 and S[13, 8] == 0 and S[13, 9] == S[13, 10]
    assert max(S[8, 11], S[9, 11]) * 80 / 1.0 < 0.5, "radius below half the pixel pitch"
    assert np.count_nonzero(g == 9) == 1
    assert float(np.dot(S[10, 0:3], S[10, 8:11])) == 0.0, "the plane passes through the camera centre"
    assert (g >= n).any() and np.count_nonzero(g >= 0) > 500, "the image is not empty"
    # the negative radius draws the disc of |r|: the same pixels as the positive one
    pos = S.copy(); pos[7, 11] = -pos[7, 11]
    with np.errstate(all="ignore"):
        kb, _ = rr.keys(c.view, [dict(c.items[0], surfels=pos)])
    assert np.array_equal((kb & np.uint64(0xFFFFFFFF)) == 7, g == 7) and np.count_nonzero(g == 7) > 20


def test_aim_f64_matrix():
    for c, (w, g, o) in _calls("f64_matrix"):
        it = c.items[0]
        assert np.abs(c.view["pose"][:3, 3]).min() > 20 and np.abs(it["pose"][:3, 3]).min() > 20
        M64 = rr.model_to_camera(rr.view_inverse(c.view["pose"]), it["pose"])
        C = c.view["pose"]
        V32 = np.eye(4, dtype=f32); V32[:3, :3] = C[:3, :3].T; V32[:3, 3] = -(C[:3, :3].T @ C[:3, 3])
        M32 = V32 @ it["pose"]
        assert np.array_equal(M64, ro.model_to_camera(c.view["pose"], it["pose"]).astype(f32))
        assert np.abs(M32[:3, 3] - M64[:3, 3]).max() > 5e-7, "an f32 product gives another translation"
        assert np.count_nonzero(M32 != M64) >= 3
        assert np.count_nonzero(g >= 0) > 600


def test_aim_odd_intrinsics():
    calls = _calls("odd_intrinsics")
    v0, v1, v2 = (c.view for c, _ in calls)
    assert not (0 <= v0["cx"] < 96) and not (0 <= v0["cy"] < 64) and v0["fx"] != v0["fy"]
    assert v1["fy"] < 0 and v2["fy"] < 0 and (v2["width"], v2["height"]) == rc.SMALL
    for c, (w, g, o) in calls:
        assert np.count_nonzero(g >= 0) > 0.15 * g.size


def test_aim_ray_cache():
    calls = _calls("ray_cache")
    key = [tuple(c.view[k] for k in ("fx", "fy", "cx", "cy", "width", "height")) for c, _ in calls]
    assert key[0] == key[2] == key[4] and key[1][:2] == key[0][:2] and key[1][2] != key[0][2] and key[1][3:] == key[0][3:]
    assert key[3][:4] == key[0][:4] and key[3][4:] == rc.SMALL, "the intrinsics alone do not tell the two sizes apart"
    img = [w[0] for _, (w, g, o) in calls]
    assert np.array_equal(img[0], img[2]) and np.array_equal(img[0], img[4]) and not np.array_equal(img[0], img[1])
    # the same rays at another row pitch: the small image is the crop of the large one, and not empty
    assert np.array_equal(img[3], img[0][:45, :83]) and img[3][..., 3].any()


def test_aim_back_to_back():
    calls = _calls("back_to_back")
    assert len(calls) == 3 and len({len(c.items) for c, _ in calls}) == 3
    labels = [set(np.unique(w[-1])) - {255} for _, (w, g, o) in calls]
    assert labels[0] and labels[1] and labels[2] and not (labels[0] & labels[1]) and not (labels[0] & labels[2]) and not (labels[1] & labels[2])


def test_aim_overflow_list_full():
    (c, (w, g, o)), (c_next, (w_next, g_next, _)), (c_last, _) = _calls("overflow_list_full")
    S = c.items[0]["surfels"]
    nb, end, tail = rc.OVERFLOW_BLOCK, rc.OVERFLOW_COPIES_END, rc.OVERFLOW_TAIL
    assert len(S) == end + tail > (1 << 18) + (1 << 12)
    assert np.array_equal(S[:end].reshape(-1, nb, 12), np.broadcast_to(S[:nb], (end // nb, nb, 12))), "exact copies of block 0, in rotation"
    assert np.array_equal(c.ref_items[0]["surfels"], np.concatenate([S[:nb], S[end:]]))
    boxes = _boxes(c, range(nb + tail))
    area = np.array([bw * bh for ok, bw, bh, *_ in boxes])
    assert all(b[0] for b in boxes) and (area > rc.K_BIG_AREA).all(), "every surfel goes to the overflow list"
    tiles = (area + rc.K_TILE - 1) // rc.K_TILE
    assert np.count_nonzero(tiles[:nb] == 2) == 4 and (tiles[nb:] == 1).all()
    total = int(tiles[:nb].sum()) * (end // nb) + int(tiles[nb:].sum())
    assert total - int(tiles[nb:].sum()) > rc.K_BIG_CAP, "the copies alone overflow the list"
    assert (end + tail - tail) > rc.K_BIG_CAP, "in launch order the tail's slots lie beyond the cap even at one tile per surfel"
    assert set(range(nb, nb + tail)) <= set(np.unique(g)), "every surfel of the tail is visible"
    assert len(set(range(nb)) & set(np.unique(g))) > 20
    A = c_next.items[0]["surfels"]
    assert len(A) == 30 and (A[:10, 3] < c_next.items[0]["thresh"]).all() and (A[:10, 2] < A[10:, 2].min()).all()
    assert all(rc.box(c_next, k)[0] for k in range(10)), "the surfels below the threshold are in view"
    assert len(c_last.items) == 3 and (g_next >= 10).any()
