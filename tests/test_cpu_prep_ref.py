"""CPU checks behind tests/test_track_prep_gpu.py: the numpy references of tests/prep_ref.py on hand-made arrays whose answers are
written out here, and the scenes of tests/prep_scenes.py -- computed from the references and the CPU oracle alone, every shape and level
the GPU tests use holds the edges they are meant to exercise.  The scene checks are conditions: when one fails, the scene changes.
"""
import numpy as np
import pytest

import orc
import prep_ref as pr
import prep_scenes as ps

INF = np.float32(np.inf)
NAN = np.float32(np.nan)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the helpers
def test_zrange_on_hand_made_runs():
    cutoff = 3.0
    d = np.zeros(64 * 4 + 6, np.float32)
    d[17] = 1.5                                   # run 0: one valid depth
    d[64:128] = NAN                               # run 1: all NaN
    d[128:192] = [3.0, 2.0, 2.5, 3.5] * 16        # run 2: a value exactly at the cutoff and one above it are invalid
    d[192:256] = 0                                # run 3: all zero
    d[256:] = [0, NAN, 0.75, 3.0, -1.0, 2.75]     # run 4, clipped at N: a negative depth is valid (z != 0 and z < cutoff)
    got = pr.zrange(d.reshape(1, -1), cutoff)
    want = np.array([[1.5, 1.5], [INF, -INF], [2.0, 2.5], [INF, -INF], [-1.0, 2.75]], np.float32)
    assert got.dtype == np.float32 and got.shape == (5, 2)
    assert np.array_equal(_bits(got), _bits(want))
    # rows do not matter, only the flat index does: 10 x 13 = 130 pixels = two full runs and one of two pixels
    img = np.full((10, 13), 1.0, np.float32); img[9, 11] = 0.5; img[9, 12] = 2.0; img[0, 0] = 0.25
    assert np.array_equal(pr.zrange(img, cutoff), np.array([[0.25, 1.0], [1.0, 1.0], [0.5, 2.0]], np.float32))


def test_occupancy_on_hand_made_blocks():
    v4 = np.zeros((4, 12, 4), np.float32)
    v4[..., 0] = 7.0                              # x and y do not matter
    v4[2, 5, 2] = NAN                             # block 1: its only non-zero z is NaN -> occupied
    v4[3, 11, 2] = -0.5                           # block 2: a negative z is occupied
    v4[1, 1, 2] = -0.0                            # block 0: -0.0 == 0 -> empty
    assert pr.occupancy(v4).tolist() == [[0, 1, 1]]


def test_bounding_keys_on_hand_made_vertices():
    v4 = np.zeros((8, 16, 4), np.float32)
    assert pr.bounding_keys(v4).tolist() == [0] * 6 and pr.describe_keys(pr.bounding_keys(v4)) == "empty"
    v4[2, 3] = (0.1, 0.2, 2.0, 1)
    v4[6, 9] = (0.3, 0.1, -1.0, 1)                # a negative depth is the lower bound
    v4[0, 15] = (NAN, 0.1, 9.0, 1)                # NaN x: not part of the box
    v4[7, 0] = (0.1, 0.1, NAN, 1)                 # NaN z: not part of the box
    keys = pr.bounding_keys(v4)
    # key(f) of the bits u of f: u ^ 0x80000000 for a positive float, ~u for a negative one; the lower bounds complemented
    assert [hex(k) for k in keys] == [hex(~(0x40400000 ^ 0x80000000) & 0xFFFFFFFF),   # x0 = 3.0
                                      hex(~(0x40000000 ^ 0x80000000) & 0xFFFFFFFF),   # y0 = 2.0
                                      hex(0xBF800000),                                # z0 = -1.0: key = ~0xbf800000, complemented
                                      hex(0x41100000 ^ 0x80000000),                   # x1 = 9.0
                                      hex(0x40C00000 ^ 0x80000000),                   # y1 = 6.0
                                      hex(0x40000000 ^ 0x80000000)]                   # z1 = 2.0
    assert pr.describe_keys(keys) == (3.0, 2.0, -1.0, 9.0, 6.0, 2.0)
    # the key map keeps the order of the floats, negative depths included, and key_float is its inverse
    fs = [-np.inf, -2.0, -1.0, -2.0 ** -100, -0.0, 0.0, 2.0 ** -100, 1.0, 2.0, np.inf]
    ks = [pr.float_key(f) for f in fs]
    assert ks == sorted(ks) and len(set(ks)) == len(ks)
    assert [pr.key_float(k) for k in ks] == fs and np.signbit(pr.key_float(ks[4]))


def test_candidates_on_a_hand_made_image():
    rows, cols = 6, 12
    img = np.full((rows, cols), 10, np.uint8)
    img[2, 3] = 0                                 # in the window [y-2, y+2) x [x-2, x+2) of x in 2..5, y in 1..4
    depth = np.ones((rows, cols), np.float32)
    depth[0, 0] = NAN
    dx = np.full((rows, cols), 40, np.int16)      # 40^2 = 1600 >= min_scale of level 0
    dy = np.zeros((rows, cols), np.int16)
    dx[5, 0] = 39; dy[5, 0] = 8                   # 1521 + 64 = 1585 < 1600 (and the last row is outside the margin anyway)
    dx[0, 6] = 39; dy[0, 6] = 8                   # gradient too small, inside the margin
    dx[1, 0] = -24; dy[1, 0] = 32                 # 576 + 1024 = 1600: equal passes
    want = np.array([[0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0],     # margin: x < 12 - 5 = 7, y < 6 - 1 = 5
                     [1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0],
                     [1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0],
                     [1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0],
                     [1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
    assert pr.min_scale(0) == np.float32(1600) and pr.min_scale(1) == np.float32(576) and pr.min_scale(2) == np.float32(64)
    got = pr.candidates(img, depth, dx, dy, pr.min_scale(0))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # a zero in the clamped-away part of a window does not exist: the top-left pixel looks at [0, 2) x [0, 2) only
    img2 = np.full((rows, cols), 10, np.uint8); img2[0, 2] = 0
    got2 = pr.candidates(img2, np.ones((rows, cols), np.float32), np.full((rows, cols), 40, np.int16), dy, pr.min_scale(0))
    assert got2[0, 0] == 1 and got2[0, 1] == 0 and got2[2, 4] == 0 and got2[3, 4] == 1 and got2[1, 5] == 1


# ---------------------------------------------------------------------------------------------- the scenes
@pytest.mark.parametrize("shape", ps.SHAPES)
def test_scene_depth_runs(shape):
    """every level: a run without a valid depth, a clipped last run (with a valid depth) where N % 64 != 0, and every kind of invalid
    depth at level 0.  A level of one run has its empty run in the all-invalid pyramid the GPU test also prepares."""
    s = ps.scene(*shape)
    for lvl in range(3):
        d = s["depth_pyr"][lvl]
        n = d.size
        zr = pr.zrange(d, ps.CUTOFF)
        blank = pr.zrange(s["blank_pyr"][lvl], ps.CUTOFF)
        assert np.isinf(blank).all() and blank.shape == zr.shape
        empty = np.isinf(zr[:, 0])
        assert not empty.all(), "the defected pyramid keeps valid depths"
        if zr.shape[0] >= 2:
            assert empty.any(), f"{shape} L{lvl}: no run without a valid depth"
            assert (~empty).sum() >= 1
        if n % 64:
            assert zr.shape[0] == n // 64 + 1 and not empty[-1], f"{shape} L{lvl}: the clipped run holds no valid depth"
    d0 = s["depth_pyr"][0]
    # a depth exactly at the cutoff in a run that also holds valid ones: counting it as valid would move that run's maximum
    at = (d0.reshape(-1) == np.float32(ps.CUTOFF))
    zr0 = pr.zrange(d0, ps.CUTOFF)
    assert any(np.isfinite(zr0[i // 64, 1]) for i in np.nonzero(at)[0]), f"{shape}: no depth at the cutoff beside valid ones"
    assert (d0 == 0).any() and np.isnan(d0).any() and (d0 == np.float32(ps.CUTOFF)).any() and (d0 > ps.CUTOFF).any()
    if shape != (16, 4):
        assert any(s["depth_pyr"][l].size % 64 for l in range(3)), "a shape with a clipped run"


@pytest.mark.parametrize("shape", ps.SHAPES)
def test_scene_predictions(shape):
    """an empty and an occupied 4x4 block, a single hole inside an occupied block, a NaN x with a valid z, a NaN z -- in the full, the
    rectangle and the alternative prediction; the rectangle is not aligned to the 16 x 4 tiles and its two NaN vertices lie outside"""
    s = ps.scene(*shape)
    W, H = shape
    for name in ("v4", "v4_rect", "alt_v4"):
        v4 = s[name]
        occ = pr.occupancy(v4)
        assert occ.shape == (H // 4, W // 4) and (occ == 0).any() and (occ == 1).any(), name
        z = v4[..., 2]
        zero_in_occupied = (z == 0) & np.repeat(np.repeat(occ, 4, 0), 4, 1).astype(bool)
        assert zero_in_occupied.any(), name
        assert (np.isnan(v4[..., 0]) & ~np.isnan(z) & (z != 0)).any() and np.isnan(z).any(), name
        assert pr.bounding_keys(v4).any(), name
    x0, x1, y0, y1 = s["rect"]
    assert x0 % 16 and x1 % 16 and y0 % 4 and y1 % 4
    box = pr.describe_keys(pr.bounding_keys(s["v4_rect"]))
    assert x0 <= box[0] and box[3] <= x1 - 1 and y0 <= box[1] and box[4] <= y1 - 1, (box, s["rect"])
    occ = pr.occupancy(s["v4_rect"])
    assert occ[(y0 - 1) // 4, (x0 - 3) // 4] == 1 and occ[y1 // 4, (x1 + 2) // 4] == 1, "the NaN vertices outside the box are occupied blocks"
    # the alternative images differ from the prediction's in content and in holes
    assert (pr.occupancy(s["alt_v4"]) != pr.occupancy(s["v4"])).any()
    assert (s["alt_img"] != s["img"]).any() and (s["rgba2"] != s["rgba1"]).any()


def _window_has_zero(src, x, y):
    """does the Gaussian pyramid's clamped 5x5 window of destination pixel (x, y) hold a zero intensity?  (oracle/orc_track.c:
    orc_pyrdown_gauss_u8: rows [2y-2, min(2y+3, srows-1)), likewise columns)"""
    srows, scols = src.shape
    win = src[max(2 * y - 2, 0):min(2 * y + 3, srows - 1), max(2 * x - 2, 0):min(2 * x + 3, scols - 1)]
    return win.size > 0 and (win == 0).any()


@pytest.mark.parametrize("shape", ps.SHAPES)
def test_scene_zero_intensities_reach_the_pyramid_windows(shape):
    """both pyramid steps of the frame image and of the prediction image: a border pixel and (where the level has any) an interior pixel
    whose 5x5 source window holds a zero intensity"""
    s = ps.scene(*shape)
    for name in ("rgba1", "img"):
        src = orc.rgba_to_intensity(s[name])
        assert (src == 0).any()
        for step in range(2):
            srows, scols = src.shape
            border = interior = have_interior = False
            for y in range(srows // 2):
                for x in range(scols // 2):
                    inside = 2 * x - 2 >= 0 and 2 * y - 2 >= 0 and 2 * x + 3 <= scols - 1 and 2 * y + 3 <= srows - 1
                    have_interior |= inside
                    if _window_has_zero(src, x, y):
                        border |= not inside
                        interior |= inside
            assert border, f"{shape} {name} step {step}: no border window with a zero"
            assert interior or not have_interior, f"{shape} {name} step {step}: no interior window with a zero"
            src = orc.pyrdown_gauss_u8(src)


@pytest.mark.parametrize("shape", ps.TRACKED)
@pytest.mark.parametrize("pred", ["full", "rect"])
def test_scene_candidates(shape, pred):
    """every level: a candidate and a non-candidate inside the margin, a pixel rejected only by a zero intensity in its window, one rejected
    only by a NaN depth; and every valid correspondence of the oracle's residual pass lies on a candidate pixel"""
    o = ps.oracle_tracked(*shape, pred)
    W, H = shape
    for lvl in range(3):
        img, depth, dx, dy = o[7][lvl], o[5][lvl], o[9][lvl], o[10][lvl]
        assert np.array_equal(dx, orc.sobel(img)[0]) and np.array_equal(dy, orc.sobel(img)[1]), "dIdx / dIdy are the Sobel of nextImage"
        margin, window, gradient, dok = pr.candidate_terms(img, depth, dx, dy, pr.min_scale(lvl))
        cand = pr.candidates(img, depth, dx, dy, pr.min_scale(lvl)).astype(bool)
        assert (cand & margin).any() and (~cand & margin).any(), f"{shape} L{lvl}"
        if pred == "full":
            # a candidate in the last column of the margin (x == cols - 6) and a would-be candidate just outside of it (x == cols - 5)
            cols = W >> lvl
            assert cand[:, cols - 6].any() and (~margin & window & gradient & dok)[:-1, cols - 5].any(), f"{shape} L{lvl}: the margin decides nothing"
            assert (margin & ~window & gradient & dok).any(), f"{shape} L{lvl}: nothing rejected only by a zero intensity"
            assert (margin & window & gradient & ~dok).any(), f"{shape} L{lvl}: nothing rejected only by a NaN depth"
        # cross-check with the oracle's own residual pass at an identity motion
        K = np.array([[o["cam"].fx / (1 << lvl), 0, o["cam"].cx / (1 << lvl)], [0, o["cam"].fy / (1 << lvl), o["cam"].cy / (1 << lvl)], [0, 0, 1]])
        for dT in (np.eye(4), ps.common.perturbed_pose(11, 0.003, 0.2).astype(np.float64)):
            krkinv = (K @ dT[:3, :3] @ np.linalg.inv(K)).astype(np.float32)
            kt = (K @ dT[:3, 3]).astype(np.float32)
            cor, _, cnt = orc.rgb_residual(float(pr.min_scale(lvl)), dx, dy, o[4][lvl], depth, o[6][lvl], img, 0.07, kt, krkinv)
            valid = cor["valid"].reshape(H >> lvl, W >> lvl) != 0
            assert cnt == valid.sum() and (cnt > 0 or lvl == 2), f"{shape} L{lvl}: the residual pass finds nothing"
            assert not (valid & ~cand).any(), f"{shape} L{lvl}: a valid correspondence on a non-candidate pixel"


def test_oracle_tracks_the_defected_scenes():
    """the tracked shapes still give the Gauss-Newton loop something to do: the oracle ends with correspondences on the full and on the
    rectangle prediction (a loop that runs away ends on the divergence guard with none, and its screen box falls back to the image)"""
    for shape in ps.TRACKED:
        for pred in ("full", "rect"):
            o = ps.oracle_tracked(*shape, pred)
            assert o["icp_count"] > 300 and o["rgb_count"] > 300, (shape, pred, o["icp_count"], o["rgb_count"])
