"""Named cases of the re-detection score: small frames and crafted surfel maps whose counts are known BY CONSTRUCTION,
shared by tests/test_cpu_redetect_cases.py (the numpy statement against the construction) and tests/test_redetect_gpu.py (the device
against the statement, for equality).

Two image sizes: 64x48, and 70x46 whose pixel count is no multiple of 32 (the last bitmap word is partly used) nor of 16 bytes.  The
focal length is a power of two and the principal point the image centre, so that "u exactly cols" is exact in f32; a surfel meant for
pixel (px, py) sits on the ray through the pixel's centre, half a pixel from every rounding boundary.  Depths, the tolerance and the
gate offsets are binary fractions in [1, 2): the sums at the two gates are exact and an offset of k ulp is k * 2^-23."""
import numpy as np

F = np.float32
SIZES = ((64, 48), (70, 46))
CUTOFF = F(3.0)
TOL = F(0.125)
L = 7                 # the new label
THETA = F(0.5)
ULP = F(2.0 ** -23)   # of every f32 in [1, 2)
GATE_K = (-3, -1, 0, 1, 3)


def cam_of(size):
    w, h = size
    return (F(64.0), F(64.0), F(w / 2.0), F(h / 2.0))


def pose_z(tz):
    """model <- camera pose whose inverse moves a point by +tz along z: ph.z = fl(z + tz), one rounding"""
    p = np.eye(4, dtype=F)
    p[2, 3] = -F(tz)
    return p


def surfels_at(size, pixels, z, conf=1.0, offset=(0.5, 0.5)):
    """surfels [n, 12] on the rays through `pixels` ((px, py) pairs, + offset) at camera depth z (scalar or per surfel)"""
    fx, fy, cx, cy = cam_of(size)
    px = np.asarray([p[0] for p in pixels], F) + F(offset[0])
    py = np.asarray([p[1] for p in pixels], F) + F(offset[1])
    z = np.broadcast_to(np.asarray(z, F), px.shape).astype(F)
    s = np.zeros((px.size, 12), F)
    s[:, 0] = (px - cx) * z / fx
    s[:, 1] = (py - cy) * z / fy
    s[:, 2] = z
    s[:, 3] = F(conf)
    s[:, 7] = 1.0      # (rows 1 and 2 are not read by the score)
    s[:, 10] = -1.0
    s[:, 11] = 0.01
    return s


def patch(size, frac=0.5):
    """a rectangle of pixels in the middle of the image, row-major (px, py) pairs"""
    w, h = size
    pw, phh = max(2, int(w * frac)) // 2 * 2, max(2, int(h * frac))
    x0, y0 = (w - pw) // 2, (h - phh) // 2
    return [(x, y) for y in range(y0, y0 + phh) for x in range(x0, x0 + pw)]


def frame(size, wall=2.5):
    w, h = size
    return np.full((h, w), wall, F), np.zeros((h, w), np.uint8)


def put(img, pixels, value):
    for x, y in pixels:
        img[y, x] = value


class Case:
    """depth, label and the candidates [(surfels, theta, pose)]; expect[k]: the counts of candidate k known by construction (a dict of
    some or all of the six counts; None: none claimed), label_pixels likewise"""

    def __init__(self, name, size, depth, label, cands, expect, n_label_pixels, cutoff=CUTOFF, tol=TOL, new_label=L):
        self.name, self.size, self.depth, self.label, self.cands, self.expect = name, size, depth, label, cands, expect
        self.label_pixels, self.cutoff, self.tol, self.new_label, self.cam = n_label_pixels, cutoff, tol, new_label, cam_of(size)


def counts(projected=0, occluded=0, seen_through=0, agree=0, agree_on_label=0, covered=0):
    return dict(projected=projected, occluded=occluded, seen_through=seen_through, agree=agree, agree_on_label=agree_on_label, covered=covered)


I4 = np.eye(4, dtype=F)


def _exact_patch(size):
    px = patch(size); k = len(px)
    d, lab = frame(size); put(d, px, 1.5); put(lab, px, L)
    return Case("exact_patch", size, d, lab, [(surfels_at(size, px, 1.5), THETA, I4)], [counts(k, 0, 0, k, k, k)], k)


def _two_per_pixel(size):
    px = patch(size); k = len(px)
    d, lab = frame(size); put(d, px, 1.5); put(lab, px, L)
    s = np.concatenate([surfels_at(size, px, 1.5, offset=(0.25, 0.5)), surfels_at(size, px, 1.5, offset=(0.75, 0.25))])
    return Case("two_per_pixel", size, d, lab, [(s, THETA, I4)], [counts(2 * k, 0, 0, 2 * k, 2 * k, k)], k)


def _gate(size, behind):
    """the map stands tol + k ulp behind (in front of) the measured surface: d = 1.5, ph.z = 1.5 +- 0.125 + k ulp, all sums exact.
    behind: lo = ph.z - tol = 1.5 + k ulp, occluded iff d < lo iff k > 0.  In front: hi = ph.z + tol = 1.5 + k ulp, seen through iff
    d > hi iff k < 0.  Otherwise the surfel agrees (both gates are inclusive)."""
    px = patch(size, 0.25); n = len(px)
    d, lab = frame(size); put(d, px, 1.5); put(lab, px, L)
    cands, expect = [], []
    for k in GATE_K:
        phz = F(F(1.625) if behind else F(1.375)) + F(k) * ULP
        s = surfels_at(size, px, phz)
        s[:, 2] = 1.0                                  # stored at z = 1, moved to ph.z by the pose: fl(1 + tz) = ph.z exactly
        cands.append((s, THETA, pose_z(phz - F(1.0))))
        if behind:
            expect.append(counts(n, n, 0, 0, 0, 0) if k > 0 else counts(n, 0, 0, n, n, n))
        else:
            expect.append(counts(n, 0, n, 0, 0, 0) if k < 0 else counts(n, 0, 0, n, n, n))
    return Case("behind_gate" if behind else "before_gate", size, d, lab, cands, expect, n)


def _occluded_half(size):
    px = patch(size); k = len(px); near = px[: k // 2]
    d, lab = frame(size); put(d, px, 1.5); put(lab, px, L); put(d, near, 1.0)
    return Case("occluded_half", size, d, lab, [(surfels_at(size, px, 1.5), THETA, I4)],
                [counts(k, k // 2, 0, k - k // 2, k - k // 2, k - k // 2)], k)


def _gone(size):
    px = patch(size); k = len(px)
    d, lab = frame(size)                               # only the wall at 2.5 m is seen; the label is on another region
    other = [(x, y) for x in range(3) for y in range(3)]; put(lab, other, L)
    return Case("gone", size, d, lab, [(surfels_at(size, px, 1.5), THETA, I4)], [counts(k, 0, k, 0, 0, 0)], len(other))


def _off_label(size):
    px = patch(size); k = len(px)
    d, lab = frame(size); put(d, px, 1.5); put(lab, px, L + 1)
    other = [(x, y) for x in range(4) for y in range(2)]; put(lab, other, L)
    return Case("off_label", size, d, lab, [(surfels_at(size, px, 1.5), THETA, I4)], [counts(k, 0, 0, k, 0, 0)], len(other))


def _invalid_depth(size):
    px = patch(size); k = len(px)
    d, lab = frame(size); put(d, px, 1.5); put(lab, px, L)
    bad = [0.0, float(CUTOFF) + 0.5, float("nan"), -1.0, float("inf")]
    n_bad = 0
    for i, p in enumerate(px):
        if i % 3 != 2:
            put(d, [p], bad[i % len(bad)]); n_bad += 1
    put(d, [px[2]], float(CUTOFF))                      # d == cutoff is still valid: 3.0 > 1.5 + tol -> seen through
    return Case("invalid_depth", size, d, lab, [(surfels_at(size, px, 1.5), THETA, I4)],
                [counts(k, 0, 1, k - n_bad - 1, k - n_bad - 1, k - n_bad - 1)], k)


def _rejects(size):
    w, h = size
    fx, fy, cx, cy = cam_of(size)
    d, lab = frame(size, wall=1.0); lab[:] = L
    ok = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2)]
    s = [surfels_at(size, ok, 1.0)]
    s.append(surfels_at(size, [(w // 2, h // 2)], -1.0))                       # z < 0
    s.append(surfels_at(size, [(w // 2, h // 2)], float(CUTOFF)))             # z == cutoff
    s.append(surfels_at(size, [(w // 2, h // 2)], float(CUTOFF) + 1.0))       # z > cutoff
    s.append(surfels_at(size, [(0, 3)], 1.0, offset=(-0.25, 0.5)))            # u just left of the image
    s.append(surfels_at(size, [(w, 3)], 1.0, offset=(0.25, 0.5)))             # ... right
    s.append(surfels_at(size, [(3, 0)], 1.0, offset=(0.5, -0.25)))            # v just above
    s.append(surfels_at(size, [(3, h)], 1.0, offset=(0.5, 0.25)))             # ... below
    s.append(surfels_at(size, [(w, 3)], 1.0, offset=(0.0, 0.5)))              # u exactly cols
    s.append(surfels_at(size, [(3, h)], 1.0, offset=(0.5, 0.0)))              # v exactly rows
    edge = surfels_at(size, [(0, 5), (5, 0)], 1.0, offset=(0.0, 0.0))          # u (v) exactly 0: inside
    edge[0, 1] = (F(5.5) - cy) / fy
    edge[1, 0] = (F(5.5) - cx) / fx
    s.append(edge)
    zero = surfels_at(size, [(w // 2, h // 2)], 1.0); zero[:, :3] = 0           # the camera centre: 0 / 0
    s.append(zero)
    n_in = len(ok) + 2
    return Case("rejects", size, d, lab, [(np.concatenate(s), THETA, I4)], [counts(n_in, 0, 0, n_in, n_in, n_in)], w * h)


def _unstable(size):
    px = patch(size, 0.25); k = len(px)
    d, lab = frame(size); put(d, px, 1.5); put(lab, px, L)
    s = surfels_at(size, px, 1.5)
    s[0::4, 3] = np.nextafter(THETA, F(0))      # just below: out
    s[1::4, 3] = THETA                          # equal: in
    s[2::4, 3] = np.nan                         # out
    s[3::4, 3] = np.nextafter(THETA, F(1))      # in
    n_in = len(range(1, k, 4)) + len(range(3, k, 4))
    return Case("unstable", size, d, lab, [(s, THETA, I4)], [counts(n_in, 0, 0, n_in, n_in, n_in)], k)


COUNT_SIZES = (0, 1, 63, 64, 65, 257, 5000)


def _counted_map(size, px, n):
    """n surfels dealt over the pixels of px in turn (more than one per pixel beyond len(px))"""
    return surfels_at(size, [px[i % len(px)] for i in range(n)], 1.5) if n else np.zeros((0, 12), F)


def _counts(size):
    px = patch(size); k = len(px)
    d, lab = frame(size); put(d, px, 1.5); put(lab, px, L)
    cands = [(_counted_map(size, px, n), THETA, I4) for n in COUNT_SIZES]
    return Case("counts", size, d, lab, cands, [counts(n, 0, 0, n, n, min(n, k)) for n in COUNT_SIZES], k)


def _batch_mixed(size, n_cands):
    """n_cands candidates of different sizes in one call -- one of them empty (the second, when there is one), some off the label"""
    px = patch(size); k = len(px)
    d, lab = frame(size); put(d, px, 1.5); put(lab, px[: k // 2], L)
    sizes = [300, 0, 65, 1, 1000, 64, 2049, 17, 128][:n_cands]
    cands, expect = [], []
    for j, n in enumerate(sizes):
        sub = px[j:] if j % 2 else px                      # (different pixel sets per candidate: their bitmaps must not mix)
        cands.append((_counted_map(size, sub, n), THETA, I4))
        hit = [sub[i % len(sub)] for i in range(n)]
        on = [p for p in hit if lab[p[1], p[0]] == L]
        expect.append(counts(n, 0, 0, n, len(on), len(set(on))))
    return Case(f"batch_mixed_{n_cands}", size, d, lab, cands, expect, k // 2)


def _posed(size):
    """no construction behind this one: random maps under rotated poses against a noisy frame -- the kernel against the statement only"""
    w, h = size
    rng = np.random.default_rng(99 + w)
    d = rng.uniform(0.8, 2.6, size=(h, w)).astype(F); d[rng.random((h, w)) < 0.1] = 0
    lab = rng.integers(0, 3, size=(h, w)).astype(np.uint8) * np.uint8(L)   # 0, L, 2L
    cands = []
    for j in range(3):
        n = (700, 2500, 129)[j]
        s = np.zeros((n, 12), F)
        s[:, :3] = rng.uniform([-1.5, -1.2, -0.5], [1.5, 1.2, 3.5], size=(n, 3))
        s[:, 3] = rng.uniform(0.0, 1.0, size=n)
        a = rng.normal(size=3); a /= np.linalg.norm(a); ang = 0.3 * (j + 1)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        p = np.eye(4)
        p[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        p[:3, 3] = rng.uniform(-0.2, 0.2, size=3)
        cands.append((s, THETA, p.astype(F)))
    return Case("posed", size, d, lab, cands, [None] * 3, None)


BUILDERS = {
    "exact_patch": _exact_patch, "two_per_pixel": _two_per_pixel, "behind_gate": lambda s: _gate(s, True), "before_gate": lambda s: _gate(s, False),
    "occluded_half": _occluded_half, "gone": _gone, "off_label": _off_label, "invalid_depth": _invalid_depth, "rejects": _rejects,
    "unstable": _unstable, "counts": _counts, "batch_mixed_1": lambda s: _batch_mixed(s, 1), "batch_mixed_3": lambda s: _batch_mixed(s, 3),
    "batch_mixed_9": lambda s: _batch_mixed(s, 9), "posed": _posed,
}
NAMES = tuple(BUILDERS)
_CACHE = {}


def get(name, size):
    key = (name, tuple(size))
    if key not in _CACHE:
        _CACHE[key] = BUILDERS[name](tuple(size))
    return _CACHE[key]
