"""The case table of the SO(3) pre-alignment launch (plain helper module, no tests in here).

Every content case is a pair of 8-bit level-2 intensity images (last, next) generated from formulas and seeds -- no files -- at each of
three shapes, with the camera fx = fy = 0.825 cols, cx = (cols - 1) / 2 - 0.375, cy = (rows - 1) / 2 - 0.375 at level 2 (the tracker
state carries the level-0 camera: four times that).  The GPU side (tests/test_so3_prealign_gpu.py) sends them through
cf_so3_prealign_step, the production launch on its own; the CPU side (tests/test_cpu_so3_cases.py) through orc_so3_prealign, the loop
of the oracle's tracking function, whose trace says which exit a case takes, at which iteration, with which error and count.
EXPECT below is that record -- (iterations, exit) of every case at every shape --, asserted on the CPU from the trace together with
the property each case is named for.

Shapes (context size -> level-2 size): 160 x 120 -> 40 x 30 (1200 pixels under 4096 threads: most workgroups of the launch have no
pixel), 176 x 132 -> 44 x 33 (an odd row count, rows that straddle waves), 640 x 480 -> 160 x 120 (the only one where the grid stride
loops: 4.69 passes, a ragged last one).

The cases, and what the oracle's trace shows for them:
 * identical: last == next, the multi-sine texture.  Ten iterations, error 0, count (cols - 2)(rows - 2), the rotation stays the
   identity bit for bit.
 * rot_small / rot_mid / rot_large / rot_wide: next is the same analytic texture sampled through K R K^-1 (no interpolation), axis
   (0.3, 1, 0.2), 0.01 / 0.03 / 0.08 / 0.2 rad.  Accepted steps, then the error-rose exit at iteration 3 (the small shapes), 5 or 6
   (rot_wide), or all ten iterations at 160 x 120.  The oracle's rotation is within 0.07 of the true angle of the true rotation (float64
   geodesic distance), which tests/test_cpu_so3_cases.py bounds by one half.
 * revert_to_identity: the 0.015 rad pair, which at 40 x 30 is left at iteration 2: the result is lastResultR, the identity, error and
   count those of iteration 1.  (At the other two shapes the same pair leaves at iteration 3 with a rotation; the property the case is
   named for is asserted at 160 x 120.)
 * noise: two independent uniform-noise images.  The first steps change nothing the rounding to pixels sees -- error and count repeat
   bit for bit -- while the rotation accumulates, until pixels move: a revert at iteration 6 (40 x 30) or 9 (44 x 33), or ten iterations.
 * stripes: vertical stripes of period 8, next shifted one column: no gradient along y.  One step, then error exactly 0 for nine more
   iterations.  (In float32 the rank-deficient matrix has tiny non-zero pivots: no pivot is taken as zero.)
 * flat / flat_offset: constant images, equal or 8 apart.  The matrix is all zero, three zero pivots in every solve, the update is zero
   (ldlt_solve / orc_ldlt_f give a zero component for a zero pivot): ten iterations at a constant error (0, or 8 / sqrt(count)), the
   identity bit for bit.
 * extreme: alternating 0 / 255 columns against their inverse.  The central differences of a period-2 pattern are exactly zero, so
   this is a third all-zero matrix, under the largest residual 8 bits can give (255 at every pixel): ten iterations, identity.
 * ejected: a slow ramp (x // 2) against the same ramp + 150: gradients of half a grey level under a residual of 150 give a first step
   of many radians, which throws every pixel out of the image.  From iteration 2 on the count is 0 and the error sqrtf(0) / 0 = NaN;
   both comparisons of the loop are false on NaN, so it solves the zero matrix and goes on, through iteration 10.  last_so3_error is NaN.
 * saturated: the texture with a 0 / 255 step two columns wide each, next shifted one column, under a camera of 256 times the focal
   length: the Jacobian entries of the step's columns (|fx gx| = 127.5 fx) exceed the fixed-point clamp 2^19 of the row entries, in
   a few hundred pixels only, so that the 64-bit sums stay far from wrapping.  Reverts at iteration 2.

NOT COVERED, so that nobody takes the table for complete: the "converged" exit (RGBDOdometry.cpp:285 compares the previous ERROR with
the pixel COUNT, sic).  It needs |lastError - count| < 0.001, and with 8-bit images the error is at most 255 / sqrt(count), so the
count must be below about 40 -- no admissible image size under a near-identity warp has that few pixels inside the border.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

import orc

SEED = 20262
SHAPES = ((160, 120), (176, 132), (640, 480))          # context (level-0) sizes; level 2 is a quarter of each
AXIS = (0.3, 1.0, 0.2)
ANGLES = {"rot_small": 0.01, "rot_mid": 0.03, "rot_large": 0.08, "rot_wide": 0.2, "revert_to_identity": 0.015}
CAMERA_SCALE = {"saturated": 256.0}
CLAMP = float(1 << 19)                                 # of the SO(3) row entries: 2^((50 - 12) / 2)
GEODESIC_CAP = 0.5                                     # the pre-alignment beats doing nothing by 2x (a condition on the inputs)

CONTENT = ("identical", "rot_small", "rot_mid", "rot_large", "rot_wide", "revert_to_identity", "noise", "stripes", "flat", "flat_offset",
           "extreme", "ejected", "saturated")
# (iterations, exit) per shape, in the order of SHAPES; exit "ten": all ten iterations ran
EXPECT = {
    "identical": ((10, "ten"), (10, "ten"), (10, "ten")),
    "rot_small": ((3, "reverted"), (3, "reverted"), (3, "reverted")),
    "rot_mid": ((3, "reverted"), (3, "reverted"), (10, "ten")),
    "rot_large": ((3, "reverted"), (3, "reverted"), (10, "ten")),
    "rot_wide": ((6, "reverted"), (5, "reverted"), (10, "ten")),
    "revert_to_identity": ((2, "reverted"), (3, "reverted"), (3, "reverted")),
    "noise": ((6, "reverted"), (9, "reverted"), (10, "ten")),
    "stripes": ((10, "ten"), (10, "ten"), (10, "ten")),
    "flat": ((10, "ten"), (10, "ten"), (10, "ten")),
    "flat_offset": ((10, "ten"), (10, "ten"), (10, "ten")),
    "extreme": ((10, "ten"), (10, "ten"), (10, "ten")),
    "ejected": ((10, "ten"), (10, "ten"), (10, "ten")),
    "saturated": ((2, "reverted"), (2, "reverted"), (2, "reverted")),
}


def level2(shape):
    return shape[0] >> 2, shape[1] >> 2


def camera2(cols, rows, scale=1.0):
    """the level-2 camera (fx, fy, cx, cy) in float32"""
    f = np.float32(0.825 * cols * scale)
    return f, f, np.float32((cols - 1) / 2 - 0.375), np.float32((rows - 1) / 2 - 0.375)


def camera0(cols, rows, scale=1.0):
    """the level-0 camera the state carries (orc.Cam): dividing by 4 is exact, so level 2 gets camera2 back bit for bit"""
    return orc.Cam(*[float(np.float32(4) * v) for v in camera2(cols, rows, scale)])


def rotation(axis, angle):
    """Rodrigues in float64"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    X = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * X + (1 - math.cos(angle)) * X.dot(X)


def geodesic(Ra, Rb):
    """angle of Ra^T Rb in float64 (atan2 of the skew part's norm and the trace: accurate near zero)"""
    D = np.asarray(Ra, np.float64).T.dot(np.asarray(Rb, np.float64))
    s = 0.5 * math.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return math.atan2(s, 0.5 * (np.trace(D) - 1))


# ------------------------------------------------------------------------------------------------------------------- images
def texture(u, v):
    """a smooth multi-sine intensity on normalised coordinates (u = x / cols, v = y / rows; defined on the whole plane), in [0, 255]"""
    t = (0.30 * np.sin(2 * np.pi * (1.1 * u + 0.3 * v) + 0.4) + 0.27 * np.sin(2 * np.pi * (-0.4 * u + 1.3 * v) + 1.9)
         + 0.23 * np.sin(2 * np.pi * (1.7 * u - 0.9 * v) + 2.6) + 0.20 * np.sin(2 * np.pi * (0.8 * u + 1.9 * v) + 0.7))
    return 127.5 + 127.5 * t


def _quantise(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def _grid(cols, rows):
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    return x, y


def _textured(cols, rows):
    x, y = _grid(cols, rows)
    return _quantise(texture(x / cols, y / rows))


def _rotated_pair(cols, rows, angle):
    """last = the texture; next = the same texture seen through K R K^-1, sampled analytically: next(K R K^-1 p) = last(p), so the
    rotation that aligns the pair is R"""
    fx, fy, cx, cy = [float(v) for v in camera2(cols, rows)]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    Hinv = K.dot(rotation(AXIS, angle).T).dot(np.linalg.inv(K))
    x, y = _grid(cols, rows)
    w = Hinv[2, 0] * x + Hinv[2, 1] * y + Hinv[2, 2]
    sx = (Hinv[0, 0] * x + Hinv[0, 1] * y + Hinv[0, 2]) / w
    sy = (Hinv[1, 0] * x + Hinv[1, 1] * y + Hinv[1, 2]) / w
    return _textured(cols, rows), _quantise(texture(sx / cols, sy / rows))


def _pair(name, cols, rows):
    x, _ = _grid(cols, rows)
    if name == "identical":
        a = _textured(cols, rows)
        return a, a.copy()
    if name in ANGLES:
        return _rotated_pair(cols, rows, ANGLES[name])
    if name == "noise":
        rng = np.random.default_rng([SEED, cols, rows])
        return rng.integers(0, 256, (rows, cols), dtype=np.uint8), rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    if name == "stripes":
        f = lambda xx: _quantise(127.5 + 100 * np.sin(2 * np.pi * xx / 8.0))
        return f(x), f(x - 1)
    if name == "flat":
        return np.full((rows, cols), 100, np.uint8), np.full((rows, cols), 100, np.uint8)
    if name == "flat_offset":
        return np.full((rows, cols), 100, np.uint8), np.full((rows, cols), 108, np.uint8)
    if name == "extreme":
        a = np.where(x.astype(np.int64) % 2 == 0, 0, 255).astype(np.uint8)
        return a, (255 - a).astype(np.uint8)
    if name == "ejected":
        a = (x.astype(np.int64) // 2).astype(np.uint8)
        return a, (a + 150).astype(np.uint8)
    if name == "saturated":
        a = _textured(cols, rows)
        c = cols // 2
        a[:, c - 1:c + 1] = 0; a[:, c + 1:c + 3] = 255
        return a, np.roll(a, 1, axis=1)
    raise KeyError(name)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    shape: tuple            # context size (width, height)
    last: np.ndarray        # [rows, cols] uint8, level 2 (read-only)
    next: np.ndarray
    intr: orc.Cam           # level 0

    @property
    def key(self):
        return "%s@%dx%d" % (self.name, self.shape[0], self.shape[1])

    @property
    def expect(self):
        return EXPECT[self.name][SHAPES.index(self.shape)]


@functools.lru_cache(maxsize=None)
def case(name, shape):
    cols, rows = level2(shape)
    last, nxt = (np.ascontiguousarray(a) for a in _pair(name, cols, rows))
    assert last.dtype == nxt.dtype == np.uint8 and last.shape == nxt.shape == (rows, cols)
    last.setflags(write=False); nxt.setflags(write=False)
    return Case(name, shape, last, nxt, camera0(cols, rows, CAMERA_SCALE.get(name, 1.0)))


def content_cases():
    return [case(n, s) for n in CONTENT for s in SHAPES]


def first_rows(c):
    """float64 restatement of the first iteration's Jacobian rows (resultR = identity) of a case: [rows - 2, cols - 2, 3].  Used to
    show that `saturated` reaches the clamp; not a reference of the kernel's arithmetic."""
    cols, rows = level2(c.shape)
    fx, fy, cx, cy = [float(v) for v in camera2(cols, rows, CAMERA_SCALE.get(c.name, 1.0))]
    grad = lambda im: ((im[1:-1, :-2] - im[1:-1, 2:]) / 2.0, (im[:-2, 1:-1] - im[2:, 1:-1]) / 2.0)
    (nx, ny), (lx, ly) = grad(c.next.astype(np.float64)), grad(c.last.astype(np.float64))
    gx, gy = (nx + lx) / 2.0, (ny + ly) / 2.0
    x, y = _grid(cols, rows)
    x, y = x[1:-1, 1:-1], y[1:-1, 1:-1]
    left = np.stack([fx * gx, fy * gy, (cx * gx + cy * gy) - gy * y - gx * x], -1)     # K R = K; point.z = 1
    point = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1)
    return np.cross(left, point)


# ------------------------------------------------------------------------------------------------------------------- batches
S, M, B = SHAPES
# lists of (content case, shape) run in ONE launch, model k on sync block k and on XCD k mod 8
BATCHES = {
    "n1": [("rot_mid", S)],
    # an early exit, a ten-iteration case and a NaN-path case: the models leave at different iterations
    "n3": [("rot_small", S), ("identical", M), ("ejected", S)],
    # models 0 and 8 share an XCD and leave at iterations 6 and 2
    "n9": [("noise", S), ("rot_mid", M), ("flat_offset", S), ("stripes", M), ("rot_wide", S), ("extreme", M), ("identical", B), ("ejected", M),
           ("revert_to_identity", S)],
    # the full batch: every content case, all three shapes
    "n16": [("identical", S), ("rot_small", M), ("rot_mid", B), ("rot_large", S), ("rot_wide", M), ("revert_to_identity", S), ("noise", M),
            ("stripes", S), ("flat", M), ("flat_offset", B), ("extreme", S), ("ejected", B), ("saturated", M), ("noise", S), ("rot_large", B),
            ("saturated", S)],
}


def batch(name):
    return [case(n, s) for n, s in BATCHES[name]]


# --------------------------------------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def reference(name, shape):
    """the oracle's (resultR, stats, trace) of a case, computed once"""
    c = case(name, shape)
    return orc.so3_prealign(c.last, c.next, c.intr, shape[0], shape[1])
