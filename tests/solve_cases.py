"""The case table of the device Gauss-Newton solve (plain helper module, no tests in here).

Every case is a hand-made 6x6 system -- the two grouped accumulators [64][32] of fixed-point words the ICP reduction and the RGB step
would have left -- plus the tracker state the solve reads, and one or more STEPS on it (a step: sums, `next_level`, `last_of_level`,
the ICP format).  The state a step returns is the state of the next step.  The GPU side (tests/test_gn_solve_gpu.py) sends the
cases through cf_gn_solve_step, the production kernel on its own; the CPU side (tests/test_cpu_solve_cases.py and `reference`
below) through orc_gn_solve_step, the same algebra as the oracle's tracking loop runs it, which also returns a trace: the pivot of
every LDL^T step, ties, zero pivots, theta, and which of the identity branch, the stop rule and the guard fired.

Each case aims at ONE branch (`aims`), so that a lane-index slip in the kernel fails with the case's name.  Systems are built from
integers and written into the words exactly; no total reaches 2^53, so the oracle's f32 unpack is the first rounding.

The oracle's own backward error ||Ax - b||inf / (||A||inf ||x||inf + ||b||inf), measured with exact rationals on the combined f64
systems of the well-conditioned families (`pivots`, `modes`; tests/test_cpu_solve_cases.py), has the maximum

    BACKWARD_ERROR_MAX = 6.17e-17   (modes 6.17e-17; pivots 4.45e-20, where the norms are those of the largest column scale; seed 20260)

and the test asserts BACKWARD_ERROR_BOUND = 2^-51 = 4.4e-16, the next power of two above four times that.
"""
from __future__ import annotations

import dataclasses
import functools
import itertools
import math

import numpy as np

import common
import orc

SEED = 20260
GROUPS, WORDS = 64, 32
FLT_MAX = float(np.finfo(np.float32).max)
EPS = 2.0 ** -52                      # the identity branch of Rodrigues: theta < DBL_EPSILON
GRAM_BITS = (20, 20, 20, 17, 17, 17, 22)
FIX_ICP = 32
GRAM = -1
BACKWARD_ERROR_MAX = 6.17e-17
BACKWARD_ERROR_BOUND = 2.0 ** -51
_M64 = 1 << 64


# ---------------------------------------------------------------------------------------------------------------- words and groups
def word_index(i, j):
    """word of the product row_i * row_j, i <= j < 7, i < 6 (j == 6: the right-hand side), in the order of reduce.cu:481-498"""
    assert 0 <= i <= j < 7 and i < 6
    return 7 * i - i * (i - 1) // 2 + (j - i)


def icp_bits(icp_fix, i, j):
    return icp_fix if icp_fix >= 0 else GRAM_BITS[i] + GRAM_BITS[j]


def _i64(v):
    """a Python integer reduced mod 2^64 into the int64 range"""
    return (int(v) + (1 << 63)) % _M64 - (1 << 63)


def icp_totals(A, b, icp_fix, down, res=0, count=12):
    """the 32 ICP totals of the integer system (A, b) / 2^down: word (i, j) = A_ij * 2^(bits_ij - down); [27] = res likewise, [28] = count"""
    t = [0] * WORDS
    for i in range(6):
        for j in range(i, 7):
            v = int(A[i][j]) if j < 6 else int(b[i])
            sh = icp_bits(icp_fix, i, j) - down
            assert sh >= 0
            t[word_index(i, j)] = v << sh
    t[27] = int(res) << ((icp_fix if icp_fix >= 0 else 2 * GRAM_BITS[6]) - down)
    t[28] = int(count)
    return t


def rgb_totals(A, b, bits, down=0):
    """the 32 RGB totals of the integer system (A, b) / 2^down under `bits` fraction bits"""
    t = [0] * WORDS
    assert bits >= down
    for i in range(6):
        for j in range(i, 7):
            t[word_index(i, j)] = (int(A[i][j]) if j < 6 else int(b[i])) << (bits - down)
    return t


def lay(tot, how="g0"):
    """32 totals (Python integers) -> the grouped accumulator [64][32] int64 whose groups sum to them mod 2^64"""
    acc = np.zeros((GROUPS, WORDS), np.int64)

    def add(g, w, v):
        acc[g, w] = _i64(int(acc[g, w]) + v)

    for w, v in enumerate(tot):
        v = int(v)
        if how == "g0":                       # the folded form of acc_fold_kernel
            add(0, w, v)
        elif how == "late":
            add(61, w, v)
        elif how == "even":                   # floor division: negative totals give negative shares, the remainder sits in one group
            q, r = divmod(v, GROUPS)
            acc[:, w] = _i64(q)
            add(37, w, r)
        elif how == "wrap+":                  # four partials of +2^62 (2^64 = 0 mod 2^64) in two of the kernel's slices of eight groups
            add(9, w, v)
            for g in (1, 2, 10, 33):
                add(g, w, 1 << 62)
        elif how == "wrap-":
            add(40, w, v)
            for g in (0, 7, 8, 63):
                add(g, w, -(1 << 62))
        elif how == "wrap63":                 # total + 2^63 and 2^63: the int64 sum overflows, the unsigned one wraps to the total
            add(20, w, v + (1 << 63))
            add(21, w, 1 << 63)
        else:
            raise ValueError(how)
    return acc


def totals(acc):
    """group totals of an accumulator [64][32] in Python integers, reduced mod 2^64 (what the kernel's unsigned sums hold)"""
    rows = [g for g in range(GROUPS) if acc[g].any()]
    return np.array([_i64(sum(int(acc[g, w]) for g in rows)) for w in range(WORDS)], np.int64)


def sigma_val(count, sigma, rgb_only):
    """sigma handed to rgbStep (RGBDOdometry.cpp:373-385): (tmpError == 0) ? 1 : count; -1 in the RGB-only mode"""
    if rgb_only:
        return -1.0
    with np.errstate(all="ignore"):
        tmp = np.float32(np.sqrt(np.float64(sigma)) / np.float64(count))
    return 1.0 if tmp == 0 else float(np.float32(count))


# ------------------------------------------------------------------------------------------------------------------- cases
STATE_FIELDS = ("intr", "width", "height", "icp", "rgb", "rgbOnly", "icpWeight", "Rprev", "tprev", "Rprev_inv", "Rcurr", "tcurr",
                "resultRt", "krkInv", "kt", "lastRGBError", "level_done", "solves", "residual", "pose_inv")


def default_state(**over):
    """the state a fresh tracking call starts its first solve with: identity poses, ICP only, 160 x 120"""
    s = dict(intr=(132.0, 132.0, 79.5, 59.5), width=160, height=120, icp=1, rgb=0, rgbOnly=0, icpWeight=10.0,
             Rprev=np.eye(3, dtype=np.float32), tprev=np.zeros(3, np.float32), Rprev_inv=np.eye(3, dtype=np.float32),
             Rcurr=np.eye(3, dtype=np.float32), tcurr=np.zeros(3, np.float32), resultRt=np.eye(4), krkInv=np.eye(3, dtype=np.float32),
             kt=np.zeros(3, np.float32), lastRGBError=FLT_MAX, level_done=0, solves=0, residual=np.zeros(2, np.float32),
             pose_inv=np.eye(4, dtype=np.float32))
    assert set(over) <= set(s), over
    s.update(over)
    return s


@dataclasses.dataclass
class Step:
    icp: np.ndarray                   # [64][32] int64
    rgb: np.ndarray
    next_level: int = 2
    last_of_level: bool = False
    icp_fix: int = FIX_ICP


@dataclasses.dataclass
class Case:
    name: str
    family: str
    aims: str
    state: dict
    steps: list
    meta: dict = dataclasses.field(default_factory=dict)


_ZERO = lay([0] * WORDS)


def _icp_case(name, family, aims, A, b, *, icp_fix=FIX_ICP, down=0, how="g0", state=None, res=0, count=12, **step):
    """an ICP-only, one-step case of the integer system (A, b)"""
    st = state if state is not None else default_state()
    return Case(name, family, aims, st, [Step(lay(icp_totals(A, b, icp_fix, down, res, count), how), _ZERO, icp_fix=icp_fix, **step)])


def _gram(J, r):
    J = np.asarray(J, object); r = np.asarray(r, object)
    return J.T.dot(J), J.T.dot(r), int(r.dot(r))


def _pivots(rng):
    """every permutation of the column scales 2^(3 rank) on one 12 x 6 integer Jacobian: all 15 transpositions (k, p), p > k"""
    J = rng.integers(-7, 8, (12, 6)); r = rng.integers(-7, 8, 12)
    assert np.linalg.matrix_rank(J) == 6
    out = []
    for perm in itertools.permutations(range(6)):
        Js = np.array([[int(J[k][c]) << (3 * perm[c]) for c in range(6)] for k in range(12)], object)
        A, b, rr = _gram(Js, r)
        out.append(_icp_case("pivots-" + "".join(map(str, perm)), "pivots", "pivot order of column scales 2^(3*%s)" % (perm,), A, b, down=32, res=rr))
    return out


def _sym(d, off=()):
    A = [[0] * 6 for _ in range(6)]
    for i, v in enumerate(d):
        A[i][i] = v
    for i, j, v in off:
        A[i][j] = A[j][i] = v
    return A


def _ties():
    b = [3, -5, 7, -2, 6, -4]
    t = [
        ("all-equal", "six equal diagonals at every step: no swap is allowed", _sym([8] * 6)),
        ("all-equal-coupled", "six equal diagonals at step 0 of a dense matrix", _sym([8] * 6, [(0, 1, 1), (1, 2, -1), (2, 3, 1), (3, 4, 1), (4, 5, -1), (0, 5, 2)])),
        ("first-of-two", "the maximum twice, at 2 and 4: the first wins, and it is a real swap", _sym([1, 2, 8, 3, 8, 4])),
        ("last-then-equal", "step 0 swaps (0, 5), then the rest ties at steps 1 to 4", _sym([1, 1, 1, 1, 1, 8])),
        ("late-pair", "distinct diagonals until the last two tie at step 4", _sym([32, 16, 8, 4, 2, 2])),
        ("late-triple", "ties at steps 3 and 4 only", _sym([32, 16, 8, 2, 2, 2])),
        ("late-coupled", "step 0 lowers a_33 below its equals: 4 and 5 tie at step 3, 4 wins, a swap (3, 4)", _sym([32, 16, 8, 2, 2, 2], [(0, 3, 1)])),
        ("opposite-signs", "equal magnitudes of opposite sign on a symmetric indefinite matrix: |4| = |-4|, the first wins",
         _sym([4, -4, 2, -2, 1, -1], [(0, 1, 1), (2, 3, 1), (4, 5, 1), (1, 4, -1)])),
        ("opposite-signs-late", "the negative of a tied pair comes first", _sym([-1, 1, -8, 8, 2, -2], [(0, 2, 1), (3, 5, 1)])),
    ]
    return [_icp_case("ties-" + n, "ties", aims, A, b) for n, aims, A in t]


def _zero_pivots(rng):
    out = []
    Z = _sym([0] * 6)
    out.append(_icp_case("zero-all", "zero pivots", "the all-zero system: six zero pivots, a zero update", Z, [0] * 6, count=0))
    out.append(_icp_case("zero-all-rhs", "zero pivots", "a zero matrix under a non-zero right-hand side still gives zero", Z, [1, -2, 3, -4, 5, -6]))
    j = [1, 2, 4, 8, 16, 32]   # powers of two: the rank-one elimination is exact, five exact zero pivots
    out.append(_icp_case("zero-one-row", "zero pivots", "one Jacobian row: five exact zero pivots", *_gram([j], [3])[:2]))
    for name, cols in (("translation-only", (0, 1, 2)), ("rotation-only", (3, 4, 5)), ("single-column", (4,)), ("two-columns", (1, 5)),
                       ("four-columns", (0, 2, 3, 5)), ("five-columns", (0, 1, 2, 3, 4))):
        J = np.zeros((12, 6), np.int64)
        J[:, cols] = rng.integers(-7, 8, (12, len(cols)))
        A, b, rr = _gram(J, rng.integers(-7, 8, 12))
        out.append(_icp_case("zero-" + name, "zero pivots", "only columns %s are non-zero: %d exact zero pivots" % (cols, 6 - len(cols)), A, b, res=rr))
    out.append(_icp_case("zero-dup-blocks", "zero pivots", "three [[p, p], [p, p]] blocks with power-of-two p: three exact zero pivots",
                         _sym([4, 4, 16, 16, 1, 1], [(0, 1, 4), (2, 3, 16), (4, 5, 1)]), [8, 8, -32, -32, 3, 3]))
    out.append(_icp_case("zero-dup-one", "zero pivots", "one duplicated column: one exact zero pivot",
                         _sym([4, 4, 8, 2, 1, 32], [(0, 1, 4)]), [4, 4, -8, 6, 5, 64]))
    return out


def _near_singular(rng):
    out = []
    for rank in (2, 3, 4, 5):
        J = rng.integers(-3, 4, (12, rank)).dot(rng.integers(-3, 4, (rank, 6)))
        assert np.linalg.matrix_rank(J) == rank
        A, b, rr = _gram(J, rng.integers(-7, 8, 12))
        c = _icp_case("near-singular-rank%d" % rank, "near-singular", "rank %d by rounding: tiny non-zero pivots, a huge update" % rank, A, b, res=rr)
        c.meta["rank"] = rank
        out.append(c)
        # ... and under a right-hand side outside the range of A, which the tiny pivots blow up: det_sincos gets a huge argument
        c = _icp_case("near-singular-rank%d-off-range" % rank, "near-singular", "rank %d by rounding, inconsistent b: an update of order 1e15" % rank,
                      A, [int(v) for v in rng.integers(-7, 8, 6)], res=rr)
        c.meta.update(rank=rank, huge=True)
        out.append(c)
    return out


def _theta_system(target):
    """f32 values (a_hi, a_lo, b) with sqrt(fl(x * x)) == target for x = fl(b / fl(a_hi + a_lo)): a diagonal entry split over the RGB
    (a_hi, 8 fraction bits) and the Gram ICP words (a_lo, 34 bits; b, 39 bits), which the f64 combine adds back together"""
    x = float(target)
    eb = max(-39, math.ceil(math.log2(x)) + 15 - 23)
    for m0 in range(1 << 23, 1 << 24, 1 << 20):
        b = np.ldexp(np.arange(m0 + 1, m0 + (1 << 20), 2, dtype=np.float64), eb)
        a_t = b / x
        a_hi = a_t.astype(np.float32).astype(np.float64)
        lo0 = (a_t - a_hi).astype(np.float32)
        for lo in (lo0, np.nextafter(lo0, np.float32(np.inf)), np.nextafter(lo0, np.float32(-np.inf))):
            a_lo = lo.astype(np.float64)
            q = b / (a_hi + a_lo)
            w = np.ldexp(a_lo, 34)
            hit = np.flatnonzero((np.sqrt(q * q) == x) & (w == np.rint(w)) & (a_hi < 2.0 ** 45))
            if hit.size:
                k = int(hit[0])
                return float(a_hi[k]), float(a_lo[k]), float(b[k])
    raise AssertionError("no system for theta = %r" % target)


def _rotations():
    out = []
    pi4 = math.pi / 4
    up, dn = (lambda v: math.nextafter(v, math.inf)), (lambda v: math.nextafter(v, 0.0))
    exact = [("1e-17", 1e-17), ("eps-pred", dn(EPS)), ("eps", EPS), ("eps-succ", up(EPS)), ("1e-8", 1e-8), ("0.5", 0.5), ("pi4-pred", dn(pi4)), ("pi4", pi4),
             ("pi4-succ", up(pi4)), ("pi2", math.pi / 2), ("pi", math.pi), ("3", 3.0), ("6.5", 6.5), ("100", 100.0)]
    for k, (name, theta) in enumerate(exact):
        # one axis (entries of r r^T and [r]x are exact zeros): |r| == theta exactly; RGB words with 8 fraction bits (count 1, sigma 1)
        # carry the diagonal and a translation, Gram ICP words the low half of the diagonal entry and the rotation's right-hand side
        c = 3 + k % 3
        sign = -1 if k % 2 else 1
        a_hi, a_lo, b = _theta_system(theta)
        Ar = _sym([256] * 6); Ar[c][c] = int(math.ldexp(a_hi, 8))
        rgb = rgb_totals(Ar, [64, -128, 32, 0, 0, 0], 8, 8)
        icp = [0] * WORDS
        icp[word_index(c, c)] = int(math.ldexp(a_lo, 34))
        icp[word_index(c, 6)] = sign * int(math.ldexp(b, 39))
        icp[27], icp[28], icp[29], icp[30] = 5 << 44, 12, 1, 1
        out.append(Case("rotation-" + name, "rotations", "theta == %r exactly about axis %d (sign %+d)" % (theta, c - 3, sign),
                        default_state(rgb=1, icpWeight=1.0), [Step(lay(icp), lay(rgb), icp_fix=GRAM)], dict(theta=theta)))
    A = _sym([1] * 6)
    out.append(_icp_case("rotation-0", "rotations", "a zero rotation vector: the identity branch", A, [1, 2, -3, 0, 0, 0], down=4))
    axes = {"x": (1, 0, 0), "y": (0, -1, 0), "z": (0, 0, 1), "xy": (2 ** -0.5, 2 ** -0.5, 0), "122": (1 / 3, 2 / 3, 2 / 3), "-212": (-2 / 3, 1 / 3, 2 / 3)}
    for name, theta in exact[4:]:
        for an, ax in axes.items():
            b = [1 << 28, -(1 << 27), 1 << 26] + [round(theta * v * 2 ** 32) for v in ax]
            t = icp_totals(_sym([1 << 32] * 6), b, FIX_ICP, 32, res=0)
            t[27] = 3 << 30
            out.append(Case("rotation-%s-axis-%s" % (name, an), "rotations", "theta about %s about axis %s" % (name, an), default_state(),
                            [Step(lay(t), _ZERO)]))
    return out


def _guard():
    out = []
    t_hi = np.float32(0.3)                       # above 0.3 in f64: the pose is reset
    t_lo = np.nextafter(t_hi, np.float32(0))     # its f32 predecessor: the pose is kept
    for tn, t in (("above", t_hi), ("below", t_lo)):
        w = int(math.ldexp(float(t), 32))
        assert math.ldexp(w, -32) == float(t)
        A, b = _sym([1 << 32] * 6), [w, 0, 0, 0, 0, 0]
        icp = icp_totals(A, b, FIX_ICP, 32)
        rgbt = rgb_totals(A, b, 32, 32)
        cnt = [0] * WORDS; cnt[29], cnt[30] = 300000, 5      # (count >= 4096: the RGB words have 32 fraction bits)
        modes = (("icp", dict(icp=1, rgb=0), icp, [0] * WORDS), ("rgb", dict(icp=0, rgb=1), cnt, rgbt),
                 ("both", dict(icp=1, rgb=1, icpWeight=1.0), [a + c for a, c in zip(icp, cnt)], [0] * WORDS))
        for mn, flags, it, rt in modes:
            for nl in (-1, 0):
                out.append(Case("guard-%s-%s-next%d" % (tn, mn, nl), "guard",
                                "|tcurr - tprev| == float32(%r), %s 0.3; rgb %s; next_level %d" % (float(t), tn, "on" if flags["rgb"] else "off", nl),
                                default_state(**flags), [Step(lay(it), lay(rt), next_level=nl, last_of_level=(nl < 0))], dict(t=float(t))))
    return out


def _modes(rng):
    out = []
    A1, b1, r1 = _gram(rng.integers(-7, 8, (12, 6)), rng.integers(-7, 8, 12))
    A2, b2, _ = _gram(rng.integers(-7, 8, (12, 6)), rng.integers(-7, 8, 12))

    def case(name, aims, *, icp, rgb, rgb_only=0, w=10.0, fmt=FIX_ICP, count=300000, sigma=77, inliers=12, res=None):
        it = icp_totals(A1, b1, fmt, 10, res=r1 if res is None else res, count=inliers)
        it[29], it[30] = count, sigma
        bits = orc.rgb_fix_bits(sigma_val(count, sigma, rgb_only))
        rt = rgb_totals(A2, b2, bits, 8)
        st = default_state(icp=icp, rgb=rgb, rgbOnly=rgb_only, icpWeight=w)
        return Case("modes-" + name, "modes", aims, st, [Step(lay(it), lay(rt), icp_fix=fmt)], dict(rgb_bits=bits if rgb else None))

    for fn, fmt in (("fixed", FIX_ICP), ("gram", GRAM)):
        out.append(case("icp-only-" + fn, "ICP sums alone, %s words" % fn, icp=1, rgb=0, fmt=fmt))
        for w in (10.0, 100.0, 0.5):
            out.append(case("both-w%g-%s" % (w, fn), "RGB + w^2 ICP with icpWeight %g, %s ICP words" % (w, fn), icp=1, rgb=1, w=w, fmt=fmt))
    out.append(case("rgb-only", "the RGB-only mode: sigma -1, 8 fraction bits", icp=0, rgb=1, rgb_only=1))
    out.append(case("rgb-alone", "RGB sums alone outside the RGB-only mode", icp=0, rgb=1))
    for count in (0, 1, 2, 3, 4095, 4096, 300000) + tuple(1 << e for e in range(2, 12)):
        for sigma in (0, 77):
            out.append(case("count%d-sigma%d" % (count, sigma),
                            "RGB format of count %d, sigma %d%s" % (count, sigma, ": 0/0 statistics" if count == 0 and sigma == 0 else ""),
                            icp=1, rgb=1, count=count, sigma=sigma))
    out.append(case("no-inliers", "ICP inlier count 0 under a non-zero residual: the ICP error is inf", icp=1, rgb=0, inliers=0))
    out.append(case("no-inliers-no-residual", "ICP inlier count 0 and residual 0: the ICP error is NaN", icp=1, rgb=0, inliers=0, res=0))
    return out


def _stop_rule():
    out = []
    count, sigma = 4, 10
    tmp = np.float32(np.sqrt(np.float64(sigma)) / np.float64(count))
    A, b, _ = _gram(np.random.default_rng(SEED + 5).integers(-7, 8, (12, 6)), np.arange(12) - 5)
    it = [0] * WORDS; it[29], it[30] = count, sigma
    rt = rgb_totals(A, b, 8)
    for name, last in (("above", np.nextafter(tmp, np.float32(0))), ("equal", tmp), ("below", np.nextafter(tmp, np.float32(1)))):
        steps = [Step(lay(it), lay(rt), next_level=2), Step(lay(it), lay(rt, "even"), next_level=2),
                 Step(lay(it), lay(rt, "late"), next_level=1, last_of_level=True), Step(lay(it), lay(rt), next_level=1)]
        out.append(Case("stop-" + name, "stop rule", "RGB-only: tmpError just %s lastRGBError; then a solve on the returned state, the end of the level, "
                        "and the first solve of the next level" % name, default_state(icp=0, rgb=1, rgbOnly=1, lastRGBError=float(last)), steps))
    A1, b1, r1 = _gram(np.random.default_rng(SEED + 6).integers(-7, 8, (12, 6)), np.arange(12) - 6)
    for nl in (1, -1):
        st = default_state(level_done=1, solves=3, Rcurr=common.perturbed_pose(7)[:3, :3].copy(), tcurr=common.perturbed_pose(7)[:3, 3].copy())
        out.append(Case("stop-inactive-next%d" % nl, "stop rule", "level_done set on entry: sums are ignored, the pose stays, solves counts", st,
                        [Step(lay(icp_totals(A1, b1, FIX_ICP, 0, res=r1)), _ZERO, next_level=nl)]))
    return out


def _groups(rng):
    out = []
    A, b, rr = _gram(rng.integers(-7, 8, (12, 6)), rng.integers(-7, 8, 12))
    A2, b2, _ = _gram(rng.integers(-7, 8, (12, 6)), rng.integers(-7, 8, 12))
    it = icp_totals(A, b, FIX_ICP, 10, res=rr)
    it[29], it[30] = 4096, 9
    rt = rgb_totals(A2, b2, 32, 8)
    for how in ("g0", "late", "even", "wrap+", "wrap-", "wrap63"):
        out.append(Case("groups-" + how, "groups", "the same totals (negative ones among them) laid over the 64 groups as '%s'" % how,
                        default_state(rgb=1), [Step(lay(it, how), lay(rt, how))]))
    return out


def _levels():
    out = []
    A, b, rr = _gram(np.random.default_rng(SEED + 8).integers(-7, 8, (12, 6)), np.arange(12) - 4)
    A2, b2, _ = _gram(np.random.default_rng(SEED + 9).integers(-7, 8, (12, 6)), 3 - np.arange(12))
    it = icp_totals(A, b, FIX_ICP, 6, res=rr, count=900)
    it[29], it[30] = 5000, 123
    rt = rgb_totals(A2, b2, 32, 2)
    P, Q = common.perturbed_pose(11), common.perturbed_pose(12, trans=0.02, rot_deg=2.0)
    for nl in (2, 1, 0, -1):
        for last in (False, True):
            st = default_state(intr=(140.25, 133.5, 71.0, 66.5), rgb=1, Rprev=P[:3, :3].copy(), tprev=P[:3, 3].copy(), Rprev_inv=P[:3, :3].T.copy(),
                               Rcurr=P[:3, :3].copy(), tcurr=P[:3, 3].copy(), resultRt=Q.astype(np.float64), residual=np.array([0.5, 7.0], np.float32))
            out.append(Case("levels-next%d-last%d" % (nl, last), "levels", "next_level %d, last_of_level %d, an off-centre camera with fx != fy and "
                            "non-trivial Rprev, tprev, resultRt" % (nl, last), st, [Step(lay(it), lay(rt), next_level=nl, last_of_level=last)]))
    return out


def _inv33f(a):
    """ORC_INV33 of oracle/orc_math.h in float32 scalars"""
    a = [np.float32(v) for v in np.asarray(a, np.float32).reshape(9)]
    c00 = a[4] * a[8] - a[5] * a[7]; c01 = a[5] * a[6] - a[3] * a[8]; c02 = a[3] * a[7] - a[4] * a[6]
    det = a[0] * c00 + a[1] * c01 + a[2] * c02
    d = np.float32(1) / det
    return np.array([c00 * d, (a[2] * a[7] - a[1] * a[8]) * d, (a[1] * a[5] - a[2] * a[4]) * d, c01 * d, (a[0] * a[8] - a[2] * a[6]) * d,
                     (a[2] * a[3] - a[0] * a[5]) * d, c02 * d, (a[1] * a[6] - a[0] * a[7]) * d, (a[0] * a[4] - a[1] * a[3]) * d], np.float32).reshape(3, 3)


CHAIN_SIZE = (160, 120)


def chain_tracker():
    """the oracle tracker the chain's sums are taken from, prepared for one frame-to-model step (and its start pose)"""
    W, H = CHAIN_SIZE
    fp = common.frame_pair(W, H, noise=True)
    cam = fp["cam"]
    pose = common.perturbed_pose(2)
    od = orc.Odometry(W, H, cam.cx, cam.cy, cam.fx, cam.fy)
    od.init_first_rgb(fp["rgba0"]); od.init_icp_model(fp["v4"], fp["n4"], pose); od.init_rgb_model(fp["img"])
    od.init_icp(orc.depth_pyramid(fp["d1"]), 20.0); od.init_rgb(fp["rgba1"])
    return od, cam, pose


def _chain():
    """One 4 / 5 / 10 schedule: the sums of every iteration come from orc.icp_step / orc.rgb_step under the pose the solves before it left"""
    od, cam, pose = chain_tracker()
    intr = orc.Cam(cam.fx, cam.fy, cam.cx, cam.cy)
    Rprev, tprev = pose[:3, :3].copy(), pose[:3, 3].copy()
    Rprev_inv = _inv33f(Rprev)
    st0 = default_state(intr=(cam.fx, cam.fy, cam.cx, cam.cy), width=CHAIN_SIZE[0], height=CHAIN_SIZE[1], rgb=1, Rprev=Rprev, tprev=tprev, Rprev_inv=Rprev_inv,
                        Rcurr=Rprev.copy(), tcurr=tprev.copy())
    dist = 0.10
    angle = float(np.float32(math.sin(float(np.float32(20.0) * np.float32(3.14159254) / np.float32(180.0)))))
    sobel_scale, max_dd, min_grad = 0.125, 0.07, (5.0, 3.0, 1.0)
    # krkInv / kt of the first iteration: an inactive solve derives them for level 2 and changes nothing else but the counter
    s, _ = orc.gn_solve_step(orc_state(dict(st0, level_done=1)), np.zeros(32, np.int64), np.zeros(32, np.int64), 2, False)
    st0["krkInv"] = np.array(s.krkInv, np.float32).reshape(3, 3); st0["kt"] = np.array(s.kt, np.float32)
    s = orc_state(st0)
    steps = []
    iterations = {2: 4, 1: 5, 0: 10}
    for L in (2, 1, 0):
        il = intr.level(L)
        B = lambda which: od.buffer(which, L)
        vc, nc, vp, npv, last_d, next_d, last_i, next_i = (B(k) for k in range(8))
        dx, dy = orc.sobel(next_i)
        cloud = orc.project_cloud(last_d, il)
        min_scale = float(np.float32(min_grad[L] ** 2 / sobel_scale ** 2))
        for j in range(iterations[L]):
            last = j == iterations[L] - 1
            corres, sigma, count = orc.rgb_residual(min_scale, dx, dy, last_d, next_d, last_i, next_i, max_dd, np.array(s.kt, np.float32), np.array(s.krkInv, np.float32))
            it, _ = orc.icp_step(np.array(s.Rcurr, np.float32), np.array(s.tcurr, np.float32), vc, nc, Rprev_inv, tprev, il, vp, npv, dist, angle)
            rt = orc.rgb_step(corres, sigma_val(count, sigma, 0), cloud, il.fx, il.fy, dx, dy, sobel_scale)
            it = [int(v) for v in it]; it[29], it[30] = count, sigma
            step = Step(lay(it, ("g0", "even", "late")[len(steps) % 3]), lay([int(v) for v in rt], "even"), next_level=(L - 1 if last else L), last_of_level=last)
            steps.append(step)
            s, _ = orc.gn_solve_step(s, totals(step.icp), totals(step.rgb), step.next_level, step.last_of_level)
    return [Case("chain-4-5-10", "chain", "19 solves of one realistic schedule on one state", st0, steps, dict(pose=pose))]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in table order"""
    rng = np.random.default_rng(SEED)
    table = (_pivots(rng) + _ties() + _zero_pivots(rng) + _near_singular(rng) + _rotations() + _guard() + _modes(rng) + _stop_rule() + _groups(rng)
             + _levels() + _chain())
    out = {c.name: c for c in table}
    assert len(out) == len(table), "case names are unique"
    return out


def family(name):
    return [c for c in cases().values() if c.family == name]


# --------------------------------------------------------------------------------------------------------------- the oracle
def orc_state(d):
    """state dictionary -> orc.GnState (the oracle keeps no Rprev_inv and no pose_inv)"""
    s = orc.GnState()
    s.intr = orc.Cam(*[float(v) for v in d["intr"]])
    for k in ("width", "height", "icp", "rgb", "rgbOnly", "level_done", "solves"):
        setattr(s, k, int(d[k]))
    s.icpWeight = float(d["icpWeight"]); s.lastRGBError = float(d["lastRGBError"])
    for k, n, t in (("Rprev", 9, np.float32), ("tprev", 3, np.float32), ("Rcurr", 9, np.float32), ("tcurr", 3, np.float32), ("resultRt", 16, np.float64),
                    ("krkInv", 9, np.float32), ("kt", 3, np.float32), ("residual", 2, np.float32)):
        v = np.ascontiguousarray(d[k], t).reshape(n)
        getattr(s, k)[:] = v.tolist()
    return s


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's (state after, trace) of every step of a case, computed once"""
    c = cases()[name]
    s = orc_state(c.state)
    out = []
    for st in c.steps:
        s, tr = orc.gn_solve_step(s, totals(st.icp), totals(st.rgb), st.next_level, st.last_of_level, st.icp_fix)
        out.append((s, tr))
    return tuple(out)
