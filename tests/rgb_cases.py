"""The case table of the photometric term's record-slot path (plain helper module, no tests in here).

A case is ONE system of cf_rgb_records_step: the level's eight images, the projection (krkInv, kt), the gate and the step's scalars, the
range of a culled tracker, and the seeds of accumulator words 29 / 30.  Every case is seeded, says what it aims at (`aims`) and aims at
one branch of rgb_residual_body<true> / rgb_slot_step_kernel / rgb_step_solve_kernel, so that a slip fails with the case's name.  The
GPU side (tests/test_rgb_records_gpu.py) runs every case under three launch shapes and gn modes 1 and 2 against
tests/rgb_rows_ref.py; the CPU side (tests/test_cpu_rgb_cases.py) checks that reference against the oracle and that every case reaches
its aim.

Size: 80 x 60 = 4800 pixels -- 18.75 slots of 256 pixels (64 threads), 4.69 of 1024 (256 threads), 1.17 of 4096 (1024 threads): the last
slot is always partial and mode 2 has an odd last quad.  64 x 48 = 3072 where a case wants a whole number of slots.

DOMAIN, kept by every case (rgb_rows_ref's docstring; asserted by test_cpu_rgb_cases.py):
  * cloud z is finite and > 0 wherever a record can point;
  * rows are finite and free of subnormals;
  * every planted stale count is <= its slot's capacity and every planted stale record holds in-range indices (`plant`).
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import rgb_rows_ref as rr

SEED = 20261
COLS, ROWS = 80, 60
SHAPES = ((256, 1), (1024, 1), (64, 4))      # (threads, pixels per thread) of cf_set_icp_launch
F32 = np.float32
MAX_DD, SOBEL, FX = F32(0.07), F32(0.125), F32(132.0)
IDENT = (1, 0, 0, 0, 1, 0, 0, 0, 1)


@dataclasses.dataclass
class Case:
    name: str
    aims: str
    cols: int
    rows: int
    cand: np.ndarray
    next_depth: np.ndarray
    last_depth: np.ndarray
    last_image: np.ndarray
    next_image: np.ndarray
    cloud: np.ndarray
    dIdx: np.ndarray
    dIdy: np.ndarray
    krk: np.ndarray
    kt: np.ndarray
    max_dd: np.float32 = MAX_DD
    sobel: np.float32 = SOBEL
    fx: np.float32 = FX
    fy: np.float32 = FX
    rgb_only: int = 0
    no_counts: int = 0
    res_range: tuple = None          # (lo_inv, hi_p1) in 256-pixel chunks, as OdomDev::res_range holds them
    res_blocks: int = 0
    count_seed: np.ndarray = None
    sigma_seed: np.ndarray = None
    min_scale: float = None          # set where cand IS the preparation's rule (cand_rule): the cases of the mode 0 cross-check
    next_level: int = 1              # of the solve under mode 2
    last_of_level: bool = False

    @property
    def n(self):
        return self.cols * self.rows


def _rng(name):
    return np.random.default_rng([SEED] + [ord(ch) for ch in name])


def blank(name, aims, cols=COLS, rows=ROWS, **over):
    """identity projection, every depth 1, intensities 100 -> 120, a plausible cloud, small gradients, NO candidate"""
    g = _rng(name)
    n = cols * rows
    u, v = np.meshgrid(np.arange(cols, dtype=F32), np.arange(rows, dtype=F32))
    z = g.uniform(0.5, 3.0, n).astype(F32)
    cloud = np.stack([(u.reshape(-1) - F32(cols / 2)) / FX * z, (v.reshape(-1) - F32(rows / 2)) / FX * z, z], axis=1).astype(F32)
    c = Case(name=name, aims=aims, cols=cols, rows=rows, cand=np.zeros(n, np.uint8), next_depth=np.ones(n, F32), last_depth=np.ones(n, F32),
             last_image=np.full(n, 100, np.uint8), next_image=np.full(n, 120, np.uint8), cloud=cloud,
             dIdx=g.integers(-40, 41, n).astype(np.int16), dIdy=g.integers(-40, 41, n).astype(np.int16),
             krk=np.array(IDENT, F32), kt=np.zeros(3, F32), count_seed=np.zeros(64, np.int64), sigma_seed=np.zeros(64, np.int64))
    for k, val in over.items():
        assert hasattr(c, k), k
        setattr(c, k, val)
    return c


def cand_rule(c, min_scale):
    """the iteration-invariant half of RGBResidual's validity test as the preparation hoists it (rgb_cand_kernel; pinned by the
    frame-preparation tests): the 4 x 4 window of the next image non-zero, squared gradient >= min_scale, d1 not NaN, off the border"""
    img = c.next_image.reshape(c.rows, c.cols)
    out = np.zeros((c.rows, c.cols), np.uint8)
    gx = c.dIdx.reshape(c.rows, c.cols).astype(np.int64); gy = c.dIdy.reshape(c.rows, c.cols).astype(np.int64)
    d1 = c.next_depth.reshape(c.rows, c.cols)
    for i in range(c.rows - 1):
        for j in range(c.cols - 5):
            win = img[max(i - 2, 0):min(i + 2, c.rows), max(j - 2, 0):min(j + 2, c.cols)]
            if (win > 0).all() and F32(gx[i, j] ** 2 + gy[i, j] ** 2) >= F32(min_scale) and not np.isnan(d1[i, j]):
                out[i, j] = 1
    return out.reshape(-1)


def spread(total, groups, name):
    """64 int64 seeds, uneven, non-zero in `groups` only, whose 64-bit sum is `total`"""
    g = _rng("seed" + name)
    out = np.zeros(64, np.int64)
    parts = g.integers(-(1 << 40), 1 << 40, len(groups) - 1)
    for k, p in zip(groups[:-1], parts):
        out[k] = p
    out[groups[-1]] = rr.wrap64(int(total) - int(sum(int(p) for p in parts)))
    assert rr.wrap64(sum(int(v) for v in out)) == rr.wrap64(total)
    return out


# ------------------------------------------------------------------------------------------------------------ the cases
def _scene():
    import common
    import orc
    c = blank("scene", "baseline: level 2 of a rendered 320 x 240 pair under a perturbed pose; sigma = count")
    fp = common.frame_pair(320, 240, noise=True)
    cam = fp["cam"]
    od = orc.Odometry(320, 240, cam.cx, cam.cy, cam.fx, cam.fy)
    pose = common.perturbed_pose(3)
    od.init_first_rgb(fp["rgba0"]); od.init_icp_model(fp["v4"], fp["n4"], pose); od.init_rgb_model(fp["img"])
    od.init_icp(orc.depth_pyramid(fp["d1"]), 20.0); od.init_rgb(fp["rgba1"])
    c.next_image = od.buffer(7, 2).reshape(-1).copy(); c.last_image = od.buffer(6, 2).reshape(-1).copy()
    c.last_depth = od.buffer(4, 2).reshape(-1).copy(); c.next_depth = od.buffer(5, 2).reshape(-1).copy()
    assert c.next_image.size == c.n
    dx, dy = orc.sobel(c.next_image.reshape(ROWS, COLS))
    c.dIdx, c.dIdy = dx.reshape(-1).copy(), dy.reshape(-1).copy()
    K = np.array([[cam.fx / 4, 0, cam.cx / 4], [0, cam.fy / 4, cam.cy / 4], [0, 0, 1]], np.float64)
    dT = common.perturbed_pose(11, 0.05, 2.0).astype(np.float64)     # (far enough for every gate to reject some candidates)
    c.krk = (K @ dT[:3, :3] @ np.linalg.inv(K)).astype(F32).reshape(9); c.kt = (K @ dT[:3, 3]).astype(F32)
    c.cloud = orc.project_cloud(c.last_depth.reshape(ROWS, COLS), orc.Cam(cam.fx, cam.fy, cam.cx, cam.cy).level(2)).reshape(-1, 3).copy()
    c.fx = c.fy = F32(cam.fx / 4)
    c.min_scale = 64.0                      # minGrad[2]^2 / sobelScale^2
    c.cand = cand_rule(c, c.min_scale)
    return c


def _project_ties():
    c = blank("project_ties", "u0 / v0 exactly on x.5: krk rows (1, 0, -1.5), kt = 1, d1 in {1, 0.5} give x - 0.5 and x + 0.5 -- even and odd "
              "neighbours, -0.5 -> 0 (valid), cols - 0.5 and rows - 0.5 -> out", max_dd=F32(1.0))
    c.krk = np.array([1, 0, -1.5, 0, 1, -1.5, 0, 0, 1], F32); c.kt = np.array([1, 1, 0], F32)
    k = np.arange(c.n)
    c.next_depth = np.where((k // 3) % 2 == 0, F32(1.0), F32(0.5)).astype(F32)
    c.last_depth[:] = 0.75
    c.cand[:] = 1
    return c


def _project_degenerate():
    c = blank("project_degenerate", "td1 = d1 - 1: d1 = 1 gives td1 == 0 -- numerator < 0, 0 / 0, > 0 along x (krk row 0 = (1, 0, -10)): -inf, "
              "NaN -> (0, 0) which the depth gate rejects, +inf --; d1 = 0.5 a negative td1; d1 = 0 at a candidate; d1 = 2 valid")
    c.krk = np.array([1, 0, -10, 0, 1, 0, 0, 0, 1], F32); c.kt = np.array([0, 0, -1], F32)
    k = np.arange(c.n); y, x = k // c.cols, k % c.cols
    c.next_depth = np.choose(y % 4, [F32(1.0), F32(2.0), F32(0.5), F32(0.0)]).astype(F32)
    c.cand[:] = 1
    return c


def _depth_gate():
    c = blank("depth_gate", "td1 = 2 * maxDepthDelta, d0 = maxDepthDelta: |td1 - d0| exactly at the gate passes, d0 one ulp lower fails; "
              "d0 of 0, negative, NaN; lastImage == 0; the rest passes")
    k = np.arange(c.n)
    c.next_depth[:] = F32(2.0) * MAX_DD
    kind = k % 8
    c.last_depth = np.choose(kind, [MAX_DD, np.nextafter(MAX_DD, F32(0)), F32(0), F32(-0.14), F32(np.nan), F32(2.0) * MAX_DD,
                                    F32(1.0), F32(2.0) * MAX_DD]).astype(F32)
    c.last_image[kind == 7] = 0
    c.cloud[:, 2] = 1.5
    c.cand[:] = 1
    return c


def _diff_extremes():
    c = blank("diff_extremes", "diff of -255, 0 and +254 (+255 needs lastImage == 0, which the gate rejects): packed fields 1, 256, 510; "
              "g == 0, g == N - 1, k == N - 1; two pixels with the same g (td1 = 1 for every d1: u0 = d1 * x)")
    c.krk = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], F32); c.kt = np.array([0, 0, 1], F32)
    n = c.n
    for k, nx in {0: 0, n - 1: 255, 5: 77, 10: 0, 20: 255, 41: 9}.items():      # pixel -> next intensity
        c.cand[k] = 1; c.next_image[k] = nx
    for g, la in {0: 255, n - 1: 1, 5: 77, 10: 255}.items():                    # pixel -> last intensity (100 elsewhere)
        c.last_image[g] = la
    c.next_depth[20] = 0.5                      # pixel 20 lands on g = 10 as pixel 10 does: diffs 255 - 255 = 0 and 0 - 255
    return c


def _filled(name, aims, lo, hi, cols=COLS, rows=ROWS, **over):
    c = blank(name, aims, cols, rows, **over)
    c.cand[lo:hi] = 1
    g = _rng(name + "img")
    c.next_image = g.integers(1, 256, c.n).astype(np.uint8)
    c.last_image = g.integers(1, 256, c.n).astype(np.uint8)
    return c


def _sparse():
    c = blank("sparse", "exactly one record in the image: pixel 4095, the last pixel of the last lane of the last wave of slot 15 / 3 / 0; "
              "the solve under mode 2 ends the schedule (twin published)", next_level=-1, last_of_level=True)
    c.cand[4095] = 1
    return c


def _empty():
    c = blank("empty", "no valid pixel (candidates everywhere, lastImage == 0): zero sums, zero counts, every slot count written as 0")
    c.cand[::3] = 1
    c.last_image[:] = 0
    return c


def _ranged(name, blocks, rng=(5, 11)):
    what = "the empty range (hi_p1 == 0): nothing visited, mode 2's stand-in workgroup solves with zero sums" if rng is None else \
        "chunks %d..%d of 19: slots 5..11 / 1..2 / 0 of the three shapes, res_blocks = %d; candidates AND stale slots outside stay out" % (rng + (blocks,))
    c = _filled(name, "a culled tracker's range -- " + what, 0, COLS * ROWS)
    c.res_range = (0, 0) if rng is None else ((~rng[0]) & 0xffffffff, rng[1] + 1)
    c.res_blocks = blocks
    return c


def _sigma(name, aims, lo, hi, **over):
    return _filled("sigma_" + name, aims, lo, hi, **over)


def _clamp(name, aims, **over):
    c = blank(name, aims, **over)
    g = _rng(name + "z")
    k = np.arange(c.n)
    c.dIdx = np.where(k % 2 == 0, 32767, -32768).astype(np.int16); c.dIdy = np.where(k % 3 == 0, -32000, 31000).astype(np.int16)
    near = k % 5 != 0
    c.cloud[:, 2] = np.where(near, F32(2.0 ** -10), F32(4.0)).astype(F32)          # small z where the rows are to leave the window
    c.cloud[:, 0] = g.uniform(-1, 1, c.n).astype(F32) * c.cloud[:, 2]; c.cloud[:, 1] = g.uniform(-1, 1, c.n).astype(F32) * c.cloud[:, 2]
    c.next_image = g.integers(1, 256, c.n).astype(np.uint8)
    c.min_scale = 1.0
    c.cand = cand_rule(c, c.min_scale)
    return c


def _sum_ties():
    c = blank("sum_ties", "F = 8 (rgbOnly, w = 1); sobel 2^-3, fx 4, fy 8, z 16, px = py = 0: row0 = k0 2^-5, row1 = k1 2^-4 with odd k -> "
              "row0 row1 2^8 = k0 k1 / 2, exact ties of both signs", rgb_only=1, fx=F32(4.0), fy=F32(8.0))
    g = _rng("sum_ties_k")
    c.dIdx = (2 * g.integers(-8, 8, c.n) + 1).astype(np.int16); c.dIdy = (2 * g.integers(-8, 8, c.n) + 1).astype(np.int16)
    c.cloud[:] = (0.0, 0.0, 16.0)
    c.next_image = g.integers(1, 256, c.n).astype(np.uint8)
    c.min_scale = 1.0
    c.cand = cand_rule(c, c.min_scale)
    return c


BUILDERS = {
    "scene": _scene,
    "project_ties": _project_ties,
    "project_degenerate": _project_degenerate,
    "depth_gate": _depth_gate,
    "diff_extremes": _diff_extremes,
    "full_slot_64": lambda: _filled("full_slot_64", "pixels 256..511: slot 1 of the 64-thread shape at capacity (256), its neighbours empty", 256, 512),
    "full_slot_256": lambda: _filled("full_slot_256", "pixels 1024..2047: slot 1 of the 256-thread shape at capacity (1024), its neighbours empty", 1024, 2048),
    "full_slot_1024": lambda: _filled("full_slot_1024", "pixels 0..4095: slot 0 of the 1024-thread shape at capacity (4096), the partial slot behind it empty", 0, 4096),
    "full_last_64x48": lambda: _filled("full_last_64x48", "64 x 48 = 12 / 3 whole slots: the LAST slot of the 64- and 256-thread shapes at capacity, no partial slot",
                                       2048, 3072, cols=64, rows=48),
    "stride_walk": lambda: _filled("stride_walk", "a slot of 257 = 256 + 1 = 2 * 128 + 1 records (pixels 1024..1280) and one of 129 (2048..2176): the "
                                   "r += stride walks of modes 1 and 2 (256-thread shape)", 1024, 1281),
    "sparse": _sparse,
    "empty": _empty,
    "tail": lambda: _filled("tail", "valid pixels 4700..4799 only: inside the partial last slot of every shape, pixel N - 1 included", 4700, 4800),
    "ranged_b1": lambda: _ranged("ranged_b1", 1),
    "ranged_b2": lambda: _ranged("ranged_b2", 2),
    "ranged_b100": lambda: _ranged("ranged_b100", 100),
    "ranged_empty": lambda: _ranged("ranged_empty", 3, None),
    "sigma_rgbonly": lambda: _sigma("rgbonly", "rgbOnly: sigma = -1, F = 8, unit weights", 900, 1500, rgb_only=1),
    "sigma_zero_diffs": lambda: _sigma("zero_diffs", "every diff 0: sigma sum 0 with count != 0 -> sigma = 1, F = 8", 900, 1500),
    "sigma_count3": lambda: _sigma("count3", "three records: sigma = 3, F = 10", 2000, 2003),
    "sigma_hundreds": lambda: _sigma("hundreds", "300 records: F = 24", 300, 600),
    "sigma_4096": lambda: _sigma("4096", "4800 records: count >= 4096, F = 32", 0, 4800),
    "sigma_wrap": lambda: _sigma("wrap", "count seeds over 7 groups whose 64-bit sum is 2^32 + 5, 40 records: the LOW word 45 is the count (F = 18)",
                                 100, 140, count_seed=spread((1 << 32) + 5, (0, 3, 15, 16, 31, 47, 63), "wrap")),
    "sigma_neg": lambda: _sigma("neg", "a sigma total whose low word is negative as int (seeds sum to 0x90000000): not zero, sigma = count",
                                100, 140, sigma_seed=spread(0x90000000, (1, 17, 33, 49), "neg")),
    "sigma_w0": lambda: _sigma("w0", "no_counts with count seeds 0, sigma seeds 77, every diff 0: sigma = 0, w = 0 + |0| -> 1", 100, 140,
                               no_counts=1, sigma_seed=spread(77, (2, 62), "w0")),
    "sigma_zero_zero": lambda: _sigma("zero_zero", "no_counts with both seeds 0 and diffs != 0: count 0 AND sigma 0 -> sigma = (float)0, w = 1 / |diff| (a rule "
                                      "that tests the sigma total alone would hand 1 on)", 100, 140, no_counts=1),
    "sigma_no_counts": lambda: _sigma("no_counts", "no_counts = 1: words 29 / 30 stay as seeded (500, 12345) and the step uses the seeds (F = 24)", 100, 140,
                                      no_counts=1, count_seed=spread(500, (5, 6, 60), "nc"), sigma_seed=spread(12345, (0, 63), "ns")),
    "clamp_f8": lambda: _clamp("clamp_f8", "rgbOnly, F = 8: rows beyond 2^21 of both signs (z = 2^-10, gradients +-2^15), others inside", rgb_only=1),
    "clamp_f32": lambda: _clamp("clamp_f32", "count seeds 5000, F = 32: rows beyond 2^9 of both signs", count_seed=spread(5000, (9, 10, 11), "c32")),
    "sum_ties": _sum_ties,
}
# next == last where every diff is to be zero
_ZERO_DIFF = ("sigma_zero_diffs", "sigma_w0")
# three / nine systems in one call: cases that share the launch's scalars (size, gate, sobel scale, intrinsics).  Nine: mode 2 decodes its
# second group of eight trackers (the idiv(q, quad_div) path)
BATCHES = {
    "batch_3": ("depth_gate", "sparse", "sigma_hundreds"),
    "batch_9": ("tail", "ranged_b2", "sigma_wrap", "empty", "diff_extremes", "clamp_f32", "ranged_empty", "stride_walk", "sigma_count3"),
}
MODE0 = ("scene", "clamp_f8", "clamp_f32", "sum_ties")
# (mutation evidence of the pull request that added this table, one GPU run per mutation: depth_gate catches `<=` -> `<`; project_ties
# f2i_rn -> truncation; every case with a diff != 0 `(int)(diff * diff)` -> `(int)diff`; sigma_zero_zero `sigma == 0 && count != 0` -> `sigma == 0`;
# clamp_f8 / clamp_f32 a halved clamp limit; sigma_wrap wave_sum_u32 fed the high word)


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert c.name == name, (c.name, name)
    if name == "stride_walk":
        c.cand[2048:2177] = 1
    if name in _ZERO_DIFF:
        c.next_image = c.last_image.copy()
    for f in ("cand", "last_image", "next_image"):
        assert getattr(c, f).dtype == np.uint8 and getattr(c, f).shape == (c.n,), f
    for f in ("next_depth", "last_depth"):
        setattr(c, f, np.ascontiguousarray(getattr(c, f), F32)); assert getattr(c, f).shape == (c.n,), f
    for f in ("dIdx", "dIdy"):
        assert getattr(c, f).dtype == np.int16 and getattr(c, f).shape == (c.n,), f
    c.cloud = np.ascontiguousarray(c.cloud, F32); assert c.cloud.shape == (c.n, 3)
    c.krk = np.ascontiguousarray(c.krk, F32).reshape(9); c.kt = np.ascontiguousarray(c.kt, F32).reshape(3)
    for a in (c.cand, c.next_depth, c.last_depth, c.last_image, c.next_image, c.cloud, c.dIdx, c.dIdy, c.krk, c.kt, c.count_seed, c.sigma_seed):
        a.setflags(write=False)          # a shared reference stays unchanged
    return c


NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def reference(name, threads):
    """rgb_rows_ref.reference of a case; the launch shape only enters through the slots a ranged case visits"""
    c = case(name)
    if c.res_range is None and threads != 64:
        ref = dict(reference(name, 64))      # same pixels, same sums: only the slot lay-out differs
        slot_px = threads * 4
        n_slots = (c.n + slot_px - 1) // slot_px
        valid, r = ref["valid"], ref["res"]
        ref.update(first=0, last=n_slots - 1, n_slots=n_slots, slot_px=slot_px,
                   slots={s: sorted(rr.pack(k, r["g"][k], r["diff"][k]) for k in np.flatnonzero(valid[s * slot_px:(s + 1) * slot_px]) + s * slot_px)
                          for s in range(n_slots)})
        return ref
    return rr.reference(c, threads)


def plant(c, threads):
    """what the record buffer and the slot counts hold BEFORE the residual pass: stale slots everywhere, inside the domain -- every count
    <= its slot's capacity (> 0 wherever the slot has room), every record in range -> (slot_counts u32 [n_slots], records u64 [N])"""
    g = _rng("plant%s%d" % (c.name, threads))
    slot_px = threads * 4
    n_slots = (c.n + slot_px - 1) // slot_px
    cap = np.minimum(slot_px, c.n - np.arange(n_slots) * slot_px)
    counts = np.maximum(1, (cap * g.uniform(0.3, 1.0, n_slots)).astype(np.int64)).astype(np.uint32)
    assert (counts <= cap).all()
    k = g.integers(0, c.n, c.n).astype(np.uint64); gg = g.integers(0, c.n, c.n).astype(np.uint64); d = g.integers(1, 512, c.n).astype(np.uint64)
    return counts, k | ((gg | (d << np.uint64(22))) << np.uint64(32))
