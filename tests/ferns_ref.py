"""numpy statement of the fern keyframe relocaliser (Core/Ferns.cpp), written as literally as the reference: per-fern loops, inverted
lists per fern and code, f32 where the reference has f32.  Test infrastructure only.

Conventions that the reference leaves open and this project states:
  * the 8x reduction is nearest sampling at source texel (8x + 4, 8y + 4);
  * the reduced vertex / normal maps are kept planar with z == 0 -> NaN in all planes (copyMaps);
  * the photometric check is evaluated in f64 from the f32 inputs, pose difference [R^T R', R^T (t' - t)], coordinates truncated
    towards zero, no correspondence -> +inf.
"""
from __future__ import annotations

import numpy as np

BAD = 255
FLT_MAX = np.float32(3.402823466e+38)
QNAN = np.array([0x7fffffff], np.uint32).view(np.float32)[0]
FERN = np.dtype([("x", "<i4"), ("y", "<i4"), ("r", "<i4"), ("g", "<i4"), ("b", "<i4"), ("d", "<i4")])


# ------------------------------------------------------------------------------- reduce
def reduce_maps(v4, n4, rgba):
    """full-size f32x4, f32x4, rgba8 -> reduced f32x4, f32x4, rgb8 (resize.frag as nearest sampling at (8x+4, 8y+4))"""
    return (np.ascontiguousarray(v4[4::8, 4::8]), np.ascontiguousarray(n4[4::8, 4::8]), np.ascontiguousarray(rgba[4::8, 4::8, :3]))


def planar(v4r, n4r):
    """copyMaps (cudafuncs.cu:271-311) of the reduced maps: [3*h, w], z == 0 -> NaN in all planes"""
    h, w = v4r.shape[:2]
    v = np.empty((3 * h, w), np.float32); n = np.empty((3 * h, w), np.float32)
    for y in range(h):
        for x in range(w):
            if not (v4r[y, x, 2] == 0):
                for c in range(3):
                    v[c * h + y, x] = v4r[y, x, c]; n[c * h + y, x] = n4r[y, x, c]
            else:
                for c in range(3):
                    v[c * h + y, x] = QNAN; n[c * h + y, x] = QNAN
    return v, n


# -------------------------------------------------------------------------------- codes
def codes_literal(table, v4r, rgb):
    """Ferns.cpp:89-109 without the inverted lists: codes u8 [n], goodCodes"""
    n = len(table)
    codes = np.empty(n, np.uint8)
    good = 0
    for i in range(n):
        f = table[i]
        code = BAD
        z = np.float32(v4r[f["y"], f["x"], 2])
        if z > 0:
            pix = rgb[f["y"], f["x"]]
            code = (int(int(pix[0]) > f["r"]) << 3 | int(int(pix[1]) > f["g"]) << 2 | int(int(pix[2]) > f["b"]) << 1 |
                    int(int(np.float32(z * np.float32(1000.0))) > f["d"]))
            good += 1
        codes[i] = code
    return codes, good


def codes_vector(table, v4r, rgb):
    z = v4r[table["y"], table["x"], 2].astype(np.float32)
    pix = rgb[table["y"], table["x"]].astype(np.int32)
    ok = z > 0
    with np.errstate(invalid="ignore", over="ignore"):
        mm = np.where(ok, z * np.float32(1000.0), np.float32(0)).astype(np.int32)
    c = ((pix[:, 0] > table["r"]).astype(np.int32) << 3 | (pix[:, 1] > table["g"]).astype(np.int32) << 2 |
         (pix[:, 2] > table["b"]).astype(np.int32) << 1 | (mm > table["d"]).astype(np.int32))
    return np.where(ok, c, BAD).astype(np.uint8), int(ok.sum())


def dissimilarity(good_q, good_k, co):
    """Ferns.cpp:115-117 in f32"""
    max_co = np.float32(min(good_q, good_k))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(np.float32(max_co - np.float32(co)) / max_co)


class Frame:
    def __init__(self, codes, good, pose, time, vmap, nmap, rgb):
        self.codes, self.good, self.pose, self.time, self.vmap, self.nmap, self.rgb = codes, good, pose, time, vmap, nmap, rgb


class Database:
    """Ferns::addFrame / findFrame with the conservatory's inverted lists ids[fern][code]"""

    def __init__(self, table, capacity=None):
        self.table = table
        self.ids = [[[] for _ in range(16)] for _ in range(len(table))]
        self.frames = []
        self.capacity = capacity
        self.full = False

    def _co(self, codes):
        co = [0] * len(self.frames)
        for i in range(len(self.table)):
            if codes[i] != BAD:
                for j in self.ids[i][codes[i]]:
                    co[j] += 1
        return co

    def add_minimum(self, codes, good):
        co = self._co(codes)
        minimum = FLT_MAX
        if good > 0:
            for k, fr in enumerate(self.frames):
                d = dissimilarity(good, fr.good, co[k])
                if d < minimum:
                    minimum = d
        return minimum, np.array(co, np.int32)

    def add_frame(self, v4, n4, rgba, pose, time, threshold):
        """-> appended, minimum, co"""
        v4r, n4r, rgb = reduce_maps(v4, n4, rgba)
        codes, good = codes_literal(self.table, v4r, rgb)
        minimum, co = self.add_minimum(codes, good)
        if (minimum > np.float32(threshold) or len(self.frames) == 0) and good > 0:
            if self.capacity is not None and len(self.frames) >= self.capacity:
                self.full = True
                return False, minimum, co
            fid = len(self.frames)
            for i in range(len(self.table)):
                if codes[i] != BAD:
                    self.ids[i][codes[i]].append(fid)
            vm, nm = planar(v4r, n4r)
            self.frames.append(Frame(codes, good, np.array(pose, np.float32).reshape(4, 4), int(time), vm, nm, rgb))
            return True, minimum, co
        return False, minimum, co

    def find(self, codes, good, time, min_age):
        """Ferns.cpp:184-196 -> minimum, minId, co"""
        co = self._co(codes)
        minimum, min_id = FLT_MAX, -1
        for k, fr in enumerate(self.frames):
            d = dissimilarity(good, fr.good, co[k])
            if d < minimum and time - fr.time > min_age:
                minimum, min_id = d, k
        return minimum, min_id, np.array(co, np.int32)


def search_vector(codes_q, good_q, db_codes, db_good, db_time, time, min_age):
    """the scan form: co[k] = #{i: q[i] != 255 and q[i] == c[k][i]} -> co, min_all, min_match, match_id"""
    K = len(db_good)
    if K == 0:
        return np.zeros(0, np.int32), FLT_MAX, FLT_MAX, -1
    co = ((db_codes == codes_q[None, :]) & (codes_q[None, :] != BAD)).sum(axis=1).astype(np.int32)
    if good_q == 0:
        return co, FLT_MAX, FLT_MAX, -1
    max_co = np.minimum(good_q, db_good).astype(np.float32)
    d = ((max_co - co.astype(np.float32)) / max_co).astype(np.float32)
    min_all = np.float32(min(FLT_MAX, d.min()))
    old = (time - db_time) > min_age
    if not old.any():
        return co, min_all, FLT_MAX, -1
    dm = np.where(old, d, np.float32(np.inf))
    k = int(np.argmin(dm))   # first minimum
    return co, min_all, np.float32(dm[k]), k


def block_hd_aware(c1, c2):
    """Ferns.cpp:321-336"""
    count = 0
    val = np.float32(0)
    for i in range(len(c1)):
        if c1[i] != BAD and c2[i] != BAD:
            count += 1
            if c1[i] == c2[i]:
                val = np.float32(val + np.float32(1.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(val / np.float32(count))


# -------------------------------------------------------------------- photometric check
def photometric_check(table, vmap_cur, rgb_cur, est_pose, fern_pose, fern_rgb, fx, fy, cx, cy, max_depth_mm):
    """Ferns.cpp:264-307 in f64 from the f32 inputs.  vmap_cur: planar [3*h, w]; fx..cy: the reduced intrinsics (f32).
    -> error (inf with no correspondence), count, the smallest distance of a correspondence coordinate to an integer"""
    h, w = rgb_cur.shape[:2]
    E = np.asarray(est_pose, np.float32).reshape(4, 4).astype(np.float64)
    F = np.asarray(fern_pose, np.float32).reshape(4, 4).astype(np.float64)
    fx, fy, cx, cy = (float(np.float32(a)) for a in (fx, fy, cx, cy))
    Rd = [[0.0] * 3 for _ in range(3)]
    td = [0.0] * 3
    for i in range(3):
        for j in range(3):
            Rd[i][j] = (F[0, i] * E[0, j] + F[1, i] * E[1, j]) + F[2, i] * E[2, j]
        td[i] = (F[0, i] * (E[0, 3] - F[0, 3]) + F[1, i] * (E[1, 3] - F[1, 3])) + F[2, i] * (E[2, 3] - F[2, 3])
    total, count, margin = 0, 0, np.inf
    for i in range(len(table)):
        f = table[i]
        z = np.float32(vmap_cur[2 * h + f["y"], f["x"]])
        if not (z > 0) or not (int(np.float32(z * np.float32(1000.0))) < max_depth_mm):
            continue
        x, y, zz = float(vmap_cur[f["y"], f["x"]]), float(vmap_cur[h + f["y"], f["x"]]), float(z)
        wx = ((Rd[0][0] * x + Rd[0][1] * y) + Rd[0][2] * zz) + td[0]
        wy = ((Rd[1][0] * x + Rd[1][1] * y) + Rd[1][2] * zz) + td[1]
        wz = ((Rd[2][0] * x + Rd[2][1] * y) + Rd[2][2] * zz) + td[2]
        with np.errstate(all="ignore"):
            u = float(np.float64(wx) * fx / np.float64(wz) + cx)
            v = float(np.float64(wy) * fy / np.float64(wz) + cy)
        if not (abs(u) < 1e9) or not (abs(v) < 1e9):
            continue
        margin = min(margin, abs(u - round(u)), abs(v - round(v)))
        iu, iv = int(u), int(v)   # truncation towards zero
        if iu < 0 or iv < 0 or iu >= w or iv >= h:
            continue
        kp = fern_rgb[iv, iu]
        if not (kp[0] > 0 or kp[1] > 0 or kp[2] > 0):
            continue
        cp = rgb_cur[f["y"], f["x"]]
        total += abs(int(kp[0]) - int(cp[0])) + abs(int(kp[1]) - int(cp[1])) + abs(int(kp[2]) - int(cp[2]))
        count += 1
    return (float(total) / float(count) if count else float("inf")), count, margin


# ------------------------------------------------------------------- the shared case table
W, H = 128, 64
RW, RH = W // 8, H // 8
MAX_DEPTH_MM = 5000
_CACHE = {}


def random_table(rng, n, rw=RW, rh=RH, max_depth_mm=MAX_DEPTH_MM):
    t = np.zeros(n, FERN)
    t["x"] = rng.integers(0, rw, n); t["y"] = rng.integers(0, rh, n)
    t["r"] = rng.integers(0, 256, n); t["g"] = rng.integers(0, 256, n); t["b"] = rng.integers(0, 256, n)
    t["d"] = rng.integers(400, max_depth_mm + 1, n)
    return t


def base_maps(seed=5):
    """full-size maps of a made-up frame: every texel random, a tenth of the depths zero"""
    key = ("base", seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        v4 = rng.uniform(-2, 2, (H, W, 4)).astype(np.float32)
        v4[..., 2] = rng.uniform(0.4, 5.5, (H, W)).astype(np.float32)
        v4[..., 2][rng.random((H, W)) < 0.1] = 0
        n4 = rng.normal(size=(H, W, 4)).astype(np.float32)
        rgba = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        _CACHE[key] = (v4, n4, rgba)
    return _CACHE[key]


def variant(i, strength=0.3, seed=5):
    """base_maps with the colours and depths of a fraction `strength` of the reduced pixels redrawn (variant 0 is the base)"""
    key = ("var", i, strength, seed)
    if key not in _CACHE:
        v4, n4, rgba = (a.copy() for a in base_maps(seed))
        if i:
            rng = np.random.default_rng(1000 + i)
            m = rng.random((RH, RW)) < strength
            ys, xs = np.nonzero(m)
            rgba[8 * ys + 4, 8 * xs + 4] = rng.integers(0, 256, (len(ys), 4), dtype=np.uint8)
            v4[8 * ys + 4, 8 * xs + 4, 2] = rng.uniform(0.4, 5.5, len(ys)).astype(np.float32)
        _CACHE[key] = (v4, n4, rgba)
    return _CACHE[key]


def pose_of(i):
    p = np.eye(4, dtype=np.float32)
    p[:3, 3] = [0.01 * i, -0.02 * i, 0.5 + i]
    return p


def edge_case_maps():
    """one reduced pixel per way a code can go wrong; the table that goes with it is edge_case_table()"""
    v4, n4, rgba = (a.copy() for a in base_maps())
    def put(x, y, z, rgb):
        v4[8 * y + 4, 8 * x + 4, 2] = np.float32(z); rgba[8 * y + 4, 8 * x + 4, :3] = rgb
    put(0, 0, 1.25, (100, 100, 100))      # int(z*1000) == 1250 exactly; colour equal to the thresholds
    put(15, 7, 1.25, (101, 99, 100))
    put(1, 0, 0.0, (200, 200, 200))       # z == 0
    put(2, 0, -1.0, (200, 200, 200))      # z < 0
    put(3, 0, 1e-30, (200, 200, 200))     # tiny z: good, int(z*1000) == 0
    put(4, 0, 1.2505, (10, 20, 30))       # int(1250.5) == 1250: truncation
    return v4, n4, rgba


def edge_case_table():
    rows = [(0, 0, 100, 100, 100, 1250), (0, 0, 99, 101, 100, 1249), (0, 0, 100, 100, 100, 1251),
            (15, 7, 100, 100, 100, 1250), (15, 7, 101, 99, 99, 1249),
            (1, 0, 0, 0, 0, 400), (2, 0, 0, 0, 0, 400), (3, 0, 0, 0, 0, 400), (3, 0, 255, 255, 255, 5000),
            (4, 0, 10, 20, 30, 1250), (4, 0, 9, 19, 29, 1249), (4, 0, 11, 21, 31, 1251)]
    t = np.zeros(len(rows), FERN)
    for i, r in enumerate(rows):
        t[i] = r
    return t
