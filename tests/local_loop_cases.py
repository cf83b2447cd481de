"""Named cases of local loop closure: the graph's local mode (tests/local_loop_ref.py) on the node sets of tests/deform_cases.py, and
crafted maps for the inactive prediction and the depth synthesis -- the smallest shapes at which each rule of DESIGN.md 4.14 "the local
half" can fail.  Fixed seeds, numpy only; test_cpu_local_loop_ref.py holds the conditions the GPU comparisons (test_local_deform_gpu.py,
test_local_loop_kernels_gpu.py) rest on."""
import numpy as np

import deform_cases as dc
import deform_ref as ref
import local_loop_ref as lref

f32 = np.float32


def last_deform_time(nodes, which):
    """zero: every node enabled (node times start at 12).  half: the time of node n/2 - 1 exactly -- that node, compared `time > ldt` at
    equality, is disabled, and so is every node that shares its time; the next time up is enabled.  all_off: the newest node's time."""
    t = nodes[:, 3].astype(np.int64)
    return {"zero": 0, "half": int(t[len(t) // 2 - 1]), "all_off": int(t[-1])}[which]


def constraints(kind, nodes):
    """dead_one: the 50 sources of the shift near the newest fifth (no pins) and one constraint 0.3 m long at node 1, whose whole weight
    set is disabled under `half`.  far: the shift by 1 m instead of 15 cm -- the first iteration leaves error > 10 (where the global mode
    stops) and the later ones keep lowering it.  Every other kind: deform_cases.constraints."""
    if kind not in ("dead_one", "far"):
        return dc.constraints(kind, nodes)
    src, dst, tm = dc.constraints("shift", nodes)
    if kind == "far":
        dst = dst.copy(); dst[0::2] = src[0::2] + f32([0.0, 1.0, 0.0])
        return src, dst, tm
    p = (nodes[1:2, :3] + f32([0.01, -0.02, 0.015])).astype(f32)
    return (np.concatenate([src[0::2], p]), np.concatenate([dst[0::2], p + f32([0.3, 0.0, 0.0])]).astype(f32),
            np.concatenate([tm[0::2], nodes[1:2, 3]]))


def big_constraints(nodes, m=768, seed=0):
    """m constraints near the newest third of the nodes moved by 4 cm, each followed by its pin near the oldest third: 2 m rows, the
    most a 640x480 local closure makes (768 + 768)"""
    rng = np.random.default_rng(7000 + seed + len(nodes))
    n = len(nodes); third = max(n // 3, 2)
    new = np.arange(n - third, n)[np.arange(m) % third]; old = np.arange(0, third)[np.arange(m) % third]
    p = nodes[new, :3] + rng.normal(0, 0.04, (m, 3)).astype(f32)
    q = nodes[old, :3] + rng.normal(0, 0.04, (m, 3)).astype(f32)
    src = np.empty((2 * m, 3), f32); dst = np.empty((2 * m, 3), f32); tm = np.empty(2 * m, f32)
    src[0::2] = p; dst[0::2] = p + f32([0.0, 0.04, 0.0]); tm[0::2] = nodes[new, 3]
    src[1::2] = q; dst[1::2] = q; tm[1::2] = nodes[old, 3]
    return src, dst, tm


# (node count, constraint kind, which last_deform_time)
IDENTICAL = [(n, "shift", "zero") for n in dc.NODE_COUNTS] + [(6, "none", "zero"), (21, "wild", "zero")]   # byte-identical to the global mode
DISABLED = [(12, "shift", "half"), (21, "shift", "half"), (45, "shift", "half"), (45, "dead_one", "half"), (21, "none", "half"),
            (21, "shift", "all_off"), (45, "dead_one", "all_off")]
# free-running optimise: the two sets the global mode turns away or stops, the disabled cases, and every node count at `zero`
FREE_RUNNING = [(12, "small", "zero"), (21, "far", "zero"), (21, "wild", "zero"), (21, "shift", "zero"), (45, "shift", "zero")] + [c for c in DISABLED if c[1] != "none"]
BIG = [(45, "zero"), (45, "half"), (200, "zero")]          # 768 + 768 constraints
_CACHE = {}


def system(n, kind, which):
    """the statement's run of one case, computed once and shared: optimise from the identity, and the system of the first iteration"""
    key = (n, kind, which)
    if key not in _CACHE:
        nodes = dc.make_nodes(n)
        ldt = last_deform_time(nodes, which)
        src, dst, tm = constraints(kind, nodes)
        trace = []
        opt = lref.optimise(nodes, src, dst, tm, ldt, trace=trace)
        jr, r, keep, en = lref.rows(nodes, ref.identity_params(n), src, dst, opt["ids"], opt["w"], opt["ok"], ldt)
        J, A, b = lref.dense_system(n, jr, r, en)
        _CACHE[key] = dict(nodes=nodes, ldt=ldt, src=src, dst=dst, tm=tm, opt=opt, trace=trace, jr=jr, r=r, keep=keep, en=en, J=J, A=A, b=b)
    return _CACHE[key]


def big_system(n, which):
    key = ("big", n, which)
    if key not in _CACHE:
        nodes = dc.make_nodes(n)
        ldt = last_deform_time(nodes, which)
        src, dst, tm = big_constraints(nodes)
        ids, w, ok = ref.weights(nodes, src, tm)
        jr, r, keep, en = lref.rows(nodes, ref.identity_params(n), src, dst, ids, w, ok, ldt)
        AB, b = lref.band_system(n, jr, r, en)
        _CACHE[key] = dict(nodes=nodes, ldt=ldt, src=src, dst=dst, tm=tm, ids=ids, w=w, ok=ok, jr=jr, r=r, keep=keep, en=en, AB=AB, b=b)
    return _CACHE[key]


def singular_half(n=6):
    """deform_cases.singular_state (coincident nodes, all parameters zero) with the older half disabled: the identity blocks factor, and
    the first enabled rotation column has a zero pivot"""
    nodes, params = dc.singular_state(n)
    return nodes, params, int(nodes[n // 2 - 1, 3])


# ------------------------------------------------------------------------------------------------ maps for the inactive prediction
# 256 x 160: two waves of 20x samples, and no multiple of the 256-thread workgroups' row length
SHAPE = (256, 160)
CAM = (200.0, 200.0, 128.0, 80.0)
MAX_TIME, TICK, SPLAT_DELTA = 100, 140, 40     # maxTime = tick - timeDelta
SPLAT_CONF, SPLAT_DEPTH = 10.0, 20.0
SPLAT_MAPS = ("mixed", "all_active", "old_in_front", "active_in_front")


def layer(rng, nx, ny, z, last_time, x0=-1.0, x1=1.0, y0=-0.6, y1=0.6, radius=0.03):
    """nx * ny surfels facing the camera on the plane of depth z, a little jitter; last_time: one value or one per surfel"""
    gx, gy = np.meshgrid(np.linspace(x0, x1, nx), np.linspace(y0, y1, ny))
    n = gx.size
    m = np.zeros((n, 12), f32)
    m[:, 0] = gx.reshape(-1) * z / 2 + rng.normal(0, 0.002, n); m[:, 1] = gy.reshape(-1) * z / 2 + rng.normal(0, 0.002, n); m[:, 2] = z + rng.normal(0, 0.01, n)
    m[:, 3] = rng.uniform(11, 30, n)
    m[:, 4] = rng.integers(1 << 16, 1 << 24, n) | 0x010101      # (no colour channel is 0)
    m[:, 7] = last_time
    m[:, 6] = np.maximum(m[:, 7] - rng.integers(0, 30, n), 1)
    nrm = np.tile(f32([0, 0, -1]), (n, 1)) + rng.normal(0, 0.05, (n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    m[:, 8:11] = nrm
    m[:, 11] = radius * z / 2
    return m


def splat_map(kind):
    """a few hundred surfels in camera coordinates (the pose of the cases is the identity):
    mixed            one wall whose surfels alternate between last_time <= MAX_TIME and > MAX_TIME, with every eighth exactly AT MAX_TIME
                     (kept: the rule is `last_time > maxTime` out) and a few below the confidence threshold
    all_active       the same wall, every last_time > MAX_TIME: the inactive set is empty
    old_in_front     an inactive patch at 1.5 m in front of an active wall at 2 m
    active_in_front  an active patch at 1.5 m in front of an inactive wall at 2 m: the inactive prediction sees through it"""
    rng = np.random.default_rng(8000 + len(kind))
    if kind in ("mixed", "all_active"):
        n = 24 * 14
        t = np.where(np.arange(n) % 2 == 0, rng.integers(40, MAX_TIME, n), rng.integers(MAX_TIME + 1, TICK + 1, n))
        t[::8] = MAX_TIME
        if kind == "all_active":
            t = rng.integers(MAX_TIME + 1, TICK + 1, n)
        m = layer(rng, 24, 14, 2.0, t)
        m[5::17, 3] = 5.0
        return m
    front_old = kind == "old_in_front"
    # (radius 0.08: both layers are closed surfaces around the image centre)
    wall = layer(rng, 24, 14, 2.0, rng.integers(MAX_TIME + 1, TICK + 1, 24 * 14) if front_old else rng.integers(40, MAX_TIME + 1, 24 * 14), radius=0.08)
    patch = layer(rng, 10, 8, 1.5, rng.integers(40, MAX_TIME + 1, 80) if front_old else rng.integers(MAX_TIME + 1, TICK + 1, 80), -0.4, 0.4, -0.3, 0.3,
                   radius=0.08)
    return np.concatenate([wall, patch])


# ------------------------------------------------------------------------------------------------ the constraint stage
# 256 x 160 -> 12 x 8 = 96 samples, visited column by column: sample k = 8 x + y, so the second wave starts in column 8
CONS_TICK, CONS_MAX_DEPTH = 140, 4.0
COV_POW2 = 2.0 ** -17          # a covariance threshold that 1 / lastA can hit exactly


def cons_pose(seed):
    rng = np.random.default_rng(9000 + seed)
    R = dc.rot(rng.normal(size=3), 0.05 + 0.02 * seed)
    m = np.eye(4, dtype=f32); m[:3, :3] = R; m[:3, 3] = rng.normal(0, 0.05, 3)
    return m


def good_track(**over):
    """a tracker result the default thresholds accept; keyword arguments replace fields"""
    est = cons_pose(1)
    t = dict(rot=est[:3, :3].copy(), trans=est[:3, 3].copy(), icp_error=f32(2e-5), icp_count=f32(52000.0), lastA=np.diag(np.full(6, 1e6)))
    t.update(over)
    return t


def spd_lastA(seed=3):
    """J^T J of 5000 rows with columns of very different scale, rows permuted so that the LU pivots: covariance diagonal around 1e-7"""
    rng = np.random.default_rng(9100 + seed)
    J = rng.normal(size=(5000, 6)) * np.array([3000.0, 40.0, 900.0, 60.0, 2000.0, 150.0])
    return (np.eye(6)[[3, 0, 5, 1, 4, 2]] @ (J.T @ J))


# name -> (track, thresholds); the exact hits: `>` / `<` strict as written, a covariance entry exactly covThresh passes
ACCEPT_CASES = {
    "accepted": (good_track(), {}),
    "pivoting_lastA": (good_track(lastA=spd_lastA()), {}),
    "cov_exactly_at_threshold": (good_track(lastA=np.diag(np.full(6, 2.0 ** 17))), dict(cov_thresh=COV_POW2)),
    "cov_one_ulp_above": (good_track(lastA=np.diag([2.0 ** 17] * 4 + [2.0 ** 17 * (1 - 2.0 ** -52)] + [2.0 ** 17])), dict(cov_thresh=COV_POW2)),
    "count_exactly_at_threshold": (good_track(icp_count=f32(40000.0)), {}),
    "count_one_above": (good_track(icp_count=f32(40001.0)), {}),
    "error_exactly_at_threshold": (good_track(icp_error=f32(5e-5)), {}),
    "error_one_ulp_below": (good_track(icp_error=np.nextafter(f32(5e-5), f32(0))), {}),
    "singular_zero": (good_track(lastA=np.zeros((6, 6))), {}),
    "singular_one_column": (good_track(lastA=np.diag([1e6, 1e6, 0.0, 1e6, 1e6, 1e6])), {}),
}
ACCEPT_WANT = {"accepted": True, "pivoting_lastA": True, "cov_exactly_at_threshold": True, "cov_one_ulp_above": False,
               "count_exactly_at_threshold": False, "count_one_above": True, "error_exactly_at_threshold": False, "error_one_ulp_below": True,
               "singular_zero": False, "singular_one_column": False}
SAMPLE_CASES = ("all_valid", "none_valid", "gaps_across_the_wave", "z_at_max_depth", "old_time_zero")


def cons_maps(kind):
    """-> vertex f32 [160, 256, 4], old_time u16 [160, 256]; every texel holds a point, so a wrong sampling position shows"""
    rng = np.random.default_rng(9200 + len(kind))
    w, h = SHAPE
    v = np.zeros((h, w, 4), f32)
    v[..., 0] = rng.uniform(-1.5, 1.5, (h, w)); v[..., 1] = rng.uniform(-1, 1, (h, w)); v[..., 2] = rng.uniform(0.5, 3.5, (h, w)); v[..., 3] = 12
    t = rng.integers(1, 100, (h, w)).astype(np.uint16)
    sx = lambda k: 20 * (k // 8) + 10
    sy = lambda k: 20 * (k % 8) + 10
    if kind == "none_valid":
        v[..., 2] = 0
    elif kind == "gaps_across_the_wave":      # samples 59..62 and 65..67 out, 63 and 64 in; the first and the last sample out
        for k in (0, 59, 60, 61, 62, 65, 66, 67, 95):
            v[sy(k), sx(k), 2] = 0
    elif kind == "z_at_max_depth":            # exactly maxDepth: invalid; one ulp below: valid; negative and NaN: invalid
        for k in range(0, 96, 5):
            v[sy(k), sx(k), 2] = CONS_MAX_DEPTH
        for k in range(1, 96, 5):
            v[sy(k), sx(k), 2] = np.nextafter(f32(CONS_MAX_DEPTH), f32(0))
        v[sy(2), sx(2), 2] = -1.0; v[sy(7), sx(7), 2] = np.nan
    elif kind == "old_time_zero":
        for k in range(3, 96, 7):
            t[sy(k), sx(k)] = 0
        t[sy(64), sx(64)] = 0
    return v, t
