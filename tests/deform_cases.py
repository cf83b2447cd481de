"""Named cases of the deformation graph (tests/deform_ref.py): the smallest shapes at which each rule of DESIGN.md 4.14 can fail.
Everything is built from fixed seeds with numpy only; test_cpu_deform_ref.py holds the conditions the GPU comparisons rest on."""
from types import SimpleNamespace as NS

import numpy as np

import deform_ref as ref

f32 = np.float32

# node counts: 5 (both end rules of connectGraphSeq meet, A dense), 6 and 12 (the window clipped at both ends), 21 and 45 (interior rows,
# a band narrower than the matrix).  4 nodes: no graph.  1024: the allocation limit.
NODE_COUNTS = (5, 6, 12, 21, 45)
BIG = 1024


def path(t):
    """a camera sweeping a room: the surface point seen at (fractional) time t, metres"""
    t = np.asarray(t, np.float64)
    return np.stack([0.012 * t + 0.2 * np.sin(0.05 * t), 0.3 * np.cos(0.031 * t), 1.5 + 0.25 * np.sin(0.017 * t + 1.0)], -1)


def make_nodes(n, seed=0, step=12):
    """n nodes along the path; times non-decreasing with runs of two and three equal times (many surfels are born in one frame)"""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    t = np.cumsum(np.where(np.arange(n) % 5 == 2, 0, np.where(np.arange(n) % 7 == 5, 0, step)))
    pos = path(t + rng.uniform(0, 0.5, n)) + rng.normal(0, 0.02, (n, 3))
    return np.concatenate([pos, t[:, None]], 1).astype(f32)


def make_map(s, per_frame, seed=0, first_time=1):
    """s surfels, per_frame born in every frame, near the path point of their frame"""
    rng = np.random.default_rng(2000 + seed)
    t = first_time + np.arange(s) // per_frame
    m = np.zeros((s, 12), f32)
    m[:, 0:3] = path(t) + rng.normal(0, 0.05, (s, 3))
    m[:, 3] = rng.uniform(0, 20, s)              # confidence around the threshold of 10
    m[:, 4] = rng.integers(0, 1 << 24, s)
    m[:, 6] = t
    m[:, 7] = t + rng.integers(0, 30, s)
    nrm = rng.normal(size=(s, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    m[:, 8:11] = nrm
    m[:, 11] = rng.uniform(0.002, 0.02, s)
    return m


def bent_params(n, seed=0, scale=0.05):
    """node parameters away from the identity (what an optimisation leaves): rotations off orthogonal, translations of centimetres"""
    rng = np.random.default_rng(3000 + seed)
    p = ref.identity_params(n)
    p[:, :9] += rng.normal(0, scale, (n, 9)).astype(f32)
    p[:, 9:] = rng.normal(0, 0.05, (n, 3)).astype(f32)
    return p


# ------------------------------------------------------------------------------------------------ maps for the sampling call
#   name: (surfels, per_frame, sample_rate) -> nodes
R = 7
MAPS = {
    "first_of_stride": (R * 11 + 1, 3, R),         # S = r (N-1) + 1: the last node is the last surfel
    "full_stride": (R * 11 + R, 3, R),             # S = r (N-1) + r
    "four_nodes": (4 * R, 3, R),                   # no graph
    "five_nodes": (4 * R + 1, 3, R),
    "workgroups": (4099, 9, 64),                   # 65 nodes; the apply pass crosses workgroup edges and ends inside one
    "stride_rule": (3000, 5, 2),                   # 1500 > 1024 candidates: stride 4, 750 nodes
    "one_frame": (300, 300, 10),                   # every node has the same time
}


def get_map(name):
    s, per, rate = MAPS[name]
    return NS(name=name, surfels=make_map(s, per, seed=len(name)), sample_rate=rate)


def non_monotone_map():
    m = make_map(R * 11 + 1, 3, seed=5)
    m[3 * R, 6] = m[2 * R, 6] - 1                  # node 3 older than node 2
    return NS(name="non_monotone", surfels=m, sample_rate=R)


# ------------------------------------------------------------------------------------------------ points for the window rule
def window_points(nodes, seed=0):
    """points (x, y, z, time) that walk every branch of the search over `nodes` (none of them with a 4th / 5th distance tie: the CPU
    suite checks; the crafted ties are tie_nodes and degenerate_nodes)"""
    rng = np.random.default_rng(4000 + seed)
    n = len(nodes); T = nodes[:, 3].astype(np.int64)
    pts = []

    def add(p, t):
        pts.append([p[0], p[1], p[2], t])
    for i in range(n):                              # a time equal to a node's (runs of equal times included)
        add(nodes[i, :3] + rng.normal(0, 0.03, 3), T[i])
    for i in range(n - 1):                          # between two nodes: nearer the first, nearer the second, exactly between
        if T[i + 1] - T[i] >= 4:
            mid = (nodes[i, :3] + nodes[i + 1, :3]) / 2 + rng.normal(0, 0.03, 3)
            add(mid, T[i] + 1); add(mid, T[i + 1] - 1)
            if (T[i + 1] - T[i]) % 2 == 0:
                add(mid, (T[i] + T[i + 1]) // 2)
    add(nodes[0, :3] + rng.normal(0, 0.03, 3), T[0] - 5)      # before the first node
    add(nodes[-1, :3] + rng.normal(0, 0.03, 3), T[-1] + 9)    # after the last
    add(nodes[n // 2, :3] + rng.normal(0, 2.0, 3), T[n // 2])  # far from every node
    return np.asarray(pts, f32)


def tie_nodes():
    """six nodes on exact binary fractions: from the origin, nodes 3 and 4 are both at distance 1 (the 4th / 5th candidate by the stable
    order), node 5 further out"""
    pos = np.array([[0.25, 0, 0], [0, 0.5, 0], [0, 0, 0.75], [1, 0, 0], [0, -1, 0], [0, 0, 2]], f32)
    return np.concatenate([pos, np.arange(6, dtype=f32)[:, None] * 3], 1)


def degenerate_nodes(coincident):
    """five candidates at one distance from the origin (weights 0 / 0), or all at the origin itself (dMax == 0)"""
    pos = np.zeros((5, 3), f32) if coincident else np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], f32)
    return np.concatenate([pos, np.arange(5, dtype=f32)[:, None]], 1)


# ------------------------------------------------------------------------------------------------ constraint sets
def _near(nodes, idx, rng, spread=0.04):
    return nodes[idx, :3] + rng.normal(0, spread, (len(idx), 3)).astype(f32), nodes[idx, 3]


def constraints(kind, nodes, seed=0):
    """-> src [m, 3], dst [m, 3], src_time [m] (pins included, in the order Deformation::addConstraint pushes them)"""
    rng = np.random.default_rng(5000 + seed + len(nodes))
    n = len(nodes)
    # the newest and the oldest fifth of the nodes.  (With thirds the 45-node shift is accepted too, but its worst source lands 2 mm off:
    # the landing bound of 3e-4 m needs more free nodes between the pinned and the shifted part.)
    third = max(n // 5, 2)
    new, old = np.arange(n - third, n), np.arange(0, third)
    if kind == "none":
        return np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, f32)
    if kind == "one":
        p, t = _near(nodes, new[-1:], rng)
        return p, p + f32([0.1, 0, 0.05]), t
    if kind == "anchored":        # (the 1024-node graph) one constraint at every 16th node: the newest fifth moves by 15 cm, the rest stays
        idx = np.arange(0, n, max(n // 64, 1))[:64]
        p, t = _near(nodes, idx, rng)
        return p, (p + np.where((idx >= n - n // 5)[:, None], f32([0.0, 0.15, 0.0]), f32(0))).astype(f32), t
    if kind in ("shift", "small", "wild"):
        m = 50
        p, t = _near(nodes, new[np.arange(m) % third], rng)
        q, tq = _near(nodes, old[np.arange(m) % third], rng)
        if kind == "shift":       # the newest part of the map moves by 15 cm, the oldest part is pinned
            d = np.tile(f32([0.0, 0.15, 0.0]), (m, 1))
        elif kind == "small":     # a mean constraint error below 0.06: not optimised
            d = np.tile(f32([0.0, 0.05, 0.0]), (m, 1))
        else:                     # targets thrown metres apart in alternating directions: the first iteration leaves error > 10
            d = (rng.choice([-1.0, 1.0], (m, 1)) * f32([3.0, -2.0, 2.5])).astype(f32)
        src = np.empty((2 * m, 3), f32); dst = np.empty((2 * m, 3), f32); tm = np.empty(2 * m, f32)
        src[0::2] = p; dst[0::2] = p + d; tm[0::2] = t
        src[1::2] = q; dst[1::2] = q; tm[1::2] = tq      # the pin: target -> target at the target's time
        return src, dst, tm
    raise KeyError(kind)


# no constraint leaves the translation of the whole graph free, one leaves its rotation about the constrained point free: A is singular
# to rounding and its solution is no yardstick.  These sets are compared up to the assembled system (weights, A, b, errors) only.
GAUGE_FREE = ("none", "one")


# (node count, constraint kind): every kind, every node count, the shift on all of them
SYSTEMS = [(n, "shift") for n in NODE_COUNTS] + [(5, "one"), (21, "one"), (6, "none"), (12, "small"), (21, "wild")]
_CACHE = {}


def system(n, kind):
    """the statement's run of one (node count, constraint kind), computed once and shared: optimise from the identity, and the system
    of the first iteration"""
    key = (n, kind)
    if key not in _CACHE:
        nodes = make_nodes(n)
        src, dst, tm = constraints(kind, nodes)
        trace = []
        opt = ref.optimise(nodes, src, dst, tm, trace=trace)
        jr, r = ref.rows(nodes, ref.identity_params(n), src, dst, opt["ids"], opt["w"], opt["ok"])
        J, A, b = ref.dense_system(n, jr, r)
        _CACHE[key] = dict(nodes=nodes, src=src, dst=dst, tm=tm, opt=opt, trace=trace, jr=jr, r=r, J=J, A=A, b=b)
    return _CACHE[key]


def singular_state(n=6):
    """coincident nodes, no constraints, all parameters zero: the rotation rows of J vanish and the first pivot is 0"""
    nodes = np.zeros((n, 4), f32); nodes[:, :3] = f32([0.5, -0.25, 2.0]); nodes[:, 3] = np.arange(n)
    return nodes, np.zeros((n, 12), f32)


# ------------------------------------------------------------------------------------------------ keyframe poses
def rot(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def poses_case(nodes, kind, seed=0):
    """keyframe poses along the nodes, and node parameters: `rotation` (every node a rigid motion) or `half` (3x3 of determinant near 0.5)"""
    rng = np.random.default_rng(6000 + seed)
    n = len(nodes)
    idx = np.arange(0, n, max(n // 8, 1))
    poses = np.zeros((len(idx), 4, 4), f32)
    for k, i in enumerate(idx):
        poses[k, :3, :3] = rot(rng.normal(size=3), rng.uniform(0, 2.5))
        poses[k, :3, 3] = nodes[i, :3] + rng.normal(0, 0.1, 3)
        poses[k, 3, 3] = 1
    params = ref.identity_params(n)
    for i in range(n):
        Rm = rot([0.2, 1.0, -0.4], 0.1 + 0.01 * i)
        if kind == "half":
            Rm = Rm * 0.5 ** (1 / 3) + rng.normal(0, 0.01, (3, 3))
        params[i, :9] = Rm.T.reshape(9)            # column-major
        params[i, 9:] = rng.normal(0, 0.05, 3)
    return poses, nodes[idx, 3].astype(np.int32), params
