"""Named cases of the relative constraints (tests/deform_rel_ref.py): the smallest shapes at which each of its rules can fail, on the node
counts of tests/deform_cases.py.  Fixed seeds, numpy only; test_cpu_deform_rel_ref.py holds the conditions the GPU comparisons rest on."""
import numpy as np

import deform_cases as dc
import deform_ref as ref
import deform_rel_ref as rel

f32 = np.float32


def loop_nodes(n=45, step=12, drift=0.03):
    """n nodes on a path that returns to its start: a circle of radius 1.2 m walked once, the end `drift` metres off the start.  The newest
    nodes lie beside the oldest ones in space and n - 1 blocks away from them in the matrix."""
    rng = np.random.default_rng(7000 + n)
    t = step * np.arange(n)
    a = 2 * np.pi * np.arange(n) / (n - 1)
    pos = np.stack([1.2 * np.cos(a), 0.1 * np.sin(3 * a) + drift * np.arange(n) / (n - 1), 1.2 * np.sin(a) + 2.0], -1)
    pos = pos + rng.normal(0, 0.01, (n, 3))
    return np.concatenate([pos, t[:, None]], 1).astype(f32)


def loop_constraints(nodes, seed=0):
    """the shift constraints of deform_cases on a loop: the newest fifth of the nodes moves by 15 cm, and the pins hold the MIDDLE fifth
    (the far side of the circle).  The oldest nodes, which lie beside the newest, are left to the regulariser -- and to the pairs."""
    rng = np.random.default_rng(7100 + seed + len(nodes))
    n = len(nodes); fifth = max(n // 5, 2); m = 50
    new = np.arange(n - fifth, n); mid = np.arange(n // 2 - fifth // 2, n // 2 - fifth // 2 + fifth)
    p, t = dc._near(nodes, new[np.arange(m) % fifth], rng)
    q, tq = dc._near(nodes, mid[np.arange(m) % fifth], rng)
    src = np.empty((2 * m, 3), f32); dst = np.empty((2 * m, 3), f32); tm = np.empty(2 * m, f32)
    src[0::2] = p; dst[0::2] = p + f32([0.0, 0.15, 0.0]); tm[0::2] = t
    src[1::2] = q; dst[1::2] = q; tm[1::2] = tq
    return src, dst, tm


def pairs_between(nodes, a, b, count, seed=0, gap=0.004, apart=False):
    """`count` pairs: sources beside the nodes a (at their times), targets `gap` metres from the sources but stamped with the times of the
    nodes b -- surfaces a local closure has registered.  apart: the targets lie beside the nodes b instead."""
    rng = np.random.default_rng(7200 + seed + len(nodes))
    a = np.asarray(a); b = np.asarray(b)
    ia = a[np.arange(count) % len(a)]; ib = b[np.arange(count) % len(b)]
    src = nodes[ia, :3] + rng.normal(0, 0.03, (count, 3)).astype(f32)
    tgt = src + rng.normal(0, gap, (count, 3)).astype(f32)
    if apart:
        tgt = nodes[ib, :3] + rng.normal(0, 0.03, (count, 3)).astype(f32)
    return np.concatenate([src, nodes[ia, 3:4], tgt, nodes[ib, 3:4]], 1).astype(f32)


def nan_nodes():
    """six nodes; from the origin five of them are at distance exactly 1: the four weights are 0 / 0"""
    pos = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -2]], f32)
    return np.concatenate([pos, 3 * np.arange(6, dtype=f32)[:, None]], 1)


def _case(name):
    if name.startswith("loop"):                       # the off-band coupling itself: newest <-> oldest nodes, >= 20 blocks apart
        nodes = loop_nodes(45)
        src, dst, tm = loop_constraints(nodes)
        pairs = pairs_between(nodes, [44, 43, 42, 41], [0, 1, 2, 3], int(name[4:]))
        return nodes, src, dst, tm, pairs
    if name.startswith("path"):                       # the straight path of deform_cases: three pairs across it
        n = int(name[4:])
        nodes = dc.make_nodes(n)
        src, dst, tm = dc.constraints("shift", nodes)
        return nodes, src, dst, tm, pairs_between(nodes, [n - 1, n - 2], [0, 1], 3)
    if name == "overlap":                             # source and target sets that share nodes: entries summed
        nodes = dc.make_nodes(21)
        src, dst, tm = dc.constraints("shift", nodes)
        return nodes, src, dst, tm, pairs_between(nodes, [9, 10], [11, 12], 3, apart=True)
    if name == "same":                                # identical source and target sets
        nodes = dc.make_nodes(21)
        src, dst, tm = dc.constraints("shift", nodes)
        return nodes, src, dst, tm, pairs_between(nodes, [10], [10], 3, gap=0.002)
    if name == "nan":                                 # a pair with a NaN weight set between two ordinary ones
        nodes = nan_nodes()
        src, dst, tm = dc.constraints("shift", nodes)
        pairs = pairs_between(nodes, [5, 4], [0, 1], 3)
        pairs[1, 0:3] = 0; pairs[1, 3] = 6
        return nodes, src, dst, tm, pairs
    raise KeyError(name)


# every case is solvable (100 absolute constraints fix the gauge)
CASES = ["loop1", "loop3", "loop4", "path5", "path6", "path12", "path21", "overlap", "same", "nan"]
_CACHE = {}


def case(name):
    """the statement's run of one case, computed once and shared: optimise from the identity (with and, for the loop, without the pairs),
    the system of the first iteration and its extended-precision solution"""
    if name not in _CACHE:
        nodes, src, dst, tm, pairs = _case(name)
        trace = []
        opt = rel.optimise(nodes, src, dst, tm, pairs, trace=trace)
        P0 = ref.identity_params(len(nodes))
        s = rel.system(nodes, P0, src, dst, opt["ids"], opt["w"], opt["ok"], pairs, opt["ws"], opt["wt"])
        _CACHE[name] = dict(nodes=nodes, src=src, dst=dst, tm=tm, pairs=pairs, opt=opt, trace=trace, sys=s)
    return _CACHE[name]


def solved(name):
    """-> star (longdouble), delta of the stated method, delta of numpy's dense Cholesky, for the first iteration (computed once)"""
    c = case(name)
    if "star" not in c:
        s = c["sys"]
        c["star"] = rel.solve_star(s["A"], s["b"])
        c["direct"], c["C"] = rel.solve(ref.to_band(s["B"]), s["U"], s["b"])
        c["dense"] = ref._tri(np.linalg.cholesky(s["A"]), s["b"])
    return c["star"], c["direct"], c["dense"]


def big_case():
    """1024 nodes, the anchored constraints of deform_cases, 128 pairs between the newest and the oldest 32 nodes"""
    if "big" not in _CACHE:
        n = dc.BIG
        nodes = dc.make_nodes(n)
        src, dst, tm = dc.constraints("anchored", nodes)
        pairs = pairs_between(nodes, np.arange(n - 32, n), np.arange(32), rel.RING, gap=0.01)
        _CACHE["big"] = dict(nodes=nodes, src=src, dst=dst, tm=tm, pairs=pairs)
    return _CACHE["big"]


def gate_case():
    """one absolute constraint 0.07 m off, one pair: the mean over both is 0.035 < 0.06 -- not optimised; without the pair it is"""
    nodes = dc.make_nodes(12)
    src = nodes[11:12, :3] + f32([0.01, 0.0, 0.02])
    dst = src + f32([0.0, 0.07, 0.0])
    return nodes, src.astype(f32), dst.astype(f32), nodes[11:12, 3].copy(), pairs_between(nodes, [10], [2], 1)


def closure_rows(n, seed=0):
    """the constraint buffers of an accepted local closure with n constraints (pinned: rows 2 i and 2 i + 1), its graph and parameters"""
    rng = np.random.default_rng(7300 + n + seed)
    nodes = dc.make_nodes(21)
    params = dc.bent_params(21, seed=n)
    idx = rng.integers(0, 21, n)
    src = (nodes[idx, :3] + rng.normal(0, 0.05, (n, 3))).astype(f32)
    dst = (src + rng.normal(0, 0.02, (n, 3))).astype(f32)
    t_src = np.full(n, nodes[-1, 3] + 5, f32)
    t_dst = nodes[rng.integers(0, 10, n), 3].astype(f32)
    return nodes, params, src, dst, t_src, t_dst


PICK_COUNTS = (1, 2, 3, 4, 5, 8, 11, 767)
# where the stated method itself (not only numpy's Cholesky) lands a quarter ulp of f32 from the extended-precision parameters with a
# factor 4 to spare: statement and device then round to parameters at most one ulp apart (test_cpu_deform_rel_ref.py checks the list)
ONE_ULP = ("loop1", "path5", "path6", "path12", "path21", "overlap", "same", "nan")
