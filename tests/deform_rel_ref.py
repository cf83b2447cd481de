"""Relative constraints of the deformation graph (csrc/deform.hip) as plain numpy, on top of tests/deform_ref.py:
the statement the GPU tests compare with.  Written from the text of ElasticFusion's loop closure as the reference carries it
(CoFusion.cpp:373, 445-458; Deformation.cpp:104-126, 139-149; DeformationGraph.cpp:578-654, 790-810, 881-893), not copied from it.

PICK     An accepted local closure leaves pairs behind.  Of its n non-pin constraints, in buffer order, the indices 0, s, 2s, ... < n with
         s = max(1, n // 3) are kept (the reference steps by n / 3, which never ends for n < 3: the max is a stated departure).  A kept pair
         is (phi(src), dst, srcTime, dstTime): phi is the accepted graph applied by the map rule (the window weights of src at srcTime,
         MOVE; in the graph's local mode a point none of whose four nodes is enabled keeps its bits, as a surfel does), dstTime the old-time
         texel of the constraint.
STORE    A ring of R = 128 pairs in slot order: append number k (from 0) lands in slot k mod R, the newest overwrites the oldest (the
         reference's list grows without bound).  Pairs are world points and are NOT moved by later deformations, as in the reference: a
         pair left before a global closure describes the map of its own time.  "Store order" below is slot order.
WEIGHTS  The one window-and-weights rule of deform_ref, applied to src at srcTime and to tgt at dstTime.
ROWS     Global mode only (every node enabled).  After the absolute constraint rows, three rows per pair in store order.  The source set's
         entries are an absolute row's, the target set's the same negated: for component c and a node of offset o = 12 id with
         e = ((p - g) * w) * 10 and w * 10 formed in f32 and widened, columns o + c, o + 3 + c, o + 6 + c (e.x, e.y, e.z) and o + 9 + c.
         The entries do not depend on c.  A node in both sets gets f64(source entry) + (-f64(target entry)).  Compact form per pair: eight
         node slots -- the source set (ids ascending), then the nodes of the target set that are not in it (ascending), then -1 -- of
         four values each.  The residual is f32(phi(src)_c - phi(tgt)_c) * 10 (widened before the product), phi by the CURRENT parameters
         with each point's own weights.  A pair one of whose weight sets is NaN keeps its rows empty and its residual present (a point with
         a NaN set does not move), the rule rows() has for ok == False.
ERRORS   error sums the relative rows too.  mean_cons_error is nonRelativeConstraintError literally: the numerator runs over the absolute
         constraints, the denominator counts ALL constraints, relative ones included.  This lowers the value the 0.06 gate and the 3e-4
         accept rule see; it is the reference's behaviour.
SYSTEM   A = B + U^T U, b = b_B - U^T r_rel with B, b_B the band system of the other rows and U the m = 3 n_rel relative rows;
         U^T r_rel is summed in row order from 0, then subtracted.
SOLVE    One direct method on the band factor: L L^T = B, y = L^-1 b, Y = L^-1 U^T, C = I + Y^T Y = Lc Lc^T, t = C^-1 (Y^T y),
         delta = L^-T (y - Y t).  A pivot <= 0 of B or of C fails the step and leaves the parameters.  Plain f64 here (numpy's products);
         the device forms C and Y^T y with compensated sums, because y - Y t cancels as many digits as Y^T Y is large.
LOCAL    Relative pairs are refused in the graph's local mode (the reference only ever gives them to the global graph).
"""
import numpy as np

import deform_ref as ref

f32 = np.float32
RING = 128
SLOTS = 8


# ------------------------------------------------------------------------------------------------ pick and store
def pick_indices(n):
    s = max(1, n // 3)
    return list(range(0, n, s))


def pick(nodes, params, src, dst, src_time, dst_time, last_deform_time=None):
    """the pairs an accepted closure (graph nodes / params) leaves: -> [k, 8] f32 rows (phi(src) xyz, srcTime, dst xyz, dstTime)"""
    nodes = np.asarray(nodes, f32)
    src = np.asarray(src, f32).reshape(-1, 3); dst = np.asarray(dst, f32).reshape(-1, 3)
    idx = pick_indices(len(src))
    if not idx:
        return np.zeros((0, 8), f32)
    p = src[idx]; ts = np.asarray(src_time, f32)[idx]
    ids, w, ok = ref.weights(nodes, p, ts)
    if last_deform_time is not None and last_deform_time >= 0:
        ok = ok & (nodes[ids, 3].astype(np.int64) > last_deform_time).any(axis=1)
    moved = ref.move_points(nodes, params, p, ids, w, ok)
    return np.concatenate([moved, ts[:, None], dst[idx], np.asarray(dst_time, f32)[idx][:, None]], 1).astype(f32)


def target_times(vertex, old_time, max_depth, sample=20):
    """the old time of every constraint an accepted registration makes, in constraint order (pin rows not counted): the maps are sampled
    at texel (20 x + 10, 20 y + 10), column by column (x outer), a sample is valid when z > 0, z < max_depth and its old time > 0
    (local_loop_ref.local_constraints, whose pin rows carry the same values as their time) -> f32 [n]"""
    h, w = old_time.shape
    out = []
    for i in range(w // sample):
        for j in range(h // sample):
            p = vertex[sample * j + sample // 2, sample * i + sample // 2]
            t = int(old_time[sample * j + sample // 2, sample * i + sample // 2])
            if p[2] > 0 and p[2] < f32(max_depth) and t > 0:
                out.append(f32(t))
    return np.asarray(out, f32)


def closure_pairs(src, dst, time, dst_time, pinned, nodes, params, last_deform_time):
    """the pairs an accepted local closure leaves, from its constraint ROWS as the constraint stage writes them (pinned: rows 2 k are the
    constraints, rows 2 k + 1 their pins) and its target times (one per constraint)"""
    step = 2 if pinned else 1
    return pick(nodes, params, np.asarray(src, f32)[::step], np.asarray(dst, f32)[::step], np.asarray(time, f32)[::step], dst_time, last_deform_time)


class Ring:
    """the store: slots [capacity, 8], appended pairs land at total mod capacity"""

    def __init__(self, capacity=RING):
        self.slots = np.zeros((capacity, 8), f32)
        self.total = 0

    def append(self, pairs):
        for row in np.asarray(pairs, f32).reshape(-1, 8):
            self.slots[self.total % len(self.slots)] = row
            self.total += 1

    @property
    def count(self):
        return min(self.total, len(self.slots))

    @property
    def overwritten(self):
        return self.total - self.count

    def pairs(self):
        return self.slots[:self.count].copy()


# ------------------------------------------------------------------------------------------------ weights and rows
def rel_weights(nodes, pairs):
    """-> (ids, w, ok) of the sources, (ids, w, ok) of the targets"""
    pairs = np.asarray(pairs, f32).reshape(-1, 8)
    if not len(pairs):
        e = (np.zeros((0, 4), np.int32), np.zeros((0, 4), f32), np.zeros(0, bool))
        return e, e
    return ref.weights(nodes, pairs[:, 0:3], pairs[:, 3]), ref.weights(nodes, pairs[:, 4:7], pairs[:, 7])


def compact_rows(nodes, pairs, ws, wt):
    """U in compact form: slot ids int32 [n, 8] (-1: unused), values f64 [n, 8, 4]"""
    nodes = np.asarray(nodes, f32); pairs = np.asarray(pairs, f32).reshape(-1, 8)
    n = len(pairs)
    uid = np.full((n, SLOTS), -1, np.int32); uval = np.zeros((n, SLOTS, 4))
    sc = ref.SQRT_CON
    for p in range(n):
        if not (ws[2][p] and wt[2][p]):
            continue
        used = 0
        for (ids, w, _), pt, sign in ((ws, pairs[p, 0:3], 1.0), (wt, pairs[p, 4:7], -1.0)):
            for k in range(ref.K):
                i = int(ids[p, k])
                d = (pt - nodes[i, :3]) * w[p, k]
                e = np.array([float(f32(d[0] * sc)), float(f32(d[1] * sc)), float(f32(d[2] * sc)), float(f32(w[p, k] * sc))])
                if sign < 0:
                    e = -e
                at = [s for s in range(used) if uid[p, s] == i]
                if at:
                    uval[p, at[0]] = uval[p, at[0]] + e
                else:
                    uid[p, used] = i; uval[p, used] = e; used += 1
    return uid, uval


def rel_residual(nodes, params, pairs, ws, wt):
    """f64 [3 n]: f32(phi(src) - phi(tgt)) * 10"""
    pairs = np.asarray(pairs, f32).reshape(-1, 8)
    if not len(pairs):
        return np.zeros(0)
    a = ref.move_points(nodes, params, pairs[:, 0:3], *ws)
    b = ref.move_points(nodes, params, pairs[:, 4:7], *wt)
    return ((a - b).astype(f32).astype(np.float64) * float(ref.SQRT_CON)).reshape(-1)


def gap(nodes, params, pairs, ws, wt):
    """|phi(src) - phi(tgt)| per pair, f64 of the f32 moved points: the property relative rows exist for"""
    pairs = np.asarray(pairs, f32).reshape(-1, 8)
    a = ref.move_points(nodes, params, pairs[:, 0:3], *ws).astype(np.float64)
    b = ref.move_points(nodes, params, pairs[:, 4:7], *wt).astype(np.float64)
    return np.sqrt(((a - b) ** 2).sum(1))


def sparse_rows(uid, uval):
    """the 3 n rows of U as (cols, vals), the form of deform_ref.rows"""
    out = []
    for p in range(len(uid)):
        for c in range(3):
            cols, vals = [], []
            for s in range(SLOTS):
                if uid[p, s] >= 0:
                    o = ref.BLOCK * int(uid[p, s])
                    cols += [o + c, o + 3 + c, o + 6 + c, o + 9 + c]; vals += list(uval[p, s])
            out.append((np.asarray(cols, np.int64), np.asarray(vals, np.float64)))
    return out


def dense_rows(n_nodes, uid, uval):
    U = np.zeros((3 * len(uid), ref.BLOCK * n_nodes))
    for i, (c, v) in enumerate(sparse_rows(uid, uval)):
        U[i, c] = v
    return U


def rel_rhs(b_band, U, r_rel):
    """b = b_B - U^T r_rel, the sum over the rows in row order from 0"""
    t = np.zeros(U.shape[1])
    for k in range(len(U)):
        t = t + U[k] * r_rel[k]
    return b_band - t


def rhs_bounds(n_nodes, jrows, r):
    """per entry of b: (number of summands, sum of |terms|) over all rows, relative ones included -- deform_ref.sum_bounds' half for b
    (its half for A assumes rows inside the band)"""
    n = ref.BLOCK * n_nodes
    mb = np.zeros(n, np.int64); sb = np.zeros(n)
    for (c, v), ri in zip(jrows, r):
        np.add.at(mb, c, 1); np.add.at(sb, c, np.abs(v * ri))
    return mb, sb


def mean_cons_error(nodes, params, cons_src, cons_dst, ids, w, ok, n_rel):
    """numerator over the absolute constraints, denominator over all"""
    total = len(cons_src) + n_rel
    if not total:
        return f32(np.nan)
    s = f32(0)
    if len(cons_src):
        d = ref.move_points(nodes, params, cons_src, ids, w, ok) - np.asarray(cons_dst, f32)
        for v in np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]):
            s = f32(s + v)
    return f32(s / f32(total))


# ------------------------------------------------------------------------------------------------ system and solve
def system(nodes, params, cons_src, cons_dst, ids, w, ok, pairs, ws, wt):
    """-> dict(jr, r (absolute rows), uid, uval, U, r_rel, B, b_B (dense f64), b, A)"""
    n = len(nodes)
    jr, r = ref.rows(nodes, params, cons_src, cons_dst, ids, w, ok)
    _, B, bB = ref.dense_system(n, jr, r)
    uid, uval = compact_rows(nodes, pairs, ws, wt)
    U = dense_rows(n, uid, uval)
    rr = rel_residual(nodes, params, pairs, ws, wt)
    return dict(jr=jr, r=r, uid=uid, uval=uval, U=U, r_rel=rr, B=B, b_B=bB, b=rel_rhs(bB, U, rr), A=B + U.T @ U)


def _forward(L, rhs):
    """L^-1 rhs with a band factor in deform_ref's storage, row order (rhs [n] or [n, k])"""
    n, bw = L.shape
    y = np.array(rhs, np.float64)
    for i in range(n):
        m = min(bw - 1, i)
        if m:
            y[i] = y[i] - L[i, 1:m + 1] @ y[i - 1::-1][:m]
        y[i] = y[i] / L[i, 0]
    return y


def _backward(L, rhs):
    n, bw = L.shape
    y = np.array(rhs, np.float64)
    for i in range(n - 1, -1, -1):
        y[i] /= L[i, 0]
        m = min(bw - 1, i)
        if m:
            y[i - m:i] -= L[i, m:0:-1] * y[i]
    return y


def solve(B_band, U, b):
    """the stated direct method in f64 -> (delta, C) or (None, None) at a pivot <= 0"""
    L = ref.band_cholesky(B_band)
    if L is None:
        return None, None
    y = _forward(L, b)
    if not len(U):
        return _backward(L, y), np.zeros((0, 0))
    Y = _forward(L, U.T)
    C = np.eye(len(U)) + Y.T @ Y
    try:
        Lc = np.linalg.cholesky(C)
    except np.linalg.LinAlgError:
        return None, None
    t = ref._tri(Lc, Y.T @ y)
    return _backward(L, y - Y @ t), C


def solve_star(A, b):
    """the extended-precision solution of the FULL system (A dense, not banded): longdouble Cholesky with refinement against residuals
    formed in longdouble from the f64 entries until the correction no longer changes x"""
    A = np.asarray(A, np.float64); n = len(A)
    Al = A.astype(np.longdouble); bl = np.asarray(b, np.float64).astype(np.longdouble)
    L = np.zeros((n, n), np.longdouble)
    for j in range(n):
        L[j, j] = np.sqrt(Al[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < n:
            L[j + 1:, j] = (Al[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]

    def sol(rhs):
        y = np.array(rhs, np.longdouble)
        for i in range(n):
            y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
        for i in range(n - 1, -1, -1):
            y[i] = (y[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
        return y
    x = sol(bl)
    for _ in range(40):
        x2 = x + sol(bl - Al @ x)
        if np.array_equal(x2, x):
            break
        x = x2
    return x


def solve_star_band(AB, U, b):
    """the same for a system too large to hold densely (1024 nodes): x in longdouble, refined until the correction no longer changes it
    against residuals b - B x - U^T (U x) formed in longdouble; the corrections come from an f64 solve of the full system (band factor of
    deform_ref.band_factor, the rows of U eliminated by their Schur complement)"""
    n, bw = AB.shape
    solve_b = ref.band_factor(AB)
    Yb = np.column_stack([solve_b(U[k]) for k in range(len(U))]) if len(U) else np.zeros((n, 0))
    S = np.linalg.cholesky(np.eye(len(U)) + U @ Yb)

    def sol(rhs):
        z = solve_b(np.asarray(rhs, np.float64))
        return z - Yb @ ref._tri(S, U @ z) if len(U) else z
    full = np.zeros((n, 2 * bw - 1), np.longdouble)
    for d in range(min(bw, n)):
        full[d:, bw - 1 - d] = AB[d:, d]
        full[:n - d, bw - 1 + d] = AB[d:, d]
    cols = np.arange(n)[:, None] - (bw - 1) + np.arange(2 * bw - 1)[None, :]
    inside = (cols >= 0) & (cols < n)
    cols = np.clip(cols, 0, n - 1)
    Ul = U.astype(np.longdouble); bl = np.asarray(b, np.float64).astype(np.longdouble)
    x = np.asarray(sol(b), np.longdouble)
    for _ in range(40):
        r = bl - (full * np.where(inside, x[cols], 0)).sum(1) - Ul.T @ (Ul @ x)
        x2 = x + np.asarray(sol(r.astype(np.float64)), np.longdouble)
        if np.array_equal(x2, x):
            break
        x = x2
    return x


def error_of(r, r_rel):
    return ref.error_of(np.concatenate([r, r_rel]))


def iterate(nodes, params, cons_src, cons_dst, ids, w, ok, pairs, ws, wt, method="direct"):
    """one Gauss-Newton step.  method "direct": the stated solve; "dense": numpy's Cholesky of A (the yardstick of e)"""
    s = system(nodes, params, cons_src, cons_dst, ids, w, ok, pairs, ws, wt)
    if method == "direct":
        delta, _ = solve(ref.to_band(s["B"]), s["U"], s["b"])
        if delta is None:
            return dict(params=np.array(params, f32), failed=True, sys=s)
    else:
        delta = ref._tri(np.linalg.cholesky(s["A"]), s["b"])
    new = (np.asarray(params, f32).astype(np.float64).reshape(-1) + delta).astype(f32).reshape(-1, 12)
    _, r2 = ref.rows(nodes, new, cons_src, cons_dst, ids, w, ok)
    return dict(params=new, delta=delta, error=error_of(r2, rel_residual(nodes, new, pairs, ws, wt)),
                delta_norm=float(np.sqrt(np.sum(delta * delta))), failed=False, sys=s)


def optimise(nodes, cons_src, cons_dst, cons_src_time, pairs, th=None, trace=None):
    """deform_ref.optimise with the relative rows of `pairs` in every step and the stated mean constraint error"""
    th = dict(ref.DEFAULTS, **(th or {}))
    nodes = np.asarray(nodes, f32); n = len(nodes)
    cons_src = np.asarray(cons_src, f32).reshape(-1, 3); cons_dst = np.asarray(cons_dst, f32).reshape(-1, 3)
    pairs = np.asarray(pairs, f32).reshape(-1, 8)
    note = (lambda v, t: trace.append((float(v), float(t)))) if trace is not None else (lambda v, t: None)
    params = ref.identity_params(n)
    ids, w, ok = ref.weights(nodes, cons_src, cons_src_time) if len(cons_src) else (np.zeros((0, 4), np.int32), np.zeros((0, 4), f32), np.zeros(0, bool))
    ws, wt = rel_weights(nodes, pairs)
    mean = lambda P: mean_cons_error(nodes, P, cons_src, cons_dst, ids, w, ok, len(pairs))
    err = lambda P: error_of(ref.rows(nodes, P, cons_src, cons_dst, ids, w, ok)[1], rel_residual(nodes, P, pairs, ws, wt))
    out = dict(optimised=False, accepted=False, failed=False, iterations=0, params=params, ids=ids, w=w, ok=ok, ws=ws, wt=wt)
    mean0 = mean(params); e0 = err(params)
    out.update(error_before=e0, mean_cons_error_before=mean0, error=e0, mean_cons_error=mean0)
    note(mean0, th["min_cons_error"])
    if not (mean0 >= f32(th["min_cons_error"])):
        return out
    out["optimised"] = True
    last = float(e0)
    it = 0
    while it < th["max_iterations"]:
        it += 1
        step = iterate(nodes, params, cons_src, cons_dst, ids, w, ok, pairs, ws, wt)
        if step["failed"]:
            out.update(failed=True, iterations=it)
            return out
        params = step["params"]; e = step["error"]; out.update(params=params, error=e, iterations=it)
        note(e, last); note(step["delta_norm"], th["min_delta"]); note(e, th["min_error"])
        note(abs(float(e) - last), th["min_change"] * float(e))
        if it == 1:
            note(e, th["max_first_error"])
        if (float(e) > last or step["delta_norm"] < th["min_delta"] or float(e) < th["min_error"]
                or abs(float(e) - last) < th["min_change"] * float(e) or (it == 1 and float(e) > th["max_first_error"])):
            break
        last = float(e)
    mean1 = mean(params)
    out["mean_cons_error"] = mean1
    note(mean1, th["accept_cons_error"]); note(out["error"], th["accept_error"])
    out["accepted"] = bool(mean1 < f32(th["accept_cons_error"]) and out["error"] < f32(th["accept_error"]))
    return out
