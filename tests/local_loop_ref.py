"""The local mode of the deformation graph (cf_deform_*_local in csrc/cabi_deform.hip, DESIGN.md 4.14 "the local mode") as plain numpy:
what ElasticFusion's optimiseGraphSparse does with fernMatch == false and a lastDeformTime (Core/Utils/DeformationGraph.cpp:385-450
and every `enabled` test below it) plus the acceptance of Deformation::constrain for that call.  Written from that text, not copied.
Everything this file does not restate (nodes, edges, the window rule, the energy rows, the orders of operations) is tests/deform_ref.py.

SCOPE     The graph solver's half of local loop closure, and (at the end of the file) the constraint stage: the accept rule on the
          model-to-model tracker's result and the surface constraints.  The tracker's frame-side overload is held against the oracle
          (test_local_tracker_gpu.py) and the frame loop around these stages by its scenario (test_local_loop_closure_gpu.py); relative constraints, the pose graph and object models stay out as in the global mode.
SPLATS    Neither splat pass of local closure needs a statement of its own.  The inactive prediction is orc_combined_predict(time = 0,
          maxTime = tick - timeDelta, timeDelta).  ModelProjection::synthesizeDepth binds splat.vert with depth_splat.frag: the vertex
          stage, the disc test and the depth range are the colour splat's, so the acceptance rule is the same and the depth plane is the z
          channel of orc_combined_predict for the same arguments, 0 where nothing lands.
ENABLED   node i is enabled iff int(time_i) > last_deform_time.  (Node times never decrease, so the enabled nodes are a suffix.)
ROWS      The rows of deform_ref.rows, in the same order, with these dropped: the six rotation rows of a disabled node; the three rows
          of a directed edge j -> n when both j and n are disabled; the three rows of a constraint when none of the four nodes of its
          weight set is enabled (whether or not its weights are finite).  A row that stays keeps only its enabled columns; its residual
          is unchanged.  Dropped rows count neither in J nor in `error`.  mean_cons_error is the mean over ALL constraints
          (nonRelativeConstraintError does not look at `enabled`).
SYSTEM    A = J^T J, b = -J^T r over all 12 N unknowns; a disabled node's columns are absent from J, so its rows and columns of A and its
          part of b are zero.  Its diagonal block is then set to the identity: the factorisation sees exact zeros from the rest, and
          delta is exactly 0 there.  Band storage and bandwidth as in the global mode.  With every node enabled nothing is dropped and
          the system is deform_ref's.
OPTIMISE  No min_cons_error gate and no `error > 10` stop.  Not optimised (and nothing changes) when no node is enabled.  At most 3
          iterations, stopping after an iteration when error grew, |delta| < 1e-2, error < 1e-3 or |error - last| < 1e-5 * error.
          Accepted unless a step failed on a pivot <= 0; a failed call leaves the parameters it started from.
"""
import numpy as np

import deform_ref as ref

f32 = np.float32
BLOCK = ref.BLOCK
MAX_CONS_SIZED = 1536


def enabled(nodes, last_deform_time):
    return np.array([int(t) > int(last_deform_time) for t in np.asarray(nodes, f32)[:, 3]], bool)


def kept_rows(nodes, ids, n_cons, en):
    """bool per row of deform_ref.rows: True where the row stays"""
    n = len(nodes); E = ref.edges(n)
    keep = []
    for j in range(n):
        keep += [bool(en[j])] * 6
    for j in range(n):
        for nb in E[j]:
            keep += [bool(en[j] or en[nb])] * 3
    for l in range(n_cons):
        keep += [bool(en[ids[l]].any())] * 3
    return np.asarray(keep, bool)


def rows(nodes, params, cons_src, cons_dst, ids, w, ok, last_deform_time):
    """-> the kept rows [(enabled cols, vals f64)], their residuals f64, keep (bool per row of the global mode), en (bool per node)"""
    jr, r = ref.rows(nodes, params, cons_src, cons_dst, ids, w, ok)
    en = enabled(nodes, last_deform_time)
    keep = kept_rows(nodes, ids, len(cons_src), en)
    assert len(keep) == len(jr)
    out = []
    for k, (c, v) in enumerate(jr):
        if keep[k]:
            m = en[c // BLOCK]
            out.append((c[m], v[m]))
    return out, r[keep], keep, en


def with_identity(A, en):
    A = np.array(A, np.float64)
    for i in np.flatnonzero(~en):
        assert not A[BLOCK * i:BLOCK * i + BLOCK].any() and not A[:, BLOCK * i:BLOCK * i + BLOCK].any()
        A[BLOCK * i:BLOCK * i + BLOCK, BLOCK * i:BLOCK * i + BLOCK] = np.eye(BLOCK)
    return A


def dense_system(n_nodes, jr, r, en):
    """J, A (identity on the disabled diagonal blocks), b"""
    J, A, b = ref.dense_system(n_nodes, jr, r)
    return J, with_identity(A, en), b


def band_system(n_nodes, jr, r, en):
    """the same in band storage, accumulated row by row"""
    AB, b = ref.band_system(n_nodes, jr, r)
    off = np.repeat(~en, BLOCK)
    assert not AB[off].any() and not b[off].any()
    AB[off, 0] = 1.0
    return AB, b


def iterate(nodes, params, cons_src, cons_dst, ids, w, ok, last_deform_time):
    """one Gauss-Newton step over the enabled unknowns -> dict(params, delta, error, delta_norm, failed)"""
    n = len(nodes)
    jr, r, _, en = rows(nodes, params, cons_src, cons_dst, ids, w, ok, last_deform_time)
    _, A, b = ref.dense_system(n, jr, r)
    on = np.repeat(en, BLOCK)
    delta = np.zeros(BLOCK * n)
    if on.any():
        try:
            Lc = np.linalg.cholesky(A[np.ix_(on, on)])
        except np.linalg.LinAlgError:
            return dict(params=np.array(params, f32), failed=True)
        delta[on] = ref._tri(Lc, b[on])
    new = (np.asarray(params, f32).astype(np.float64).reshape(-1) + delta).astype(f32).reshape(-1, 12)
    _, r2, _, _ = rows(nodes, new, cons_src, cons_dst, ids, w, ok, last_deform_time)
    return dict(params=new, delta=delta, error=ref.error_of(r2), delta_norm=float(np.sqrt(np.sum(delta * delta))), failed=False)


def optimise(nodes, cons_src, cons_dst, cons_src_time, last_deform_time, th=None, trace=None, params=None):
    """optimiseGraphSparse(fernMatch = false, lastDeformTime) + Deformation::constrain's acceptance of it.  trace (a list) receives every
    compared (value, threshold) pair of the stop rules."""
    th = dict(ref.DEFAULTS, **(th or {}))
    nodes = np.asarray(nodes, f32); n = len(nodes)
    cons_src = np.asarray(cons_src, f32).reshape(-1, 3); cons_dst = np.asarray(cons_dst, f32).reshape(-1, 3)
    note = (lambda v, t: trace.append((float(v), float(t)))) if trace is not None else (lambda v, t: None)
    params = ref.identity_params(n) if params is None else np.array(params, f32)
    start = params
    if len(cons_src):
        ids, w, ok = ref.weights(nodes, cons_src, cons_src_time)
    else:
        ids, w, ok = np.zeros((0, 4), np.int32), np.zeros((0, 4), f32), np.zeros(0, bool)
    en = enabled(nodes, last_deform_time)
    out = dict(optimised=False, accepted=False, failed=False, iterations=0, params=params, ids=ids, w=w, ok=ok, enabled=int(en.sum()))
    mean0 = ref.cons_error(nodes, params, cons_src, cons_dst, ids, w, ok)
    _, r0, _, _ = rows(nodes, params, cons_src, cons_dst, ids, w, ok, last_deform_time)
    out.update(error_before=ref.error_of(r0), mean_cons_error_before=mean0, error=ref.error_of(r0), mean_cons_error=mean0)
    if not en.any():
        return out
    out["optimised"] = True
    last = float(out["error"])
    it = 0
    while it < th["max_iterations"]:
        it += 1
        step = iterate(nodes, params, cons_src, cons_dst, ids, w, ok, last_deform_time)
        if step["failed"]:
            out.update(failed=True, iterations=it, params=start)
            return out
        params = step["params"]; err = step["error"]; out.update(params=params, error=err, iterations=it)
        note(err, last); note(step["delta_norm"], th["min_delta"]); note(err, th["min_error"])
        note(abs(float(err) - last), th["min_change"] * float(err))
        if (float(err) > last or step["delta_norm"] < th["min_delta"] or float(err) < th["min_error"]
                or abs(float(err) - last) < th["min_change"] * float(err)):
            break
        last = float(err)
    out["mean_cons_error"] = ref.cons_error(nodes, params, cons_src, cons_dst, ids, w, ok)
    out["accepted"] = True
    return out


# ------------------------------------------------------------------------------------------------ the constraint stage
# CONSTRAINTS  (csrc/local_loop.hip; CoFusion.cpp:407-443.)  Accept: every diagonal entry of inverse(lastA) <= f64(covThresh) -- the
#           partial-pivot LU inverse in f64 in the order of orc_covariance / cf_odom_get_covariance; a NaN rejects (the reference's
#           `covar > covThresh -> reject` lets a NaN pass: a stated departure) -- and icp_count > f32(icpCountThresh) and icp_error <
#           icpErrThresh, all strict as written.  Accepted: vertex and old-time maps are reduced by 20, nearest, at source texel
#           (20 x + 10, 20 y + 10), W // 20 by H // 20 samples; visited column by column (x outer, y inner); valid when z > 0 and
#           z < maxDepth and oldTime > 0; src = currPose * p, dst = estPose * p, each coordinate ((m0 x + m1 y) + m2 z) + m3 in f32
#           (ElasticFusion's rule; the reference's text forms both with currPose); srcTime = tick; with pin the row (dst, dst, oldTime)
#           follows each constraint.
CONS_SAMPLE = 20
LOCAL_DEFAULTS = dict(cov_thresh=1e-5, icp_count_thresh=40000, icp_err_thresh=5e-5)


def covariance(lastA):
    """inverse(lastA) by partial-pivot LU, f64, the operations of orc_covariance in its order"""
    lu = np.array(lastA, np.float64).reshape(6, 6).copy()
    perm = list(range(6))
    with np.errstate(all="ignore"):
        for k in range(6):
            piv, big = k, abs(lu[k, k])
            for r in range(k + 1, 6):
                if abs(lu[r, k]) > big:
                    big, piv = abs(lu[r, k]), r
            if piv != k:
                lu[[k, piv]] = lu[[piv, k]]
                perm[k], perm[piv] = perm[piv], perm[k]
            if big != 0.0:
                for r in range(k + 1, 6):
                    lu[r, k] = lu[r, k] / lu[k, k]
            for r in range(k + 1, 6):
                for c in range(k + 1, 6):
                    lu[r, c] = lu[r, c] - lu[r, k] * lu[k, c]
        cov = np.zeros((6, 6))
        for j in range(6):
            x = np.array([1.0 if perm[i] == j else 0.0 for i in range(6)])
            for i in range(6):
                for c in range(i):
                    x[i] = x[i] - lu[i, c] * x[c]
            for i in range(5, -1, -1):
                for c in range(i + 1, 6):
                    x[i] = x[i] - lu[i, c] * x[c]
                x[i] = x[i] / lu[i, i]
            cov[:, j] = x
    return cov


def _mul_pose(m, p):
    m = np.asarray(m, f32).reshape(4, 4); x, y, z = f32(p[0]), f32(p[1]), f32(p[2])
    return np.array([f32(f32(f32(f32(m[r, 0] * x) + f32(m[r, 1] * y)) + f32(m[r, 2] * z)) + m[r, 3]) for r in range(3)], f32)


def local_constraints(track, vertex, old_time, curr_pose, tick, max_depth, pin, th=None):
    """track: dict(rot 3x3, trans 3, icp_error, icp_count, lastA 6x6); vertex f32 [H, W, 4]; old_time u16 [H, W]
    -> dict(accepted, max_covariance, est_pose, n, src [n, 3], dst [n, 3], time [n])"""
    th = dict(LOCAL_DEFAULTS, **(th or {}))
    diag = np.diagonal(covariance(track["lastA"]))
    cov_ok = all(bool(d <= np.float64(f32(th["cov_thresh"]))) for d in diag)
    worst = np.nan if np.isnan(diag).any() else float(diag.max())
    accepted = bool(cov_ok and f32(track["icp_count"]) > f32(th["icp_count_thresh"]) and f32(track["icp_error"]) < f32(th["icp_err_thresh"]))
    est = np.eye(4, dtype=f32); est[:3, :3] = np.asarray(track["rot"], f32).reshape(3, 3); est[:3, 3] = np.asarray(track["trans"], f32)
    src, dst, tm = [], [], []
    if accepted:
        h, w = old_time.shape
        for i in range(w // CONS_SAMPLE):
            for j in range(h // CONS_SAMPLE):
                p = vertex[CONS_SAMPLE * j + CONS_SAMPLE // 2, CONS_SAMPLE * i + CONS_SAMPLE // 2]
                t = int(old_time[CONS_SAMPLE * j + CONS_SAMPLE // 2, CONS_SAMPLE * i + CONS_SAMPLE // 2])
                if p[2] > 0 and p[2] < f32(max_depth) and t > 0:
                    a, b = _mul_pose(curr_pose, p), _mul_pose(est, p)
                    src.append(a); dst.append(b); tm.append(f32(tick))
                    if pin:
                        src.append(b); dst.append(b); tm.append(f32(t))
    arr = lambda x, c: np.asarray(x, f32).reshape(-1, c) if c > 1 else np.asarray(x, f32).reshape(-1)
    return dict(accepted=accepted, max_covariance=worst, est_pose=est, n=len(tm), src=arr(src, 3), dst=arr(dst, 3), time=arr(tm, 1))
