"""The deformation-graph map correction (csrc/deform.hip) as plain numpy: the statement the GPU tests compare with.

Written from the text of ElasticFusion's loop closure as the reference carries it (Core/Model/Deformation.*, Core/Utils/DeformationGraph.*,
the node branch of Core/Shaders/copy_unstable.vert, sample.geom), not copied from it.  Conventions, each of which the kernels follow:

SCOPE    Global closure of one map from absolute constraints (fernMatch == true).  No local closure, no relative constraints, no
         lastDeformTime (every node is enabled), no pose graph.
SURFEL   12 f32: x y z conf | colour _ init_time last_time | nx ny nz radius.
NODES    Every surfel whose buffer index is a multiple of `stride` is a node (x, y, z, init_time), in buffer order.  stride = the smallest
         multiple of sample_rate with ceil(S / stride) <= 1024.  Fewer than K + 1 = 5 nodes: no graph.  Node times must be non-decreasing
         (`monotone`); equal times on neighbouring nodes are normal.
PARAMS   12 f32 per node: the 3x3 "rotation" column-major (R(r, c) at 3 c + r), then the translation.  Identity / zero at the start.
EDGES    connectGraphSeq with K = 4: nodes 0, 1 -> every other node of 0..4; the last two -> every other node of the last five; node i
         between them -> i-1, i+1, i-2, i+2, in that order.  Four directed edges per node.
WINDOW   ONE rule for constraint points, map surfels and keyframe poses (the reference's host code and its shader differ; a solve that
         models one window while the map moves by another is not copied).  For a point p of integer time t = int(time) over node times
         T[i] = int(node.w):
           imin = 0, imax = N-1, imid = (imin+imax)/2; while imax >= imin: imid = (imin+imax)/2; T[imid] < t: imin = imid+1;
           T[imid] > t: imax = imid-1; else stop.  Then imin = min(imin, N-1), imax = max(imax, 0) (the reference reads T[-1] there).
           found = imin if |T[imin]-t| <= |T[imid]-t| and <= |T[imax]-t|; else imid if |T[imid]-t| <= both others; else imax.
           Candidates: found, found-1, ... (at most 10, stopping at node 0), then found+1, found+2, ... until 20 in all or node N-1.
         d_j = sqrt((dx*dx + dy*dy) + dz*dz) with dx = p.x - g.x ..., all f32, no FMA, IEEE sqrt.  The candidates are ordered by d
         ascending, ties in candidate order; dMax = the 5th distance; w_j = (1 - d_j / dMax)^2 (x * x) for the first four,
         s = ((w0 + w1) + w2) + w3, w_j / s.  The four (id, w) are then sorted by id ascending.  If any of the four weights is not finite
         (dMax == 0, or all five distances equal) the point is left unchanged everywhere.
MOVE     v_k = (R(r,0)*dx + R(r,1)*dy) + R(r,2)*dz, + g_r, + t_r per component with d = p - g_k; p' = sum over the four nodes in id order of
         acc = acc + w_k * v_k from acc = 0.  Normal: C = cofactors of R (C00 = R11*R22 - R12*R21, ...), det = (R00*C00 + R01*C01) + R02*C02,
         M = C / det entry by entry, m_r = (M(r,0)*nx + M(r,1)*ny) + M(r,2)*nz, acc = acc + w_k * m_r; n' = acc / sqrt((x*x + y*y) + z*z).
STAMP    After the move, last_time = tick when conf > threshold and, with l = T_inv * (p', 1) (row-wise, left to right),
         x = ((fx*l.x)/l.z) + cx, y = ((fy*l.y)/l.z) + cy: l.z > 0, l.z < max_depth, x > 0, y > 0, x < cols, y < rows, d = depth[floor(y)][floor(x)]
         > 0 and l.z < d + 0.1.  (The reference samples its own prediction texture; here the frame's filtered depth.)
ENERGY   Rows in this order: E_rot, six per node (col0.col1, col0.col2, col1.col2, |col0|^2 - 1, |col1|^2 - 1, |col2|^2 - 1; weight 1);
         E_reg, three per directed edge j -> n in node then edge order: (R_j (g_n - g_j) + g_j + t_j) - (g_n + t_n), times sqrt(10) as f32;
         E_con, three per constraint: (moved source - target) times 10.  Residual values are formed in f32 and widened; the weight is
         multiplied in f64.  Jacobian entries are formed in f32 (weight included) and widened.  A = J^T J, b = -J^T r and the solve in f64;
         the update is f32(f64(param) + delta).  error = f32(sum r^2), mean_cons_error = f32 mean over ALL constraints of |moved - target|.
BAND     A couples nodes at most 19 apart: half-bandwidth 239 scalars.  Band Cholesky without pivoting; a pivot <= 0 fails the step.
OPTIMISE not optimised when mean_cons_error < 0.06; else at most 3 iterations, stopping after an iteration when error grew, |delta| < 1e-2,
         error < 1e-3, |error - last| < 1e-5 * error, or (first iteration) error > 10.  Accepted: mean_cons_error < 3e-4 and error < 0.12.
POSES    A keyframe pose moves by the same window rule at its translation and time; its 3x3 becomes the orthogonal polar factor of
         (sum w_k R_k) * P33, by Newton's iteration X <- (X + X^-T) / 2 in f64 to a fixed point or 20 steps.
"""
import math

import numpy as np

f32 = np.float32
K = 4
LOOK = 20
MAX_NODES = 1024
MAX_CONS = 128
BLOCK = 12
HALF_BLOCKS = 19
HALF_BAND = HALF_BLOCKS * BLOCK + BLOCK - 1     # 239
SQRT_REG = f32(np.sqrt(f32(10.0)))
SQRT_CON = f32(10.0)
DEFAULTS = dict(min_cons_error=0.06, max_iterations=3, min_delta=1e-2, min_error=1e-3, min_change=1e-5, max_first_error=10.0,
                accept_cons_error=3e-4, accept_error=0.12)


# ------------------------------------------------------------------------------------------------ nodes, edges
def stride_for(n_surfels, sample_rate):
    m = 1
    while -(-n_surfels // (m * sample_rate)) > MAX_NODES:
        m += 1
    return m * sample_rate


def sample(surfels, sample_rate):
    """-> nodes f32 [N, 4], stride, monotone"""
    surfels = np.asarray(surfels, f32).reshape(-1, 12)
    stride = stride_for(len(surfels), sample_rate)
    pick = surfels[::stride]
    nodes = np.concatenate([pick[:, 0:3], pick[:, 6:7]], axis=1).astype(f32)
    t = nodes[:, 3]
    return nodes, stride, bool(np.all(t[1:] >= t[:-1]))


def edges(n):
    """int32 [n, 4]: the neighbours of every node, in connectGraphSeq's order"""
    assert n >= K + 1
    out = np.zeros((n, K), np.int32)
    for i in range(n):
        if i < K // 2:
            out[i] = [m for m in range(K + 1) if m != i]
        elif i < n - K // 2:
            out[i] = [i - 1, i + 1, i - 2, i + 2]
        else:
            out[i] = [m for m in range(n - (K + 1), n) if m != i]
    return out


def identity_params(n):
    p = np.zeros((n, 12), f32)
    p[:, 0] = p[:, 4] = p[:, 8] = 1
    return p


# ------------------------------------------------------------------------------------------------ window and weights
def window(times, t):
    """times: int node times; -> (found, candidates in candidate order)"""
    n = len(times)
    imin, imax = 0, n - 1
    imid = (imin + imax) // 2
    while imax >= imin:
        imid = (imin + imax) // 2
        if times[imid] < t:
            imin = imid + 1
        elif times[imid] > t:
            imax = imid - 1
        else:
            break
    imin = min(imin, n - 1)
    imax = max(imax, 0)
    a, b, c = abs(times[imin] - t), abs(times[imid] - t), abs(times[imax] - t)
    if a <= b and a <= c:
        found = imin
    elif b <= a and b <= c:
        found = imid
    else:
        found = imax
    cand = list(range(found, max(found - LOOK // 2, -1), -1))
    j = found + 1
    while len(cand) < LOOK and j < n:
        cand.append(j)
        j += 1
    return found, cand


def weights(nodes, points, times, with_dists=False):
    """-> ids int32 [M, 4] ascending, w f32 [M, 4], ok bool [M]"""
    nodes = np.asarray(nodes, f32); points = np.asarray(points, f32).reshape(-1, 3)
    node_t = [int(x) for x in nodes[:, 3]]
    m = len(points)
    cand = np.full((m, LOOK), -1, np.int64)
    for v in range(m):
        _, c = window(node_t, int(times[v]))
        cand[v, :len(c)] = c
    g = nodes[np.maximum(cand, 0), :3]
    d = points[:, None, :] - g
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(f32)
    dist[cand < 0] = np.inf
    order = np.argsort(dist, axis=1, kind="stable")
    ids = np.take_along_axis(cand, order, 1)[:, :K + 1]
    ds = np.take_along_axis(dist, order, 1)[:, :K + 1]
    with np.errstate(all="ignore"):
        q = f32(1) - ds[:, :K] / ds[:, K:K + 1]
        w = q * q
        s = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        w = (w / s[:, None]).astype(f32)
    ok = np.isfinite(w).all(axis=1)
    o2 = np.argsort(ids[:, :K], axis=1, kind="stable")
    out = np.take_along_axis(ids[:, :K], o2, 1).astype(np.int32), np.take_along_axis(w, o2, 1), ok
    return out + (ds,) if with_dists else out


# ------------------------------------------------------------------------------------------------ moving points
def _R(params, r, c):
    return params[..., 3 * c + r]


def move_points(nodes, params, points, ids, w, ok):
    nodes = np.asarray(nodes, f32); params = np.asarray(params, f32); points = np.asarray(points, f32).reshape(-1, 3)
    acc = np.zeros_like(points)
    for k in range(K):
        g = nodes[ids[:, k], :3]; P = params[ids[:, k]]
        d = points - g
        for r in range(3):
            v = (_R(P, r, 0) * d[:, 0] + _R(P, r, 1) * d[:, 1]) + _R(P, r, 2) * d[:, 2]
            v = v + g[:, r]
            v = v + P[:, 9 + r]
            acc[:, r] = acc[:, r] + w[:, k] * v
    return np.where(ok[:, None], acc, points).astype(f32)


def move_normals(params, normals, ids, w, ok):
    params = np.asarray(params, f32); normals = np.asarray(normals, f32).reshape(-1, 3)
    acc = np.zeros_like(normals)
    with np.errstate(all="ignore"):
        for k in range(K):
            P = params[ids[:, k]]
            R = [[_R(P, r, c) for c in range(3)] for r in range(3)]
            C = [[None] * 3 for _ in range(3)]
            for r in range(3):
                r1, r2 = (r + 1) % 3, (r + 2) % 3
                for c in range(3):
                    c1, c2 = (c + 1) % 3, (c + 2) % 3
                    C[r][c] = R[r1][c1] * R[r2][c2] - R[r1][c2] * R[r2][c1]
            det = (R[0][0] * C[0][0] + R[0][1] * C[0][1]) + R[0][2] * C[0][2]
            for r in range(3):
                mr = ((C[r][0] / det) * normals[:, 0] + (C[r][1] / det) * normals[:, 1]) + (C[r][2] / det) * normals[:, 2]
                acc[:, r] = acc[:, r] + w[:, k] * mr
        ln = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
        out = acc / ln[:, None]
    return np.where(ok[:, None], out, normals).astype(f32)


def apply_map(nodes, params, surfels, reactivate=None):
    """the map pass.  reactivate: None or dict(t_inv 4x4, cam (fx, fy, cx, cy), cols, rows, max_depth, depth [rows, cols], threshold, tick)"""
    s = np.array(surfels, f32).reshape(-1, 12)
    ids, w, ok = weights(nodes, s[:, 0:3], s[:, 6])
    s[:, 0:3] = move_points(nodes, params, s[:, 0:3], ids, w, ok)
    s[:, 8:11] = move_normals(params, s[:, 8:11], ids, w, ok)
    if reactivate is not None:
        a = reactivate
        T = np.asarray(a["t_inv"], f32).reshape(4, 4); fx, fy, cx, cy = (f32(v) for v in a["cam"])
        depth = np.asarray(a["depth"], f32)
        with np.errstate(all="ignore"):
            l = [((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)]
            x = ((fx * l[0]) / l[2]) + cx
            y = ((fy * l[1]) / l[2]) + cy
            inside = (l[2] > 0) & (l[2] < f32(a["max_depth"])) & (x > 0) & (y > 0) & (x < f32(a["cols"])) & (y < f32(a["rows"]))
            px = np.where(inside, np.floor(x), 0).astype(np.int64); py = np.where(inside, np.floor(y), 0).astype(np.int64)
            d = depth[py, px]
            hit = inside & (s[:, 3] > f32(a["threshold"])) & (d > 0) & (l[2] < d + f32(0.1))
        s[hit, 7] = f32(a["tick"])
    return s


# ------------------------------------------------------------------------------------------------ energy
def rows(nodes, params, cons_src, cons_dst, ids, w, ok):
    """the sparse rows of J and the residual, in row order: [(cols, vals f64)], r f64"""
    nodes = np.asarray(nodes, f32); params = np.asarray(params, f32)
    n = len(nodes); E = edges(n)
    out, res = [], []
    sr, sc = SQRT_REG, SQRT_CON
    for j in range(n):
        P = params[j]; o = BLOCK * j
        R = lambda r, c: P[3 * c + r]
        dot = lambda a, b: (R(0, a) * R(0, b) + R(1, a) * R(1, b)) + R(2, a) * R(2, b)
        for (a, b) in ((0, 1), (0, 2), (1, 2)):
            out.append(([o + 3 * a, o + 3 * a + 1, o + 3 * a + 2, o + 3 * b, o + 3 * b + 1, o + 3 * b + 2],
                        [R(0, b), R(1, b), R(2, b), R(0, a), R(1, a), R(2, a)]))
            res.append(float(dot(a, b)))
        for a in range(3):
            out.append(([o + 3 * a, o + 3 * a + 1, o + 3 * a + 2], [f32(2) * R(0, a), f32(2) * R(1, a), f32(2) * R(2, a)]))
            res.append(float(dot(a, a)) - 1.0)
    for j in range(n):
        P = params[j]; o = BLOCK * j; g = nodes[j, :3]
        for nb in E[j]:
            gn = nodes[nb, :3]; on = BLOCK * int(nb); d = gn - g
            for c in range(3):
                first = ([on + 9 + c], [-sr]) if nb < j else ([], [])
                last = ([on + 9 + c], [-sr]) if nb > j else ([], [])
                out.append((first[0] + [o + c, o + 3 + c, o + 6 + c, o + 9 + c] + last[0],
                            first[1] + [d[0] * sr, d[1] * sr, d[2] * sr, sr] + last[1]))
                v = (P[c] * d[0] + P[3 + c] * d[1]) + P[6 + c] * d[2]
                v = v + g[c]
                v = v + P[9 + c]
                v = v - (gn[c] + params[nb, 9 + c])
                res.append(float(v) * float(sr))
    if len(cons_src):
        moved = move_points(nodes, params, cons_src, ids, w, ok)
        for l in range(len(cons_src)):
            for c in range(3):
                cols, vals = [], []
                if ok[l]:
                    for k in range(K):
                        o = BLOCK * int(ids[l, k]); d = (cons_src[l] - nodes[ids[l, k], :3]) * w[l, k]
                        cols += [o + c, o + 3 + c, o + 6 + c, o + 9 + c]
                        vals += [d[0] * sc, d[1] * sc, d[2] * sc, w[l, k] * sc]
                out.append((cols, vals))
                res.append(float(f32(moved[l, c] - cons_dst[l, c])) * float(sc))
    return [(np.asarray(c, np.int64), np.asarray([float(f32(x)) for x in v], np.float64)) for c, v in out], np.asarray(res, np.float64)


def dense_system(n_nodes, jrows, r):
    """J dense, A = J^T J, b = -J^T r in f64"""
    J = np.zeros((len(jrows), BLOCK * n_nodes))
    for i, (c, v) in enumerate(jrows):
        J[i, c] = v
    return J, J.T @ J, -(J.T @ r)


def _band_terms(jrows):
    """every product J[k, a] * J[k, b] (column b <= column a) of every row k, in row order: flat band index, value, row"""
    at, val, row = [], [], []
    tri = {}
    for k, (c, v) in enumerate(jrows):
        m = len(c)
        if not m:
            continue
        if m not in tri:
            a, b = np.indices((m, m))
            tri[m] = (a.reshape(-1), b.reshape(-1))
        a, b = tri[m]
        keep = c[b] <= c[a]
        a, b = a[keep], b[keep]
        at.append(c[a] * (HALF_BAND + 1) + (c[a] - c[b])); val.append(v[a] * v[b]); row.append(np.full(len(a), k))
    cat = lambda x, t: np.concatenate(x) if x else np.zeros(0, t)
    return cat(at, np.int64), cat(val, np.float64), cat(row, np.int64)


def band_system(n_nodes, jrows, r):
    """the same sums accumulated row by row into band storage AB[i, d] = A[i, i - d] (d = 0..239), and b"""
    n = BLOCK * n_nodes
    AB = np.zeros(n * (HALF_BAND + 1)); b = np.zeros(n)
    at, val, _ = _band_terms(jrows)
    np.add.at(AB, at, val)
    for (c, v), ri in zip(jrows, r):
        np.subtract.at(b, c, v * ri)
    return AB.reshape(n, HALF_BAND + 1), b


def to_band(A):
    n = len(A)
    AB = np.zeros((n, HALF_BAND + 1))
    for d in range(min(n, HALF_BAND + 1)):
        AB[d:, d] = np.diagonal(A, -d)
    return AB


def sum_bounds(n_nodes, jrows, r):
    """per entry of the band of A and of b: (number of summands, sum of |terms|) -- the bound of a sum taken in another order"""
    n = BLOCK * n_nodes
    mA = np.zeros(n * (HALF_BAND + 1), np.int64); sA = np.zeros(n * (HALF_BAND + 1))
    mb = np.zeros(n, np.int64); sb = np.zeros(n)
    at, val, _ = _band_terms(jrows)
    np.add.at(mA, at, 1); np.add.at(sA, at, np.abs(val))
    for (c, v), ri in zip(jrows, r):
        np.add.at(mb, c, 1); np.add.at(sb, c, np.abs(v * ri))
    return mA.reshape(n, -1), sA.reshape(n, -1), mb, sb


def band_cholesky(AB, dtype=np.float64):
    """L in the same band storage, or None at a pivot <= 0.  No pivoting."""
    L = np.array(AB, dtype); n, bw = L.shape
    ta, tb = np.tril_indices(bw - 1)           # row j+1+ta, column j+1+tb of the trailing window, tb <= ta
    for j in range(n):
        if not L[j, 0] > 0:
            return None
        L[j, 0] = np.sqrt(L[j, 0])
        m = min(bw - 1, n - 1 - j)
        if m == 0:
            continue
        i = np.arange(1, m + 1)
        col = L[j + i, i] / L[j, 0]
        L[j + i, i] = col
        a, b = (ta, tb) if m == bw - 1 else (ta[ta < m], tb[ta < m])
        L[j + 1 + a, a - b] -= col[a] * col[b]
    return L


def band_solve(L, b):
    n, bw = L.shape
    y = np.array(b, L.dtype)
    for i in range(n):
        m = min(bw - 1, i)
        if m:
            y[i] -= np.dot(L[i, 1:m + 1], y[i - 1::-1][:m])
        y[i] /= L[i, 0]
    for i in range(n - 1, -1, -1):
        y[i] /= L[i, 0]
        m = min(bw - 1, i)
        if m:
            y[i - m:i] -= L[i, m:0:-1] * y[i]
    return y


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp, f64)"""
    p = a * b
    def split(x):
        t = 134217729.0 * x
        hi = t - (t - x)
        return hi, x - hi
    ah, al = split(a); bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _two_sum(a, b):
    s = a + b
    t = s - a
    return s, (a - (s - t)) + (b - t)


def band_factor(AB, dtype=np.float64):
    """-> solve(rhs) with a band Cholesky factor of A: LAPACK's (scipy) for large f64 systems where it is installed, else the loops above"""
    n, bw = AB.shape
    if dtype == np.float64 and n > 1000:
        try:
            from scipy.linalg import cho_solve_banded, cholesky_banded
            ab = np.zeros((bw, n))
            for d in range(min(bw, n)):
                ab[d, :n - d] = AB[d:, d]
            cb = cholesky_banded(ab, lower=True)
            return lambda rhs: cho_solve_banded((cb, True), np.asarray(rhs, np.float64))
        except ImportError:
            pass
    L = band_cholesky(AB, dtype)
    assert L is not None
    return lambda rhs: band_solve(L, np.asarray(rhs, dtype))


def solve_star(AB, b):
    """the solution of A x = b in extended precision: x is held in numpy.longdouble and refined until the correction no longer changes
    it, against residuals b - A x formed from error-free products (Dekker) and summed with a compensated (two-sum) accumulation -- exact
    to about twice the f64 precision, far below a longdouble ulp.  The factor that turns a residual into a correction is a longdouble
    band Cholesky (f64 above 1000 unknowns, where it only costs refinement steps).  Returned as longdouble."""
    n, bw = AB.shape
    solve = band_factor(AB, np.longdouble if n <= 1000 else np.float64)
    x = np.asarray(solve(b), np.longdouble)
    # the full rows of the symmetric A: full[i, k] = A[i, i - (bw - 1) + k]
    full = np.zeros((n, 2 * bw - 1))
    for d in range(min(bw, n)):
        full[d:, bw - 1 - d] = AB[d:, d]
        full[:n - d, bw - 1 + d] = AB[d:, d]
    cols = np.arange(n)[:, None] - (bw - 1) + np.arange(2 * bw - 1)[None, :]
    inside = (cols >= 0) & (cols < n)
    cols = np.clip(cols, 0, n - 1)
    for _ in range(40):
        xh = x.astype(np.float64); xl = (x - xh).astype(np.float64)
        p1, e1 = _two_prod(full, np.where(inside, xh[cols], 0.0)); p2, e2 = _two_prod(full, np.where(inside, xl[cols], 0.0))
        acc = np.asarray(b, np.float64).copy(); comp = np.zeros(n)
        for part in (p1, p2, e1, e2):
            for k in range(part.shape[1]):
                acc, err = _two_sum(acc, -part[:, k])
                comp += err
        r = acc.astype(np.longdouble) + comp.astype(np.longdouble)
        x2 = x + np.asarray(solve(r), np.longdouble)
        if np.array_equal(x2, x):
            break
        x = x2
    return x


def cons_error(nodes, params, cons_src, cons_dst, ids, w, ok):
    if not len(cons_src):
        return f32(np.nan)
    d = move_points(nodes, params, cons_src, ids, w, ok) - np.asarray(cons_dst, f32)
    norm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    s = f32(0)
    for v in norm:
        s = f32(s + v)
    return f32(s / f32(len(norm)))


def error_of(r):
    s = 0.0
    for v in r:
        s += v * v
    return f32(s)


def iterate(nodes, params, cons_src, cons_dst, ids, w, ok):
    """one Gauss-Newton step -> dict(params, delta, error, delta_norm, failed)"""
    n = len(nodes)
    jr, r = rows(nodes, params, cons_src, cons_dst, ids, w, ok)
    _, A, b = dense_system(n, jr, r)
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return dict(params=np.array(params, f32), failed=True)
    delta = _tri(Lc, b)
    new = (np.asarray(params, f32).astype(np.float64).reshape(-1) + delta).astype(f32).reshape(-1, 12)
    _, r2 = rows(nodes, new, cons_src, cons_dst, ids, w, ok)
    return dict(params=new, delta=delta, error=error_of(r2), delta_norm=float(np.sqrt(np.sum(delta * delta))), failed=False)


def _tri(Lc, b):
    """forward and backward substitution with the dense Cholesky factor (f64, row order)"""
    n = len(b); y = np.array(b, np.float64)
    for i in range(n):
        y[i] = (y[i] - Lc[i, :i] @ y[:i]) / Lc[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - Lc[i + 1:, i] @ y[i + 1:]) / Lc[i, i]
    return y


def optimise(nodes, cons_src, cons_dst, cons_src_time, th=None, trace=None):
    """optimiseGraphSparse with fernMatch + the acceptance of Deformation::constrain.  trace (a list) receives every compared
    (value, threshold) pair of the stop and accept rules."""
    th = dict(DEFAULTS, **(th or {}))
    nodes = np.asarray(nodes, f32); n = len(nodes)
    cons_src = np.asarray(cons_src, f32).reshape(-1, 3); cons_dst = np.asarray(cons_dst, f32).reshape(-1, 3)
    note = (lambda v, t: trace.append((float(v), float(t)))) if trace is not None else (lambda v, t: None)
    params = identity_params(n)
    ids, w, ok = weights(nodes, cons_src, cons_src_time) if len(cons_src) else (np.zeros((0, 4), np.int32), np.zeros((0, 4), f32), np.zeros(0, bool))
    out = dict(optimised=False, accepted=False, failed=False, iterations=0, params=params, ids=ids, w=w, ok=ok)
    mean0 = cons_error(nodes, params, cons_src, cons_dst, ids, w, ok)
    _, r0 = rows(nodes, params, cons_src, cons_dst, ids, w, ok)
    out.update(error_before=error_of(r0), mean_cons_error_before=mean0, error=error_of(r0), mean_cons_error=mean0)
    note(mean0, th["min_cons_error"])
    if not (mean0 >= f32(th["min_cons_error"])):       # (no constraints: nan -> not optimised)
        return out
    out["optimised"] = True
    last = float(out["error"])
    it = 0
    while it < th["max_iterations"]:
        it += 1
        step = iterate(nodes, params, cons_src, cons_dst, ids, w, ok)
        if step["failed"]:
            out.update(failed=True, iterations=it)
            return out
        params = step["params"]; err = step["error"]; out.update(params=params, error=err, iterations=it)
        note(err, last); note(step["delta_norm"], th["min_delta"]); note(err, th["min_error"])
        note(abs(float(err) - last), th["min_change"] * float(err))
        if it == 1:
            note(err, th["max_first_error"])
        if (float(err) > last or step["delta_norm"] < th["min_delta"] or float(err) < th["min_error"]
                or abs(float(err) - last) < th["min_change"] * float(err) or (it == 1 and float(err) > th["max_first_error"])):
            break
        last = float(err)
    mean1 = cons_error(nodes, params, cons_src, cons_dst, ids, w, ok)
    out["mean_cons_error"] = mean1
    note(mean1, th["accept_cons_error"]); note(out["error"], th["accept_error"])
    out["accepted"] = bool(mean1 < f32(th["accept_cons_error"]) and out["error"] < f32(th["accept_error"]))
    return out


# ------------------------------------------------------------------------------------------------ keyframe poses
def polar_newton(M):
    X = np.array(M, np.float64)
    for _ in range(20):
        Xn = 0.5 * (X + np.linalg.inv(X).T)
        if np.array_equal(Xn, X):
            break
        X = Xn
    return X


def inv_t_3x3(X):
    """X^-T by cofactors over the determinant in f64, in the order the kernel uses"""
    C = np.zeros((3, 3))
    for r in range(3):
        r1, r2 = (r + 1) % 3, (r + 2) % 3
        for c in range(3):
            c1, c2 = (c + 1) % 3, (c + 2) % 3
            C[r, c] = X[r1, c1] * X[r2, c2] - X[r1, c2] * X[r2, c1]
    det = (X[0, 0] * C[0, 0] + X[0, 1] * C[0, 1]) + X[0, 2] * C[0, 2]
    return C / det


def apply_poses(nodes, params, poses, times):
    """-> (translations bit for bit f32 [M, 3], blended 3x3 f32 [M, 3, 3] = (sum w R) P33, ok)"""
    poses = np.asarray(poses, f32).reshape(-1, 4, 4); params = np.asarray(params, f32)
    p = poses[:, :3, 3]
    ids, w, ok = weights(nodes, p, times)
    t = move_points(nodes, params, p, ids, w, ok)
    B = np.zeros((len(poses), 3, 3), f32)
    for k in range(K):
        P = params[ids[:, k]]
        for r in range(3):
            for c in range(3):
                B[:, r, c] = B[:, r, c] + w[:, k] * _R(P, r, c)
    M = np.zeros_like(B)
    for r in range(3):
        for c in range(3):
            M[:, r, c] = (B[:, r, 0] * poses[:, 0, c] + B[:, r, 1] * poses[:, 1, c]) + B[:, r, 2] * poses[:, 2, c]
    return t, M, ok


def polar_svd(M):
    U, _, Vt = np.linalg.svd(np.asarray(M, np.float64))
    return U @ Vt
