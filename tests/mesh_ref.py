"""The numpy statement of the mesh export (csrc/mesh.hip): surfels -> integer signed-distance grid -> marching
tetrahedra.  Every f32 operation is written out in the order the kernels use (no contraction), every sum is an integer sum, and the
output ORDER is part of the statement: the device equals all of it bit for bit.

Sign.  The fusion computes a surfel's normal as cross(del_x, del_y) of BACKWARD differences of the camera-frame vertices
(cf_surfel_device.h: get_normal_central; del_x runs towards -x, del_y towards -y), which is +z for a wall seen head on: stored normals
point AWAY from the camera that saw the surfel, into the surface.  savePly negates them on export for that reason.  The mesher does
the same: n_out = -n_stored, d = n_out . (c - p), positive on the side the surfel was observed from.  Positive means outside.

Stage (a), per confident surfel (conf > conf_threshold) and grid sample c = origin + (f32)index * voxel inside its clipped box:
    e = c - p;  d = (n.x*e.x + n.y*e.y) + n.z*e.z;  t2 = max(((e.x*e.x + e.y*e.y) + e.z*e.z) - d*d, 0)
    support: |d| <= tau and t2 <= rho2, tau = trunc_voxels*voxel, rho = min(max(radius, 1.5*voxel), max_support_voxels*voxel)
    wq = rint(max(min(conf, conf_cap) * (1 - t2/rho2), 0) * 2^12);  dq = rint((d/tau) * 2^15)
    planes 0..4 of the accumulator: sum wq*dq (i64), sum wq, sum wq*r, sum wq*g, sum wq*b
Stage (b): Kuhn's six tetrahedra per cell, vertices on the 7 edge kinds of a sample (kind = dx | dy<<1 | dz<<2, minus one).
"""
import numpy as np

f32 = np.float32
DEFAULT_PARAMS = dict(trunc_voxels=3.0, max_support_voxels=4.0, conf_cap=100.0)
DEFAULT_MAX_VOXELS = 1 << 24
W_SCALE = f32(4096.0)
D_SCALE = f32(32768.0)
R_SCALE = f32(65536.0)

# edge kind k -> the offset of its far end: code k + 1 = dx | dy << 1 | dz << 2
KIND_DELTA = [((k + 1) & 1, (k + 1) >> 1 & 1, (k + 1) >> 2 & 1) for k in range(7)]
# the six tetrahedra: a path 000 -> +axis p0 -> +axis p1 -> 111 per permutation of the axes, in lexicographic order; the sign of the
# permutation is the orientation of (v0, v1, v2, v3)
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
TET_SIGN = [1, -1, -1, 1, 1, -1]
TET_CORNERS = [[0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7] for p in PERMS]
LOCAL_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def _parity(seq):
    inv = sum(1 for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[i] > seq[j])
    return -1 if inv & 1 else 1


def case_triangles(mask):
    """triangles of a POSITIVELY oriented tetrahedron whose local vertex i is inside iff bit i of mask: a list of triples of local
    edges (i, j), i < j, wound so that the geometric normal points to the outside; a negative tetrahedron swaps the last two"""
    ins = [i for i in range(4) if mask >> i & 1]
    out = [i for i in range(4) if not mask >> i & 1]
    e = lambda i, j: (min(i, j), max(i, j))
    if len(ins) == 1:
        a, (b, c, d) = ins[0], out
        t = [[e(a, b), e(a, c), e(a, d)]]
        par = _parity([a, b, c, d])
    elif len(ins) == 3:
        a, (b, c, d) = out[0], ins
        t = [[e(a, b), e(a, d), e(a, c)]]
        par = _parity([a, b, c, d])
    elif len(ins) == 2:
        (a, b), (c, d) = ins, out
        t = [[e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]]
        par = _parity([a, b, c, d])
    else:
        return []
    if par < 0:
        t = [[x[0], x[2], x[1]] for x in t]
    return t


CASES = [case_triangles(m) for m in range(16)]


def make_grid(origin, voxel, dims):
    return dict(origin=np.asarray(origin, f32).copy(), voxel=f32(voxel), dims=tuple(int(v) for v in dims))


def nvox(grid):
    nx, ny, nz = grid["dims"]
    return nx * ny * nz


def _params(params):
    p = dict(DEFAULT_PARAMS)
    p.update(params or {})
    return {k: f32(v) for k, v in p.items()}


def _axis_range(p, reach, o, voxel, n):
    lo = np.fmin(np.fmax(np.floor(((p - reach) - o) / voxel), f32(-1.0)), f32(n))
    hi = np.fmin(np.fmax(np.ceil(((p + reach) - o) / voxel), f32(-1.0)), f32(n))
    return max(int(lo), 0), min(int(hi), n - 1)


def surfel_terms(s, grid, params, idx):
    """(wq, dq) of surfel record s at the samples idx = (ix, iy, iz) (integer arrays), and the support mask; all f32 as stated"""
    p = _params(params)
    voxel, o = grid["voxel"], grid["origin"]
    s = np.asarray(s, f32)
    tau = p["trunc_voxels"] * voxel
    rho = np.fmin(np.fmax(s[11], f32(1.5) * voxel), p["max_support_voxels"] * voxel)
    rho2 = rho * rho
    n = (-s[8], -s[9], -s[10])
    with np.errstate(all="ignore"):
        e = [(o[a] + idx[a].astype(f32) * voxel) - s[a] for a in range(3)]
        d = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
        t2 = np.fmax(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) - d * d, f32(0.0))
        ok = (np.abs(d) <= tau) & (t2 <= rho2)
        w = np.fmax(np.fmin(s[3], p["conf_cap"]) * (f32(1.0) - t2 / rho2), f32(0.0))
        wq = np.rint(w * W_SCALE)
        dq = np.rint((d / tau) * D_SCALE)
    wq = np.where(ok, wq, 0).astype(np.int64)
    dq = np.where(ok, dq, 0).astype(np.int64)
    return wq, dq, ok


def surfel_box(s, grid, params):
    p = _params(params)
    voxel, o = grid["voxel"], grid["origin"]
    s = np.asarray(s, f32)
    tau = p["trunc_voxels"] * voxel
    rho = np.fmin(np.fmax(s[11], f32(1.5) * voxel), p["max_support_voxels"] * voxel)
    reach = tau + rho
    with np.errstate(all="ignore"):
        return [_axis_range(s[a], reach, o[a], voxel, grid["dims"][a]) for a in range(3)]


def colour_of(s):
    c = int(np.fmin(np.fmax(f32(s[4]), f32(0.0)), f32(16777215.0)))
    return c >> 16 & 255, c >> 8 & 255, c & 255


def accumulate(surfels, conf_threshold, grid, params=None):
    """the five integer planes [5, nz*ny*nx] (i64; planes 1..4 are non-negative)"""
    nx, ny, nz = grid["dims"]
    acc = np.zeros((5, nx * ny * nz), np.int64)
    surfels = np.asarray(surfels, f32).reshape(-1, 12)
    thr = f32(conf_threshold)
    for s in surfels:
        if not (s[3] > thr):
            continue
        (x0, x1), (y0, y1), (z0, z1) = surfel_box(s, grid, params)
        if x0 > x1 or y0 > y1 or z0 > z1:
            continue
        iz, iy, ix = np.meshgrid(np.arange(z0, z1 + 1), np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        wq, dq, ok = surfel_terms(s, grid, params, (ix, iy, iz))
        lin = ((iz * ny + iy) * nx + ix)[ok]
        wq, dq = wq[ok], dq[ok]
        r, g, b = colour_of(s)
        # (every sample appears once per surfel: plain fancy-index adds are exact)
        acc[0, lin] += wq * dq
        acc[1, lin] += wq
        acc[2, lin] += wq * r
        acc[3, lin] += wq * g
        acc[4, lin] += wq * b
    return acc


def w_min_q(w_min):
    return max(int(np.rint(np.float64(f32(w_min)) * 4096.0)), 1)


def field_of(acc, w_min):
    """(sdf f32 [n], valid bool [n], rgb f32 [n, 3]); invalid samples hold zeros"""
    sw = acc[1].astype(np.float64)
    valid = acc[1] >= w_min_q(w_min)
    den = np.where(valid, sw, 1.0)
    sdf = np.where(valid, acc[0].astype(np.float64) / den, 0.0).astype(f32)
    rgb = np.stack([np.where(valid, acc[k].astype(np.float64) / den, 0.0).astype(f32) for k in (2, 3, 4)], axis=1)
    return sdf, valid, rgb


VERTEX = np.dtype([("pos", f32, 3), ("nrm", f32, 3), ("rgba", np.uint8, 4)])
assert VERTEX.itemsize == 28


def _unit(v):
    """rows of v scaled by 1/sqrt(|v|^2) in f32; (ok: |v|^2 > 0 and finite)"""
    with np.errstate(all="ignore"):
        l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        ok = (l2 > 0) & np.isfinite(l2)
        rn = f32(1.0) / np.sqrt(np.where(ok, l2, f32(1.0)))
    return v * rn[:, None], ok


def extract(grid, sdf, valid, rgb=None):
    """marching tetrahedra on a field: (vertices VERTEX [V], triangles u32 [T, 3])"""
    nx, ny, nz = grid["dims"]
    n = nx * ny * nz
    sdf = np.asarray(sdf, f32).reshape(-1)
    valid = np.asarray(valid).reshape(-1).astype(bool)
    rgb = np.zeros((n, 3), f32) if rgb is None else np.asarray(rgb, f32).reshape(n, 3)
    empty = (np.zeros(0, VERTEX), np.zeros((0, 3), np.uint32))
    if n == 0 or nx < 2 or ny < 2 or nz < 2:
        return empty
    S = sdf.reshape(nz, ny, nx)
    Vd = valid.reshape(nz, ny, nx)
    inside = S < 0
    corner_off = [(c & 1) + nx * ((c >> 1 & 1) + ny * (c >> 2 & 1)) for c in range(8)]
    sl = lambda a, c: a[(c >> 2 & 1):nz - 1 + (c >> 2 & 1), (c >> 1 & 1):ny - 1 + (c >> 1 & 1), (c & 1):nx - 1 + (c & 1)]
    allv = np.ones((nz - 1, ny - 1, nx - 1), bool)
    nin = np.zeros((nz - 1, ny - 1, nx - 1), np.int32)
    for c in range(8):
        allv &= sl(Vd, c)
        nin += sl(inside, c)
    active = allv & (nin > 0) & (nin < 8)
    zz, yy, xx = np.nonzero(active)            # (row-major: ascending linear cell index)
    flags = np.zeros((n, 7), bool)
    tris = []                                  # (owner sample, kind) x 3 per triangle
    insf = inside.reshape(-1)
    for z, y, x in zip(zz, yy, xx):
        base = (z * ny + y) * nx + x
        for t in range(6):
            cs = TET_CORNERS[t]
            m = sum(int(insf[base + corner_off[cs[i]]]) << i for i in range(4))
            for tri in CASES[m]:
                if TET_SIGN[t] < 0:
                    tri = [tri[0], tri[2], tri[1]]
                ent = []
                for i, j in tri:
                    owner = base + corner_off[cs[i]]
                    kind = (cs[i] ^ cs[j]) - 1
                    flags[owner, kind] = True
                    ent.append((owner, kind))
                tris.append(ent)
    if not tris:
        return empty
    vs, vk = np.nonzero(flags)                 # (row-major: ordered by sample, then kind)
    vid = np.full((n, 7), -1, np.int64)
    vid[vs, vk] = np.arange(len(vs))
    T = np.array([[vid[o, k] for o, k in ent] for ent in tris], np.int64)
    assert (T >= 0).all()
    # vertices
    delta = np.array(KIND_DELTA, np.int64)[vk]
    ax, ay, az = vs % nx, vs // nx % ny, vs // (nx * ny)
    bidx = vs + delta[:, 0] + nx * (delta[:, 1] + ny * delta[:, 2])
    sa, sb = sdf[vs], sdf[bidx]
    o, voxel = grid["origin"], grid["voxel"]
    with np.errstate(all="ignore"):
        tt = sa / (sa - sb)
        A = np.stack([o[0] + ax.astype(f32) * voxel, o[1] + ay.astype(f32) * voxel, o[2] + az.astype(f32) * voxel], axis=1)
        B = np.stack([o[0] + (ax + delta[:, 0]).astype(f32) * voxel, o[1] + (ay + delta[:, 1]).astype(f32) * voxel,
                      o[2] + (az + delta[:, 2]).astype(f32) * voxel], axis=1)
        pos = A + (B - A) * tt[:, None]
        col = rgb[vs] + (rgb[bidx] - rgb[vs]) * tt[:, None]
        col8 = np.rint(np.fmin(np.fmax(col, f32(0.0)), f32(255.0))).astype(np.uint8)

    def gradient(idx):
        x, y, z = idx % nx, idx // nx % ny, idx // (nx * ny)
        ok = (x > 0) & (x < nx - 1) & (y > 0) & (y < ny - 1) & (z > 0) & (z < nz - 1)
        g = np.zeros((len(idx), 3), f32)
        for a, step in enumerate((1, nx, nx * ny)):
            hi = np.where(ok, idx + step, idx)
            lo = np.where(ok, idx - step, idx)
            ok = ok & valid[hi] & valid[lo]
            g[:, a] = sdf[hi] - sdf[lo]
        return g, ok

    ga, oka = gradient(vs)
    gb, okb = gradient(bidx)
    with np.errstate(all="ignore"):
        g = ga + (gb - ga) * tt[:, None]
    nrm, okn = _unit(g)
    use_grad = oka & okb & okn
    # the face normal of the first triangle (lowest index) using each vertex
    first = np.full(len(vs), len(T), np.int64)
    np.minimum.at(first, T.reshape(-1), np.repeat(np.arange(len(T)), 3))
    assert (first < len(T)).all(), "an unreferenced vertex"
    ft = T[first]
    with np.errstate(all="ignore"):
        p0, p1, p2 = pos[ft[:, 0]], pos[ft[:, 1]], pos[ft[:, 2]]
        u, v = p1 - p0, p2 - p0
        fn = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    fnu, okf = _unit(fn)
    fnu = np.where(okf[:, None], fnu, f32(0.0))
    out = np.zeros(len(vs), VERTEX)
    out["pos"] = pos
    out["nrm"] = np.where(use_grad[:, None], nrm, fnu)
    out["rgba"][:, :3] = col8
    out["rgba"][:, 3] = 255
    return out, T.astype(np.uint32)


def default_grid(surfels, conf_threshold, voxel=0.0, max_voxels=DEFAULT_MAX_VOXELS):
    """the default placement: exact AABB of the confident surfels padded by tau (of the default trunc_voxels), voxel = mean confident
    radius when 0, raised by a quarter at a time until the grid fits max_voxels (None after 256 steps: the device's CF_ERANGE).  No
    confident surfel (or no positive voxel): the empty grid"""
    p = _params(None)
    surfels = np.asarray(surfels, f32).reshape(-1, 12)
    thr = f32(conf_threshold)
    c = surfels[surfels[:, 3] > thr]
    if len(c) == 0:
        return make_grid([0, 0, 0], 0, (0, 0, 0))
    lo, hi = c[:, 0:3].min(axis=0), c[:, 0:3].max(axis=0)
    voxel = f32(voxel)
    if not voxel > 0:
        rq = np.rint(np.fmin(np.fmax(c[:, 11], f32(0.0)), f32(1024.0)) * R_SCALE).astype(np.int64)
        voxel = f32(np.float64(int(rq.sum())) / np.float64(len(c)) / 65536.0)
    if not (voxel > 0 and np.isfinite(voxel)):
        return make_grid([0, 0, 0], 0, (0, 0, 0))
    for _ in range(256):
        tau = p["trunc_voxels"] * voxel
        o = lo - tau
        with np.errstate(all="ignore"):
            dims = [np.fmin(np.ceil(((hi[a] + tau) - o[a]) / voxel), f32(1 << 30)) for a in range(3)]
        dims = tuple(int(d) + 1 for d in dims)
        if dims[0] * dims[1] * dims[2] <= max_voxels:
            return make_grid(o, voxel, dims)
        voxel = voxel * f32(1.25)
    return None


def mesh_of(surfels, conf_threshold, voxel=0.0, w_min=1.0, max_voxels=DEFAULT_MAX_VOXELS, params=None):
    """the whole export of one map with the default grid: (vertices, triangles, grid)"""
    grid = default_grid(surfels, conf_threshold, voxel, max_voxels)
    if nvox(grid) == 0:
        return np.zeros(0, VERTEX), np.zeros((0, 3), np.uint32), grid
    acc = accumulate(surfels, conf_threshold, grid, params)
    sdf, valid, rgb = field_of(acc, w_min)
    v, t = extract(grid, sdf, valid, rgb)
    return v, t, grid


def write_ply(path, vertices, triangles):
    """binary little-endian PLY in the facade's layout (x y z nx ny nz red green blue; list uchar int vertex_indices)"""
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(vertices), len(triangles))).encode())
        rec = np.zeros(len(vertices), np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))
        rec["p"], rec["n"], rec["c"] = vertices["pos"], vertices["nrm"], vertices["rgba"][:, :3]
        f.write(rec.tobytes())
        face = np.zeros(len(triangles), np.dtype([("k", "u1"), ("v", "<i4", 3)]))
        face["k"], face["v"] = 3, triangles
        f.write(face.tobytes())


def read_ply(path):
    """the reader the tests parse mesh files with: (vertices VERTEX, triangles u32 [T, 3])"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in head if h.startswith("element face")][0].split()[-1])
    props = [h.split()[1:] for h in head if h.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["float", "nx"], ["float", "ny"], ["float", "nz"], ["uchar", "red"],
                     ["uchar", "green"], ["uchar", "blue"], ["list", "uchar", "int", "vertex_indices"]]
    vt = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)])
    ft = np.dtype([("k", "u1"), ("v", "<i4", 3)])
    assert len(raw) == end + nv * vt.itemsize + nf * ft.itemsize
    rec = np.frombuffer(raw, vt, nv, end)
    face = np.frombuffer(raw, ft, nf, end + nv * vt.itemsize)
    assert (face["k"] == 3).all()
    out = np.zeros(nv, VERTEX)
    out["pos"], out["nrm"] = rec["p"], rec["n"]
    out["rgba"][:, :3] = rec["c"]
    out["rgba"][:, 3] = 255
    return out, face["v"].astype(np.uint32)
