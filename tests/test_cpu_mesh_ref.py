"""CPU suite: properties of the numpy statement of the mesh export (tests/mesh_ref.py) on the case table (tests/mesh_cases.py), and the
facade's PLY writer read back.  The GPU suite holds the device against the same statement bit for bit (test_mesh_kernels_gpu.py)."""
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest

import mesh_cases as mc
import mesh_ref as mr

f32 = np.float32
MESHED = [c for c in mc.CASES if not c.get("empty")]
ids = lambda cs: [c["name"] for c in cs]


def _edges(T):
    """directed edge -> count"""
    d = Counter()
    for a, b, c in T.astype(np.int64):
        d[(a, b)] += 1; d[(b, c)] += 1; d[(c, a)] += 1
    return d


def _components(nv, T):
    parent = list(range(nv))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b, c in T.astype(np.int64):
        ra, rb, rc = find(a), find(b), find(c)
        parent[rb] = ra; parent[rc] = ra
    return np.array([find(i) for i in range(nv)])


@pytest.mark.parametrize("case", mc.CASES, ids=ids(mc.CASES))
def test_every_vertex_is_referenced_and_indices_are_in_range(case):
    r = mc.reference(case)
    V, T = r["vertices"], r["triangles"]
    if case.get("empty"):
        assert len(V) == 0 and len(T) == 0
        return
    assert len(V) > 0 and len(T) > 0
    assert T.max() < len(V)
    assert len(np.unique(T)) == len(V)
    assert (T[:, 0] != T[:, 1]).all() and (T[:, 1] != T[:, 2]).all() and (T[:, 0] != T[:, 2]).all()
    if "min_counts" in case:
        assert len(V) >= case["min_counts"][0] and len(T) >= case["min_counts"][1], (len(V), len(T))


@pytest.mark.parametrize("case", MESHED, ids=ids(MESHED))
def test_manifold_edges(case):
    """closed: every undirected edge in exactly two triangles, once per direction, and V - E + F = 2 per component;
    open: one or two triangles per edge, never the same direction twice, and the boundary edges form closed loops"""
    r = mc.reference(case)
    V, T = r["vertices"], r["triangles"]
    d = _edges(T)
    assert max(d.values()) == 1, "an edge traversed twice in the same direction"
    und = Counter()
    for (a, b), n in d.items():
        und[(min(a, b), max(a, b))] += n
    assert set(und.values()) <= {1, 2}
    boundary = [(a, b) for (a, b) in d if (b, a) not in d]
    if case["closed"]:
        assert not boundary
        comp = _components(len(V), T)
        for root in np.unique(comp):
            vs = np.nonzero(comp == root)[0]
            ts = T[comp[T[:, 0]] == root]
            e = len({(min(a, b), max(a, b)) for a, b, c in ts for a, b in ((a, b), (b, c), (c, a))})
            assert len(vs) - e + len(ts) == 2, (case["name"], len(vs), e, len(ts))
    else:
        if case["closed"] is False:
            assert boundary, "an open case without a boundary"
        out_deg, in_deg = Counter(a for a, b in boundary), Counter(b for a, b in boundary)
        assert out_deg == in_deg, "boundary edges do not form closed loops"


@pytest.mark.parametrize("case", [c for c in MESHED if c["outside"]], ids=ids([c for c in MESHED if c["outside"]]))
def test_winding_agrees_with_the_crafted_outside(case):
    r = mc.reference(case)
    V, T = r["vertices"], r["triangles"].astype(np.int64)
    p = V["pos"].astype(np.float64)
    fn = np.cross(p[T[:, 1]] - p[T[:, 0]], p[T[:, 2]] - p[T[:, 0]])
    area = np.linalg.norm(fn, axis=1)
    cen = p[T].mean(axis=1)
    kind, what = case["outside"]
    if kind == "dir":
        out = np.broadcast_to(np.asarray(what, np.float64), fn.shape)
    else:
        cs = np.asarray(what, np.float64)
        near = np.argmin(np.linalg.norm(cen[:, None, :] - cs[None], axis=2), axis=1)
        out = cen - cs[near]
    s = (fn * out).sum(axis=1)
    # by area: slivers at a kink of the blended field may face anywhere; the surface as a whole must not
    assert area[s > 0].sum() > 0.98 * area.sum(), (area[s > 0].sum(), area.sum())
    # the vertex normals point the same way
    vn = V["nrm"].astype(np.float64)
    assert np.abs(np.linalg.norm(vn, axis=1) - 1).max() < 1e-5   # (a zero normal arises only from a first triangle without area)
    if kind == "dir":
        assert ((vn * np.asarray(what)).sum(axis=1) > 0).mean() > 0.98


@pytest.mark.parametrize("case", mc.MAP_CASES, ids=ids(mc.MAP_CASES))
def test_accumulators_equal_a_brute_force_loop(case):
    """every (surfel, sample) pair of the whole grid in Python integers: the clipped box of the statement drops no pair in the support"""
    acc = mc.reference(case)["acc"]
    g = case["grid"]
    nx, ny, nz = g["dims"]
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx = (ix.reshape(-1), iy.reshape(-1), iz.reshape(-1))
    want = [[0] * (nx * ny * nz) for _ in range(5)]
    for s in case["surfels"]:
        if not f32(s[3]) > f32(case["thr"]):
            continue
        wq, dq, ok = mr.surfel_terms(s, g, case["params"], idx)
        r, gg, b = mr.colour_of(s)
        for i in np.nonzero(ok)[0]:
            w, d = int(wq[i]), int(dq[i])
            want[0][i] += w * d; want[1][i] += w; want[2][i] += w * r; want[3][i] += w * gg; want[4][i] += w * b
    assert acc.dtype == np.int64 and acc.tolist() == want
    if case.get("empty") and not case.get("all_zero"):
        assert not acc.any()
    if case.get("all_zero"):
        sdf, valid = mc.reference(case)["sdf"], mc.reference(case)["valid"]
        assert valid.any() and not acc[0].any() and (sdf[valid] == 0).all()     # the sums cancel exactly: zero is outside, no surface
    if case["name"].startswith(("single", "clipped", "radius")):
        assert acc[1].any()
    if case["name"] == "radius_floor":
        assert np.count_nonzero(acc[1]) < np.count_nonzero(mc.reference(mc.BY_NAME["radius_cap"])["acc"][1])


def test_plane_vertices_lie_on_the_plane():
    """all surfels share the plane and the normal, so every contribution to a sample is the same dq: the field is dq / 2^15 * tau exactly,
    linear in z up to half a quantum per sample, and the interpolated crossing is off by no more than tau * 2^-15 plus f32 rounding"""
    case = mc.BY_NAME["plane_patch"]
    V = mc.reference(case)["vertices"]
    axis, at = case["plane"]
    tau = 3.0 * float(case["grid"]["voxel"])
    err = np.abs(V["pos"][:, axis].astype(np.float64) - at).max()
    print("plane: largest distance", err)
    assert len(V) > 100 and err <= tau * 2.0 ** -15 + 8 * np.finfo(f32).eps * 1.6


def test_sphere_radial_error():
    case = mc.BY_NAME["sphere"]
    V = mc.reference(case)["vertices"]
    centre, R = case["sphere"]
    err = np.abs(np.linalg.norm(V["pos"].astype(np.float64) - np.asarray(centre), axis=1) - R).max()
    print("sphere: largest radial error %.6f (table: %.6f)" % (err, case["max_radial_error"]))
    assert err < 0.5 * float(case["grid"]["voxel"])
    assert err <= 2.0 * case["max_radial_error"]


def test_two_spheres_stay_two_components():
    case = mc.BY_NAME["two_spheres"]
    r = mc.reference(case)
    assert len(np.unique(_components(len(r["vertices"]), r["triangles"]))) == 2


def test_zero_area_triangles_stay():
    r = mc.reference(mc.BY_NAME["exact_zero_plane"])
    p = r["vertices"]["pos"].astype(np.float64)
    T = r["triangles"].astype(np.int64)
    area = np.linalg.norm(np.cross(p[T[:, 1]] - p[T[:, 0]], p[T[:, 2]] - p[T[:, 0]]), axis=1)
    assert (area == 0).any() and (area > 0).any()


def test_the_case_tables_of_header_and_statement_agree():
    """csrc/cf_mesh.h carries the 16 cases as literals: they are the statement's"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "co_fusion_amd", "csrc", "cf_mesh.h")).read().replace("\\\n", " ")
    body = re.search(r"#define CF_MESH_CASES \{(.*?)\}\}", src, flags=re.S).group(1) + "}"
    rows = [[int(v) for v in row.split(",")] for row in re.findall(r"\{([0-9, ]+)\}", body)]
    want = []
    for t in mr.CASES:
        e = [mr.LOCAL_EDGES.index(x) for tri in t for x in tri]
        want.append([len(t)] + e + [0] * (6 - len(e)))
    assert rows == want
    tets = re.search(r"#define CF_MESH_TET_CORNERS \{(.*?)\}\}", src).group(1) + "}"
    assert [[int(v) for v in row.split(",")] for row in re.findall(r"\{([0-9, ]+)\}", tets)] == mr.TET_CORNERS
    neg = re.search(r"#define CF_MESH_TET_NEGATIVE \{([0-9, ]+)\}", src).group(1)
    assert [int(v) for v in neg.split(",")] == [1 if s < 0 else 0 for s in mr.TET_SIGN]


def test_default_grid_of_the_statement():
    case = mc.BY_NAME["sphere"]
    g = mr.default_grid(case["surfels"], case["thr"])
    conf = case["surfels"][case["surfels"][:, 3] > case["thr"]]
    assert abs(float(g["voxel"]) - conf[:, 11].astype(np.float64).mean()) < 2.0 ** -16
    tau = 3 * float(g["voxel"])
    hi = g["origin"].astype(np.float64) + (np.array(g["dims"]) - 1) * float(g["voxel"])
    assert (g["origin"] <= conf[:, :3].min(axis=0) - tau + 1e-6).all() and (hi >= conf[:, :3].max(axis=0) + tau - 1e-6).all()
    small = mr.default_grid(case["surfels"], case["thr"], max_voxels=4096)
    assert mr.nvox(small) <= 4096 and small["voxel"] > g["voxel"]
    assert mr.nvox(mr.default_grid(case["surfels"], 1000.0)) == 0
    assert mr.default_grid(case["surfels"], case["thr"], voxel=0.05)["voxel"] == f32(0.05)


def test_ply_writer_round_trip(tmp_path):
    """cofusion_write_mesh_ply (host code, no GPU): the file parsed back by the tests' reader equals the arrays, and equals the bytes of
    the statement's own writer"""
    import __graft_entry__ as g
    g.build()
    from co_fusion_amd import lib as cflib
    host = cflib.load_host()
    r = mc.reference(mc.BY_NAME["sphere"])
    V, T = np.ascontiguousarray(r["vertices"]), np.ascontiguousarray(r["triangles"])
    path = str(tmp_path / "mesh.ply")
    host.cofusion_write_mesh_ply.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    assert host.cofusion_write_mesh_ply(path.encode(), V.ctypes.data, len(V), T.ctypes.data, len(T)) == 0
    v2, t2 = mr.read_ply(path)
    assert v2.tobytes() == V.tobytes() and t2.tobytes() == T.tobytes()
    mine = str(tmp_path / "ref.ply")
    mr.write_ply(mine, V, T)
    assert open(mine, "rb").read() == open(path, "rb").read()
    empty = str(tmp_path / "empty.ply")
    assert host.cofusion_write_mesh_ply(empty.encode(), None, 0, None, 0) == 0
    v0, t0 = mr.read_ply(empty)
    assert len(v0) == 0 and len(t0) == 0
    assert host.cofusion_write_mesh_ply(str(tmp_path / "no" / "dir.ply").encode(), V.ctypes.data, len(V), T.ctypes.data, len(T)) != 0
