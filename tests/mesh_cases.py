"""Case table of the mesh export (tests/mesh_ref.py, csrc/mesh.hip): one named case per branch.  A "map" case is a crafted surfel map
on an explicit grid (both stages); a "field" case is a crafted distance field (stage (b) alone).  Every grid is at most 40 samples a
side.  `outside` is the crafted outside the winding must agree with: ("dir", v) a direction, ("centres", [c..]) away from the nearest."""
import numpy as np

import mesh_ref as mr

f32 = np.float32
THR = 10.0


def surfel(p, n_stored, radius, conf=20.0, rgb=(200, 120, 40), t0=1.0, t1=2.0):
    """one 12-float record; n_stored points AWAY from the observer (the fusion's convention)"""
    n = np.asarray(n_stored, np.float64)
    n = n / np.linalg.norm(n)
    c = float((rgb[0] << 16) | (rgb[1] << 8) | rgb[2])
    return np.array([p[0], p[1], p[2], conf, c, 0.0, t0, t1, n[0], n[1], n[2], radius], f32)


def _sphere_surfels(centre, R, count, radius, seed):
    """a Fibonacci sphere seen from outside: stored normals point inwards"""
    rng = np.random.default_rng(seed)
    k = np.arange(count) + 0.5
    phi = np.arccos(1 - 2 * k / count)
    th = np.pi * (1 + 5 ** 0.5) * k
    d = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    out = []
    for i in range(count):
        rgb = tuple(int(v) for v in rng.integers(0, 256, 3))
        out.append(surfel(np.asarray(centre) + R * d[i], -d[i], radius, conf=float(rng.uniform(11, 40)), rgb=rgb))
    return np.stack(out)


def _map(name, surfels, origin, voxel, dims, closed=None, outside=None, params=None, thr=THR, w_min=1.0, **kw):
    s = np.zeros((0, 12), f32) if len(surfels) == 0 else np.stack(surfels).astype(f32)
    return dict(name=name, kind="map", surfels=s, grid=mr.make_grid(origin, voxel, dims), closed=closed, outside=outside, params=params, thr=thr,
                w_min=w_min, **kw)


def _field(name, dims, fn, invalid=(), closed=None, outside=None, voxel=0.1, origin=(0.0, 0.0, 0.0), **kw):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    sdf = fn(x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)).astype(f32).reshape(-1)
    valid = np.ones(nx * ny * nz, np.uint8)
    for (ix, iy, iz) in invalid:
        valid[(iz * ny + iy) * nx + ix] = 0
    rng = np.random.default_rng(len(name))
    rgb = rng.uniform(0, 255, (nx * ny * nz, 3)).astype(f32)
    return dict(name=name, kind="field", grid=mr.make_grid(origin, voxel, dims), sdf=sdf, valid=valid, rgb=rgb, closed=closed, outside=outside, **kw)


def _cases():
    c = []
    down = (0.0, 0.0, 1.0)   # stored normal +z: seen from -z, outside is -z
    c.append(_map("single_centre", [surfel((0.75, 0.75, 0.75), down, 0.2)], (0, 0, 0), 0.1, (16, 16, 16), closed=False, outside=("dir", (0, 0, -1))))
    for tag, p in (("xlo", (0.02, 0.75, 0.75)), ("xhi", (1.48, 0.75, 0.75)), ("ylo", (0.75, 0.02, 0.75)), ("yhi", (0.75, 1.48, 0.75)),
                   ("zlo", (0.75, 0.75, 0.02)), ("zhi", (0.75, 0.75, 1.48))):
        c.append(_map("clipped_" + tag, [surfel(p, (0.3, -0.2, 0.9), 0.25)], (0, 0, 0), 0.1, (16, 16, 16)))
    c.append(_map("wholly_outside", [surfel((5.0, 5.0, 5.0), down, 0.2), surfel((-3.0, 0.7, 0.7), down, 0.2)], (0, 0, 0), 0.1, (16, 16, 16), empty=True))
    c.append(_map("at_threshold", [surfel((0.75, 0.75, 0.75), down, 0.2, conf=THR)], (0, 0, 0), 0.1, (16, 16, 16), empty=True))
    c.append(_map("radius_floor", [surfel((0.73, 0.77, 0.71), (0.1, 0.2, 0.9), 0.01)], (0, 0, 0), 0.1, (16, 16, 16)))
    c.append(_map("radius_cap", [surfel((0.73, 0.77, 0.71), (0.1, 0.2, 0.9), 1.0)], (0, 0, 0), 0.1, (16, 16, 16)))
    c.append(_map("opposed_cancel", [surfel((0.75, 0.75, 0.72), down, 0.2), surfel((0.75, 0.75, 0.72), (0, 0, -1.0), 0.2)], (0, 0, 0), 0.1, (16, 16, 16),
                  empty=True, all_zero=True))
    plane = [surfel((x, y, 0.83), down, 0.08, conf=15.0 + 10 * ((i + j) % 3), rgb=(10 * i % 256, 10 * j % 256, 77))
             for i, x in enumerate(np.arange(0.2, 1.31, 0.05)) for j, y in enumerate(np.arange(0.2, 1.31, 0.05))]
    c.append(_map("plane_patch", plane, (0, 0, 0), 0.1, (16, 16, 16), closed=False, outside=("dir", (0, 0, -1)), plane=(2, 0.83)))
    # max_radial_error: measured with the statement on the CPU (test_cpu_mesh_ref.py prints it); the test bounds the error by twice this
    # figure and by half a voxel (the tangent-plane part alone: rho^2 / (2 R) = 0.15^2 / 1.2 = 0.019)
    c.append(_map("sphere", list(_sphere_surfels((1.0, 1.0, 1.0), 0.6, 2000, 0.06, 5)), (0, 0, 0), 0.1, (21, 21, 21), closed=True,
                  outside=("centres", [(1.0, 1.0, 1.0)]), sphere=((1.0, 1.0, 1.0), 0.6), max_radial_error=SPHERE_MAX_RADIAL_ERROR))
    two = list(_sphere_surfels((0.6, 0.65, 0.65), 0.35, 700, 0.05, 6)) + list(_sphere_surfels((1.4, 0.65, 0.65), 0.35, 700, 0.05, 7))
    c.append(_map("two_spheres", two, (0, 0, 0), 0.1, (21, 14, 14), closed=True, outside=("centres", [(0.6, 0.65, 0.65), (1.4, 0.65, 0.65)]),
                  params=dict(trunc_voxels=2.0)))
    c.append(_map("empty_map", [], (0, 0, 0), 0.1, (8, 8, 8), empty=True))
    c.append(_field("hole_in_surface", (12, 12, 12), lambda x, y, z: z - 5.3 + 0.043 * x, invalid=[(5, 5, 5)], closed=False, outside=("dir", (0, 0, 1))))
    c.append(_field("exact_zero_plane", (9, 8, 10), lambda x, y, z: z - 5.0, closed=False, outside=None, zero_area=True))
    c.append(_field("odd_dims", (33, 17, 9), lambda x, y, z: np.sqrt(((x - 16.2) / 3.5) ** 2 + ((y - 8.1) / 1.9) ** 2 + (z - 4.3) ** 2) - 3.1,
                    closed=True, outside=("centres", [(1.62, 0.81, 0.43)])))
    c.append(_field("many_tiles", (40, 38, 36), lambda x, y, z: np.sqrt((x - 19.3) ** 2 + (y - 18.4) ** 2 + (z - 17.6) ** 2) - 14.2,
                    closed=True, outside=("centres", [(1.93, 1.84, 1.76)]), min_counts=(4 * 1024, 4 * 1024)))
    c.append(_field("thin_grid", (1, 5, 5), lambda x, y, z: z - 2.5, empty=True))
    return c


SPHERE_MAX_RADIAL_ERROR = 0.006977
CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
MAP_CASES = [c for c in CASES if c["kind"] == "map"]
FIELD_CASES = [c for c in CASES if c["kind"] == "field"]

_memo = {}


def reference(case):
    """the statement's result for a case, computed once: dict(acc, sdf, valid, rgb, vertices, triangles)"""
    name = case["name"]
    if name not in _memo:
        if case["kind"] == "map":
            acc = mr.accumulate(case["surfels"], case["thr"], case["grid"], case["params"])
            sdf, valid, rgb = mr.field_of(acc, case["w_min"])
        else:
            acc, sdf, valid, rgb = None, case["sdf"], case["valid"].astype(bool), case["rgb"]
        v, t = mr.extract(case["grid"], sdf, valid, rgb)
        for a in (acc, sdf, valid, rgb, v, t):
            if a is not None:
                a.setflags(write=False)
        _memo[name] = dict(acc=acc, sdf=sdf, valid=valid, rgb=rgb, vertices=v, triangles=t)
    return _memo[name]
