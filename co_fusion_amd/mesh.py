"""Python binding of the mesh export (cf_mesh_*, include/cofusion_hip.h): a triangle mesh of one surfel map, extracted on the device in
two stages -- surfels into an integer signed-distance grid, marching tetrahedra on the grid.  Semantics: DESIGN.md 4.15."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .api import CofusionError, Context

ERANGE = -5
DEFAULT_MAX_VOXELS = 1 << 24
VERTEX = np.dtype([("pos", np.float32, 3), ("nrm", np.float32, 3), ("rgba", np.uint8, 4)])
assert VERTEX.itemsize == 28


class Grid(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("voxel", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32)]

    @property
    def dims(self):
        return (self.nx, self.ny, self.nz)

    @property
    def samples(self):
        return self.nx * self.ny * self.nz


class Params(C.Structure):
    _fields_ = [("trunc_voxels", C.c_float), ("max_support_voxels", C.c_float), ("conf_cap", C.c_float)]


def make_grid(origin, voxel, dims):
    return Grid((C.c_float * 3)(*[float(v) for v in origin]), float(voxel), int(dims[0]), int(dims[1]), int(dims[2]))


def make_params(trunc_voxels=3.0, max_support_voxels=4.0, conf_cap=100.0):
    return Params(float(trunc_voxels), float(max_support_voxels), float(conf_cap))


class MeshRangeError(CofusionError):
    """CF_ERANGE: a grid over max_voxels, or more than 2^32 - 1 vertices or triangles"""


class Mesher:
    """cf_mesher of a context: owns the grid and the scan scratch for max_voxels samples (64 bytes each)."""

    def __init__(self, ctx: Context, max_voxels=DEFAULT_MAX_VOXELS):
        self.ctx = ctx
        self.h = C.c_void_p()
        lib = ctx.lib
        lib.cf_mesh_create.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        lib.cf_mesh_default_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.POINTER(Grid)]
        lib.cf_mesh_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.POINTER(Grid), C.POINTER(Params)]
        lib.cf_mesh_extract.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.cf_mesh_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.cf_mesh_grid_download.argtypes = [C.c_void_p, C.c_void_p]
        lib.cf_mesh_extract_grid.argtypes = [C.c_void_p, C.POINTER(Grid), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.cf_mesh_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.cf_mesh_destroy.argtypes = [C.c_void_p]
        lib.cf_mesh_destroy.restype = None
        self._check(lib.cf_mesh_create(ctx.h, int(max_voxels), C.byref(self.h)))
        self.grid = None

    def _check(self, rc):
        if rc == ERANGE:
            msg = self.ctx.lib.cf_last_error(self.ctx.h)
            raise MeshRangeError(f"cofusion_hip error {rc}: {msg.decode() if msg else ''}")
        self.ctx._check(rc)

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.cf_mesh_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def default_grid(self, model, conf_threshold, voxel=0.0) -> Grid:
        """model: a model.Model or a raw cf_model handle"""
        g = Grid()
        self._check(self.ctx.lib.cf_mesh_default_grid(self.h, getattr(model, "h", model), conf_threshold, voxel, C.byref(g)))
        return g

    def accumulate(self, grid: Grid, conf_threshold, model=None, surfels=None, params: Params | None = None):
        """stage (a) for a model (model.Model or handle), or for a torch tensor of surfels [n, 12] on the device"""
        ptr, n = None, 0
        if model is None and surfels is not None:
            assert surfels.is_cuda and surfels.is_contiguous() and surfels.element_size() == 4
            ptr, n = C.c_void_p(surfels.data_ptr()), surfels.numel() // 12
        self._check(self.ctx.lib.cf_mesh_accumulate(self.h, getattr(model, "h", model), ptr, n, conf_threshold, C.byref(grid),
                                                    C.byref(params) if params is not None else None))
        self.grid = grid

    def accumulators(self):
        """int64 [5, samples]: sum wq dq, sum wq, sum wq r, sum wq g, sum wq b"""
        out = np.zeros((5, self.grid.samples), np.int64)
        self._check(self.ctx.lib.cf_mesh_grid_download(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def extract(self, w_min=1.0):
        nv, nt = C.c_uint32(), C.c_uint32()
        self._check(self.ctx.lib.cf_mesh_extract(self.h, w_min, C.byref(nv), C.byref(nt)))
        return nv.value, nt.value

    def extract_grid(self, grid: Grid, sdf, valid, rgb=None):
        """stage (b) on a caller's field (numpy: sdf f32 [n], valid u8 [n], rgb f32 [n, 3] or None)"""
        sdf = np.ascontiguousarray(sdf, np.float32).reshape(-1)
        valid = np.ascontiguousarray(valid, np.uint8).reshape(-1)
        assert len(sdf) == grid.samples and len(valid) == grid.samples
        if rgb is not None:
            rgb = np.ascontiguousarray(rgb, np.float32).reshape(-1)
            assert len(rgb) == 3 * grid.samples
        nv, nt = C.c_uint32(), C.c_uint32()
        self._check(self.ctx.lib.cf_mesh_extract_grid(self.h, C.byref(grid), sdf.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p),
                                                      rgb.ctypes.data_as(C.c_void_p) if rgb is not None else None, C.byref(nv), C.byref(nt)))
        self.grid = grid
        return nv.value, nt.value

    def download(self, n_vertices, n_triangles):
        v = np.zeros(n_vertices, VERTEX)
        t = np.zeros((n_triangles, 3), np.uint32)
        self._check(self.ctx.lib.cf_mesh_download(self.h, v.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)))
        return v, t

    def timing(self):
        """(accumulate ms, extraction ms) of the last calls, by device events"""
        a, e = C.c_float(), C.c_float()
        self._check(self.ctx.lib.cf_mesh_timing(self.h, C.byref(a), C.byref(e)))
        return a.value, e.value

    def mesh(self, model, conf_threshold, voxel=0.0, w_min=1.0, params: Params | None = None):
        """the whole export of one model with the default grid: (vertices, triangles, grid)"""
        g = self.default_grid(model, conf_threshold, voxel)
        self.accumulate(g, conf_threshold, model=model, params=params)
        nv, nt = self.extract(w_min)
        v, t = self.download(nv, nt)
        return v, t, g
