"""Python mirror of the reference interface for the hot path, over the C-ABI.

PyTorch is used for device memory and streams only (tensors are passed to the library as raw
device pointers); every computation happens in the hand-written HIP kernels.

Names follow the reference: `Odometry` mirrors RGBDOdometry (Core/Utils/RGBDOdometry.h:42-60),
the free functions mirror Core/Cuda/cudafuncs.cuh:64-193.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib as _libmod

NUM_PYRS = 3


class Cam(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]

    def level(self, l):
        d = float(1 << l)
        return Cam(self.fx / d, self.fy / d, self.cx / d, self.cy / d)


class Config(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("device", C.c_int), ("max_models", C.c_int), ("max_surfels", C.c_int)]


class TrackOpts(C.Structure):
    _fields_ = [("rgb_only", C.c_int), ("pyramid", C.c_int), ("fast_odom", C.c_int), ("so3", C.c_int),
                ("icp_weight", C.c_float)]


class TrackStats(C.Structure):
    _fields_ = [("last_icp_error", C.c_float), ("last_icp_count", C.c_float), ("last_rgb_error", C.c_float),
                ("last_rgb_count", C.c_float), ("last_so3_error", C.c_float), ("last_so3_count", C.c_float),
                ("lastA", C.c_double * 36), ("lastb", C.c_double * 6), ("so3_iterations", C.c_int), ("fault", C.c_int), ("cull_box", C.c_int * 4)]


class GnState(C.Structure):
    """cf_gn_state: the words of a tracker's device-resident state the Gauss-Newton solve reads and writes"""
    _fields_ = [("intr", Cam), ("width", C.c_int32), ("height", C.c_int32), ("icp", C.c_int32), ("rgb", C.c_int32),
                ("rgbOnly", C.c_int32), ("icpWeight", C.c_float), ("Rprev", C.c_float * 9), ("tprev", C.c_float * 3),
                ("Rprev_inv", C.c_float * 9), ("Rcurr", C.c_float * 9), ("tcurr", C.c_float * 3), ("resultRt", C.c_double * 16),
                ("krkInv", C.c_float * 9), ("kt", C.c_float * 3), ("lastRGBError", C.c_float), ("level_done", C.c_int32),
                ("solves", C.c_int32), ("residual", C.c_float * 2), ("cull_z", C.c_float * 2), ("pose_inv", C.c_float * 16),
                ("stats", TrackStats)]


class GnSystem(C.Structure):
    """cf_gn_system: one system of cf_gn_solve_step (grouped sums [64][32], state, pinned-host twin, the derived hot block)"""
    _fields_ = [("icp_acc", C.c_int64 * (64 * 32)), ("rgb_acc", C.c_int64 * (64 * 32)), ("state", GnState), ("twin", GnState),
                ("hot", C.c_uint32 * 48)]


class So3System(C.Structure):
    """cf_so3_system: one system of cf_so3_prealign_step (the two level-2 images on the device, the state in and out, the derived hot
    block, the system's sync block as the launch left it)"""
    _fields_ = [("last_next_image", C.c_void_p), ("next_image", C.c_void_p), ("state_in", GnState), ("state_out", GnState), ("hot", C.c_uint32 * 48),
                ("sync", C.c_uint64 * 418)]


class RgbSystem(C.Structure):
    """cf_rgb_system: one system of cf_rgb_records_step (the level's device images, the range of a culled tracker, the record buffer and
    the accumulator words before and after the residual pass, the RGB sums, the state / twin / hot block of the solve under mode 2)"""
    _fields_ = [("cand", C.c_void_p), ("next_depth", C.c_void_p), ("last_depth", C.c_void_p), ("last_image", C.c_void_p), ("next_image", C.c_void_p),
                ("cloud", C.c_void_p), ("dIdx", C.c_void_p), ("dIdy", C.c_void_p), ("no_counts", C.c_int32), ("ranged", C.c_int32),
                ("res_range", C.c_uint32 * 2), ("res_blocks", C.c_int32), ("records", C.c_void_p), ("slot_counts", C.c_void_p),
                ("count_seed", C.c_int64 * 64), ("sigma_seed", C.c_int64 * 64), ("count_total", C.c_int64), ("sigma_total", C.c_int64),
                ("rgb_sums", C.c_int64 * 32), ("state", GnState), ("twin", GnState), ("hot", C.c_uint32 * 48)]


class Profile(C.Structure):
    _fields_ = [("icp_ms_total", C.c_double), ("icp_launches", C.c_uint64), ("icp_bytes", C.c_uint64),
                ("surfel_ms_total", C.c_double), ("surfel_calls", C.c_uint64), ("surfel_bytes", C.c_uint64)]


DATATERM = np.dtype([("zero_x", "<i2"), ("zero_y", "<i2"), ("one_x", "<i2"), ("one_y", "<i2"), ("diff", "<f4"),
                     ("valid", "<i4")])


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def _f(a):
    return (C.c_float * len(a))(*[float(x) for x in a])


class CofusionError(RuntimeError):
    pass


class Context:
    """One context per GPU (cf_ctx): owns scratch memory; work is enqueued on torch's current stream."""

    def __init__(self, width=640, height=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, device=0, max_models=8,
                 max_surfels=3072 * 3072):
        if not torch.cuda.is_available():
            raise CofusionError("no GPU visible: the Co-Fusion hot path has no CPU fallback")
        self.lib = _libmod.load()
        self.width, self.height = width, height
        self.cam = Cam(fx, fy, cx, cy)
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        cfg = Config(width, height, fx, fy, cx, cy, device, max_models, max_surfels)
        h = C.c_void_p()
        rc = self.lib.cf_create(C.byref(cfg), C.byref(h))
        self.h = h
        self._check(rc)
        self._check(self.lib.cf_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.cf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = self.lib.cf_last_error(self.h) if self.h else b""
            raise CofusionError(f"cofusion_hip error {rc}: {msg.decode() if msg else ''}")

    def synchronize(self):
        self._check(self.lib.cf_synchronize(self.h))

    # ---- the library's own RCCL communicator (csrc/rccl_comm.hip) ----
    @staticmethod
    def rccl_unique_id():
        buf = (C.c_ubyte * 128)()
        if _libmod.load().cf_rccl_unique_id(buf) != 0:
            raise CofusionError("cf_rccl_unique_id failed")
        return bytes(buf)

    def rccl_init(self, unique_id, rank, world):
        self._check(self.lib.cf_rccl_init(self.h, C.c_char_p(unique_id), int(rank), int(world)))

    def rccl_allreduce(self, tensor, op=0):
        """in place on the context's stream: op 0 = SUM of int64 words, op 1 = MIN of unsigned 64-bit words"""
        assert tensor.element_size() == 8 and tensor.is_contiguous()
        self._check(self.lib.cf_rccl_allreduce(self.h, C.c_void_p(tensor.data_ptr()), C.c_uint64(tensor.numel()), int(op), None))

    def rccl_broadcast(self, tensor, root=0):
        self._check(self.lib.cf_rccl_broadcast(self.h, C.c_void_p(tensor.data_ptr()), C.c_uint64(tensor.numel() * tensor.element_size()), int(root), None))

    def rccl_info(self):
        r, w, v = C.c_int(), C.c_int(), C.c_int()
        rc = self.lib.cf_rccl_info(self.h, C.byref(r), C.byref(w), C.byref(v))
        return dict(active=rc == 0, rank=r.value, world=w.value, version=v.value)

    def empty(self, shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def to_device(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    # ---- map preparation (cudafuncs.cuh) -------------------------------------------------
    def create_vmap(self, depth, cam, cutoff):
        rows, cols = depth.shape
        out = torch.zeros((3 * rows, cols), dtype=torch.float32, device=self.device)
        self._check(self.lib.cf_create_vmap(self.h, _p(depth), cols, rows, cam, C.c_float(cutoff), _p(out)))
        return out

    def create_nmap(self, vmap):
        rows, cols = vmap.shape[0] // 3, vmap.shape[1]
        out = torch.zeros_like(vmap)
        self._check(self.lib.cf_create_nmap(self.h, _p(vmap), cols, rows, _p(out)))
        return out

    def copy_maps(self, v4, n4):
        rows, cols = v4.shape[:2]
        v = self.empty((3 * rows, cols))
        n = self.empty((3 * rows, cols))
        self._check(self.lib.cf_copy_maps(self.h, _p(v4), _p(n4), cols, rows, _p(v), _p(n)))
        return v, n

    def resize_map(self, m, normalize):
        rows, cols = m.shape[0] // 3, m.shape[1]
        out = torch.zeros((3 * (rows // 2), cols // 2), dtype=torch.float32, device=self.device)
        self._check(self.lib.cf_resize_map(self.h, _p(m), cols, rows, _p(out), int(normalize)))
        return out

    def transform_maps(self, v, n, R, t):
        rows, cols = v.shape[0] // 3, v.shape[1]
        self._check(self.lib.cf_transform_maps(self.h, _p(v), _p(n), cols, rows, _f(np.asarray(R).reshape(9)),
                                               _f(np.asarray(t).reshape(3))))

    def vertices_to_depth(self, v4, cutoff):
        rows, cols = v4.shape[:2]
        out = self.empty((rows, cols))
        self._check(self.lib.cf_vertices_to_depth(self.h, _p(v4), cols, rows, C.c_float(cutoff), _p(out)))
        return out

    def pyrdown_gauss_f32(self, src):
        rows, cols = src.shape
        out = self.empty((rows // 2, cols // 2))
        self._check(self.lib.cf_pyrdown_gauss_f32(self.h, _p(src), cols, rows, _p(out)))
        return out

    def pyrdown_gauss_u8(self, src):
        rows, cols = src.shape
        out = self.empty((rows // 2, cols // 2), torch.uint8)
        self._check(self.lib.cf_pyrdown_gauss_u8(self.h, _p(src), cols, rows, _p(out)))
        return out

    def rgba_to_intensity(self, rgba):
        rows, cols = rgba.shape[:2]
        out = self.empty((rows, cols), torch.uint8)
        self._check(self.lib.cf_rgba_to_intensity(self.h, _p(rgba), cols, rows, _p(out)))
        return out

    def sobel(self, img):
        rows, cols = img.shape
        dx = self.empty((rows, cols), torch.int16)
        dy = self.empty((rows, cols), torch.int16)
        self._check(self.lib.cf_sobel(self.h, _p(img), cols, rows, _p(dx), _p(dy)))
        return dx, dy

    def project_cloud(self, depth, cam_level):
        rows, cols = depth.shape
        out = self.empty((rows, cols, 3))
        self._check(self.lib.cf_project_cloud(self.h, _p(depth), cols, rows, cam_level, _p(out)))
        return out

    def depth_pyramid(self, depth):
        rows, cols = depth.shape
        l1 = self.empty((rows // 2, cols // 2))
        l2 = self.empty((rows // 4, cols // 4))
        self._check(self.lib.cf_depth_pyramid(self.h, _p(depth), cols, rows, _p(l1), _p(l2)))
        return [depth, l1, l2]

    # ---- reductions (cudafuncs.cuh) ---------------------------------------------------------
    def icp_step(self, Rcurr, tcurr, vmap_curr, nmap_curr, Rprev_inv, tprev, cam, vmap_g_prev, nmap_g_prev, dist_thres,
                 angle_thres, err_surface=None):
        rows, cols = vmap_curr.shape[0] // 3, vmap_curr.shape[1]
        A = (C.c_float * 36)(); b = (C.c_float * 6)(); res = (C.c_float * 2)(); sums = (C.c_int64 * 32)()
        self._check(self.lib.cf_icp_step(self.h, _f(np.asarray(Rcurr).reshape(9)), _f(tcurr), _p(vmap_curr),
                                         _p(nmap_curr), _f(np.asarray(Rprev_inv).reshape(9)), _f(tprev), cam,
                                         _p(vmap_g_prev), _p(nmap_g_prev), C.c_float(dist_thres), C.c_float(angle_thres),
                                         cols, rows, A, b, res, sums, _p(err_surface)))
        return (np.array(A, np.float32).reshape(6, 6), np.array(b, np.float32), np.array(res, np.float32),
                np.array(sums, np.int64))

    def icp_step_band(self, Rcurr, tcurr, vmap_curr, nmap_curr, Rprev_inv, tprev, cam, vmap_g_prev, nmap_g_prev, dist_thres,
                      angle_thres, row_begin, row_end):
        """icpStep over the row band [row_begin, row_end) only: returns the exact int64[32] sums of the band"""
        rows, cols = vmap_curr.shape[0] // 3, vmap_curr.shape[1]
        A = (C.c_float * 36)(); b = (C.c_float * 6)(); res = (C.c_float * 2)(); sums = (C.c_int64 * 32)()
        self._check(self.lib.cf_icp_step_band(self.h, _f(np.asarray(Rcurr).reshape(9)), _f(tcurr), _p(vmap_curr),
                                              _p(nmap_curr), _f(np.asarray(Rprev_inv).reshape(9)), _f(tprev), cam,
                                              _p(vmap_g_prev), _p(nmap_g_prev), C.c_float(dist_thres), C.c_float(angle_thres),
                                              cols, rows, int(row_begin), int(row_end), A, b, res, sums, None))
        return np.array(sums, np.int64)

    def rgb_residual(self, min_scale, dIdx, dIdy, last_depth, next_depth, last_image, next_image, max_depth_delta, kt,
                     krkinv):
        rows, cols = next_image.shape
        corres = torch.zeros((rows * cols, 16), dtype=torch.uint8, device=self.device)
        sig = C.c_int(); cnt = C.c_int()
        self._check(self.lib.cf_rgb_residual(self.h, C.c_float(min_scale), _p(dIdx), _p(dIdy), _p(last_depth),
                                             _p(next_depth), _p(last_image), _p(next_image), _p(corres),
                                             C.c_float(max_depth_delta), _f(kt), _f(np.asarray(krkinv).reshape(9)),
                                             cols, rows, C.byref(sig), C.byref(cnt)))
        return corres, sig.value, cnt.value

    def rgb_step(self, corres, sigma, cloud, fx, fy, dIdx, dIdy, sobel_scale):
        rows, cols = dIdx.shape
        A = (C.c_float * 36)(); b = (C.c_float * 6)(); sums = (C.c_int64 * 32)()
        self._check(self.lib.cf_rgb_step(self.h, _p(corres), C.c_float(sigma), _p(cloud), C.c_float(fx), C.c_float(fy),
                                         _p(dIdx), _p(dIdy), C.c_float(sobel_scale), cols, rows, A, b, sums))
        return np.array(A, np.float32).reshape(6, 6), np.array(b, np.float32), np.array(sums, np.int64)

    def so3_step(self, last_image, next_image, basis, kinv, krlr):
        rows, cols = next_image.shape
        A = (C.c_float * 9)(); b = (C.c_float * 3)(); res = (C.c_float * 2)(); sums = (C.c_int64 * 16)()
        self._check(self.lib.cf_so3_step(self.h, _p(last_image), _p(next_image), _f(np.asarray(basis).reshape(9)),
                                         _f(np.asarray(kinv).reshape(9)), _f(np.asarray(krlr).reshape(9)), cols, rows,
                                         A, b, res, sums))
        return (np.array(A, np.float32).reshape(3, 3), np.array(b, np.float32), np.array(res, np.float32),
                np.array(sums, np.int64))

    def gn_solve_step(self, systems, next_level, last_of_level, icp_fix=32):
        """cf_gn_solve_step: the per-iteration Gauss-Newton solve as the schedule launches it, one workgroup per system.  systems: a
        ctypes array of 1..16 GnSystem (updated in place) or a sequence of them (copied); returns the array with state, twin, hot
        block and both accumulators as the kernel left them"""
        arr = systems if isinstance(systems, C.Array) else (GnSystem * len(systems))(*systems)
        self._check(self.lib.cf_gn_solve_step(self.h, len(arr), arr, int(next_level), int(bool(last_of_level)), int(icp_fix)))
        return arr

    def so3_prealign_step(self, systems, do_so3=True, first_level=2):
        """cf_so3_prealign_step: the first launch of a tracking call on its own -- state hand-over and, when do_so3, the SO(3)
        pre-alignment loop, 16 workgroups per system.  systems: a ctypes array of So3System (updated in place) or a sequence of
        them (copied); returns the array with the device state, the hot block and the sync block of every system"""
        arr = systems if isinstance(systems, C.Array) else (So3System * len(systems))(*systems)
        self._check(self.lib.cf_so3_prealign_step(self.h, len(arr), arr, int(bool(do_so3)), int(first_level)))
        return arr

    def rgb_records_step(self, systems, cols, rows, max_depth_delta, sobel_scale, fx, fy, next_level=2, last_of_level=False):
        """cf_rgb_records_step: the compact residual pass and the RGB step over its record slots as the schedule launches them under the
        context's gn mode (1 or 2) and launch shape.  systems: a ctypes array of 1..16 RgbSystem (updated in place; `records` and
        `slot_counts` point at host arrays the caller keeps alive) or a sequence of them (copied); returns the array"""
        arr = systems if isinstance(systems, C.Array) else (RgbSystem * len(systems))(*systems)
        self._check(self.lib.cf_rgb_records_step(self.h, len(arr), arr, int(cols), int(rows), C.c_float(max_depth_delta), C.c_float(sobel_scale),
                                                 C.c_float(fx), C.c_float(fy), int(next_level), int(bool(last_of_level))))
        return arr

    def set_icp_launch(self, threads, ppt):
        self._check(self.lib.cf_set_icp_launch(self.h, threads, ppt))

    def set_gn_mode(self, mode):
        self._check(self.lib.cf_set_gn_mode(self.h, int(mode)))

    def track_batch(self, odoms, poses, rgb_only=False, icp_weight=10.0, pyramid=True, fast_odom=False, so3=True, err_surfaces=None):
        """cf_odom_track_batch_async: all trackers advance through the Gauss-Newton schedule inside the same launches; nothing is waited
        for -- Odometry.fetch() of every tracker afterwards.  poses: one 4x4 per tracker; err_surfaces: None or one (nullable) per tracker"""
        n = len(odoms)
        keep = [_f(np.asarray(p, np.float32).reshape(16)) for p in poses]
        pp = (C.POINTER(C.c_float) * max(n, 1))(*[C.cast(k, C.POINTER(C.c_float)) for k in keep])
        oo = (C.c_void_p * max(n, 1))(*[o.h for o in odoms])
        ee = None
        if err_surfaces is not None:
            ee = (C.c_void_p * max(n, 1))(*[e.data_ptr() if e is not None else None for e in err_surfaces])
        opts = TrackOpts(int(rgb_only), int(pyramid), int(fast_odom), int(so3), icp_weight)
        self._check(self.lib.cf_odom_track_batch_async(self.h, oo, n, pp, C.byref(opts), ee))

    def _batch_args(self, odoms, poses):
        n = len(odoms)
        self._keep_poses = [_f(np.asarray(p, np.float32).reshape(16)) for p in poses]
        pp = (C.POINTER(C.c_float) * max(n, 1))(*[C.cast(k, C.POINTER(C.c_float)) for k in self._keep_poses])
        oo = (C.c_void_p * max(n, 1))(*[o.h for o in odoms])

        def ptrs(ts):
            if ts is None:
                return None
            assert len(ts) == n
            return (C.c_void_p * max(n, 1))(*[None if t is None else t.data_ptr() for t in ts])
        return n, oo, pp, ptrs

    def init_models_batch_select(self, odoms, pred_v4, pred_n4, pred_rgba, poses, frame_rgba, alt_v4=None, alt_n4=None, alt_rgba=None,
                                 fill_counts=None, ratio=0.0):
        """cf_odom_init_models_batch_select: initICPModel + initRGBModel + initRGB of all trackers in the same launches.  One device
        tensor per tracker in every list; alt_* / fill_counts (int32 [2] device tensors holding the u32 counts covered, total) may be
        None, and so may single entries of fill_counts"""
        n, oo, pp, ptrs = self._batch_args(odoms, poses)
        self._check(self.lib.cf_odom_init_models_batch_select(self.h, oo, n, ptrs(pred_v4), ptrs(pred_n4), ptrs(pred_rgba), ptrs(alt_v4),
                                                              ptrs(alt_n4), ptrs(alt_rgba), ptrs(fill_counts), C.c_float(ratio), pp,
                                                              ptrs(frame_rgba)))

    def init_models_batch_frames(self, odoms, pred_v4, pred_n4, pred_rgba, poses, frame_rgba):
        """cf_odom_init_models_batch_frames: one frame image per tracker, no device-side choice"""
        n, oo, pp, ptrs = self._batch_args(odoms, poses)
        self._check(self.lib.cf_odom_init_models_batch_frames(self.h, oo, n, ptrs(pred_v4), ptrs(pred_n4), ptrs(pred_rgba), pp, ptrs(frame_rgba)))

    def init_models_batch(self, odoms, pred_v4, pred_n4, pred_rgba, poses, frame_rgba):
        """cf_odom_init_models_batch: all trackers track the one frame image"""
        n, oo, pp, ptrs = self._batch_args(odoms, poses)
        self._check(self.lib.cf_odom_init_models_batch(self.h, oo, n, ptrs(pred_v4), ptrs(pred_n4), ptrs(pred_rgba), pp, _p(frame_rgba)))

    def set_icp_arith(self, mode):
        """rounding specification of the ICP sums: 0 / "product" (default), 1 / "gram" or 2 / "reference" (the reference's own f32 trees and host loop; include/cofusion_hip.h: cf_set_icp_arith)"""
        self._check(self.lib.cf_set_icp_arith(self.h, {"product": 0, "gram": 1, "reference": 2}.get(mode, mode)))

    def profile_enable(self, on=True):
        self._check(self.lib.cf_profile_enable(self.h, int(on)))

    def profile_read(self, reset=True):
        p = Profile()
        self._check(self.lib.cf_profile_read(self.h, C.byref(p), int(reset)))
        return p


class Odometry:
    """Device-resident RGBDOdometry (Core/Utils/RGBDOdometry.h:42-60)."""

    _BUF = {0: (np.float32, 3), 1: (np.float32, 3), 2: (np.float32, 3), 3: (np.float32, 3), 4: (np.float32, 1),
            5: (np.float32, 1), 6: (np.uint8, 1), 7: (np.uint8, 1), 8: (np.uint8, 1), 9: (np.int16, 1),
            10: (np.int16, 1)}

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.h = C.c_void_p()
        ctx._check(ctx.lib.cf_odom_create(ctx.h, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.cf_odom_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def init_icp_model(self, pred_v4, pred_n4, pose):
        self.ctx._check(self.ctx.lib.cf_odom_init_icp_model(self.h, _p(pred_v4), _p(pred_n4),
                                                            _f(np.asarray(pose, np.float32).reshape(16))))

    def init_rgb_model(self, rgba):
        self.ctx._check(self.ctx.lib.cf_odom_init_rgb_model(self.h, _p(rgba)))

    def set_band(self, row_begin, row_end, add_counts=1):
        """this rank's rows of the model's reductions (cf_odom_set_band); (0, 0): all rows, no collective"""
        self.ctx._check(self.ctx.lib.cf_odom_set_band(self.h, int(row_begin), int(row_end), int(add_counts)))

    def set_culling(self, on=True):
        self.ctx._check(self.ctx.lib.cf_odom_set_culling(self.h, int(bool(on))))

    def init_rgb(self, rgba):
        self.ctx._check(self.ctx.lib.cf_odom_init_rgb(self.h, _p(rgba)))

    def init_first_rgb(self, rgba):
        self.ctx._check(self.ctx.lib.cf_odom_init_first_rgb(self.h, _p(rgba)))

    def init_icp(self, depth_pyr, cutoff):
        arr = (C.c_void_p * 3)(*[d.data_ptr() for d in depth_pyr])
        self._keep = depth_pyr
        self.ctx._check(self.ctx.lib.cf_odom_init_icp(self.h, arr, C.c_float(cutoff)))

    def init_icp_maps(self, vertex4, normal4):
        """the frame side from device maps f32 [H, W, 4] (cf_odom_init_icp_maps): the model-to-model tracker"""
        self.ctx._check(self.ctx.lib.cf_odom_init_icp_maps(self.h, _p(vertex4), _p(normal4)))

    def track(self, trans, rot, rgb_only=False, icp_weight=10.0, pyramid=True, fast_odom=False, so3=True,
              err_surface=None):
        t = _f(np.asarray(trans, np.float32).reshape(3))
        r = _f(np.asarray(rot, np.float32).reshape(9))
        opts = TrackOpts(int(rgb_only), int(pyramid), int(fast_odom), int(so3), icp_weight)
        st = TrackStats()
        self.ctx._check(self.ctx.lib.cf_odom_get_incremental_transformation(self.h, t, r, C.byref(opts),
                                                                            _p(err_surface), C.byref(st)))
        return np.array(t, np.float32), np.array(r, np.float32).reshape(3, 3), st

    def fetch(self):
        """cf_odom_fetch_result of the tracking call Context.track_batch enqueued for this tracker -> (trans, rot, stats)"""
        t = (C.c_float * 3)(); r = (C.c_float * 9)()
        st = TrackStats()
        self.ctx._check(self.ctx.lib.cf_odom_fetch_result(self.h, t, r, C.byref(st)))
        return np.array(t, np.float32), np.array(r, np.float32).reshape(3, 3), st

    def level0_visited(self):
        """cf_odom_level0_visited -> (icp_pixels, residual_pixels) of the last fetched tracking call"""
        a = C.c_uint64(); b = C.c_uint64()
        self.ctx._check(self.ctx.lib.cf_odom_level0_visited(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_launch_shape(self):
        """cf_odom_last_launch_shape -> (icp_blocks[3], residual_blocks[3], icp_blocks_err) of the last tracking call"""
        a = (C.c_int * 3)(); b = (C.c_int * 3)(); e = C.c_int()
        self.ctx._check(self.ctx.lib.cf_odom_last_launch_shape(self.h, a, b, C.byref(e)))
        return list(a), list(b), e.value

    def share_frame_maps(self, owner):
        """cf_odom_share_frame_maps: track against the current-frame pyramids `owner` computed with init_icp"""
        self.ctx._check(self.ctx.lib.cf_odom_share_frame_maps(self.h, owner.h))

    def bench_icp(self, level, iters=200):
        us = C.c_float()
        self.ctx._check(self.ctx.lib.cf_odom_bench_icp(self.h, level, iters, C.byref(us)))
        return us.value

    def buffer_address(self, which, level):
        """device address of an internal buffer (cf_odom_buffer); which == 0 has the side effect described in the header"""
        ptr = C.c_void_p()
        self.ctx._check(self.ctx.lib.cf_odom_buffer(self.h, which, level, C.byref(ptr), None))
        return ptr.value

    def buffer(self, which, level):
        """host copy of an internal buffer (cf_odom_buffer: 0..12 as the oracle numbers them, 13 cand, 14 zrange, 15 occ, 16 aabb)"""
        ptr = C.c_void_p(); nbytes = C.c_uint64()
        self.ctx._check(self.ctx.lib.cf_odom_buffer(self.h, which, level, C.byref(ptr), C.byref(nbytes)))
        host = np.empty(nbytes.value, np.uint8)
        self.ctx._check(self.ctx.lib.cf_memcpy_d2h(self.ctx.h, host.ctypes.data_as(C.c_void_p), ptr, nbytes))
        w, h = self.ctx.width >> level, self.ctx.height >> level
        if which == 11:
            return host.view(np.float32).reshape(h, w, 3)
        if which == 12:
            return host.view(DATATERM).reshape(h * w)
        if which == 13:
            return host.reshape(h, w)
        if which == 14:
            return host.view(np.float32).reshape((h * w + 63) // 64, 2)
        if which == 15:
            return host.reshape(self.ctx.height // 4, self.ctx.width // 4)
        if which == 16:
            return host.view(np.uint32)
        dt, planes = self._BUF[which]
        return host.view(dt).reshape(planes * h, w)


class FrameDecoder:
    """cf_frame_decoder (csrc/frame_decode.hip): finishes the frames of a .klg log on the device.  A slot's pinned staging is filled
    through the numpy views of `slot(s)`, `submit` copies and launches on the decoder's own stream, `acquire` returns the output
    frame as torch tensors VIEWING the decoder's buffers (depth f32 [H, W], rgba u8 [H, W, 4]), valid until the slot's next submit."""

    def __init__(self, ctx: Context, max_w, max_h, slots=4):
        from . import klg as _klg
        self._klg = _klg
        self.ctx, self.lib = ctx, ctx.lib
        self.max_w, self.max_h, self.slots = int(max_w), int(max_h), int(slots)
        self.lib.cf_frame_decoder_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.cf_frame_decoder_destroy.argtypes = [C.c_void_p]
        self.lib.cf_frame_decoder_destroy.restype = None
        self.lib.cf_frame_decoder_slot.argtypes = [C.c_void_p, C.c_int, C.POINTER(_klg.FrameSlot)]
        self.lib.cf_frame_decoder_submit.argtypes = [C.c_void_p, C.c_int, C.POINTER(_klg.FrameDesc)]
        self.lib.cf_frame_decoder_acquire.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        self.lib.cf_frame_decoder_timing.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        from . import images as _im
        self._im = _im
        self.lib.cf_frame_decoder_enable_images.argtypes = [C.c_void_p]
        self.lib.cf_frame_decoder_image_slot.argtypes = [C.c_void_p, C.c_int, C.POINTER(_im.ImageSlot)]
        self.lib.cf_frame_decoder_submit_images.argtypes = [C.c_void_p, C.c_int, C.POINTER(_im.ImageDesc)]
        self.lib.cf_frame_decoder_acquire_mask.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.cf_frame_decoder_image_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        self.h = C.c_void_p()
        ctx._check(self.lib.cf_frame_decoder_create(ctx.h, self.max_w, self.max_h, self.slots, C.byref(self.h)))
        self._size = {}

    def slot(self, s):
        """numpy views of slot s's pinned staging: dict(header=JpegHeader (in place), coef int16 [blocks, 64], depth u16 [max_h*max_w],
        rgb u8 [max_h*max_w*3])"""
        m = self._klg.FrameSlot()
        self.ctx._check(self.lib.cf_frame_decoder_slot(self.h, int(s), C.byref(m)))
        n = self.max_w * self.max_h
        return dict(header=m.header.contents, coef=np.ctypeslib.as_array(m.coef, shape=(int(m.coef_blocks), 64)),
                    depth=np.ctypeslib.as_array(m.depth, shape=(n,)), rgb=np.ctypeslib.as_array(m.rgb, shape=(n * 3,)))

    def fill(self, s, width, height, depth_mm, kind, colour=None):
        """stage a frame in slot s: depth_mm u16 [H, W]; colour = (JpegHeader, coef) for COLOR_JPEG, u8 [H, W, 3] for COLOR_RAW /
        COLOR_DECODED"""
        m = self.slot(s)
        n = width * height
        m["depth"][:n] = np.ascontiguousarray(depth_mm, np.uint16).reshape(n)
        if kind == self._klg.COLOR_JPEG:
            hd, coef = colour
            C.memmove(C.byref(m["header"]), C.byref(hd), C.sizeof(hd))
            m["coef"][:hd.total_blocks] = np.ascontiguousarray(coef, np.int16).reshape(hd.total_blocks, 64)
        elif kind != self._klg.COLOR_NONE:
            m["rgb"][:n * 3] = np.ascontiguousarray(colour, np.uint8).reshape(n * 3)

    def submit(self, s, width, height, kind, flip_colors=False):
        d = self._klg.FrameDesc(int(width), int(height), int(kind), int(bool(flip_colors)))
        self.ctx._check(self.lib.cf_frame_decoder_submit(self.h, int(s), C.byref(d)))
        self._size[int(s)] = (int(height), int(width))

    def acquire(self, s, complete=True):
        dp, cp = C.c_void_p(), C.c_void_p()
        self.ctx._check(self.lib.cf_frame_decoder_acquire(self.h, int(s), int(bool(complete)), C.byref(dp), C.byref(cp)))
        H, W = self._size[int(s)]
        dev = self.ctx.device

        def view(ptr, shape, typestr):
            holder = type("_DevView", (), {})()
            holder.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(int(ptr), False), version=2)
            return torch.as_tensor(holder, device=dev)

        return view(dp.value, (H, W), "<f4"), view(cp.value, (H, W, 4), "|u1")

    # ---- image-sequence frames (csrc/image_decode.hip) ----
    def enable_images(self):
        """allocate the image staging of every slot (once); without it the image entries are refused"""
        self.ctx._check(self.lib.cf_frame_decoder_enable_images(self.h))

    def image_slot(self, s):
        """slot s's pinned image staging: the ImageSlot itself and numpy views dict(color, depth, mask, palette u8; blocks EXR_BLOCK)"""
        _im = self._im
        m = _im.ImageSlot()
        self.ctx._check(self.lib.cf_frame_decoder_image_slot(self.h, int(s), C.byref(m)))
        v = dict(color=np.ctypeslib.as_array(m.color, shape=(int(m.color_bytes),)), depth=np.ctypeslib.as_array(m.depth, shape=(int(m.depth_bytes),)),
                 mask=np.ctypeslib.as_array(m.mask, shape=(int(m.mask_bytes),)), palette=np.ctypeslib.as_array(m.palette, shape=(768,)),
                 blocks=np.ctypeslib.as_array(C.cast(m.blocks, C.POINTER(C.c_uint32)), shape=(int(m.max_blocks), 4)))
        return m, v

    def submit_images(self, s, desc):
        """cf_frame_decoder_submit_images with an images.ImageDesc the caller filled beside the slot's staging"""
        self.ctx._check(self.lib.cf_frame_decoder_submit_images(self.h, int(s), C.byref(desc)))
        self._size[int(s)] = (int(desc.height), int(desc.width))

    def submit_image_files(self, s, color=None, depth=None, mask=None, flip_colors=False, depth_scale=None, size=None):
        """Stage the files of one frame in slot s and submit it: what a worker of the image player does.  Each plane is (ext, bytes) or
        None: color ".png" / ".jpg" / ".ppm", depth ".png" / ".exr", mask ".png" / ".pgm".  The host parsers (cofusion_png_decode,
        cofusion_exr_decode, cofusion_jpeg_front) write straight into the pinned staging.  size = (W, H) where no PNG / EXR / PNM
        plane gives it.  Returns the ImageDesc."""
        _im, host = self._im, self._im._host()
        m, v = self.image_slot(s)
        d = _im.ImageDesc()
        d.flip_colors = int(bool(flip_colors))
        d.depth_scale = _im.DEFAULT_DEPTH_SCALE if depth_scale is None else float(depth_scale)
        dims = [tuple(size)] if size else []

        def png(data, role, dst, cap, palette=None):
            info = _im.PngInfo()
            data = bytes(data)
            if host.cofusion_png_decode(data, C.c_uint64(len(data)), role, C.byref(info), dst, C.c_uint64(cap), palette) != 0:
                raise CofusionError(host.cofusion_last_error().decode())
            dims.append((info.width, info.height))
            return info

        if depth is not None and depth[0] == ".png":
            png(depth[1], _im.ROLE_DEPTH, m.depth, m.depth_bytes)
            d.depth_kind = _im.IMAGE_PNG
        elif depth is not None:
            info, data = _im.ExrInfo(), bytes(depth[1])
            if host.cofusion_exr_decode(data, C.c_uint64(len(data)), C.byref(info), m.depth, C.c_uint64(m.depth_bytes), m.blocks, C.c_uint64(m.max_blocks)) != 0:
                raise CofusionError(host.cofusion_last_error().decode())
            dims.append((info.width, info.height))
            d.depth_kind = _im.IMAGE_EXR
            d.exr_blocks, d.exr_lines_per_block, d.exr_line_bytes = info.blocks, info.lines_per_block, info.line_bytes
            d.exr_chan_offset, d.exr_chan_half = info.chan_offset, info.chan_half
        if mask is not None and mask[0] == ".png":
            png(mask[1], _im.ROLE_MASK, m.mask, m.mask_bytes)
            d.mask_kind = _im.IMAGE_PNG
        elif mask is not None:
            from . import masks as _masks
            g = _masks.parse_pgm(bytes(mask[1]))
            dims.append((g.shape[1], g.shape[0]))
            v["mask"][:g.size] = g.reshape(-1)
            d.mask_kind = _im.IMAGE_RAW
        if color is not None and color[0] == ".png":
            info = png(color[1], _im.ROLE_COLOR, m.color, m.color_bytes, m.palette)
            d.color_kind, d.png_color_type, d.png_palette_entries = _im.IMAGE_PNG, info.color_type, info.palette_entries
        elif color is not None and color[0] == ".ppm":
            rgb = _im.decode_ppm(color[1])
            dims.append((rgb.shape[1], rgb.shape[0]))
            self.slot(s)["rgb"][:rgb.size] = rgb.reshape(-1)
            d.color_kind = _im.IMAGE_RAW
        elif color is not None:
            W, H = dims[0]
            ks = self._klg.FrameSlot()
            self.ctx._check(self.lib.cf_frame_decoder_slot(self.h, int(s), C.byref(ks)))
            data = bytes(color[1])
            rc = host.cofusion_jpeg_front(data, C.c_uint64(len(data)), W, H, ks.header, ks.coef, C.c_uint64(ks.coef_blocks))
            if rc != 0:
                raise CofusionError("JPEG front end: " + (host.cofusion_last_error().decode() if rc < 0 else "refused"))
            d.color_kind = _im.IMAGE_JPEG
        if len(set(dims)) != 1:
            raise CofusionError(f"the planes of the frame differ in size: {dims}")
        d.width, d.height = dims[0]
        self.submit_images(s, d)
        return d

    def acquire_mask(self, s, complete=True):
        """the u8 mask [H, W] of the slot's last image frame as a torch tensor viewing the decoder's buffer, None where it had none"""
        mp = C.c_void_p()
        self.ctx._check(self.lib.cf_frame_decoder_acquire_mask(self.h, int(s), int(bool(complete)), C.byref(mp)))
        if not mp.value:
            return None
        H, W = self._size[int(s)]
        holder = type("_DevView", (), {})()
        holder.__cuda_array_interface__ = dict(shape=(H, W), typestr="|u1", data=(int(mp.value), False), version=2)
        return torch.as_tensor(holder, device=self.ctx.device)

    def image_timing(self):
        """device-event durations of the two image kernels over the image frames submitted while timing(True) was on:
        (exr_depth_kernel ms, frames that launched it, png_finish_kernel ms, frames that launched it); resets the sums"""
        a, na, b, nb = C.c_double(), C.c_uint64(), C.c_double(), C.c_uint64()
        self.ctx._check(self.lib.cf_frame_decoder_image_timing(self.h, C.byref(a), C.byref(na), C.byref(b), C.byref(nb)))
        return a.value, na.value, b.value, nb.value

    def timing(self, on=True):
        """kernel durations from device events accumulated while timing was on: (idct ms, finish ms, frames); resets the sums"""
        a, b, n = C.c_double(), C.c_double(), C.c_uint64()
        self.ctx._check(self.lib.cf_frame_decoder_timing(self.h, int(bool(on)), C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.cf_frame_decoder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PngBand(C.Structure):
    _fields_ = [("offset", C.c_uint32), ("bytes", C.c_uint32), ("adler", C.c_uint32), ("stream_bytes", C.c_uint32)]


class PngStream(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("rows_per_band", C.c_int32), ("bands", C.c_int32),
                ("table", C.POINTER(PngBand)), ("data", C.POINTER(C.c_uint8)), ("data_bytes", C.c_uint64)]


PNG_LABELS = 1


class PngEncoder:
    """cf_png_encoder (csrc/png_encode.hip): a device image (torch CUDA u8 [H, W] or [H, W, 4]) becomes the bands of a PNG data stream
    in a pinned slot.  `submit` enqueues on the context's stream without a host wait; `acquire` waits for the slot and returns the
    stream's description plus the bands as bytes objects with their (adler, stream_bytes) -- the host's part (chunk framing, CRC) is
    host/ExportWriter.cpp's, or the caller's."""

    def __init__(self, ctx: Context, max_w, max_h, slots=2, rows_per_band=8):
        self.ctx, self.lib = ctx, ctx.lib
        self.lib.cf_png_encoder_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.cf_png_encoder_destroy.argtypes = [C.c_void_p]
        self.lib.cf_png_encoder_destroy.restype = None
        self.lib.cf_png_encoder_submit.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        self.lib.cf_png_encoder_acquire.argtypes = [C.c_void_p, C.c_int, C.POINTER(PngStream)]
        self.lib.cf_png_encoder_timing.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        self.h = C.c_void_p()
        ctx._check(self.lib.cf_png_encoder_create(ctx.h, int(max_w), int(max_h), int(slots), int(rows_per_band), C.byref(self.h)))

    def submit(self, s, image, flags=0):
        if image.dtype != torch.uint8 or not image.is_cuda or not image.is_contiguous() or image.dim() not in (2, 3):
            raise CofusionError("PngEncoder.submit: a contiguous CUDA uint8 tensor [H, W] or [H, W, 4] is expected")
        channels = 1 if image.dim() == 2 else int(image.shape[2])
        self.submit_ptr(s, image.data_ptr(), int(image.shape[1]), int(image.shape[0]), channels, flags)

    def submit_ptr(self, s, ptr, width, height, channels, flags=0):
        self.ctx._check(self.lib.cf_png_encoder_submit(self.h, int(s), C.c_void_p(ptr), int(width), int(height), int(channels), int(flags)))

    def acquire(self, s):
        """(PngStream, [(bytes of the band, adler, stream_bytes)])"""
        st = PngStream()
        self.ctx._check(self.lib.cf_png_encoder_acquire(self.h, int(s), C.byref(st)))
        bands = []
        for k in range(st.bands):
            b = st.table[k]
            if b.offset + b.bytes > st.data_bytes:
                raise CofusionError("PngEncoder.acquire: a band lies outside the slot")
            bands.append((C.string_at(C.addressof(st.data.contents) + b.offset, b.bytes), int(b.adler), int(b.stream_bytes)))
        return st, bands

    def timing(self, on=True):
        """(kernel ms, images) from device events accumulated while timing was on; resets the sums"""
        a, n = C.c_double(), C.c_uint64()
        self.ctx._check(self.lib.cf_png_encoder_timing(self.h, int(bool(on)), C.byref(a), C.byref(n)))
        return a.value, n.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.cf_png_encoder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
