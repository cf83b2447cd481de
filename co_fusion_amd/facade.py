"""ctypes binding of the C++ facade (libcofusion.so, include/cofusion.h): the reference's
`CoFusion` object as GUI/MainController.cpp drives it (construct, processFrame, getters)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import lib as _libmod
from .api import Profile


class Config(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("device", C.c_int), ("max_surfels", C.c_int), ("max_models", C.c_int), ("conf_global_init", C.c_float),
                ("conf_object_init", C.c_float), ("depth_cutoff", C.c_float), ("icp_weight", C.c_float),
                ("outlier_coefficient", C.c_float), ("fast_odom", C.c_int), ("so3", C.c_int), ("frame_to_frame_rgb", C.c_int),
                ("pyramid", C.c_int), ("rgb_only", C.c_int), ("model_spawn_offset", C.c_uint), ("enable_multiple_models", C.c_int),
                ("enable_pose_logging", C.c_int), ("rank", C.c_int), ("world", C.c_int), ("device_frames_complete", C.c_int),
                ("mid_frame_predict", C.c_int), ("shard_background", C.c_int), ("enqueue_threads", C.c_int),
                ("colocate_background", C.c_int), ("reloc", C.c_int), ("early_index_maps", C.c_int), ("time_delta", C.c_int)]


class RedetectCandidate(C.Structure):
    """cofusion_redetect_candidate (include/cofusion.h)"""
    _fields_ = [("id", C.c_uint), ("projected", C.c_uint32), ("occluded", C.c_uint32), ("seen_through", C.c_uint32), ("agree", C.c_uint32),
                ("agree_on_label", C.c_uint32), ("covered", C.c_uint32), ("fit", C.c_float), ("cover", C.c_float), ("eligible", C.c_int)]


class RedetectSearchCandidate(C.Structure):
    """cofusion_redetect_search_candidate (include/cofusion.h)"""
    _fields_ = [("id", C.c_uint), ("colour", C.c_float), ("registered", C.c_int), ("converged", C.c_int), ("iterations", C.c_int),
                ("first_inliers", C.c_uint32), ("last_inliers", C.c_uint32), ("rms", C.c_float), ("moved", C.c_float),
                ("projected", C.c_uint32), ("occluded", C.c_uint32), ("seen_through", C.c_uint32), ("agree", C.c_uint32),
                ("agree_on_label", C.c_uint32), ("covered", C.c_uint32), ("fit", C.c_float), ("cover", C.c_float), ("eligible", C.c_int)]


class CoFusionError(RuntimeError):
    pass


class _DevWords:
    """a device address as an int64 array (the __cuda_array_interface__ protocol): torch.as_tensor turns it into a tensor VIEW of the
    library's buffer, so that torch.distributed reduces it in place -- no staging copies"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(int(n),), typestr="<i8", data=(int(ptr), False), version=2)


def rccl_unique_id():
    """ncclGetUniqueId through the facade (128 bytes): rank 0 creates it, every rank passes it to CoFusion.init_rccl"""
    lib = _libmod.load_host()
    buf = (C.c_ubyte * 128)()
    if lib.cofusion_rccl_unique_id(buf) != 0:
        raise CoFusionError(f"cofusion_rccl_unique_id: {lib.cofusion_last_error().decode()}")
    return bytes(buf)


def _check_mask_tensor(mask, depth_t):
    if mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous() or tuple(mask.shape) != tuple(depth_t.shape):
        raise CoFusionError("mask: a contiguous CUDA uint8 tensor of the depth image's shape is expected")
    if mask.data_ptr() % 16:
        raise CoFusionError("mask: the tensor's storage must be 16-byte aligned")


def _make_config(lib, width, height, fx, fy, cx, cy, device, kw):
    cfg = Config()
    lib.cofusion_default_config(C.byref(cfg))
    cfg.width, cfg.height, cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.device = width, height, fx, fy, cx, cy, device
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown CoFusion option {k}")
        setattr(cfg, k, v)
    return cfg


class CoFusion:
    def __init__(self, width=640, height=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, device=0, _borrowed=None, **kw):
        if not torch.cuda.is_available():
            raise CoFusionError("no GPU visible: the Co-Fusion hot path has no CPU fallback")
        self.lib = _libmod.load_host()
        self.abi = _libmod.load()
        cfg = _make_config(self.lib, width, height, fx, fy, cx, cy, device, kw)
        self.cfg = cfg
        self.width, self.height = width, height
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self._owned = _borrowed is None
        if _borrowed is not None:   # a sequence of a CoFusionGroup: the handle belongs to the group
            self.h = C.c_void_p(_borrowed)
            return
        self.h = C.c_void_p()
        self._check(self.lib.cofusion_create(C.byref(cfg), C.byref(self.h)))
        self._check(self.lib.cofusion_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _check(self, rc):
        if rc != 0:
            raise CoFusionError(f"cofusion error {rc}: {self.lib.cofusion_last_error().decode()}")

    def init_rccl(self, unique_id=None):
        """The library's own RCCL communicator as this instance's collective (cofusion_init_rccl): ncclAllReduce / ncclBroadcast in
        place on the context's stream, no Python in the frame loop.  unique_id: the 128 bytes rank 0 got from rccl_unique_id(); None:
        created on rank 0 and distributed through the default torch.distributed process group.  Collective call (every rank)."""
        if unique_id is None:
            import torch.distributed as dist
            cuda = dist.get_backend() == "nccl"
            t = torch.zeros(128, dtype=torch.uint8)
            if self.cfg.rank == 0:
                t = torch.frombuffer(bytearray(rccl_unique_id()), dtype=torch.uint8).clone()
            if cuda:
                t = t.to(self.device)
            dist.broadcast(t, src=0)
            unique_id = bytes(t.cpu().numpy().tobytes())
        assert len(unique_id) == 128
        self._check(self.lib.cofusion_init_rccl(self.h, C.c_char_p(unique_id)))
        self.rccl = True

    def broadcast(self, tensor, root=0):
        """a device tensor (a frame: depth + colour in one buffer) from rank `root` to every rank: ncclBroadcast on the context's stream"""
        self._check(self.lib.cofusion_broadcast(self.h, C.c_void_p(tensor.data_ptr()), C.c_uint64(tensor.numel() * tensor.element_size()), int(root)))

    def set_allreduce(self, fn=None):
        """model-parallel mode (rank / world given at construction): register the SUM all-reduce of int64 buffers.
        Default: torch.distributed.all_reduce on the default process group (gloo: CPU tensor, nccl: staged through the GPU)."""
        import torch.distributed as dist

        def default(arr):
            t = torch.from_numpy(arr)
            if dist.get_backend() == "nccl":
                g = t.to(self.device)
                dist.all_reduce(g, op=dist.ReduceOp.SUM)
                t.copy_(g.cpu())
            else:
                dist.all_reduce(t, op=dist.ReduceOp.SUM)

        impl = fn or default

        def thunk(buf, n, _user):
            try:
                impl(np.ctypeslib.as_array(buf, shape=(n,)))
                return 0
            except Exception:  # noqa: BLE001 -- reported through the C return code
                return -1

        self._allreduce_cb = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_int64), C.c_uint64, C.c_void_p)(thunk)  # keep alive
        self._check(self.lib.cofusion_set_allreduce(self.h, self._allreduce_cb, None))
        if fn is None:
            self.set_allreduce_device()   # nccl: RCCL on the stream; gloo (dry runs): the same path, staged by gloo itself
            if self.cfg.shard_background:
                self.set_collective()

    def set_collective(self):
        """C-ABI level collective (cf_set_collective) for a background split over the ranks (shard_background=1): op 0 = SUM of int64 words
        (the normal-equation accumulators, after every launch of the Gauss-Newton loop), op 1 = MIN of unsigned 64-bit words (the z-keys
        of the index map).  torch.distributed in place on a tensor view of the library's buffer, on the stream the library hands over."""
        import torch.distributed as dist
        sign = torch.tensor(-2 ** 63, dtype=torch.int64, device=self.device)

        def thunk(_user, op, dev_buf, words, hip_stream):
            try:
                t = torch.as_tensor(_DevWords(dev_buf, words), device=self.device)   # a view of the library's buffer: reduced in place
                stream = torch.cuda.ExternalStream(int(hip_stream), device=self.device) if hip_stream else torch.cuda.current_stream(self.device)
                with torch.cuda.stream(stream):   # everything on the stream the library enqueues this model's work on
                    if op == 0:
                        dist.all_reduce(t, op=dist.ReduceOp.SUM)
                    else:  # unsigned order through the signed collective: flip the sign bit, MIN, flip back
                        t.bitwise_xor_(sign)
                        dist.all_reduce(t, op=dist.ReduceOp.MIN)
                        t.bitwise_xor_(sign)
                return 0
            except Exception:  # noqa: BLE001 -- reported through the C return code
                import traceback
                traceback.print_exc()
                return -1

        self._collective_cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p)(thunk)  # keep alive
        assert self.abi.cf_set_collective(self._ctx(), self._collective_cb, None) == 0

    def set_allreduce_device(self):
        """The collective for buffers that live in HBM (per-superpixel segmentation sums): RCCL all-reduce of an int64 torch tensor,
        enqueued after the library's work on the context's stream -- no host visit.  torch.distributed takes tensors, not raw
        addresses: the library's buffer is wrapped as a tensor VIEW (_DevWords) and reduced in place.  This is the path of process groups
        that are not RCCL (the gloo tests on a one-GPU box); with RCCL use init_rccl (the library's own communicator)."""
        import torch.distributed as dist

        def thunk(dev_buf, n, hip_stream, _user):
            try:
                t = torch.as_tensor(_DevWords(dev_buf, n), device=self.device)   # a view of the library's buffer: reduced in place
                # the library enqueues on the torch stream it was handed (set_stream / the current stream at construction)
                stream = torch.cuda.ExternalStream(int(hip_stream), device=self.device) if hip_stream else torch.cuda.current_stream(self.device)
                with torch.cuda.stream(stream):
                    dist.all_reduce(t, op=dist.ReduceOp.SUM)
                return 0
            except Exception:  # noqa: BLE001 -- reported through the C return code
                import traceback
                traceback.print_exc()
                return -1

        self._allreduce_dev_cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p)(thunk)  # keep alive
        self._check(self.lib.cofusion_set_allreduce_device(self.h, self._allreduce_dev_cb, None))

    def model_owned(self, index):
        return self.lib.cofusion_model_owned(self.h, index) == 1

    def set_stream(self, stream):
        """enqueue all work of this instance on a torch.cuda.Stream (or a raw hipStream_t value)"""
        ptr = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
        self._check(self.lib.cofusion_set_stream(self.h, C.c_void_p(ptr)))

    def save_ply(self, prefix):
        """CoFusion::savePly: <prefix>cloud-<id>.ply per model; returns the number of files"""
        n = self.lib.cofusion_save_ply(self.h, str(prefix).encode())
        if n < 0:
            raise CoFusionError(self.lib.cofusion_last_error().decode())
        return n

    def save_mesh(self, prefix, voxel=0.0):
        """CoFusion::saveMesh: <prefix>mesh-<id>.ply per model, a triangle mesh of its confident surfels extracted on the device
        (voxel 0: the model's mean confident radius); returns the number of files"""
        self.lib.cofusion_save_mesh.argtypes = [C.c_void_p, C.c_char_p, C.c_float]
        n = self.lib.cofusion_save_mesh(self.h, str(prefix).encode(), float(voxel))
        if n < 0:
            raise CoFusionError(self.lib.cofusion_last_error().decode())
        return n

    def model_mesh(self, index, voxel=0.0, with_transform=False):
        """one model's mesh in the model's own frame: (vertices, triangles) -- records of co_fusion_amd.mesh.VERTEX (pos, nrm f32 x 3,
        rgba u8 x 4) and u32 [T, 3].  index >= 0: the active models (0 = background); index < 0: the kept inactive model -1 - index.
        with_transform: also the 4x4 Tp = globalPose * modelPose^-1 that save_mesh applies."""
        from .mesh import VERTEX
        f = self.lib.cofusion_model_mesh
        f.argtypes = [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        nv, nt = C.c_uint32(), C.c_uint32()
        tp = np.zeros((4, 4), np.float32)
        self._check(f(self.h, int(index), float(voxel), C.byref(nv), C.byref(nt), None, 0, None, 0, tp.ctypes.data_as(C.c_void_p)))
        v = np.zeros(nv.value, VERTEX)
        t = np.zeros((nt.value, 3), np.uint32)
        if nv.value:
            self._check(f(self.h, int(index), float(voxel), C.byref(nv), C.byref(nt), v.ctypes.data_as(C.c_void_p), len(v), t.ctypes.data_as(C.c_void_p),
                          len(t), None))
        return (v, t, tp) if with_transform else (v, t)

    def set_mesh_max_voxels(self, max_voxels):
        """grid samples the mesher is created for (default 2^24, 64 bytes each); the default grid's voxel grows until the map fits"""
        self.lib.cofusion_set_mesh_max_voxels.argtypes = [C.c_void_p, C.c_uint64]
        self._check(self.lib.cofusion_set_mesh_max_voxels(self.h, int(max_voxels)))

    def set_export_segmentation(self, prefix):
        """every segmented frame writes <prefix>Segmentation<tick>.png (labels, rejected superpixels as 0); '' switches it off"""
        self._check(self.lib.cofusion_set_export_segmentation(self.h, str(prefix or "").encode()))

    def render(self, pose=None, intrinsics=None, size=None, near=0.0, far=0.0, background_mode=2, object_mode=4, flags=0,
               depth=False, labels=False, as_torch=False):
        """CoFusion::renderScene: every active model drawn into one view (DESIGN.md "Scene rendering").  pose: camera -> world 4x4
        (None: the current camera), intrinsics (fx, fy, cx, cy) and size (w, h) default to the frame's.  Colour modes and flags as
        co_fusion_amd.render (GREY .. LABEL; UNSTABLE | WINDOW | PHONG).  Returns rgba u8 [h, w, 4], plus depth f32 [h, w] (0 = empty)
        and labels u8 [h, w] (255 = empty) when asked for: numpy arrays, or torch tensors on the device with as_torch=True."""
        from .render import make_view
        view = None
        if pose is not None or intrinsics is not None or size is not None or near or far:
            cur = self.model_info(0)["pose"] if pose is None else pose   # (the background's pose is the camera's)
            fx, fy, cx, cy = intrinsics if intrinsics is not None else (self.cfg.fx, self.cfg.fy, self.cfg.cx, self.cfg.cy)
            w, h = size if size is not None else (self.width, self.height)
            view = make_view(cur, fx, fy, cx, cy, w, h, near, far)
        w, h = (view.width, view.height) if view is not None else (self.width, self.height)
        vref = C.byref(view) if view is not None else None
        if as_torch:
            r = C.c_void_p(); d = C.c_void_p(); lb = C.c_void_p()
            self._check(self.lib.cofusion_render_device(self.h, vref, int(background_mode), int(object_mode), int(flags), C.byref(r),
                                                        C.byref(d), C.byref(lb)))
            out = [(r, torch.empty((h, w, 4), dtype=torch.uint8, device=self.device))]
            if depth:
                out.append((d, torch.empty((h, w), dtype=torch.float32, device=self.device)))
            if labels:
                out.append((lb, torch.empty((h, w), dtype=torch.uint8, device=self.device)))
            ctx = self._ctx()
            for src, t in out:
                assert self.abi.cf_memcpy_d2d_async(ctx, C.c_void_p(t.data_ptr()), src, C.c_uint64(t.numel() * t.element_size())) == 0
            assert self.abi.cf_synchronize(ctx) == 0
            res = [t for _, t in out]
        else:
            rgba = np.empty((h, w, 4), np.uint8)
            dep = np.empty((h, w), np.float32) if depth else None
            lab = np.empty((h, w), np.uint8) if labels else None
            ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
            self._check(self.lib.cofusion_render(self.h, vref, int(background_mode), int(object_mode), int(flags), ptr(rgba), ptr(dep),
                                                 ptr(lab)))
            res = [a for a in (rgba, dep, lab) if a is not None]
        return res[0] if len(res) == 1 else tuple(res)

    def set_export_views(self, prefix, labels=False, normals=False, viewport=False):
        """after every processed frame write <prefix>Labels<n>.png / Normals<n>.png / Viewport<n>.png (RGBA) from the current camera,
        <n> as in Segmentation<n>.png (the reference's head-less -el / -en / -ev); all False switches it off"""
        which = (1 if labels else 0) | (2 if normals else 0) | (4 if viewport else 0)
        self._check(self.lib.cofusion_set_export_views(self.h, str(prefix or "").encode(), which))

    def set_export_async(self, on=True, workers=2, slots=8):
        """the per-frame exports (set_export_segmentation, set_export_views) through the device PNG encoder and `workers` (1..8)
        writer threads: same file names, numbering and pixels, no read-back or zlib on the frame thread.  The frame loop waits only
        when all `slots` (2..16) are busy; a failed write raises from the next process_frame* or from export_flush."""
        self._check(self.lib.cofusion_set_export_async(self.h, int(bool(on)), int(workers), int(slots)))

    def export_flush(self):
        """returns when every exported file submitted so far is closed"""
        self._check(self.lib.cofusion_export_flush(self.h))

    def export_stats(self, timing=False):
        """dict(images, bytes, stalls, device_ms, device_images) of the asynchronous exports; timing: measure the encoding kernel with
        device events from here on (device_ms / device_images cover the images since the last call)"""
        im, by, stl, n = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        ms = C.c_double()
        self._check(self.lib.cofusion_export_stats(self.h, C.byref(im), C.byref(by), C.byref(stl), C.byref(ms), C.byref(n), int(bool(timing))))
        return dict(images=im.value, bytes=by.value, stalls=stl.value, device_ms=ms.value, device_images=n.value)

    def export_poses(self, prefix):
        """CoFusion::exportPoses: <prefix>poses-<id>.txt per logged model (needs enable_pose_logging=1)"""
        n = self.lib.cofusion_export_poses(self.h, str(prefix).encode())
        if n < 0:
            raise CoFusionError(self.lib.cofusion_last_error().decode())
        return n

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "_owned", True):
                self.lib.cofusion_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_crf(self, unary_weight_error=75.0, unary_k_error=0.0375, threshold_new=5.5, weight_appearance=7.0, weight_smoothness=2.0,
                sigma_rgb=10.0, sigma_depth=0.9, sigma_pos=1.8, min_rel_size_new=0.015, max_rel_size_new=0.4, iterations=10):
        f = C.c_float
        self._check(self.lib.cofusion_set_crf(self.h, f(unary_weight_error), f(unary_k_error), f(threshold_new), f(weight_appearance),
                                              f(weight_smoothness), f(sigma_rgb), f(sigma_depth), f(sigma_pos), f(min_rel_size_new),
                                              f(max_rel_size_new), C.c_uint(iterations)))

    def set_seg_early(self, on=True):
        """The motion segmentation's tracking-independent half beside the tracking launches (default on); the results do not depend on it."""
        self._check(self.lib.cofusion_set_seg_early(self.h, 1 if on else 0))

    def process_frame(self, depth, rgb, mask=None, in_pose=None, timestamp=0):
        """Host numpy inputs: depth f32 [H,W] metres, rgb u8 [H,W,3], optional GT mask u8 [H,W]."""
        d = np.ascontiguousarray(depth, np.float32); c = np.ascontiguousarray(rgb, np.uint8)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        p = None if in_pose is None else np.ascontiguousarray(in_pose, np.float32).reshape(16)
        self._check(self.lib.cofusion_process_frame(self.h, C.c_int64(timestamp), c.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                                    None if m is None else m.ctypes.data_as(C.c_void_p),
                                                    None if p is None else p.ctypes.data_as(C.c_void_p)))

    def process_frame_device(self, depth_t, rgba_t, in_pose=None, timestamp=0, mask=None):
        """Frame already resident in HBM: torch CUDA tensors depth f32 [H,W], rgba u8 [H,W,4]; mask (optional): its label mask, a
        contiguous torch CUDA tensor u8 [H,W] -- the mask branch of the segmentation then runs as kernels (world == 1 only)."""
        p = None if in_pose is None else np.ascontiguousarray(in_pose, np.float32).reshape(16)
        if mask is not None:
            _check_mask_tensor(mask, depth_t)
            self._check(self.lib.cofusion_process_frame_device_masked(self.h, C.c_int64(timestamp), C.c_void_p(depth_t.data_ptr()),
                                                                      C.c_void_p(rgba_t.data_ptr()), C.c_void_p(mask.data_ptr()),
                                                                      None if p is None else p.ctypes.data_as(C.c_void_p)))
            return
        self._check(self.lib.cofusion_process_frame_device(self.h, C.c_int64(timestamp), C.c_void_p(depth_t.data_ptr()),
                                                           C.c_void_p(rgba_t.data_ptr()),
                                                           None if p is None else p.ctypes.data_as(C.c_void_p)))

    def process_frame_device_ptr(self, depth_ptr, rgba_ptr, mask_ptr=None, in_pose=None, timestamp=0):
        """the same with plain device addresses (e.g. the frame klg.KlgPlayer's iteration hands out); mask_ptr: 16-byte aligned or None"""
        p = None if in_pose is None else np.ascontiguousarray(in_pose, np.float32).reshape(16)
        self._check(self.lib.cofusion_process_frame_device_masked(self.h, C.c_int64(timestamp), C.c_void_p(depth_ptr), C.c_void_p(rgba_ptr),
                                                                  C.c_void_p(mask_ptr) if mask_ptr else None,
                                                                  None if p is None else p.ctypes.data_as(C.c_void_p)))

    @property
    def num_models(self):
        return self.lib.cofusion_num_models(self.h)

    @property
    def tick(self):
        return self.lib.cofusion_tick(self.h)

    @property
    def lost(self):
        """CoFusion::getLost: the camera is lost (option reloc=1)"""
        return bool(self.lib.cofusion_is_lost(self.h))

    def set_relocalisation(self, on=True, n_ferns=500, fern_threshold=0.3095, photo_threshold=115.0, min_age=300, seed=0, capacity=1024):
        """The recovery half of reloc=1 (cofusion_set_relocalisation): a fern keyframe database built from the tracked frames, asked for
        a keyframe while the camera is lost.  Defaults are the reference's."""
        self._check(self.lib.cofusion_set_relocalisation(self.h, int(bool(on)), int(n_ferns), C.c_float(fern_threshold), C.c_float(photo_threshold),
                                                         int(min_age), C.c_uint64(seed), int(capacity)))

    def reloc_stats(self):
        k = C.c_int(); c = C.c_int(); r = C.c_int(); f = C.c_int()
        self._check(self.lib.cofusion_reloc_stats(self.h, C.byref(k), C.byref(c), C.byref(r), C.byref(f)))
        return dict(keyframes=k.value, last_closest=c.value, recoveries=r.value, database_full=bool(f.value))

    def deform_background(self, src, dst, src_time, dst_time=None, pin=False, sample_rate=25000):
        """Loop closure of the background map from caller-supplied constraints (cofusion_deform_background): surface
        points src [n, 3] seen at ticks src_time [n] belong at dst [n, 3]; pin: every dst also stays where it is (at tick dst_time).
        The deformation graph is sampled from the map, optimised and, when accepted, applied to every surfel.  -> the optimisation's
        outcome (co_fusion_amd.deform.RESULT_FIELDS) + nodes"""
        from . import deform as _deform
        s = np.ascontiguousarray(src, np.float32).reshape(-1, 3); d = np.ascontiguousarray(dst, np.float32).reshape(-1, 3)
        ts = np.ascontiguousarray(src_time, np.float32).reshape(-1)
        td = None if dst_time is None else np.ascontiguousarray(dst_time, np.float32).reshape(-1)
        assert len(s) == len(d) == len(ts) and (td is None or len(td) == len(s))
        res = _deform.Result(); nodes = C.c_int()
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.cofusion_deform_background(self.h, vp(s), vp(d), vp(ts), vp(td), len(s), int(bool(pin)), int(sample_rate), C.byref(res),
                                                        C.byref(nodes)))
        out = {k: getattr(res, k) for k in _deform.RESULT_FIELDS}
        for k in ("optimised", "accepted", "failed"):
            out[k] = bool(out[k])
        out["nodes"] = nodes.value
        return out

    def set_loop_closure(self, on=True, sample_rate=25000):
        """Global loop closure in the frame loop (cofusion_set_loop_closure): every tracked frame is gated against the
        keyframe database; an accepted fern match deforms the background map from constraints generated on the device, and an accepted
        graph corrects the map, the keyframe poses and the camera pose.  Needs set_relocalisation first."""
        self._check(self.lib.cofusion_set_loop_closure(self.h, int(bool(on)), int(sample_rate)))

    def loop_stats(self):
        """-> frames gated, candidates, fern accepts, graphs optimised / accepted / failed, the last accept's keyframe, its srcTime, node count
        and tick, and its optimisation outcome under `last` (co_fusion_amd.deform.RESULT_FIELDS)"""
        from . import deform as _deform

        class _Stats(C.Structure):
            _fields_ = [(k, C.c_int32) for k in ("gated", "candidates", "fern_accepts", "optimised", "accepted", "failed", "last_keyframe",
                                                "last_keyframe_time", "last_nodes", "last_tick")] + [("last", _deform.Result)]
        s = _Stats()
        self._check(self.lib.cofusion_loop_stats(self.h, C.byref(s)))
        out = {k: getattr(s, k) for k, _ in _Stats._fields_[:-1]}
        last = {k: getattr(s.last, k) for k in _deform.RESULT_FIELDS}
        for k in ("optimised", "accepted", "failed"):
            last[k] = bool(last[k])
        out["last"] = last
        return out

    def set_local_loop_closure(self, on=True, sample_rate=5000, icp_count_thresh=40000, icp_err_thresh=5e-5, cov_thresh=1e-5,
                               min_inactive_pixels=None):
        """Local (model-to-model) loop closure in the frame loop (cofusion_set_local_loop_closure): a tracked frame
        registers the active view of the background map onto the inactive one with a second tracker; an accepted registration deforms
        the map with a graph sampled at `sample_rate`, reactivates the old surfels in view and corrects the camera pose.
        min_inactive_pixels: frames with fewer covered inactive texels stop behind the registration (None: icp_count_thresh; 0: no
        gate).  Needs time_delta > 0; needs no set_relocalisation."""
        f = C.c_float
        self._check(self.lib.cofusion_set_local_loop_closure(self.h, int(bool(on)), int(sample_rate), int(icp_count_thresh), f(icp_err_thresh),
                                                             f(cov_thresh), -1 if min_inactive_pixels is None else int(min_inactive_pixels)))

    def local_loop_stats(self):
        """-> frames examined / skipped by the pixel gate / accepted by the second tracker, graphs optimised / accepted / failed, the last
        accept's node and constraint counts, whether it was pinned and its tick, deforms, last_deform_time, and of the last examined
        frame the covered texels, the accept rule's outcome and figures and the estimated pose [4, 4]; the last optimisation's outcome
        under `last` (co_fusion_amd.deform.RESULT_FIELDS)"""
        from . import deform as _deform
        ints = ("examined", "skipped_by_gate", "tracker_accepts", "optimised", "accepted", "failed", "last_nodes", "last_constraints",
                "last_pinned", "last_tick", "deforms", "last_deform_time")

        class _Stats(C.Structure):
            _fields_ = ([(k, C.c_int32) for k in ints] + [("last_covered", C.c_uint32), ("last_tracker_accepted", C.c_int32),
                        ("last_icp_error", C.c_float), ("last_icp_count", C.c_float), ("last_max_covariance", C.c_double),
                        ("last_est_pose", C.c_float * 16), ("last", _deform.Result)])
        assert C.sizeof(_Stats) == 168
        s = _Stats()
        self._check(self.lib.cofusion_local_loop_stats(self.h, C.byref(s)))
        out = {k: getattr(s, k) for k in ints + ("last_covered", "last_icp_error", "last_icp_count", "last_max_covariance")}
        out["last_pinned"] = bool(out["last_pinned"]); out["last_tracker_accepted"] = bool(s.last_tracker_accepted)
        out["last_est_pose"] = np.array(list(s.last_est_pose), np.float32).reshape(4, 4)
        last = {k: getattr(s.last, k) for k in _deform.RESULT_FIELDS}
        for k in ("optimised", "accepted", "failed"):
            last[k] = bool(last[k])
        out["last"] = last
        return out

    def set_relative_constraints(self, on=True):
        """Relative constraints (cofusion_set_relative_constraints): an accepted local closure leaves a few point pairs in
        a device ring of 128, and every later global closure (the fern seam's, deform_background's) keeps each pair together, so it
        cannot pull apart what a local closure registered.  Off, or with an empty store, every closure is what it was."""
        self._check(self.lib.cofusion_set_relative_constraints(self.h, int(bool(on))))

    def add_relative_constraints(self, src, dst, src_time, dst_time):
        """append caller-supplied pairs: src, dst [n, 3], src_time, dst_time [n]"""
        src = np.ascontiguousarray(src, np.float32).reshape(-1, 3); dst = np.ascontiguousarray(dst, np.float32).reshape(-1, 3)
        ts = np.ascontiguousarray(src_time, np.float32).reshape(-1); td = np.ascontiguousarray(dst_time, np.float32).reshape(-1)
        assert len(src) == len(dst) == len(ts) == len(td)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.cofusion_add_relative_constraints(self.h, vp(src), vp(dst), vp(ts), vp(td), len(src)))

    def relative_constraints(self):
        """the stored pairs in store order -> f32 [n, 8]: source xyz, srcTime, target xyz, dstTime"""
        n = C.c_int()
        out = np.zeros((128, 8), np.float32)
        self._check(self.lib.cofusion_relative_constraints(self.h, out.ctypes.data_as(C.c_void_p), 128, C.byref(n)))
        return out[:n.value].copy()

    def local_closure(self):
        """test access: the last accepted local closure, until the next frame -> None, or dict(pinned, last_deform_time, src [rows, 3],
        dst [rows, 3], time [rows], target_time [constraints], nodes [n, 4], params [n, 12])"""
        found, rows, pinned, ldt, n = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        src = np.zeros((1536, 3), np.float32); dst = np.zeros((1536, 3), np.float32); tm = np.zeros(1536, np.float32); tt = np.zeros(1536, np.float32)
        nodes = np.zeros((1024, 4), np.float32); params = np.zeros((1024, 12), np.float32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.cofusion_local_closure_download(self.h, C.byref(found), C.byref(rows), C.byref(pinned), C.byref(ldt), vp(src), vp(dst), vp(tm),
                                                             vp(tt), 1536, C.byref(n), vp(nodes), vp(params), 1024))
        if not found.value:
            return None
        r, c = rows.value, rows.value // (2 if pinned.value else 1)
        return dict(pinned=bool(pinned.value), last_deform_time=ldt.value, src=src[:r].copy(), dst=dst[:r].copy(), time=tm[:r].copy(),
                    target_time=tt[:c].copy(), nodes=nodes[:n.value].copy(), params=params[:n.value].copy())

    def relative_stats(self):
        """-> dict(appended, overwritten, stored, used_by_last_closure, last_picked)"""
        class _Stats(C.Structure):
            _fields_ = [("appended", C.c_int64), ("overwritten", C.c_int64), ("stored", C.c_int32), ("used_by_last_closure", C.c_int32),
                        ("last_picked", C.c_int32), ("pad", C.c_int32)]
        assert C.sizeof(_Stats) == 32
        s = _Stats()
        self._check(self.lib.cofusion_relative_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _Stats._fields_[:-1]}

    def set_redetection(self, on=True, min_fit=0.5, min_cover=0.044, depth_tol=0.10, max_candidates=8, keep_min_surfels=4000,
                        keep_conf_threshold=0.3):
        """Re-detection of inactive object models (cofusion_set_redetection): a frame with a new label scores the most
        recent `max_candidates` kept models, each where it would be had it not moved in the world, before anything is spawned; a
        candidate with fit >= min_fit and cover >= min_cover comes back with its old id and map.  keep_*: the rule by which a
        deactivated model is kept at all.  Off by default; world == 1 only; works on a sequence of a CoFusionGroup."""
        f = C.c_float
        self._check(self.lib.cofusion_set_redetection(self.h, int(bool(on)), f(min_fit), f(min_cover), f(depth_tol), int(max_candidates),
                                                      int(keep_min_surfels), f(keep_conf_threshold)))

    def redetect_stats(self):
        a = C.c_int(); r = C.c_int(); i = C.c_int()
        self._check(self.lib.cofusion_redetect_stats(self.h, C.byref(a), C.byref(r), C.byref(i)))
        return dict(attempts=a.value, reactivations=r.value, last_id=i.value)

    def redetect_last(self):
        """the last attempt: dict(label_pixels, winner (position or -1), candidates=[dict(id, projected, occluded, seen_through, agree,
        agree_on_label, covered, fit, cover, eligible)] in list order)"""
        cap = 16
        out = (RedetectCandidate * cap)()
        n = C.c_int(); px = C.c_uint32(); w = C.c_int()
        self._check(self.lib.cofusion_redetect_last(self.h, out, cap, C.byref(n), C.byref(px), C.byref(w)))
        cands = [{k: getattr(out[q], k) for k, _ in RedetectCandidate._fields_} for q in range(min(n.value, cap))]
        for c in cands:
            c["eligible"] = bool(c["eligible"])
        return dict(label_pixels=px.value, winner=w.value, candidates=cands)

    def set_redetection_search(self, on=True, iterations=10, min_colour=-1.0, max_registered=2):
        """The search behind the static hypothesis (cofusion_set_redetection_search, DESIGN.md 4.13 "Search"): in a frame whose new label
        no kept model explains where it stood, the models whose colours resemble the label's (histogram intersection >= min_colour;
        negative: the default) are registered onto the label's pixels, the `max_registered` most similar first, and judged at the
        registered pose.  Needs set_redetection(True) first; off by default; world == 1 only."""
        self._check(self.lib.cofusion_set_redetection_search(self.h, int(bool(on)), int(iterations), C.c_float(min_colour), int(max_registered)))

    def redetect_search_last(self):
        """the search of the last attempt: dict(winner (position or -1), attempts (frames that searched), candidates=[dict(id, colour,
        registered, converged, iterations, first_inliers, last_inliers, rms, moved, the six counts, fit, cover, eligible)] in the order of
        redetect_last -- empty when that attempt did not search)"""
        cap = 16
        out = (RedetectSearchCandidate * cap)()
        n = C.c_int(); w = C.c_int(); a = C.c_int()
        self._check(self.lib.cofusion_redetect_search_last(self.h, out, cap, C.byref(n), C.byref(w), C.byref(a)))
        cands = [{k: getattr(out[q], k) for k, _ in RedetectSearchCandidate._fields_} for q in range(min(n.value, cap))]
        for c in cands:
            for k in ("registered", "converged", "eligible"):
                c[k] = bool(c[k])
        return dict(winner=w.value, attempts=a.value, candidates=cands)

    @property
    def num_inactive_models(self):
        return self.lib.cofusion_num_inactive_models(self.h)

    def model_info(self, index):
        mid = C.c_uint(); cnt = C.c_uint(); conf = C.c_float(); pose = (C.c_float * 16)()
        self._check(self.lib.cofusion_model_info(self.h, index, C.byref(mid), C.byref(cnt), pose, C.byref(conf)))
        return dict(id=mid.value, count=cnt.value, pose=np.array(pose, np.float32).reshape(4, 4), conf_threshold=conf.value)

    def model_cull_box(self, index):
        b = (C.c_int * 4)()
        self._check(self.lib.cofusion_model_cull_box(self.h, index, b))
        return list(b)

    def model_level0_visited(self, index):
        """(ICP pixels, residual pixels) the level-0 launch of the model's last tracking call visited for it (include/cofusion.h)"""
        a = C.c_uint64(); b = C.c_uint64()
        self._check(self.lib.cofusion_model_level0_visited(self.h, index, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def model_icp_stats(self, index):
        e = C.c_float(); c = C.c_float()
        self._check(self.lib.cofusion_model_icp_stats(self.h, index, C.byref(e), C.byref(c)))
        return e.value, c.value

    def model_tracking_inputs(self, index):
        """host copies of the prediction the next frame's tracking of this model reads: vertex4, normal4 (f32 [H,W,4]), image (u8 [H,W,4])"""
        H, W = self.height, self.width
        v = np.empty((H, W, 4), np.float32); n = np.empty((H, W, 4), np.float32); img = np.empty((H, W, 4), np.uint8)
        self._check(self.lib.cofusion_model_tracking_inputs(self.h, index, v.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p),
                                                            img.ctypes.data_as(C.c_void_p)))
        return v, n, img

    def set_gn_mode(self, mode):
        assert self.abi.cf_set_gn_mode(self._ctx(), int(mode)) == 0

    def set_extent_culling(self, on=True):
        """the batched surfel passes skip the texels outside the models' extents (default on; results unchanged: cf_set_extent_culling)"""
        assert self.abi.cf_set_extent_culling(self._ctx(), int(bool(on))) == 0

    def model_download(self, index):
        n = self.model_info(index)["count"]
        out = np.zeros((max(n, 1), 12), np.float32)
        c = C.c_uint32()
        self._check(self.lib.cofusion_model_download(self.h, index, out.ctypes.data_as(C.c_void_p), n, C.byref(c)))
        return out[:n]

    def mask(self):
        ptr = self.lib.cofusion_mask_device(self.h)
        host = np.empty(self.width * self.height, np.uint8)
        ctx = C.c_void_p(self.lib.cofusion_context(self.h))
        rc = self.abi.cf_memcpy_d2h(ctx, host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_uint64(host.size))
        if rc != 0:
            raise CoFusionError("mask readback failed")
        return host.reshape(self.height, self.width)

    # profiling hooks of the underlying C-ABI context
    def _ctx(self):
        return C.c_void_p(self.lib.cofusion_context(self.h))

    def set_icp_launch(self, threads, ppt):
        assert self.abi.cf_set_icp_launch(self._ctx(), threads, ppt) == 0

    def set_icp_arith(self, mode):
        """rounding specification of the ICP sums: 0 / "product" (default), 1 / "gram" or 2 / "reference" (the reference's own f32 trees and host loop; include/cofusion_hip.h: cf_set_icp_arith)"""
        assert self.abi.cf_set_icp_arith(self._ctx(), {"product": 0, "gram": 1, "reference": 2}.get(mode, mode)) == 0

    def profile_enable(self, on=True):
        """on: False / True, or N > 1 = events on the level-0 launches of every N-th tracking call"""
        assert self.abi.cf_profile_enable(self._ctx(), int(on)) == 0

    def profile_read(self, reset=True):
        p = Profile()
        assert self.abi.cf_profile_read(self._ctx(), C.byref(p), int(reset)) == 0
        return p


class CoFusionGroup:
    """Several independent RGB-D sequences on ONE GPU in lock-step (include/cofusion.h: cofusion_group_*): one context, one set of
    tracking launches for the trackers of all sequences.  `sequences[s]` is a CoFusion view of sequence s for the getters (model_info,
    model_download, mask, ...); frames are fed to all sequences at once with process_frames / process_frames_device."""

    def __init__(self, n_sequences, width=640, height=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, device=0, **kw):
        if not torch.cuda.is_available():
            raise CoFusionError("no GPU visible: the Co-Fusion hot path has no CPU fallback")
        self.lib = _libmod.load_host()
        cfg = _make_config(self.lib, width, height, fx, fy, cx, cy, device, kw)
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.n = int(n_sequences)
        self.g = C.c_void_p()
        if self.lib.cofusion_group_create(C.byref(cfg), self.n, C.byref(self.g)) != 0:
            raise CoFusionError(f"cofusion_group_create: {self.lib.cofusion_last_error().decode()}")
        self._check(self.lib.cofusion_group_set_stream(self.g, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        self.sequences = [CoFusion(width, height, fx, fy, cx, cy, device, _borrowed=self.lib.cofusion_group_sequence(self.g, s), **kw)
                          for s in range(self.n)]

    def _check(self, rc):
        if rc != 0:
            raise CoFusionError(f"cofusion error {rc}: {self.lib.cofusion_last_error().decode()}")

    def set_stream(self, stream):
        ptr = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
        self._check(self.lib.cofusion_group_set_stream(self.g, C.c_void_p(ptr)))

    def process_frames(self, depths, rgbs, masks=None, timestamp=0):
        """one frame per sequence from host arrays: depths[s] f32 [H,W] metres, rgbs[s] u8 [H,W,3], masks[s] u8 [H,W] or None"""
        keep = [np.ascontiguousarray(d, np.float32) for d in depths] + [np.ascontiguousarray(r, np.uint8) for r in rgbs]
        mk = [None if (masks is None or m is None) else np.ascontiguousarray(m, np.uint8) for m in (masks or [None] * self.n)]
        P = C.c_void_p * self.n
        ts = (C.c_int64 * self.n)(*([timestamp] * self.n))
        self._check(self.lib.cofusion_group_process_frames(
            self.g, ts, P(*[r.ctypes.data for r in keep[self.n:]]), P(*[d.ctypes.data for d in keep[:self.n]]),
            P(*[None if m is None else m.ctypes.data for m in mk]) if masks is not None else None))

    def process_frames_device(self, depth_ts, rgba_ts, timestamp=0, masks=None):
        """one frame per sequence already resident in HBM: torch CUDA tensors depth f32 [H,W], rgba u8 [H,W,4]; masks (optional):
        masks[s] a contiguous torch CUDA tensor u8 [H,W] or None (that sequence runs the motion segmentation)"""
        P = C.c_void_p * self.n
        ts = (C.c_int64 * self.n)(*([timestamp] * self.n))
        if masks is not None:
            for m, d in zip(masks, depth_ts):
                if m is not None:
                    _check_mask_tensor(m, d)
            self._check(self.lib.cofusion_group_process_frames_device_masked(
                self.g, ts, P(*[t.data_ptr() for t in depth_ts]), P(*[t.data_ptr() for t in rgba_ts]),
                P(*[None if m is None else m.data_ptr() for m in masks])))
            return
        self._check(self.lib.cofusion_group_process_frames_device(self.g, ts, P(*[t.data_ptr() for t in depth_ts]),
                                                                  P(*[t.data_ptr() for t in rgba_ts])))

    def close(self):
        if getattr(self, "g", None):
            for s in self.sequences:
                s.h = None
            self.lib.cofusion_group_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
