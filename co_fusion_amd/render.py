"""Python binding of the scene renderer (cf_render_*, include/cofusion_hip.h): several models' surfel maps drawn into one view as
disc splats, depth-tested against each other.  Semantics: DESIGN.md "Scene rendering"."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .api import Context

UNSTABLE, WINDOW, PHONG = 1, 2, 4
GREY, NORMALS, COLOUR, TIMES, LABEL, ITEM_MODE = 0, 1, 2, 3, 4, -1
RGBA, DEPTH, LABELS = 0, 1, 2
MAX_ITEMS = 256


class View(C.Structure):
    _fields_ = [("pose", C.c_float * 16), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("width", C.c_int), ("height", C.c_int), ("near_z", C.c_float), ("far_z", C.c_float), ("flags", C.c_int),
                ("tick", C.c_int), ("time_delta", C.c_int)]


class Item(C.Structure):
    _fields_ = [("surfels", C.c_void_p), ("count", C.c_uint32), ("pose", C.c_float * 16), ("conf_threshold", C.c_float),
                ("model_id", C.c_int), ("colour_mode", C.c_int)]


class Output(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("kind", C.c_int), ("mode", C.c_int)]


def _mat(a):
    return (C.c_float * 16)(*[float(x) for x in np.asarray(a, np.float32).reshape(16)])


def make_view(pose, fx, fy, cx, cy, width, height, near=0.0, far=0.0, flags=0, tick=1, time_delta=2 ** 30 - 1):
    return View(_mat(pose), fx, fy, cx, cy, width, height, near, far, flags, tick, time_delta)


def make_item(surfels_ptr, count, pose, conf_threshold, model_id, colour_mode):
    return Item(C.c_void_p(surfels_ptr), int(count), _mat(pose), float(conf_threshold), int(model_id), int(colour_mode))


def palette():
    from . import lib as _libmod
    out = np.zeros((256, 3), np.uint8)
    if _libmod.load().cf_render_palette(out.ctypes.data_as(C.c_void_p)) != 0:
        raise RuntimeError("cf_render_palette failed")
    return out


class Renderer:
    """cf_renderer of a context, for views up to max_w x max_h.  render() enqueues on the context's stream and returns torch
    tensors on the device (RGBA outputs u8 [H, W, 4], depth f32 [H, W], labels u8 [H, W])."""

    def __init__(self, ctx: Context, max_w, max_h):
        self.ctx = ctx
        self.h = C.c_void_p()
        ctx._check(ctx.lib.cf_render_create(ctx.h, int(max_w), int(max_h), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.cf_render_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, view: View, items, rgba_modes=(ITEM_MODE,), depth=False, labels=False):
        """items: Item structs in draw order; rgba_modes: one colour output per entry"""
        H, W = view.height, view.width
        dev = self.ctx.device
        outs, res = [], []
        for m in rgba_modes:
            t = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
            outs.append(Output(C.c_void_p(t.data_ptr()), RGBA, int(m))); res.append(t)
        if depth:
            t = torch.empty((H, W), dtype=torch.float32, device=dev)
            outs.append(Output(C.c_void_p(t.data_ptr()), DEPTH, 0)); res.append(t)
        if labels:
            t = torch.empty((H, W), dtype=torch.uint8, device=dev)
            outs.append(Output(C.c_void_p(t.data_ptr()), LABELS, 0)); res.append(t)
        arr = (Item * max(len(items), 1))(*items)
        oarr = (Output * max(len(outs), 1))(*outs)
        self.ctx._check(self.ctx.lib.cf_render(self.h, C.byref(view), arr, len(items), oarr, len(outs)))
        return res
