"""Host bookkeeping of the tracker object, seen through cf_odom_buffer alone (pointers and byte sizes, no kernel beyond cf_odom_init_icp):
which current-frame maps a tracker reports -- its own, an owner's after cf_odom_share_frame_maps (an owner with maps of its own and an
owner that was itself bound with cf_odom_bind_frame_maps), its own again after unbinding or a cf_odom_init_icp of its own --, the
argument checks of cf_odom_buffer and the byte size of every buffer it hands out.

What tracking computes from shared maps is held by tests/test_track_batch_gpu.py; this file holds the pointers.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 64, 48
CF_EINVAL = -1
LEVELS = (0, 1, 2)


@pytest.fixture(scope="module")
def box():
    from co_fusion_amd import api
    ctx = api.Context(W, H, 60.0, 60.0, 32.0, 24.0)
    ods = [api.Odometry(ctx) for _ in range(3)]
    yield ctx, ods
    for g in ods:
        g.close()
    ctx.close()


def _maps(g):
    """(vmap, nmap) addresses the tracker reports as its current frame maps, per level"""
    return [(g.buffer_address(0, l), g.buffer_address(1, l)) for l in LEVELS]


def _bind(ctx, g, vmaps, nmaps):
    arr = lambda ts: None if ts is None else (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    ctx._check(ctx.lib.cf_odom_bind_frame_maps(g.h, arr(vmaps), arr(nmaps)))


def test_frame_map_pointers(box):
    ctx, (od, owner, bound) = box
    own = {g: _maps(g) for g in (od, owner, bound)}
    flat = [p for g in own for pair in own[g] for p in pair]
    assert all(flat) and len(set(flat)) == len(flat), "every tracker has vertex and normal maps of its own at every level"

    owner.init_icp(ctx.depth_pyramid(ctx.to_device(np.full((H, W), 1.5, np.float32))), 20.0)
    assert _maps(owner) == own[owner], "cf_odom_init_icp fills the tracker's own maps"

    od.share_frame_maps(owner)
    assert _maps(od) == own[owner], "sharing from an owner with maps of its own"
    assert _maps(owner) == own[owner]

    ext_v = [ctx.empty((3 * (H >> l), W >> l)) for l in LEVELS]
    ext_n = [ctx.empty((3 * (H >> l), W >> l)) for l in LEVELS]
    ext = [(v.data_ptr(), n.data_ptr()) for v, n in zip(ext_v, ext_n)]
    _bind(ctx, bound, ext_v, ext_n)
    assert _maps(bound) == ext, "a bound tracker reports the caller's maps"
    od.share_frame_maps(bound)
    assert _maps(od) == ext, "sharing from an owner that was itself bound"

    _bind(ctx, od, None, None)
    assert _maps(od) == own[od], "unbinding returns the tracker to its own maps"
    _bind(ctx, bound, None, None)
    assert _maps(bound) == own[bound]

    od.share_frame_maps(owner)
    od.init_icp(ctx.depth_pyramid(ctx.to_device(np.full((H, W), 1.5, np.float32))), 20.0)
    assert _maps(od) == own[od], "a cf_odom_init_icp of its own ends the sharing"


def test_buffer_argument_checks(box):
    ctx, (od, _, _) = box
    ptr, nbytes = C.c_void_p(), C.c_uint64()
    call = lambda which, level: ctx.lib.cf_odom_buffer(od.h, which, level, C.byref(ptr), C.byref(nbytes))
    assert call(15, 1) == CF_EINVAL and call(16, 1) == CF_EINVAL, "occupancy and bounding box exist at level 0 only"
    assert call(15, 0) == 0 and call(16, 0) == 0
    assert call(17, 0) == CF_EINVAL and call(-1, 0) == CF_EINVAL, "unknown buffer"
    assert call(2, 3) == CF_EINVAL and call(2, -1) == CF_EINVAL, "unknown level"
    assert ctx.lib.cf_odom_buffer(od.h, 2, 0, None, C.byref(nbytes)) == CF_EINVAL
    assert ctx.lib.cf_odom_buffer(None, 2, 0, C.byref(ptr), C.byref(nbytes)) == CF_EINVAL


def test_buffer_sizes(box):
    ctx, (od, _, _) = box
    per_pixel = {0: 12, 1: 12, 2: 12, 3: 12, 4: 4, 5: 4, 6: 1, 7: 1, 8: 1, 9: 2, 10: 2, 11: 12, 12: 16, 13: 1}
    for level in LEVELS:
        n = (W >> level) * (H >> level)
        want = {which: n * b for which, b in per_pixel.items()}
        want[14] = (n + 63) // 64 * 8            # one float2 per 64-pixel run
        if level == 0:
            want[15] = (W >> 2) * (H >> 2)       # one byte per 4x4 block
            want[16] = 6 * 4                     # six keys
        for which, size in want.items():
            ptr, nbytes = C.c_void_p(), C.c_uint64()
            ctx._check(ctx.lib.cf_odom_buffer(od.h, which, level, C.byref(ptr), C.byref(nbytes)))
            assert ptr.value and nbytes.value == size, f"buffer {which}, level {level}: {nbytes.value} bytes, expected {size}"
