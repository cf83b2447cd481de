"""GPU suite: cf_odom_init_icp_maps, the frame side of the model-to-model tracker (the initICP(GPUTexture*, GPUTexture*, cutoff) overload
of RGBDOdometry.cpp:120-141), against the CPU oracle.  The oracle's tracker builds its frame side from a depth image only, so its
frame-side buffers are written through orc_odom_buffer the way tests/test_ferns_reloc_gpu.py writes level 0: vmap_curr / nmap_curr at
all three levels from orc_copy_maps + orc_resize_map, nextDepth from orc_vertices_to_depth + orc_pyrdown_gauss_f32 of the frame-side
vertices.  All device pyramids bit for bit; nextDepth differs from lastDepth on two views that differ; the tracked pose and lastA / lastb
bit for bit under the default exact arithmetic (rgb_only 0, icp_weight 10, pyramid, so3 0: CoFusion.cpp:405); a following
cf_odom_init_icp leaves the tracker as one that never saw the overload."""
import ctypes as C

import numpy as np
import pytest

import common
import orc
from co_fusion_amd import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 320, 240
MAX_DEPTH_RGB = 6.0      # RGBDOdometry::maxDepthRGB


def _comparable(m, which):
    """createVMap / createNMap write only the x plane of an invalid texel (NaN); its y / z planes are undefined, and a NaN has no one bit
    pattern: both are set to a fixed value before the bytes are compared (tests/test_refpin_gpu.py does the same)"""
    m = np.array(m, f32)
    if which <= 1:
        m = m.reshape(3, -1)
        bad = np.isnan(m[0])
        m[:, bad] = 0
    return np.ascontiguousarray(m)


@pytest.fixture(scope="module")
def views():
    fp = common.frame_pair(W, H, noise=True)
    v4b, n4b, imgb = synth.ideal_prediction(fp["cam"], fp["d1"], fp["rgb1"])
    return fp, f32(v4b), f32(n4b), imgb


def _oracle(fp, v4b, n4b, imgb, pose):
    cam = fp["cam"]
    od = orc.Odometry(W, H, cam.cx, cam.cy, cam.fx, cam.fy)
    od.init_icp_model(fp["v4"], fp["n4"], pose)
    od.init_rgb_model(fp["img"])
    v, n = orc.copy_maps(v4b, n4b)
    vs, ns = [v], [n]
    for _ in range(2):
        vs.append(orc.resize_map(vs[-1], False)); ns.append(orc.resize_map(ns[-1], True))
    od.init_rgb(imgb)
    ds = [orc.vertices_to_depth(v4b, MAX_DEPTH_RGB)]
    for _ in range(2):
        ds.append(orc.pyrdown_gauss_f32(ds[-1]))
    for level in range(3):
        for which, arr in ((0, vs[level]), (1, ns[level]), (5, ds[level])):
            arr = np.ascontiguousarray(arr, f32)
            C.memmove(orc.lib.orc_odom_buffer(C.c_void_p(od.h_), which, level), arr.ctypes.data, arr.nbytes)
    return od, vs, ns, ds


def test_init_icp_maps_against_the_oracle(views):
    from co_fusion_amd import api
    fp, v4b, n4b, imgb = views
    cam = fp["cam"]
    pose = common.perturbed_pose(2)
    od, vs, ns, ds = _oracle(fp, v4b, n4b, imgb, pose)
    ctx = api.Context(W, H, cam.fx, cam.fy, cam.cx, cam.cy)
    g, plain = api.Odometry(ctx), api.Odometry(ctx)
    try:
        d = ctx.to_device
        runs = []
        for _ in range(2):
            g.init_icp_model(d(fp["v4"]), d(fp["n4"]), pose)
            g.init_rgb_model(d(fp["img"]))
            g.init_icp_maps(d(v4b), d(n4b))
            g.init_rgb(d(imgb))
            ctx.synchronize()
            for level in range(3):
                for which, want in ((0, vs[level]), (1, ns[level]), (5, ds[level])):
                    got = np.ascontiguousarray(g.buffer(which, level)).view(np.uint8).reshape(-1)
                    assert got.tobytes() == np.ascontiguousarray(want, f32).tobytes(), (which, level)
                for which in (2, 3, 4, 6, 7):      # the model side and the images: what the oracle's own calls left
                    assert np.ascontiguousarray(g.buffer(which, level)).tobytes() == np.ascontiguousarray(od.buffer(which, level)).tobytes(), (which, level)
                assert np.ascontiguousarray(g.buffer(5, level)).tobytes() != np.ascontiguousarray(g.buffer(4, level)).tobytes()   # nextDepth is genuine
            tr, rot, st = g.track(pose[:3, 3], pose[:3, :3], rgb_only=False, icp_weight=10.0, pyramid=True, fast_odom=False, so3=False)
            runs.append((f32(tr).tobytes(), f32(rot).tobytes(), bytes(st.lastA), bytes(st.lastb)))
        assert runs[0] == runs[1]
        otr, orot, ost = od.track(pose[:3, 3], pose[:3, :3], rgb_only=False, icp_weight=10.0, pyramid=True, fast_odom=False, so3=False)
        assert f32(tr).tobytes() == f32(otr).tobytes() and f32(rot).tobytes() == f32(orot).tobytes()
        assert bytes(st.lastA) == bytes(ost.lastA) and bytes(st.lastb) == bytes(ost.lastb)
        assert st.last_icp_count == ost.last_icp_count > 1000 and st.last_icp_error == ost.last_icp_error
        assert np.abs(f32(tr) - pose[:3, 3]).max() > 1e-4              # the registration moved the pose
        # a following cf_odom_init_icp: the frame side is the oracle's initICP again, and the result that of a tracker that never saw
        # the overload (and the oracle's)
        pyr = ctx.depth_pyramid(d(fp["d1"]))
        od2 = orc.Odometry(W, H, cam.cx, cam.cy, cam.fx, cam.fy)
        od2.init_icp_model(fp["v4"], fp["n4"], pose)
        od2.init_rgb_model(fp["img"])
        od2.init_icp(orc.depth_pyramid(fp["d1"]), 20.0)
        od2.init_rgb(fp["rgba1"])
        res = []
        for name, t in (("after the overload", g), ("plain", plain)):
            t.init_icp_model(d(fp["v4"]), d(fp["n4"]), pose)
            t.init_rgb_model(d(fp["img"]))
            t.init_icp(pyr, 20.0)
            t.init_rgb(d(fp["rgba1"]))
            ctx.synchronize()
            for level in range(3):
                for which in (0, 1, 4, 5):
                    got, want = _comparable(t.buffer(which, level), which), _comparable(od2.buffer(which, level), which)
                    same = got.tobytes() == want.tobytes()
                    print(f"   {name}: buffer {which} level {level} {'identical' if same else 'DIFFERS'}")
                    assert same, (name, which, level)
            tr2, rot2, st2 = t.track(pose[:3, 3], pose[:3, :3], so3=False)
            res.append((f32(tr2).tobytes(), f32(rot2).tobytes(), bytes(st2.lastA), bytes(st2.lastb)))
        otr2, orot2, ost2 = od2.track(pose[:3, 3], pose[:3, :3], so3=False)
        assert res[0] == res[1] == (f32(otr2).tobytes(), f32(orot2).tobytes(), bytes(ost2.lastA), bytes(ost2.lastb))
    finally:
        g.close(); plain.close(); ctx.close()
