"""GPU tests of the scene renderer through the facade (CoFusion::renderScene, cofusion_render*, cofusion_set_export_views): the frame
loop is untouched by rendering and exporting, render() agrees with the numpy restatement (tests/render_ref.py) fed with the downloaded
maps and poses, and the exported PNGs are render()'s bytes."""
import glob
import os
import re
import struct
import warnings
import zlib

import numpy as np
import pytest

import render_ref as rr
from co_fusion_amd import synth

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

W, H = 320, 240
FRAMES = 20
TIME_DELTA = 2147483647 // 2   # CoFusion::Config::timeDelta default
f32 = np.float32


def _inverse(a):
    """Mat4f::inverse (host/CoFusion.cpp) in f32, same operation order"""
    a = [f32(x) for x in np.asarray(a, np.float32).reshape(16)]
    c00 = a[5] * a[10] - a[6] * a[9]; c01 = a[6] * a[8] - a[4] * a[10]; c02 = a[4] * a[9] - a[5] * a[8]
    det = a[0] * c00 + a[1] * c01 + a[2] * c02
    i = f32(1.0) / det
    L = [c00 * i, (a[2] * a[9] - a[1] * a[10]) * i, (a[1] * a[6] - a[2] * a[5]) * i,
         c01 * i, (a[0] * a[10] - a[2] * a[8]) * i, (a[2] * a[4] - a[0] * a[6]) * i,
         c02 * i, (a[1] * a[8] - a[0] * a[9]) * i, (a[0] * a[5] - a[1] * a[4]) * i]
    r = np.zeros(16, np.float32)
    for k in range(3):
        r[k * 4:k * 4 + 3] = L[k * 3:k * 3 + 3]
        r[k * 4 + 3] = -(L[k * 3] * a[3] + L[k * 3 + 1] * a[7] + L[k * 3 + 2] * a[11])
    r[15] = 1
    return r.reshape(4, 4)


def _mul(A, B):
    """Mat4f::operator* in f32"""
    A = np.asarray(A, np.float32); B = np.asarray(B, np.float32)
    R = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            s = f32(0)
            for k in range(4):
                s = s + A[i, k] * B[k, j]
            R[i, j] = s
    return R


def _read_png_rgba(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat = 8, b""
    w = h = None
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if typ == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert depth == 8 and ctype == 6, "8-bit RGBA"
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    assert (raw[:, 0] == 0).all(), "filter type 0 on every row"
    return raw[:, 1:].reshape(h, w, 4)


def _state(cf):
    out = []
    for i in range(cf.num_models):
        info = cf.model_info(i)
        out.append((info["id"], info["count"], info["pose"].tobytes(), np.float32(info["conf_threshold"]).tobytes(),
                    cf.model_download(i).tobytes()))
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from co_fusion_amd import facade
    out = str(tmp_path_factory.mktemp("views")) + "/"
    cam = synth.Camera.scaled(W, H)
    sc = synth.Scene(n_obj=2)
    kw = dict(max_surfels=1 << 19, conf_global_init=0.5, model_spawn_offset=2, enable_multiple_models=1)
    plain = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, **kw)
    rend = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, **kw)
    rend.set_export_views(out, labels=True, normals=True, viewport=True)
    rend.set_export_segmentation(out)
    diffs, max_models = [], 0
    for t in range(FRAMES):
        d, rgb, lab, _ = sc.render(cam, t, noise=True)
        gt = (lab * 40).astype(np.uint8)
        plain.process_frame(d, rgb, mask=gt, timestamp=t)
        rend.process_frame(d, rgb, mask=gt, timestamp=t)
        # every mode and flag after every frame, host and device flavours
        for m in range(5):
            rend.render(background_mode=m, object_mode=m, depth=True, labels=True)
        rend.render(pose=np.eye(4), flags=7, as_torch=True, depth=True, labels=True)
        if plain.num_models != rend.num_models:
            diffs.append(f"frame {t}: {plain.num_models} vs {rend.num_models} models")
            continue
        if _state(plain) != _state(rend):
            diffs.append(f"frame {t}: model state differs")
        if plain.mask().tobytes() != rend.mask().tobytes():
            diffs.append(f"frame {t}: label mask differs")
        max_models = max(max_models, rend.num_models)
    yield dict(cam=cam, plain=plain, rend=rend, out=out, diffs=diffs, max_models=max_models)
    plain.close()
    rend.close()


def test_the_frame_loop_is_untouched_by_rendering_and_export(run):
    assert run["max_models"] >= 2, "no object model was spawned"
    assert not run["diffs"], run["diffs"]


def _ref(cf, cam, pose, fx, fy, cx, cy, w, h, bg_mode, obj_mode, flags):
    items = []
    glob_pose = cf.model_info(0)["pose"]
    for i in range(cf.num_models):
        info = cf.model_info(i)
        Tp = np.eye(4, dtype=np.float32) if i == 0 else _mul(glob_pose, _inverse(info["pose"]))
        items.append(dict(surfels=cf.model_download(i), pose=Tp, thresh=info["conf_threshold"], model_id=info["id"],
                          mode=bg_mode if i == 0 else obj_mode))
    view = dict(pose=pose, fx=fx, fy=fy, cx=cx, cy=cy, width=w, height=h, flags=flags, tick=cf.tick, time_delta=TIME_DELTA)
    return rr.render(view, items, [("rgba", -1), ("depth",), ("labels",)])


def test_render_matches_the_restatement_from_downloaded_maps(run):
    cf, cam = run["rend"], run["cam"]
    cur = cf.model_info(0)["pose"]
    got = cf.render(depth=True, labels=True)
    want = _ref(cf, cam, cur, cam.fx, cam.fy, cam.cx, cam.cy, W, H, 2, 4, 0)
    for g, w_, name in zip(got, want, ("rgba", "depth", "labels")):
        assert g.tobytes() == w_.tobytes(), f"current camera: {name}"
    assert len(np.unique(got[2])) >= 3, "background and objects visible"
    # an offset viewpoint with other intrinsics and size, every flag
    off = _mul(cur, np.array([[0.98, 0.0, 0.199, -0.15], [0.0, 1.0, 0.0, 0.05], [-0.199, 0.0, 0.98, -0.2], [0, 0, 0, 1]], np.float32))
    got = cf.render(pose=off, intrinsics=(200.0, 205.0, 150.0, 101.0), size=(288, 208), flags=7, background_mode=0, object_mode=3,
                    depth=True, labels=True)
    want = _ref(cf, cam, off, 200.0, 205.0, 150.0, 101.0, 288, 208, 0, 3, 7)
    for g, w_, name in zip(got, want, ("rgba", "depth", "labels")):
        assert g.tobytes() == w_.tobytes(), f"offset view: {name}"
    # the torch flavour returns the same bytes
    t = cf.render(as_torch=True, depth=True, labels=True)
    h = cf.render(depth=True, labels=True)
    for a, b in zip(t, h):
        assert a.cpu().numpy().tobytes() == b.tobytes()


def test_background_depth_agrees_with_its_own_prediction(run):
    """pose conventions: where the background wins, its rendered depth is the depth of its own splat prediction at the camera"""
    cf = run["rend"]
    _, depth, labels = cf.render(depth=True, labels=True)
    v4, _, _ = cf.model_tracking_inputs(0)
    both = (labels == cf.model_info(0)["id"]) & (v4[..., 2] > 0)
    assert both.sum() > 0.3 * W * H
    assert np.median(np.abs(depth[both] - v4[..., 2][both])) < 1e-3


def test_exported_views_are_the_rendered_bytes(run):
    cf, out = run["rend"], run["out"]
    segs = sorted(int(re.findall(r"(\d+)\.png", p)[0]) for p in glob.glob(out + "Segmentation*.png"))
    for name in ("Labels", "Normals", "Viewport"):
        ns = sorted(int(re.findall(r"(\d+)\.png", p)[0]) for p in glob.glob(out + name + "*.png"))
        assert len(ns) == FRAMES, (name, ns)
        assert ns == list(range(ns[0], ns[0] + FRAMES))
        assert set(segs) <= set(ns), "the same frame numbers as Segmentation<n>.png"
    last = max(int(re.findall(r"(\d+)\.png", p)[0]) for p in glob.glob(out + "Labels*.png"))
    for name, (bg, obj) in (("Labels", (2, 4)), ("Normals", (1, 1)), ("Viewport", (2, 2))):
        img = _read_png_rgba(os.path.join(out, f"{name}{last}.png"))
        assert img.tobytes() == cf.render(background_mode=bg, object_mode=obj).tobytes(), name
