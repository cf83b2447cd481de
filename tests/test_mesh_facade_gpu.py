"""GPU suite of the facade's mesh export (CoFusion::saveMesh / cofusion_model_mesh): a synth scene with one moving object
at 160x128, fused for a handful of frames with ground-truth masks.  The poses are tracked, not injected: a frame with an injected pose
skips the segmentation (CoFusion::frameSegment), so no object model would ever be spawned.  The meshes equal the numpy statement
(tests/mesh_ref.py) run on the downloaded maps bit for bit; the files are the meshes mapped by Tp; the background faces the camera
that saw it; and the frame loop computes the same with and without the mesh calls."""
import os

import numpy as np
import pytest

import mesh_ref as mr
from co_fusion_amd import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 160, 128
FRAMES = 8
MAX_VOXELS = 1 << 19      # (small on purpose: the background's default voxel has to grow to fit, and the statement stays quick)
KW = dict(max_surfels=1 << 18, conf_global_init=0.5, model_spawn_offset=2, enable_multiple_models=1)


def _frames():
    cam = synth.Camera.scaled(W, H)
    sc = synth.Scene(n_obj=1)
    out = []
    for t in range(FRAMES + 1):
        d, rgb, lab, pose = sc.render(cam, t, noise=True)
        out.append((d, rgb, (lab * 40).astype(np.uint8), pose.astype(f32)))
    return cam, out


def _run(with_mesh, tmp):
    from co_fusion_amd import facade
    cam, frames = _frames()
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, **KW)
    r = dict(dir=tmp)
    try:
        for t, (d, rgb, gt, pose) in enumerate(frames[:FRAMES]):
            cf.process_frame(d, rgb, mask=gt, timestamp=t)
        r["n"] = cf.num_models
        r["info"] = [cf.model_info(i) for i in range(r["n"])]
        r["maps"] = [cf.model_download(i) for i in range(r["n"])]
        if with_mesh:
            cf.set_mesh_max_voxels(MAX_VOXELS)
            r["meshes"] = [cf.model_mesh(i, with_transform=True) for i in range(r["n"])]
            r["again"] = cf.model_mesh(0)
            os.makedirs(tmp, exist_ok=True)
            r["saved"] = cf.save_mesh(tmp + os.sep)
            r["clouds"] = cf.save_ply(tmp + os.sep)
            r["files"] = sorted(os.listdir(tmp))
            with pytest.raises(facade.CoFusionError, match="out of range"):
                cf.model_mesh(-1)                     # no inactive model is kept in this run
            with pytest.raises(facade.CoFusionError, match="out of range"):
                cf.model_mesh(r["n"])
        r["maps_after"] = [cf.model_download(i) for i in range(r["n"])]
        d, rgb, gt, pose = frames[FRAMES]
        cf.process_frame(d, rgb, mask=gt, timestamp=FRAMES)
        r["next"] = [cf.model_info(i) for i in range(cf.num_models)]
        r["next_maps"] = [cf.model_download(i) for i in range(cf.num_models)]
    finally:
        cf.close()
    return r


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return _run(True, str(tmp_path_factory.mktemp("mesh")))


def test_the_scene_has_a_background_and_an_object(run):
    assert run["n"] == 2
    for i in range(2):
        m = run["maps"][i]
        assert (m[:, 3] > run["info"][i]["conf_threshold"]).sum() > 200, "too few confident surfels to mesh"


@pytest.mark.parametrize("i", [0, 1], ids=["background", "object"])
def test_model_mesh_equals_the_statement_on_the_downloaded_map(run, i):
    v, t, tp = run["meshes"][i]
    wv, wt, grid = mr.mesh_of(run["maps"][i], run["info"][i]["conf_threshold"], 0.0, max_voxels=MAX_VOXELS)
    print("model", i, "grid", grid["dims"], "voxel", grid["voxel"], "vertices", len(wv), "triangles", len(wt))
    assert len(wv) > 100 and len(wt) > 100
    assert (len(v), len(t)) == (len(wv), len(wt))
    assert np.array_equal(t, wt)
    assert v.tobytes() == wv.tobytes()
    if i == 0:
        assert np.array_equal(tp, np.eye(4, dtype=f32))
        v2, t2 = run["again"]
        assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()


def test_save_mesh_writes_one_file_per_model_named_like_the_clouds(run):
    ids = [m["id"] for m in run["info"]]
    assert run["saved"] == 2 and run["clouds"] == 2
    assert run["files"] == sorted(["mesh-%d.ply" % i for i in ids] + ["cloud-%d.ply" % i for i in ids])


@pytest.mark.parametrize("i", [0, 1], ids=["background", "object"])
def test_the_files_equal_model_mesh_after_the_mapping(run, i):
    v, t, tp = run["meshes"][i]
    fv, ft = mr.read_ply(os.path.join(run["dir"], "mesh-%d.ply" % run["info"][i]["id"]))
    assert np.array_equal(ft, t)
    T = tp.astype(f32)
    p, n = v["pos"], v["nrm"]
    want_p = np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1)
    want_n = np.stack([(T[r, 0] * n[:, 0] + T[r, 1] * n[:, 1]) + T[r, 2] * n[:, 2] for r in range(3)], axis=1)
    assert fv["pos"].tobytes() == want_p.astype(f32).tobytes()
    assert fv["nrm"].tobytes() == want_n.astype(f32).tobytes()
    assert np.array_equal(fv["rgba"][:, :3], v["rgba"][:, :3])
    if i == 1:
        assert not np.array_equal(T, np.eye(4, dtype=f32))


def test_the_background_faces_the_camera_that_saw_it(run):
    """the sign test: positive = outside = the observed side, so the geometric normals point back at the camera (within centimetres of the
    world origin in every frame of this run).  A flipped convention gives about none; one half separates the two outcomes."""
    v, t, _ = run["meshes"][0]
    p = v["pos"].astype(np.float64)
    t = t.astype(np.int64)
    fn = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    area = 0.5 * np.linalg.norm(fn, axis=1)
    to_cam = -p[t].mean(axis=1)
    facing = (fn * to_cam).sum(axis=1) > 0
    print("area facing the camera: %.4f of %.4f" % (area[facing].sum(), area.sum()))
    assert area[facing].sum() > 0.5 * area.sum()


def test_the_frame_loop_computes_the_same_with_and_without_the_mesh_calls(run, tmp_path):
    plain = _run(False, str(tmp_path))
    for i in range(2):
        assert run["maps"][i].tobytes() == plain["maps"][i].tobytes()
        assert run["maps_after"][i].tobytes() == run["maps"][i].tobytes(), "the mesh calls wrote to a map"
    assert len(run["next"]) == len(plain["next"])
    for a, b in zip(run["next"], plain["next"]):
        assert np.asarray(a["pose"], f32).tobytes() == np.asarray(b["pose"], f32).tobytes() and a["count"] == b["count"]
    for a, b in zip(run["next_maps"], plain["next_maps"]):
        assert a.tobytes() == b.tobytes()
