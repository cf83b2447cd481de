"""GPU suite of the mesh export's kernels (csrc/mesh.hip through co_fusion_amd/mesh.py): every case of tests/mesh_cases.py against the
numpy statement tests/mesh_ref.py.  Crafted maps go in with cf_model_upload_map, crafted fields with cf_mesh_extract_grid; the
integer accumulators, the counts, the triangle indices IN ORDER and the vertex records are equal bit for bit."""
import numpy as np
import pytest

import mesh_cases as mc
import mesh_ref as mr

pytestmark = pytest.mark.gpu
MAX_VOXELS = 40 * 40 * 40
ids = lambda cs: [c["name"] for c in cs]


@pytest.fixture(scope="module")
def rig():
    from co_fusion_amd import api, mesh, model
    ctx = api.Context(64, 48, 60.0, 60.0, 32.0, 24.0, max_models=2, max_surfels=4096)
    m = model.Model(ctx, max_surfels=4096)
    ms = mesh.Mesher(ctx, MAX_VOXELS)
    yield ctx, m, ms
    ms.close(); m.close(); ctx.close()


def _grid(case):
    from co_fusion_amd import mesh
    g = case["grid"]
    return mesh.make_grid(g["origin"], g["voxel"], g["dims"])


def _params(case):
    from co_fusion_amd import mesh
    return mesh.make_params(**case["params"]) if case.get("params") else None


def _run(rig, case):
    """(accumulators or None, vertices, triangles) of the device for a case"""
    ctx, m, ms = rig
    if case["kind"] == "map":
        m.upload_map(case["surfels"])
        ms.accumulate(_grid(case), case["thr"], model=m, params=_params(case))
        acc = ms.accumulators()
        nv, nt = ms.extract(case["w_min"])
    else:
        acc = None
        nv, nt = ms.extract_grid(_grid(case), case["sdf"], case["valid"], case["rgb"])
    v, t = ms.download(nv, nt)
    return acc, v, t


@pytest.mark.parametrize("case", mc.CASES, ids=ids(mc.CASES))
def test_case_equals_the_statement(rig, case):
    want = mc.reference(case)
    acc, v, t = _run(rig, case)
    if acc is not None:
        assert acc.shape == want["acc"].shape and np.array_equal(acc, want["acc"]), "integer accumulators differ"
    assert (len(v), len(t)) == (len(want["vertices"]), len(want["triangles"]))
    assert np.array_equal(t, want["triangles"]), "triangle indices (in order) differ"
    for f in ("pos", "rgba", "nrm"):
        assert v[f].tobytes() == want["vertices"][f].tobytes(), f
    if "min_counts" in case:
        assert len(v) > 4 * 1024 and len(t) > 4 * 1024      # several scan tiles
    # a second run on the same input: byte-identical
    acc2, v2, t2 = _run(rig, case)
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()
    if acc is not None:
        assert acc2.tobytes() == acc.tobytes()


def test_surfels_from_a_device_array_equal_the_model_path(rig):
    ctx, m, ms = rig
    case = mc.BY_NAME["sphere"]
    dev = ctx.to_device(case["surfels"])
    ms.accumulate(_grid(case), case["thr"], surfels=dev)
    assert np.array_equal(ms.accumulators(), mc.reference(case)["acc"])


def test_a_grid_over_max_voxels_is_an_error_code(rig):
    from co_fusion_amd import api, mesh
    ctx, m, ms = rig
    m.upload_map(mc.BY_NAME["single_centre"]["surfels"])
    big = mesh.make_grid((0, 0, 0), 0.1, (41, 40, 40))
    with pytest.raises(mesh.MeshRangeError, match="max_voxels"):
        ms.accumulate(big, 10.0, model=m)
    with pytest.raises(mesh.MeshRangeError, match="max_voxels"):
        ms.extract_grid(big, np.zeros(big.samples, np.float32), np.ones(big.samples, np.uint8))
    huge = mesh.make_grid((0, 0, 0), 0.1, (1 << 28, 1 << 28, 1 << 28))
    with pytest.raises(mesh.MeshRangeError):
        ms.accumulate(huge, 10.0, model=m)
    with pytest.raises(api.CofusionError):
        ms.accumulate(mesh.make_grid((0, 0, 0), 0.0, (4, 4, 4)), 10.0, model=m)
    with pytest.raises(api.CofusionError):
        ms.extract(1.0)                         # no accumulation stands behind the failed calls
    # ... and the mesher still works
    case = mc.BY_NAME["single_centre"]
    acc, v, t = _run(rig, case)
    assert np.array_equal(t, mc.reference(case)["triangles"])


@pytest.mark.parametrize("name,voxel,max_voxels", [("sphere", 0.0, MAX_VOXELS), ("sphere", 0.0, 4096), ("plane_patch", 0.07, MAX_VOXELS),
                                                   ("at_threshold", 0.0, MAX_VOXELS), ("empty_map", 0.0, MAX_VOXELS)])
def test_default_grid_equals_the_statement(rig, name, voxel, max_voxels):
    from co_fusion_amd import mesh
    ctx, m, ms = rig
    case = mc.BY_NAME[name]
    m.upload_map(case["surfels"])
    small = mesh.Mesher(ctx, max_voxels) if max_voxels != MAX_VOXELS else ms
    try:
        g = small.default_grid(m, case["thr"], voxel)
        want = mr.default_grid(case["surfels"], case["thr"], voxel, max_voxels)
        assert g.dims == want["dims"]
        assert np.float32(g.voxel).tobytes() == want["voxel"].tobytes()
        assert np.array(list(g.origin), np.float32).tobytes() == want["origin"].tobytes()
        # the whole export on the default grid
        v, t, _ = small.mesh(m, case["thr"], voxel)
        wv, wt, _ = mr.mesh_of(case["surfels"], case["thr"], voxel, max_voxels=max_voxels)
        assert v.tobytes() == wv.tobytes() and np.array_equal(t, wt)
        assert (len(v) > 0) == (name in ("sphere", "plane_patch"))
    finally:
        if small is not ms:
            small.close()
