"""GPU parity of the lock-step surfel chain (cf_models_frame_passes, csrc/cabi_model.hip: index map, association, compaction, update,
second index map, clean, second compaction, splat prediction -- each one batched launch) on the cases of tests/surfel_cases.py.

After every call and for every model, bit for bit (NaN equals NaN; `_same` of tests/test_surfel_gpu.py):
  - against the CPU oracle's chain for the same arguments: the surfel map and its count, the new unstable surfels the fuse appended
    (buffer 12), the index-map buffers 0..3, the packed texel records of the clean stage (buffer 13), the splat buffers 4..7;
  - a twin model driven through the per-model calls in the reference's order (cf_model_predict_indices, _fuse, _predict_indices, _clean,
    _combined_predict: separate launches, the clean stage without packed records) against the same oracle results.
Together: the chain against the oracle, the per-model path against the oracle, and the header's promise that the two are identical.

CF_NO_CLEAN_REC / CF_NO_SIDE_BY_SIDE are read once per process and are not toggled here: the twins cover those paths.
"""
import numpy as np
import pytest

import common
import surfel_cases as sc
from test_surfel_gpu import _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts():
    from co_fusion_amd import api
    made = {}

    def get(shape, cam):
        key = (shape, cam.fx, cam.fy, cam.cx, cam.cy)
        if key not in made:
            made[key] = api.Context(shape[0], shape[1], cam.fx, cam.fy, cam.cx, cam.cy, max_models=16)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def _dev(ctx, a):
    return ctx.to_device(np.array(a))   # (a writable copy: the cases are read-only)


def _clean_records(r, fr):
    """what index_resolve_kernel packs per texel for clean_kernel, from the oracle's second index map and the frame's filtered depth"""
    idx, vc, ct, _ = r.index
    rec = np.zeros(idx.shape + (8,), np.float32)
    rec[..., 0:4] = vc
    rec[..., 4:6] = ct[..., 2:4]
    rec[..., 6] = idx.view(np.float32)
    rec[..., 7] = fr.depth_filt
    return rec


def _compare(m, r, fr, what, chain):
    """one model after a call against the oracle's Result"""
    assert m.count() == r.map.shape[0], f"{what}: count {m.count()} != {r.map.shape[0]}"
    _same(m.download_map(), r.map, f"{what}: map")
    _same(m.buffer(11), r.map, f"{what}: buffer 11")
    if r.index is not None:
        _same(m.buffer(12), r.fresh, f"{what}: new unstable surfels")
        for k, name in enumerate(("index", "vertConf", "colorTime", "normRad")):
            _same(m.buffer(k), r.index[k], f"{what}: {name}")
        if chain:
            _same(m.buffer(13), _clean_records(r, fr), f"{what}: packed clean records")
    for k, name in enumerate(("splat image", "splat vertexConf", "splat normalRad", "splat time")):
        _same(m.buffer(4 + k), r.splat[k], f"{what}: {name}")


def _per_model(m, it, fr, case):
    """the statements of the chain for one model, through the per-model calls in the reference's order"""
    if it.do_fuse:
        m.predict_indices(it.pose, it.time, sc.DEPTH_CUTOFF, case.time_delta)
        m.fuse(it.pose, it.time, fr["rgba"], fr["mask"], fr["depth"], fr["depth_filt"], it.fuse_max_depth, it.weighting, it.mask_id)
        m.predict_indices(it.pose, it.time, sc.DEPTH_CUTOFF, case.time_delta)
        m.clean(it.pose, it.time, it.conf, case.outlier, fr["depth_filt"], fr["mask"], it.mask_id, case.time_delta)
    m.combined_predict(it.pose, sc.DEPTH_CUTOFF, it.conf, it.time, it.time, case.time_delta)


def _item(m, it, fr):
    return dict(model=m, pose=it.pose, rgba=fr["rgba"], mask=fr["mask"], depth_raw=fr["depth"], depth_filt=fr["depth_filt"], do_fuse=it.do_fuse,
                time=it.time, fuse_max_depth=it.fuse_max_depth, weighting=it.weighting, mask_id=it.mask_id, conf_threshold=it.conf)


@pytest.mark.parametrize("name", sc.NAMES)
def test_chain_and_twins_against_the_oracle(contexts, name):
    from co_fusion_amd import model as M
    case, want = sc.get(name), sc.oracle(name)
    ctx = contexts(case.shape, case.cam)
    frames = {k: dict(rgba=_dev(ctx, f.rgba), mask=_dev(ctx, f.mask), depth=_dev(ctx, f.depth), depth_filt=_dev(ctx, f.depth_filt))
              for k, f in case.frames.items()}
    chain = [M.Model(ctx, case.max_surfels) for _ in case.maps]
    twins = [M.Model(ctx, case.max_surfels) for _ in case.maps]
    try:
        for ms in (chain, twins):
            for m, s in zip(ms, case.maps):
                m.upload_map(s)
        for k, call in enumerate(case.calls):
            for _, model, frame, time in case.between.get(k, []):
                f = frames[frame]
                for ms in (chain, twins):
                    ms[model].initialise(f["rgba"], f["depth"], f["depth_filt"], time, sc.DEPTH_CUTOFF)
            M.frame_passes(ctx, [_item(chain[it.model], it, frames[it.frame]) for it in call], sc.DEPTH_CUTOFF, case.outlier, case.time_delta)
            for q, it in enumerate(call):
                _per_model(twins[it.model], it, frames[it.frame], case)
            for q, it in enumerate(call):
                what = f"{name} call {k} item {q} (model {it.model}, time {it.time})"
                _compare(chain[it.model], want[k][q], case.frames[it.frame], what + ", chain", True)
                _compare(twins[it.model], want[k][q], case.frames[it.frame], what + ", per-model calls", False)
    finally:
        for m in chain + twins:
            m.close()


def test_preindexed_chain(contexts):
    """cf_models_preindex rasterises the first index map with the tracker's pose from device memory (t_inv_dev); the chain that follows
    skips its first index pass when it is handed the tracker's pose bit for bit, and rasterises again for any other pose"""
    from co_fusion_amd import api, model as M
    import prep_scenes as ps
    shape = (80, 36)
    s = ps.scene(*shape)
    cam = s["cam"]
    ctx = contexts(shape, cam)
    fp = common.frame_pair(shape[0], shape[1], noise=True)
    f0 = sc.Frame(fp["rgba0"], fp["d0"], sc.op.bilateral(fp["d0"], sc.FILTER_CUTOFF), np.zeros(shape[::-1], np.uint8))
    f1 = sc.Frame(fp["rgba1"], fp["d1"], sc.op.bilateral(fp["d1"], sc.FILTER_CUTOFF), np.zeros(shape[::-1], np.uint8))
    start = sc.confident(sc.bootstrap(f0, cam, 1))
    case = sc.Case("preindex", shape, cam, [start], {"f": f1}, [], max_surfels=1 << 14)
    fr = dict(rgba=_dev(ctx, f1.rgba), mask=_dev(ctx, f1.mask), depth=_dev(ctx, f1.depth), depth_filt=_dev(ctx, f1.depth_filt))
    g = api.Odometry(ctx)
    m, twin = M.Model(ctx, case.max_surfels), M.Model(ctx, case.max_surfels)
    try:
        g.init_first_rgb(_dev(ctx, s["rgba0"]))
        g.init_icp_model(_dev(ctx, s["v4"]), _dev(ctx, s["n4"]), s["pose"])
        g.init_rgb_model(_dev(ctx, s["img"]))
        g.init_icp([_dev(ctx, l) for l in s["depth_pyr"]], ps.CUTOFF)
        g.init_rgb(_dev(ctx, s["rgba1"]))
        m.upload_map(start); twin.upload_map(start)
        ctx.track_batch([g], [s["pose"]])
        M.preindex(ctx, [(m, g, 2)], sc.DEPTH_CUTOFF)
        tr, rot, st = g.fetch()
        o = ps.oracle_tracked(*shape)
        assert st.last_icp_count == o["icp_count"] > 0
        pose = np.eye(4, dtype=np.float32); pose[:3, :3] = rot; pose[:3, 3] = tr
        assert not np.array_equal(pose, s["pose"])
        it = sc.Item(0, "f", pose, 2)
        r = sc.oracle_item(case, it, start)
        # what cf_models_preindex rasterised with the pose in device memory, before the chain touches anything (reading changes nothing)
        assert np.count_nonzero(r.index_first[0]) > 1000
        for k, name in enumerate(("index", "vertConf", "colorTime", "normRad")):
            _same(m.buffer(k), r.index_first[k], f"preindex: {name}")
        M.frame_passes(ctx, [_item(m, it, fr)], sc.DEPTH_CUTOFF, case.outlier)
        M.frame_passes(ctx, [_item(twin, it, fr)], sc.DEPTH_CUTOFF, case.outlier)
        assert np.count_nonzero(r.upd_trace[:, 0]) > 100
        _compare(m, r, f1, "preindexed with the tracker's pose", True)
        _compare(twin, r, f1, "twin without preindex", True)
        # the tracker's pose again on the device, another pose (one bit) in the chain: it rasterises again
        M.preindex(ctx, [(m, g, 3)], sc.DEPTH_CUTOFF)
        at3 = sc.op.predict_indices(r.map, pose, sc.ocam(cam), shape[0], shape[1], sc.DEPTH_CUTOFF, 3, sc.TIME_DELTA)
        for k, name in enumerate(("index", "vertConf", "colorTime", "normRad")):
            _same(m.buffer(k), at3[k], f"second preindex: {name}")
        other = pose.copy()
        other[0, 3] = np.nextafter(other[0, 3], np.float32(np.inf))
        it2 = sc.Item(0, "f", other, 3)
        M.frame_passes(ctx, [_item(m, it2, fr)], sc.DEPTH_CUTOFF, case.outlier)
        _compare(m, sc.oracle_item(case, it2, r.map), f1, "preindexed, then a pose that differs in one bit", True)
    finally:
        m.close(); twin.close(); g.close()
