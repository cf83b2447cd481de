"""GPU suite: the kernels of the re-detection search (csrc/redetect_search.hip through cf_redetect_frame_moments / _model_moments /
_register_step) on the cases of tests/redetect_search_cases.py against the numpy statement tests/redetect_search_ref.py -- for EQUALITY:
every output is an integer that does not depend on execution order -- and cf_redetect_register's final pose against the statement's
within 2 ulp of f32 per entry: the sums are identical, the host loop performs the statement's f64 operations in the statement's order,
so a difference can only come from the f64 solve and the final rounding.  Every call is made twice: a result buffer that was not cleared
shows in the second."""
import numpy as np
import pytest

import redetect_search_cases as sc

pytestmark = pytest.mark.gpu

POOL = 9            # the largest batch of the cases
MAX_SURFELS = 8192  # >= the largest map


@pytest.fixture(scope="module")
def rig():
    from co_fusion_amd import api, model
    ctx = api.Context(64, 48, 64.0, 64.0, 32.0, 24.0, max_models=4, max_surfels=MAX_SURFELS)   # (the entries take their image as arguments)
    models = [model.Model(ctx, MAX_SURFELS) for _ in range(POOL)]
    yield ctx, models
    for m in models:
        m.close()
    ctx.close()


def _upload(ctx, models, case):
    assert len(case.models) <= POOL and max(len(s) for s in case.models) <= 5000
    for m, s in zip(models, case.models):
        m.upload_map(s)
    dev = (ctx.to_device(np.array(case.depth)), ctx.to_device(np.array(case.label)), ctx.to_device(np.array(case.rgba)))
    cands = [(models[mi], pose, theta) for mi, theta, pose in case.cands]
    return dev, cands


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sc.NAMES)
def test_kernels_equal_the_statement(rig, name, size):
    from co_fusion_amd import redetect
    ctx, models = rig
    case = sc.get(name, size)
    st = sc.statement(case)
    (depth, label, rgba), cands = _upload(ctx, models, case)
    frame = (depth, label, case.cam, case.new_label, case.cutoff, case.tol)
    for rep in range(2):
        m, h = redetect.frame_moments(ctx, depth, label, rgba, case.cam, case.new_label, case.cutoff)
        assert [int(v) for v in m] == st["frame"][0], f"{name} frame moments, call {rep}"
        assert np.array_equal(h, st["frame"][1]), f"{name} frame histogram, call {rep}"
        mm, mh = redetect.model_moments(ctx, cands, st["dhat"])
        for k, c in enumerate(st["cands"]):
            assert [int(v) for v in mm[k]] == c["moments"], f"{name} candidate {k} batched, call {rep}"
            assert np.array_equal(mh[k], c["hist"]), f"{name} candidate {k} batched histogram, call {rep}"
        for k, c in enumerate(st["cands"]):
            m1, h1 = redetect.model_moments(ctx, [cands[k]], st["dhat"])
            assert [int(v) for v in m1[0]] == c["moments"] and np.array_equal(h1[0], c["hist"]), f"{name} candidate {k} alone, call {rep}"
            for which in ("T0", "seed"):
                if c[which] is None:
                    continue
                got = redetect.register_step(ctx, cands[k][0], cands[k][2], c[which], *frame, st["centre"])
                assert [int(v) for v in got] == c["step_" + which], f"{name} candidate {k} step at {which}, call {rep}"


def _ulps(a, b):
    a = np.asarray(a, np.float32).reshape(-1); b = np.asarray(b, np.float32).reshape(-1)
    ia = a.view(np.int32).astype(np.int64); ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia); ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return int(np.abs(ia - ib).max())


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sc.NAMES)
def test_register_ends_where_the_statement_ends(rig, name, size):
    from co_fusion_amd import redetect
    ctx, models = rig
    case = sc.get(name, size)
    st = sc.statement(case)
    (depth, label, _), cands = _upload(ctx, models, case)
    frame = (depth, label, case.cam, case.new_label, case.cutoff, case.tol)
    n = 0
    for k, c in enumerate(st["cands"]):
        seed = c["seed"] if c["seed"] is not None else c["T0"]     # (no seed: the loop is still run, from the static pose, and must say "failed" alike)
        want = c["reg"]
        if want is None:
            import redetect_search_ref as ref
            want = ref.register(case.models[case.cands[k][0]], cands[k][2], seed, case.depth, case.label, case.new_label, case.cam, case.cutoff,
                                case.tol, st["centre"])
        got = redetect.register(ctx, cands[k][0], cands[k][2], seed, *frame, st["centre"], iterations=10)
        d = _ulps(got["cam_from_model"], want["cam_from_model"])
        print(f"{name} {size} candidate {k}: ok {got['ok']} after {got['iterations']} steps, inliers {got['first_inliers']} -> {got['last_inliers']}, "
              f"rms {got['rms']:.6f}; largest difference to the statement {d} ulp")
        for key in ("ok", "iterations", "first_inliers", "last_inliers"):
            assert got[key] == want[key], f"{name} candidate {k}: {key} {got[key]} != {want[key]}"
        assert d <= 2, f"{name} candidate {k}: {d} ulp"
        assert _ulps([got["rms"]], [want["rms"]]) <= 1
        n += 1
    assert n == len(case.cands)


def test_bad_arguments_are_refused(rig):
    from co_fusion_amd import api, redetect
    ctx, models = rig
    case = sc.get("gate_0", (70, 46))
    st = sc.statement(case)
    (depth, label, _), cands = _upload(ctx, models, case)
    assert redetect.MAX_CANDIDATES == 16 and redetect.BINS == 512
    mm, _ = redetect.model_moments(ctx, cands * 16, st["dhat"])
    assert [[int(v) for v in row] for row in mm] == [st["cands"][0]["moments"]] * 16
    with pytest.raises(api.CofusionError):
        redetect.model_moments(ctx, cands * 17, st["dhat"])
    with pytest.raises(api.CofusionError):
        redetect.register(ctx, cands[0][0], cands[0][2], st["cands"][0]["T0"], depth, label, case.cam, case.new_label, case.cutoff, case.tol,
                          st["centre"], iterations=0)
