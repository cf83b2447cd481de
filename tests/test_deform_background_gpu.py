"""GPU suite of the facade's loop-closure entry (cofusion_deform_background): the room of tests/ferns_scene.py at 640x480,
six frames of the approach fused at their ground-truth poses, then constraints from the caller.  The entry must give the map the
cf_deform_* calls give on a copy of it (those are held against the numpy statement in test_deform_gpu.py), accept a consistent
correction and reject nothing-to-do, and leave the frame loop running."""
import numpy as np
import pytest

import ferns_scene as fs

pytestmark = pytest.mark.gpu
f32 = np.float32
FRAMES = tuple(range(0, 18, 3))
RATE = 5000
SHIFT = f32([0.07, 0.0, 0.0])     # a mean constraint error above the 0.06 gate


def _open(**kw):
    from co_fusion_amd import facade
    c = fs.CAM
    return facade.CoFusion(fs.W, fs.H, c.fx, c.fy, c.cx, c.cy, enable_multiple_models=0, max_models=2, max_surfels=1 << 20, **kw)


@pytest.fixture(scope="module")
def closed():
    """the run: map before, constraints, outcome, map after, and the state one frame later"""
    cf = _open()
    try:
        for i, t in enumerate(FRAMES):
            d, rgb, gt = fs.view(t)
            cf.process_frame(d, rgb, timestamp=i, in_pose=gt)
        before = cf.model_download(0)
        pick = np.linspace(0, len(before) - 1, 40).astype(np.int64)
        src = before[pick, 0:3].copy(); tm = before[pick, 6].copy()
        small = cf.deform_background(src, src + f32([0.01, 0, 0]), tm, sample_rate=RATE)
        untouched = cf.model_download(0)
        out = cf.deform_background(src, src + SHIFT, tm, sample_rate=RATE)
        after = cf.model_download(0)
        tick = cf.tick
        d, rgb, gt = fs.view(FRAMES[-1] + 3)
        cf.process_frame(d, rgb, timestamp=len(FRAMES), in_pose=gt)
        return dict(before=before, src=src, tm=tm, small=small, untouched=untouched, out=out, after=after, tick=tick, later=cf.model_info(0)["count"],
                    later_tick=cf.tick)
    finally:
        cf.close()


def test_a_small_error_is_not_optimised_and_moves_nothing(closed):
    s = closed["small"]
    assert not s["optimised"] and not s["accepted"] and s["nodes"] == -(-len(closed["before"]) // RATE)
    assert abs(s["mean_cons_error_before"] - 0.01) < 1e-6
    assert closed["untouched"].tobytes() == closed["before"].tobytes()


def test_a_consistent_shift_is_accepted_and_moves_the_map(closed):
    o, before, after = closed["out"], closed["before"], closed["after"]
    print("outcome", o)
    assert o["optimised"] and o["accepted"] and not o["failed"] and 1 <= o["iterations"] <= 3
    assert o["nodes"] == -(-len(before) // RATE) and 5 <= o["nodes"] <= 1024
    assert abs(o["mean_cons_error_before"] - 0.07) < 1e-5 and o["mean_cons_error"] < 3e-4 and o["error"] < 0.12
    assert len(after) == len(before)
    move = after[:, 0:3] - before[:, 0:3]
    assert np.abs(move - SHIFT).max() < 3e-3 and np.linalg.norm(move - SHIFT, axis=1).mean() < 3e-4
    assert np.abs(np.linalg.norm(after[:, 8:11], axis=1) - 1).max() < 1e-5
    assert np.array_equal(after[:, [3, 4, 5, 6, 11]], before[:, [3, 4, 5, 6, 11]])
    stamped = after[:, 7] != before[:, 7]
    assert (after[stamped, 7] == closed["tick"] - 1).all()       # the reactivation stamp: the tick of the last fused frame


def test_the_entry_equals_the_deform_calls_on_a_copy(closed):
    from co_fusion_amd import api, deform
    before, after = closed["before"], closed["after"]
    c = fs.CAM
    ctx = api.Context(fs.W, fs.H, c.fx, c.fy, c.cx, c.cy, max_models=2, max_surfels=1 << 16)
    d = deform.Deform(ctx)
    try:
        dev = ctx.to_device(before)
        n, stride, mono = d.sample(dev, RATE)
        assert (n, stride, mono) == (closed["out"]["nodes"], RATE, True)
        d.weights(closed["src"], closed["src"] + SHIFT, closed["tm"])
        got = d.optimise()
        for k in deform.RESULT_FIELDS:
            assert np.asarray(got[k]).tobytes() == np.asarray(type(got[k])(closed["out"][k])).tobytes(), k
        d.apply(dev)
        ctx.synchronize()
        mine = dev.cpu().numpy()
        cols = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11]
        assert mine[:, cols].tobytes() == after[:, cols].tobytes()
    finally:
        d.close()
        ctx.close()


def test_the_frame_loop_goes_on(closed):
    assert closed["later_tick"] == closed["tick"] + 1 and closed["later"] >= len(closed["after"]) // 2


def test_refusals():
    from co_fusion_amd import facade
    cf = _open()
    try:
        p = np.zeros((1, 3), f32)
        with pytest.raises(facade.CoFusionError, match="no frame"):
            cf.deform_background(p, p, [1])
        with pytest.raises(facade.CoFusionError, match="constraints"):
            cf.deform_background(np.zeros((0, 3), f32), np.zeros((0, 3), f32), [])
        with pytest.raises(facade.CoFusionError, match="constraints"):
            cf.deform_background(np.zeros((65, 3), f32), np.zeros((65, 3), f32), np.zeros(65), dst_time=np.zeros(65), pin=True)
    finally:
        cf.close()
    g = facade.CoFusionGroup(2, 128, 64, 100.0, 100.0, 64.0, 32.0, enable_multiple_models=0, max_models=2, max_surfels=1 << 16)
    try:
        p = np.zeros((1, 3), f32)
        with pytest.raises(facade.CoFusionError, match="group"):
            g.sequences[0].deform_background(p, p, [1])
    finally:
        g.close()

