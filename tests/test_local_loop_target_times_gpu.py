"""GPU suite: the fourth buffer of the local constraint stage (cf_local_loop_target_times, csrc/local_loop.hip) -- the old time of every
constraint, one per constraint whether the rows carry pins or not -- against deform_rel_ref.target_times on the sampling cases of
tests/local_loop_cases.py (96 samples at 256x160, two waves; gaps across the wave edge, z at the depth limit, old time 0), bit for bit,
twice each.  With pins the values are also the times of the pin rows; record and rows are what test_local_loop_kernels_gpu.py holds."""
import numpy as np
import pytest

import deform_rel_ref as rel
import local_loop_cases as lc
import local_loop_ref as lref

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = lc.SHAPE


@pytest.fixture(scope="module")
def loop():
    from co_fusion_amd import api, local_loop
    ctx = api.Context(W, H, *lc.CAM, max_models=2)
    l = local_loop.LocalLoop(ctx)
    yield ctx, l
    l.close()
    ctx.close()


@pytest.mark.parametrize("pin", [False, True], ids=["no_pins", "pins"])
@pytest.mark.parametrize("kind", lc.SAMPLE_CASES)
def test_target_times_are_the_old_time_texels(loop, kind, pin):
    ctx, l = loop
    v, t = lc.cons_maps(kind)
    pose = lc.cons_pose(0)
    rows = lref.local_constraints(lc.good_track(), v, t, pose, lc.CONS_TICK, lc.CONS_MAX_DEPTH, pin)
    want = rel.target_times(v, t, lc.CONS_MAX_DEPTH)
    stride = 2 if pin else 1
    assert len(want) * stride == rows["n"] and (kind == "none_valid") == (len(want) == 0)
    if pin:
        assert want.tobytes() == rows["time"][1::2].tobytes()
    dv, dt = ctx.to_device(v), ctx.to_device(t)
    runs = []
    for _ in range(2):
        l.constraints_async(dv, dt, pose, lc.CONS_TICK, lc.CONS_MAX_DEPTH, pin, track=lc.good_track())
        rec = l.wait()
        assert rec["accepted"] and rec["n_constraints"] == rows["n"]
        got = l.target_times(len(want))
        assert got.tobytes() == want.tobytes()
        src, dst, tm = l.rows(rows["n"])
        assert src.tobytes() == rows["src"].tobytes() and dst.tobytes() == rows["dst"].tobytes() and tm.tobytes() == rows["time"].tobytes()
        runs.append(got.tobytes())
    assert runs[0] == runs[1]
