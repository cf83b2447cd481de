"""GPU suite: the re-detection score and the relabel pass (csrc/redetect.hip through cf_redetect_score / cf_relabel) on the cases of
tests/redetect_cases.py, against the numpy statement tests/redetect_ref.py -- for EQUALITY: every output is an integer count that does
not depend on execution order.  Each case is scored candidate by candidate and as one batch, twice each: a bitmap or a counter that was
not cleared shows in the second call (and in the next case)."""
import numpy as np
import pytest

import redetect_cases as rc
import redetect_ref as ref

pytestmark = pytest.mark.gpu

POOL = 9            # the largest batch of the cases
MAX_SURFELS = 8192  # >= the largest map (5000)


@pytest.fixture(scope="module")
def rig():
    from co_fusion_amd import api, model
    ctx = api.Context(64, 48, 64.0, 64.0, 32.0, 24.0, max_models=4, max_surfels=MAX_SURFELS)   # (the score takes its image as arguments)
    models = [model.Model(ctx, MAX_SURFELS) for _ in range(POOL)]
    yield ctx, models
    for m in models:
        m.close()
    ctx.close()


_STATEMENT = {}


def _statement(case):
    """the statement's counts for every candidate of a case, computed once and shared"""
    key = (case.name, case.size)
    if key not in _STATEMENT:
        _STATEMENT[key] = ([ref.score(s, th, p, case.depth, case.label, case.new_label, case.cam, case.cutoff, case.tol) for s, th, p in case.cands],
                           ref.label_pixels(case.label, case.new_label))
    return _STATEMENT[key]


def _score(ctx, case, depth, label, cands):
    from co_fusion_amd import redetect
    return redetect.score(ctx, cands, depth, label, case.cam, case.new_label, case.cutoff, case.tol)


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", rc.NAMES)
def test_score_equals_the_statement(rig, name, size):
    ctx, models = rig
    case = rc.get(name, size)
    want, want_px = _statement(case)
    depth, label = ctx.to_device(np.array(case.depth)), ctx.to_device(np.array(case.label))
    assert len(case.cands) <= POOL
    for m, (s, _, _) in zip(models, case.cands):
        m.upload_map(s)
    cands = [(m, p, th) for m, (_, th, p) in zip(models, case.cands)]
    for rep in range(2):
        for k, c in enumerate(cands):
            got, px = _score(ctx, case, depth, label, [c])
            assert got == [want[k]], f"{name} candidate {k} alone, call {rep}: {got[0]} != {want[k]}"
            assert px == want_px
        got, px = _score(ctx, case, depth, label, cands)
        assert got == want, f"{name} batched, call {rep}"
        assert px == want_px


def test_nothing_is_left_from_the_previous_call(rig):
    """a map that covers a large patch, then one that covers nothing in the same slot, then a smaller image: the bitmaps start from zero"""
    ctx, models = rig
    big, none = rc.get("counts", (70, 46)), rc.get("gone", (64, 48))
    for case, k in ((big, len(big.cands) - 1), (none, 0), (big, 2)):
        s, th, p = case.cands[k]
        models[0].upload_map(s)
        got, px = _score(ctx, case, ctx.to_device(np.array(case.depth)), ctx.to_device(np.array(case.label)), [(models[0], p, th)])
        assert got == [_statement(case)[0][k]] and px == _statement(case)[1]


def test_more_candidates_than_a_launch_holds_are_refused(rig):
    from co_fusion_amd import api, redetect
    ctx, models = rig
    case = rc.get("exact_patch", (64, 48))
    s, th, p = case.cands[0]
    models[0].upload_map(s)
    depth, label = ctx.to_device(np.array(case.depth)), ctx.to_device(np.array(case.label))
    assert redetect.MAX_CANDIDATES == 16
    got, _ = _score(ctx, case, depth, label, [(models[0], p, th)] * 16)
    assert got == [_statement(case)[0][0]] * 16
    with pytest.raises(api.CofusionError):
        _score(ctx, case, depth, label, [(models[0], p, th)] * 17)


@pytest.mark.parametrize("n", [70 * 46, 16 * 5, 15, 4096 + 7])
def test_relabel_changes_exactly_the_from_pixels(rig, n):
    import torch
    from co_fusion_amd import redetect
    ctx, _ = rig
    assert n in (80,) or n % 16 != 0
    rng = np.random.default_rng(n)
    img = rng.integers(0, 6, size=n).astype(np.uint8)
    img[-1] = 3; img[0] = 3
    t = ctx.to_device(img)
    guard = torch.full((n + 64,), 3, dtype=torch.uint8, device=t.device)   # the image in the middle of a larger buffer: nothing beyond it is written
    guard[16:16 + n] = t
    view = guard[16:16 + n]
    assert view.data_ptr() % 16 == 0
    redetect.relabel(ctx, view, 3, 200)
    ctx.synchronize()
    want = np.where(img == 3, np.uint8(200), img)
    assert np.array_equal(view.cpu().numpy(), want)
    out = guard.cpu().numpy()
    assert np.all(out[:16] == 3) and np.all(out[16 + n:] == 3)
    redetect.relabel(ctx, view, 9, 1)      # a value that does not occur
    redetect.relabel(ctx, view, 4, 4)      # from == to
    ctx.synchronize()
    assert np.array_equal(view.cpu().numpy(), want)
