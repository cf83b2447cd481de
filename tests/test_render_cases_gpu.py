"""GPU suite over the case table of the scene renderer (tests/render_cases.py): every case's calls run in order on one shared 96x64
render object (csrc/render.hip through cf_render), all of them enqueued before any output is read, and every output is compared
byte for byte with the restatement tests/render_ref.py and, off its ambiguity mask, with the f64 oracle tests/render_oracle.py.
Each case runs twice; the second run is byte-identical.  The CPU side of the table is tests/test_cpu_render_cases.py."""
import warnings

import numpy as np
import pytest

import render_cases as rc

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)


@pytest.fixture(scope="module")
def env():
    from co_fusion_amd import api, render as R
    ctx = api.Context(320, 240, 277.0, 277.0, 160.0, 120.0)
    renderers = {}          # by maximum size; the cases share the 96x64 one, so that one case's leftovers meet the next

    def renderer(size):
        if size not in renderers:
            renderers[size] = R.Renderer(ctx, *size)
        return renderers[size]
    yield dict(ctx=ctx, R=R, renderer=renderer)
    for r in renderers.values():
        r.close()
    ctx.close()


def _upload(env, call):
    """the surfel rows of all items of a call in one device buffer (one spare row behind the last); the cf_render items over it"""
    R = env["R"]
    rows = [it["surfels"] for it in call.items]
    buf = env["ctx"].to_device(np.concatenate(rows + [np.zeros((1, 12), np.float32)]))
    items, first = [], 0
    for it in call.items:
        n = len(it["surfels"])
        items.append(R.make_item(buf.data_ptr() + first * 48 if n else 0, n, it["pose"], it["thresh"], it["model_id"], it["mode"]))
        first += n
    return buf, items


def _view(R, v):
    return R.make_view(v["pose"], v["fx"], v["fy"], v["cx"], v["cy"], v["width"], v["height"], v.get("near", 0.0), v.get("far", 0.0),
                       v.get("flags", 0), v.get("tick", 1), v.get("time_delta", 2 ** 30 - 1))


def _run(env, case, uploads):
    """every call of the case enqueued in order without a host wait in between; then all outputs"""
    rnd = env["renderer"](case.size)
    outs = [rnd.render(_view(env["R"], c.view), items, c.modes, depth=c.depth, labels=c.labels) for c, (_, items) in zip(case.calls, uploads)]
    return [[t.cpu().numpy() for t in o] for o in outs]


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_matches_the_restatement_and_the_oracle(env, name):
    case = rc.case(name)
    uploads = [_upload(env, c) for c in case.calls]
    first = _run(env, case, uploads)
    second = _run(env, case, uploads)
    for k, (call, got, again, (want, gid, orc)) in enumerate(zip(case.calls, first, second, rc.reference(name))):
        what = f"{name} call {k} {call.note}"
        assert len(got) == len(want) == len(call.outputs())
        for o, g, a, w in zip(call.outputs(), got, again, want):
            assert g.shape == w.shape and g.dtype == w.dtype, (what, o)
            bad = np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)
            assert not bad.any(), f"{what} {o}: {np.count_nonzero(bad)} of {bad.size} bytes differ from the restatement"
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(g).view(np.uint8)), f"{what} {o}: second run differs"
        rc.against_oracle(call, got, orc, what)
        if call.labels:
            for px, py, label in call.probes:
                assert got[-1][py, px] == label, f"{what}: label {got[-1][py, px]} at ({px}, {py}), not {label}"


def test_a_ninth_colour_output_is_refused(env):
    from co_fusion_amd import api
    R = env["R"]
    call = rc.case("item_mode_and_eight_outputs").calls[0]
    buf, items = _upload(env, call)
    with pytest.raises(api.CofusionError, match="CF_RENDER_MAX_COLOUR"):
        env["renderer"](rc.SIZE).render(_view(R, call.view), items, call.modes + (R.GREY,))
    # nothing was enqueued and nothing is left behind: the same call with eight outputs is the expected one
    got = env["renderer"](rc.SIZE).render(_view(R, call.view), items, call.modes)
    want = rc.reference("item_mode_and_eight_outputs")[0][0]
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
