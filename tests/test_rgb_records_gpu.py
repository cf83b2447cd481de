"""GPU suite: the record-slot path of the photometric term on crafted images.

Every case of tests/rgb_cases.py goes through cf_rgb_records_step -- the compact residual pass (rgb_residual_body<true>, through the
{ICP || residual} launcher as an rgb_only call issues it) and the RGB step over the slots it leaves (rgb_slot_step_kernel under gn mode 1,
rgb_step_solve_kernel under mode 2) -- under the three launch shapes, and is compared with tests/rgb_rows_ref.py: numpy f32 rows, sums in
unbounded integers and exact rationals, nothing of the oracle.  What the cases cover is asserted on the CPU
(tests/test_cpu_rgb_cases.py); a failing case's name says which branch is wrong.

After the residual pass: per visited slot the multiset of records (sorted: the order inside a slot is schedule-dependent by design) and
the slot's count, every slot outside a culled range exactly as planted, the totals of accumulator words 29 / 30.  After the step: under
mode 1 all 32 totals of the RGB accumulator; under mode 2 state, twin and hot block byte for byte against cf_gn_solve_step fed the
reference's sums.  Integer or byte equality everywhere, no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import rgb_cases as rc
import rgb_rows_ref as rr
from co_fusion_amd import api

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
SHAPE_IDS = ["%dx%d" % s for s in rc.SHAPES]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(rc.COLS, rc.ROWS, 132.0, 132.0, 40.0, 30.0)
    c._rgb_images = {}
    yield c
    c.close()


@pytest.fixture
def mode(ctx, request):
    """the context under gn mode request.param for one test; skipped with the library's own refusal text where mode 2 is unavailable"""
    try:
        ctx.set_gn_mode(request.param)
    except api.CofusionError as e:
        if request.param == 2 and "cf_set_gn_mode 2:" in str(e):
            pytest.skip(str(e))
        raise
    yield request.param
    ctx.set_gn_mode(1)
    ctx.set_icp_launch(256, 0)


def images(ctx, c):
    """the case's eight images on the device, uploaded once"""
    if c.name not in ctx._rgb_images:
        ctx._rgb_images[c.name] = {f: ctx.to_device(np.array(getattr(c, f))) for f in ("cand", "next_depth", "last_depth", "last_image", "next_image", "cloud", "dIdx", "dIdy")}
    return ctx._rgb_images[c.name]


def gn_state(c):
    s = api.GnState()
    s.intr = api.Cam(float(c.fx), float(c.fy), c.cols / 2.0, c.rows / 2.0)
    s.width, s.height, s.icp, s.rgb, s.rgbOnly, s.icpWeight = c.cols, c.rows, 0, 1, int(c.rgb_only), 10.0
    eye = np.eye(3).reshape(9).tolist()
    for f in ("Rprev", "Rprev_inv", "Rcurr"):
        getattr(s, f)[:] = eye
    s.resultRt[:] = np.eye(4).reshape(16).tolist()
    s.krkInv[:] = [float(v) for v in c.krk]; s.kt[:] = [float(v) for v in c.kt]
    s.lastRGBError = FLT_MAX
    s.cull_z[:] = [float("-inf"), float("inf")]
    s.stats.cull_box[:] = [0, 0, c.cols - 1, c.rows - 1]
    return s


def make_system(ctx, c, threads):
    """-> (api.RgbSystem, what it points at: the planted slot counts and records, and copies of them as planted)"""
    y = api.RgbSystem()
    for f, t in images(ctx, c).items():
        setattr(y, f, t.data_ptr())
    y.no_counts = int(c.no_counts)
    if c.res_range is not None:
        y.ranged = 1; y.res_range[:] = [int(v) for v in c.res_range]; y.res_blocks = int(c.res_blocks)
    counts, recs = rc.plant(c, threads)
    hold = dict(counts=counts.copy(), recs=recs.copy(), counts0=counts.copy(), recs0=recs.copy())
    y.records = hold["recs"].ctypes.data; y.slot_counts = hold["counts"].ctypes.data
    y.count_seed[:] = [int(v) for v in c.count_seed]; y.sigma_seed[:] = [int(v) for v in c.sigma_seed]
    y.state = gn_state(c)
    C.memset(C.byref(y.twin), 0x5A, C.sizeof(api.GnState))
    C.memset(y.hot, 0xA5, C.sizeof(y.hot))
    return y, hold


def run(ctx, cases, threads, ppt, next_level, last_of_level):
    ctx.set_icp_launch(threads, ppt)
    made = [make_system(ctx, c, threads) for c in cases]
    arr = (api.RgbSystem * len(made))(*[m[0] for m in made])
    before = [api.RgbSystem.from_buffer_copy(y) for y in arr]
    c0 = cases[0]
    ctx.rgb_records_step(arr, c0.cols, c0.rows, float(c0.max_dd), float(c0.sobel), float(c0.fx), float(c0.fy), next_level, last_of_level)
    return arr, before, [m[1] for m in made]


def check_residual(tag, c, threads, y, hold):
    """stage (a): records per slot as multisets, slot counts, untouched slots of a culled tracker, the two totals"""
    ref = rc.reference(c.name, threads)
    px = ref["slot_px"]
    bad = []
    for s in range(ref["n_slots"]):
        lo, hi = s * px, min((s + 1) * px, c.n)
        if s in ref["slots"]:
            want = ref["slots"][s]
            if int(hold["counts"][s]) != len(want):
                bad.append("slot %d: count %d, reference %d" % (s, hold["counts"][s], len(want)))
            elif sorted(int(v) for v in hold["recs"][lo:lo + len(want)]) != want:
                bad.append("slot %d: its %d records differ from the reference's" % (s, len(want)))
        elif hold["counts"][s] != hold["counts0"][s] or not np.array_equal(hold["recs"][lo:hi], hold["recs0"][lo:hi]):
            bad.append("slot %d lies outside the range and was written" % s)
    if (int(y.count_total), int(y.sigma_total)) != (ref["count_total"], ref["sigma_total"]):
        bad.append("totals of words 29 / 30: %d, %d; reference %d, %d" % (y.count_total, y.sigma_total, ref["count_total"], ref["sigma_total"]))
    assert not bad, "%s [%s]: %s" % (tag, c.aims, "; ".join(bad[:6]))
    return ref


def check_step(ctx, tag, gn_mode, cases, threads, arr, before, refs, next_level, last_of_level):
    if gn_mode == 1:
        for c, y, ref in zip(cases, arr, refs):
            got = np.array(y.rgb_sums, np.int64)
            assert np.array_equal(got, ref["sums64"]), "%s, %s [%s]: words %s of rgb_acc differ from the reference integers (F = %d, sigma = %s)" % (
                tag, c.name, c.aims, np.flatnonzero(got != ref["sums64"]).tolist(), ref["F"], ref["sigma"])
        return
    # mode 2: the step's last workgroup has solved -- against cf_gn_solve_step fed the reference's sums and the same state and twin
    want = []
    for y0, ref in zip(before, refs):
        g = api.GnSystem()
        acc = np.zeros((64, 32), np.int64); acc[0, 29] = ref["count_total"]; acc[0, 30] = ref["sigma_total"]
        C.memmove(g.icp_acc, acc.ctypes.data, acc.nbytes)
        acc = np.zeros((64, 32), np.int64); acc[0] = ref["sums64"]
        C.memmove(g.rgb_acc, acc.ctypes.data, acc.nbytes)
        g.state = y0.state; g.twin = y0.twin
        want.append(g)
    want = ctx.gn_solve_step((api.GnSystem * len(want))(*want), next_level, last_of_level)
    for c, y, w in zip(cases, arr, want):
        for f in ("state", "twin", "hot"):
            assert bytes(getattr(y, f)) == bytes(getattr(w, f)), "%s, %s [%s]: %s after the solve differs from cf_gn_solve_step on the reference's sums" % (tag, c.name, c.aims, f)
        assert y.state.solves == 1 and not any(y.rgb_sums)


MODES = pytest.mark.parametrize("mode", [1, 2], indirect=True, ids=["gn1", "gn2"])


@MODES
@pytest.mark.parametrize("shape", rc.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", rc.NAMES)
def test_case(ctx, mode, name, shape):
    c = rc.case(name)
    if (c.cols, c.rows) != (rc.COLS, rc.ROWS):
        assert c.n <= rc.COLS * rc.ROWS
    tag = "%s, %d threads, gn mode %d" % (name, shape[0], mode)
    arr, before, holds = run(ctx, [c], shape[0], shape[1], c.next_level, c.last_of_level)
    ref = check_residual(tag, c, shape[0], arr[0], holds[0])
    check_step(ctx, tag, mode, [c], shape[0], arr, before, [ref], c.next_level, c.last_of_level)


@MODES
@pytest.mark.parametrize("shape", rc.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("batch", list(rc.BATCHES))
def test_batch(ctx, mode, batch, shape):
    """several different cases as the systems of one call: a system's result does not depend on its neighbours or its position"""
    cases = [rc.case(n) for n in rc.BATCHES[batch]]
    tag = "%s, %d threads, gn mode %d" % (batch, shape[0], mode)
    arr, before, holds = run(ctx, cases, shape[0], shape[1], 1, False)
    refs = [check_residual("%s, system %d (%s)" % (tag, k, c.name), c, shape[0], arr[k], holds[k]) for k, c in enumerate(cases)]
    check_step(ctx, tag, mode, cases, shape[0], arr, before, refs, 1, False)


@pytest.mark.parametrize("name", rc.MODE0)
def test_mode0_path_gives_the_reference_integers(ctx, name):
    """the DataTerm image and rgb_step_kernel (cf_rgb_residual + cf_rgb_step, what cf_set_gn_mode 0 runs) against the same reference: the
    old path's oracle-independent check.  These cases' candidate masks ARE the preparation's rule under `min_scale`."""
    c = rc.case(name)
    ref = rc.reference(name, 64)
    im = images(ctx, c)
    two = lambda t: t.reshape(c.rows, c.cols)
    cor, sig, cnt = ctx.rgb_residual(c.min_scale, two(im["dIdx"]), two(im["dIdy"]), two(im["last_depth"]), two(im["next_depth"]), two(im["last_image"]),
                                     two(im["next_image"]), float(c.max_dd), c.kt, c.krk)
    dt = cor.cpu().numpy().view(api.DATATERM).reshape(-1)
    assert np.array_equal(dt["valid"] != 0, ref["valid"])
    k = np.flatnonzero(ref["valid"])
    assert np.array_equal(dt["zero_y"][k].astype(np.int64) * c.cols + dt["zero_x"][k], ref["res"]["g"][k])
    assert np.array_equal(dt["diff"][k], ref["res"]["diff"][k].astype(np.float32))
    assert (cnt, sig) == (ref["count"], ref["sq32"])
    _, _, sums = ctx.rgb_step(cor, float(ref["sigma"]), im["cloud"], float(c.fx), float(c.fy), two(im["dIdx"]), two(im["dIdy"]), float(c.sobel))
    assert np.array_equal(sums[:29], ref["sums64"][:29]), np.flatnonzero(sums[:29] != ref["sums64"][:29])


def test_refusals(ctx):
    c = rc.case("depth_gate")
    ctx.set_gn_mode(1); ctx.set_icp_launch(256, 0)
    y, hold = make_system(ctx, c, 256)
    args = (float(c.max_dd), float(c.sobel), float(c.fx), float(c.fy), 1, 0)
    call = lambda n, arr, cols, rows: ctx.lib.cf_rgb_records_step(ctx.h, n, arr, cols, rows, C.c_float(args[0]), C.c_float(args[1]), C.c_float(args[2]),
                                                                 C.c_float(args[3]), args[4], args[5])
    many = (api.RgbSystem * 17)(*([y] * 17))
    assert call(0, many, c.cols, c.rows) == -1 and call(17, many, c.cols, c.rows) == -1            # n outside 1..16
    assert call(1, many, 78, 60) == -1                                                             # cols % 4 != 0
    assert call(1, many, 84, 60) == -1 and call(1, many, 80, 64) == -1                             # cols * rows above the context's size
    assert call(1, None, c.cols, c.rows) == -1
    try:                                                                                           # mode 2 where the library refuses it
        ctx.set_gn_mode(2)
    except api.CofusionError as e:
        assert "cf_set_gn_mode 2:" in str(e)
    ctx.set_gn_mode(0)                                                                             # no record slots under mode 0
    assert call(1, many, c.cols, c.rows) == -1
    ctx.set_gn_mode(1)
    # nothing was enqueued or written: the planted arrays are as they were, and a valid call is unaffected
    assert np.array_equal(hold["counts"], hold["counts0"]) and np.array_equal(hold["recs"], hold["recs0"])
    arr, before, holds = run(ctx, [c], 256, 0, 1, False)
    ref = check_residual("after the refusals", c, 256, arr[0], holds[0])
    check_step(ctx, "after the refusals", 1, [c], 256, arr, before, [ref], 1, False)
    torch.cuda.synchronize()
