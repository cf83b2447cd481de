"""GPU parity of the batched, culled Gauss-Newton launch, case by case (tests/track_cases.py), against the CPU oracle's plain per-tracker
Odometry.track -- which knows nothing of batches, slots, boxes or hints.

Per case the SAME api.Odometry objects are re-prepared step after step, so from step 1 on their hint is live and the ICP reduction runs on
the culled-slot mapping (icp_reduce_body, the box_blocks > 0 branch); every case asserts through cf_odom_last_launch_shape that it did.
Everything is compared bit for bit: culled == unculled == oracle.

Where the launcher is specified to drop the culled-slot mapping (launch_icp_rgbres), and what the tests therefore expect:
  * step 0 of every case: no hint yet (icp_blocks == 0 everywhere);
  * trackers with culling off (the full-image tracker of the batched cases), and rgb_only (no ICP slots): 0;
  * pyramid=False: levels 1 and 2 do not run: 0 there;
  * the LAST level-0 iteration writes the error surfaces.  It keeps the mapping only when a culled tracker of the call has a surface,
    which a launch of its own then writes (IcpArgs::flags 3): icp_blocks_err > 0 in interior_320, narrow_208x156 and batch_mixed_5;
    without one (flags 1) that launch runs every tracker on the whole-image mapping: icp_blocks_err == 0 in all other cases;
  * the Gram form and row bands are not part of this table (tests/test_icp_gram_gpu.py, tests/test_distributed_gpu.py).
"""
import numpy as np
import pytest

import track_cases as tc

pytestmark = pytest.mark.gpu

_ctxs = {}


@pytest.fixture(scope="module")
def contexts():
    """one Context per image size, 32 trackers each (batch_17_rejected must get past the max_models check to reach kMaxBatch)"""
    from co_fusion_amd import api

    def get(case):
        if case.size not in _ctxs:
            cam = tc.camera(case)
            _ctxs[case.size] = api.Context(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, max_models=32)
        return _ctxs[case.size]
    yield get
    for c in _ctxs.values():
        c.close()
    _ctxs.clear()


class Run:
    """the trackers of one case on the GPU: prepared and tracked step by step on the same Odometry objects"""

    def __init__(self, ctx, case, cull, order=None):
        from co_fusion_amd import api
        self.ctx, self.case = ctx, case
        self.order = list(order) if order is not None else list(range(len(case.trackers)))
        self.od = {}
        for k in self.order:
            self.od[k] = api.Odometry(ctx)
            self.od[k].set_culling(cull and case.trackers[k].cull)
        self.err = {}

    def close(self):
        for o in self.od.values():
            o.close()

    def prepare(self, s):
        ctx, case, d = self.ctx, self.case, self.ctx.to_device
        fi = tc.frame_inputs(case, s)
        rgba_prev, rgba_cur, depth = d(fi["rgba_prev"]), d(fi["rgba_cur"]), d(fi["d_cur"])
        pyr = ctx.depth_pyramid(depth)
        self.starts = {}
        for k in self.order:
            ti = tc.tracker_inputs(case, k, s)
            g = self.od[k]
            g.init_first_rgb(rgba_prev)
            g.init_icp_model(d(ti["v4"]), d(ti["n4"]), ti["pose"])
            g.init_rgb_model(d(ti["img"]))
            if case.batched and k != self.order[0]:
                # all trackers of a frame track the same frame: the first one computes its maps (and the per-run depth intervals the culled
                # reduction tests), the others share them -- the frame-map path of a frame with several models
                g.share_frame_maps(self.od[self.order[0]])
            else:
                g.init_icp(pyr, tc.CUTOFF)
            g.init_rgb(rgba_cur)
            self.starts[k] = ti["start"]
            if case.err:
                self.err[k] = ctx.empty((case.size[1], case.size[0])); self.err[k].zero_()

    def track_single(self, s):
        """Odometry.track per tracker -> {k: (trans, rot, stats)}"""
        self.prepare(s)
        out = {}
        for k in self.order:
            st = self.starts[k]
            out[k] = self.od[k].track(st[:3, 3], st[:3, :3], err_surface=self.err.get(k), **tc.track_opts(self.case))
        return out

    def enqueue_batch(self, s, extra=(), prepare=True):
        if prepare:
            self.prepare(s)
        ods = [self.od[k] for k in self.order] + list(extra)
        poses = [self.starts[k] for k in self.order] + [self.starts[self.order[0]]] * len(extra)
        errs = [self.err[k] for k in self.order] if self.case.err else None
        self.ctx.track_batch(ods, poses, err_surfaces=errs, **tc.track_opts(self.case))

    def track_batch(self, s, fetch=None, prepare=True):
        """one Context.track_batch call, then Odometry.fetch of every tracker (or of `fetch` only)"""
        self.enqueue_batch(s, prepare=prepare)
        return {k: self.od[k].fetch() for k in (self.order if fetch is None else fetch)}

    def track(self, s, fetch=None):
        return self.track_batch(s, fetch) if self.case.batched else self.track_single(s)


def _same_as_oracle(case, k, s, got, err, what):
    tr, rot, st = got
    o = tc.oracle_step(case, k, s)
    assert tr.tobytes() == o["trans"].tobytes(), f"{what}: translation {tr} != oracle {o['trans']}"
    assert rot.tobytes() == o["rot"].tobytes(), f"{what}: rotation differs from the oracle's by {np.abs(rot - o['rot']).max()}"
    assert st.last_icp_count == o["icp_count"], f"{what}: ICP count {st.last_icp_count} != {o['icp_count']}"
    assert st.last_rgb_count == o["rgb_count"], f"{what}: RGB count {st.last_rgb_count} != {o['rgb_count']}"
    assert st.so3_iterations == o["so3_iterations"], what
    if tc.track_opts(case).get("so3", True):   # the pre-alignment's statistics, bit for bit (0 / 0 where it does not run)
        assert np.float32(st.last_so3_error).tobytes() == o["so3_error"].tobytes(), f"{what}: SO3 error {st.last_so3_error} != {o['so3_error']}"
        assert np.float32(st.last_so3_count).tobytes() == o["so3_count"].tobytes(), f"{what}: SO3 count {st.last_so3_count} != {o['so3_count']}"
    assert np.array_equal(np.array(st.lastA), o["lastA"]), f"{what}: lastA"
    assert np.array_equal(np.array(st.lastb), o["lastb"]), f"{what}: lastb"
    np.testing.assert_allclose(st.last_icp_error, o["icp_error"], rtol=1e-6, err_msg=what)
    if case.err:
        e = err.cpu().numpy()
        assert e.tobytes() == o["err"].tobytes(), f"{what}: error surface, {np.count_nonzero(e != o['err'])} pixels differ"


def _same_stats(a, b, what):
    (ta, ra, sa), (tb, rb, sb) = a, b
    assert ta.tobytes() == tb.tobytes() and ra.tobytes() == rb.tobytes(), f"{what}: pose"
    assert (sa.last_icp_count, sa.last_rgb_count, sa.so3_iterations) == (sb.last_icp_count, sb.last_rgb_count, sb.so3_iterations), what
    assert np.array_equal(np.array(sa.lastA), np.array(sb.lastA)) and np.array_equal(np.array(sa.lastb), np.array(sb.lastb)), f"{what}: lastA / lastb"


def _structure(case, run, k, s, got, what):
    """the box, the pixels visited and the launch shape of tracker k after step s of a CULLED run"""
    W, H = case.size
    tr = case.trackers[k]
    ti = tc.tracker_inputs(case, k, s)
    st = got[2]
    box = list(st.cull_box)
    icp_blocks, res_blocks, icp_err = run.od[k].last_launch_shape()
    opts = tc.track_opts(case)
    levels = [0, 1, 2] if opts.get("pyramid", True) else [0]
    if not tr.cull:
        assert box == [0, 0, W - 1, H - 1], f"{what}: an unculled tracker reports the whole image, not {box}"
        assert icp_blocks == [0, 0, 0] and icp_err == 0, f"{what}: an unculled tracker on the culled-slot mapping {icp_blocks}"
        assert res_blocks == [0, 0, 0], f"{what}: an unculled tracker on compact residual slots {res_blocks}"
        return
    if tr.masks[s] == tc.EMPTY:
        assert box[0] > box[2], f"{what}: an empty prediction must give an empty box, not {box}"
    else:
        # the box is the screen box of the LAST iteration, in the camera that iteration started from: the mask's rectangle seen from the
        # tracked pose, which is one converged Gauss-Newton update (well under a pixel) further on -- hence rounded inwards
        x0, y0, x1, y1 = tc.projected_rect(case, k, s, got[0], got[1])
        assert box[0] <= x0 and box[1] <= y0 and box[2] >= x1 and box[3] >= y1, \
            f"{what}: box {box} does not contain the mask {ti['rect']} as the tracked pose sees it {(x0, y0, x1, y1)}"
        visited = run.od[k].level0_visited()[0]
        if tc.uses_icp(case):   # the library's run table of the final box against the documented formula, recomputed here
            assert visited == min(64 * tc.cull_runs_total(box, 0, W, H), W * H), f"{what}: {visited} pixels visited for box {box}"
        if tr.masks[s] is not tc.FULL:
            area = (min(box[2], W - 1) - max(box[0], 0) + 1) * (min(box[3], H - 1) - max(box[1], 0) + 1)
            assert area < W * H, f"{what}: the box {box} culls nothing"
            if tc.uses_icp(case):
                assert visited < W * H, f"{what}: {visited} pixels visited, the whole image"
    # the culled-slot branch must have been taken: a run that silently falls back to the whole image is a failure, not a pass
    if s == 0 or not tc.uses_icp(case):
        assert icp_blocks == [0, 0, 0] and icp_err == 0, f"{what}: no hint / no ICP slots, but icp_blocks {icp_blocks} / {icp_err}"
    else:
        for l in range(3):
            if l in levels:
                assert icp_blocks[l] > 0, f"{what}: level {l} ran on the whole-image mapping (icp_blocks {icp_blocks}): the culled-slot branch was not taken"
                assert icp_blocks[l] % 8 == 0, what
            else:
                assert icp_blocks[l] == 0, what
        assert (icp_err > 0) == case.err, f"{what}: error-surface iteration icp_blocks_err {icp_err}, error surface requested: {case.err}"
    # ... and the residual pass: 0 (one workgroup per record slot of the level) where there is no count from a fetched previous call to
    # size it from, or no RGB term.  (With a count, residual_blocks_for's seen + 25 % + 2 workgroups are taken where they are fewer than
    # the level's slots; `seen` is not exposed, so the figure is not asserted beyond its sign.)
    if s == 0 or not tc.uses_rgb(case):
        assert res_blocks == [0, 0, 0], f"{what}: residual_blocks {res_blocks} without a count to size them from"
    assert min(res_blocks) >= 0, what
    return icp_blocks


LAUNCHES = [(256, 1), (1024, 1), (64, 4)]


@pytest.mark.parametrize("launch", LAUNCHES, ids=lambda l: f"{l[0]}x{l[1]}")
@pytest.mark.parametrize("name", tc.SINGLE)
def test_single_tracker_case(contexts, name, launch):
    """culled == unculled == oracle for every step; the culled-slot branch is taken from step 1 on; under three workgroup shapes (wpb and
    the run stride follow the workgroup size)"""
    case = tc.BY_NAME[name]
    ctx = contexts(case)
    W, H = case.size
    ctx.set_icp_launch(*launch)
    runs = []
    try:
        culled, plain = Run(ctx, case, True), Run(ctx, case, False)
        runs = [culled, plain]
        for s in range(case.steps):
            what = f"{name} step {s} launch {launch}"
            a = culled.track(s)[0]
            _same_as_oracle(case, 0, s, a, culled.err.get(0), what + " (culled)")
            icp_blocks = _structure(case, culled, 0, s, a, what)
            b = plain.track(s)[0]
            _same_as_oracle(case, 0, s, b, plain.err.get(0), what + " (unculled)")
            _same_stats(a, b, what + ": culled vs unculled")
            assert list(b[2].cull_box) == [0, 0, W - 1, H - 1] and plain.od[0].last_launch_shape()[0] == [0, 0, 0], what
            if case.trackers[0].masks[s] == tc.EMPTY:
                st = tc.tracker_inputs(case, 0, s)["start"]
                assert a[0].tobytes() == st[:3, 3].tobytes(), f"{what}: translation moved"
                if not tc.track_opts(case).get("so3", True):   # (with it the rotation is the pre-alignment's, the oracle's bits: asserted above)
                    assert a[1].tobytes() == np.ascontiguousarray(st[:3, :3]).tobytes(), f"{what}: rotation moved"
                assert a[2].last_icp_count == 0 and a[2].last_rgb_count == 0, what
            if name == "whole_image" and s > 0:
                # capped at the full grid of the launch (launch_icp_rgbres: `full`, at the level's pixels per lane)
                for l in range(3):
                    ppt = launch[1] if launch[1] else (2 if l == 0 else 1)
                    n = (W >> l) * (H >> l)
                    full = (((n + launch[0] * ppt - 1) // (launch[0] * ppt)) + 7) // 8 * 8
                    assert 0 < icp_blocks[l] <= full, f"{what}: level {l}: {icp_blocks[l]} workgroups, the full grid has {full}"
                    if launch == (64, 4):   # one wave per workgroup: half the image's runs + 25 % are more workgroups than the grid of 256 pixels each
                        assert icp_blocks[l] == full, f"{what}: level {l}: {icp_blocks[l]} workgroups, not capped at the full grid's {full}"
            if name == "grown" and s > 0:
                # the launch was sized from step 0's small box: more than two runs per wave are left, the walk-on loop iterates
                total = tc.cull_runs_total(list(a[2].cull_box), 0, W, H)
                assert total > 2 * (launch[0] // 64) * icp_blocks[0], \
                    f"{what}: {total} runs for {icp_blocks[0]} workgroups of {launch[0] // 64} waves: no wave walks more than two runs"
    finally:
        ctx.set_icp_launch(256, 1)
        for r in runs:
            r.close()


def _batched(contexts, name, order=None, launch=(256, 1)):
    case = tc.BY_NAME[name]
    ctx = contexts(case)
    ctx.set_icp_launch(*launch)
    runs = []
    try:
        culled, plain = Run(ctx, case, True, order), Run(ctx, case, False, order)
        runs = [culled, plain]
        for s in range(case.steps):
            a, b = culled.track(s), plain.track(s)
            for k in culled.order:
                what = f"{name} step {s} tracker {k} (position {culled.order.index(k)} of {culled.order})"
                _same_as_oracle(case, k, s, a[k], culled.err.get(k), what + " (culled)")
                _structure(case, culled, k, s, a[k], what)
                _same_as_oracle(case, k, s, b[k], plain.err.get(k), what + " (unculled)")
    finally:
        ctx.set_icp_launch(256, 1)
        for r in runs:
            r.close()


@pytest.mark.parametrize("launch", LAUNCHES, ids=lambda l: f"{l[0]}x{l[1]}")
def test_batch_mixed_5(contexts, launch):
    _batched(contexts, "batch_mixed_5", launch=launch)


@pytest.mark.parametrize("gn_mode", [0, 2])
def test_batch_mixed_5_gn_modes(contexts, gn_mode):
    """the same case, the same comparison with the oracle, under the two other data paths of the RGB step (cf_set_gn_mode 0: DataTerm records and
    rgb_step_kernel, the culled trackers' error surfaces by a launch of their own; 2: rgb_step_solve_kernel, the step's last workgroup solves),
    which share their sums with the default path's kernels.  Mode 2 needs workgroups dealt round-robin over 8 XCDs: refused with CF_ESTATE elsewhere."""
    from co_fusion_amd import api
    ctx = contexts(tc.BY_NAME["batch_mixed_5"])
    try:
        ctx.set_gn_mode(gn_mode)
    except api.CofusionError as e:
        if gn_mode == 2 and "cf_set_gn_mode 2:" in str(e):   # the library's own refusal (CF_ESTATE): no round-robin placement here
            pytest.skip(str(e))
        raise
    try:
        _batched(contexts, "batch_mixed_5", launch=LAUNCHES[0])
    finally:
        ctx.set_gn_mode(1)


@pytest.mark.parametrize("order", list(tc.BATCH_ORDERS), ids=lambda o: o)
def test_batch_orders(contexts, order):
    """every order is compared with the oracle's per-tracker result, which has no order: a tracker's result is independent of its position"""
    _batched(contexts, "batch_orders", order=tc.BATCH_ORDERS[order])


def test_batch_9(contexts):
    _batched(contexts, "batch_9")


def test_batch_16(contexts):
    _batched(contexts, "batch_16")


@pytest.mark.parametrize("name", [c.name for c in tc.CASES if c.name.startswith("batch_opts_")])
def test_batch_opts(contexts, name):
    _batched(contexts, name)


def test_batch_17_rejected(contexts):
    """seventeen trackers in one call: CF_EINVAL from the host check, nothing enqueued, nothing prepared -- the trackers' pending results,
    hints and the stream are as before, so the valid sixteen-tracker call behind it gives the oracle's bits on the culled-slot mapping"""
    from co_fusion_amd import api
    case = tc.BY_NAME["batch_17_rejected"]
    ctx = contexts(case)
    run, plain = Run(ctx, case, True), Run(ctx, case, False)
    extra = api.Odometry(ctx)
    try:
        run.track(0)
        plain.track(0)
        with pytest.raises(api.CofusionError, match=r"error -1\b"):
            run.enqueue_batch(1, extra=[extra])
        a = run.track_batch(1, prepare=False)   # (the evidence that nothing was enqueued or re-prepared: this call's bits and launch shape)
        b = plain.track(1)
        for k in run.order:
            what = f"batch_17_rejected step 1 tracker {k}"
            _same_as_oracle(case, k, 1, a[k], None, what)
            _structure(case, run, k, 1, a[k], what)
            _same_stats(a[k], b[k], what + ": culled vs unculled")
    finally:
        extra.close()
        run.close()
        plain.close()


def test_batch_partial_fetch(contexts):
    """step 1 fetches two of the five trackers only; step 2 tracks all of them again (the library drains the unfetched calls first) and
    must still give the oracle's bits, with every culled tracker on the culled-slot mapping"""
    case = tc.BY_NAME["batch_partial_fetch"]
    ctx = contexts(case)
    run, plain = Run(ctx, case, True), Run(ctx, case, False)
    try:
        for s, fetch in ((0, None), (1, tc.PARTIAL_FETCH), (2, None)):
            a, b = run.track(s, fetch), plain.track(s, fetch)
            for k in (run.order if fetch is None else fetch):
                what = f"batch_partial_fetch step {s} tracker {k}"
                _same_as_oracle(case, k, s, a[k], None, what)
                _structure(case, run, k, s, a[k], what)
                _same_stats(a[k], b[k], what + ": culled vs unculled")
    finally:
        run.close()
        plain.close()


# ---------------------------------------------------------------- exact sums against the bignum reference (tests/icp_rows_ref.py)
@pytest.mark.parametrize("poisoned", [False, True], ids=["clean", "nan_inf_at_wave_boundaries"])
@pytest.mark.parametrize("name", ["scene", "clamp", "ties"])
def test_icp_step_sums_equal_the_bignum_reference(contexts, name, poisoned):
    """cf_icp_step at 80 x 60 against sums formed with exact rationals and unbounded integers -- not against the oracle, which shares the
    kernels' way of computing RNE(clamp(a) * clamp(b) * 2^32): an ordinary scene, rows beyond the clamp, exact ties of both signs, and
    NaN / +-Inf at lanes 0, 63 and 64, which must be gated out and leave count and sums otherwise unaffected"""
    from co_fusion_amd import api
    import icp_rows_ref as ex
    ctx = contexts(tc.BY_NAME["interior_320"])
    inp = ex.INPUTS[name]()
    if poisoned:
        inp, _ = ex.poison(inp)
    rows, found, sums = ex.reference(inp)
    if not poisoned:
        ex.check_preconditions(name, rows, found)
    d = ctx.to_device
    for launch in LAUNCHES:
        ctx.set_icp_launch(*launch)
        try:
            _, _, res, got = ctx.icp_step(inp["Rcurr"], inp["tcurr"], d(inp["vc"]), d(inp["nc"]), inp["Rprev_inv"], inp["tprev"],
                                          api.Cam(*[float(v) for v in inp["cam"]]), d(inp["vp"]), d(inp["npv"]), inp["dist"], inp["angle"])
        finally:
            ctx.set_icp_launch(256, 1)
        assert [int(v) for v in got[:29]] == sums, f"{name} launch {launch}: words {[k for k in range(29) if int(got[k]) != sums[k]]} differ"
        assert res[1] == sums[28]


def test_right_edge_of_the_run_table_on_a_64_column_boundary(contexts):
    """cull_runs widens the box by one pixel on every side before it counts runs: `bx1 = (box[2] >> L) + 1`.  The column it adds holds no
    inlier (the box is already the dilated frustum piece), so no sum can show whether it is there; the run table can, where that column
    starts a new run: box[2] % 64 == 63 at level 0 of a 320-wide image.  A sweep of the mask's right edge over 130 columns moves
    the box's right edge over two such boundaries; for every mask the pixels the library says it visited must be the documented formula's,
    and the sweep must have met the boundary (if it has not, widen the sweep)."""
    import dataclasses
    base = tc.BY_NAME["interior_320"]
    ctx = contexts(base)
    W, H = base.size
    on_boundary = 0
    for x1 in range(70, 200):
        case = dataclasses.replace(base, name=f"edge_{x1}", err=False, trackers=(tc.Tracker(((40, x1, 60, 150),), seed=15),), steps=1)
        run = Run(ctx, case, True)
        try:
            got = run.track(0)[0]
            box = list(got[2].cull_box)
            visited = run.od[0].level0_visited()[0]
        finally:
            run.close()
        assert got[2].last_icp_count >= 100, (x1, got[2].last_icp_count)
        assert 0 <= box[0] and box[2] < W - 2, f"mask right edge {x1}: the box {box} is clamped, the sweep does not test what it is meant to"
        assert visited == 64 * tc.cull_runs_total(box, 0, W, H), f"mask right edge {x1}: {visited} pixels visited for box {box}"
        on_boundary += box[2] % 64 == 63
    assert on_boundary >= 1, "no box of the sweep ended on column 63 mod 64"
