"""GPU parity of the fill-in and the fill ratio that cf_models_frame_passes evaluates inside its last launch for the items that ask
for it (cf_model_pass::fill_in; csrc/surf_splat_dev.h: splat_resolve_kernel with SplatFillArgs -> fill_in_px, fill_ratio_sample, the
completion ticket) against twin models driven through the separate calls: the chain's statements per model, then
cf_model_prefetch_fill_ratio + cf_model_perform_fill_in (fill_ratio_kernel, fill_in_kernel).  Bit for bit, NaN equal to NaN:
the splat buffers 4..7, the fill maps 8..10, the two counts in device memory, and the host's answers (cf_model_requires_fill_in reads
the pinned copy of the counts: asked at 0.75 and on both sides of covered / total, which pins that copy to the device's counts).

Every call carries two models: one that asks for the fill-in and one that does not (its fill maps stay untouched and it has no pending
ratio).  Each call is made twice in a row on the same models, so a count or a ticket left over from the first would show in the second.
Where the chain does not fuse, the covered count is also checked against the CPU oracle's prediction sampled here in numpy.

Shapes: 80x60 (4 x 3 samples, on several workgroups), 176x100 (8 x 5) and 16x4 (cols / 20 == 0: both counts 0).
"""
import numpy as np
import pytest

import common
import surfel_cases as sc
from co_fusion_amd import synth
from test_surfel_chain_gpu import _item, _per_model
from test_surfel_gpu import _same

pytestmark = pytest.mark.gpu

SHAPES = [(80, 60), (176, 100), (16, 4)]
# (map of the model that fills in, (passthrough_geom, passthrough_rgb), do_fuse)
CASES = [("part", (0, 0), 0), ("part", (0, 1), 1), ("part", (1, 1), 0), ("empty", (0, 0), 0), ("full", (0, 0), 0), ("full", (0, 1), 1)]
TIME = 42


def _scene(shape):
    w, h = shape
    cam = synth.Camera.scaled(w, h)
    fr = sc.plane_frame(shape, cam, 900 + w)
    base = sc._plane_base(cam, fr)   # surfel id = column * rows + row, confident, every pixel covered
    # the frame the chain runs on: the plane with holes in its depth (the fill-in's normals and vertices meet z = 0)
    d = fr.depth.copy()
    d[h // 2:h // 2 + 3, w // 3:w // 3 + 5] = 0
    d[0, :3] = 0; d[h - 1, w - 2:] = 0
    frame = sc.refilter(sc.Frame(fr.rgba, d, None, fr.mask))
    col, row = np.arange(base.shape[0]) // h, np.arange(base.shape[0]) % h
    part = base[(col < (6 * w) // 10) & (row < (7 * h) // 10)].copy()
    other = base[(col >= w // 4) & (row >= h // 3)].copy()
    return cam, frame, dict(part=part, empty=np.zeros((0, sc.SURFEL), np.float32), full=base.copy(), other=other)


def _nearest_texel(u, size):
    return int(np.clip(np.floor(np.float32(u) * np.float32(size)), 0, size - 1))


def _sampled_count(image, shape):
    """fill_ratio_kernel on a host image: (covered, total)"""
    w, h = shape
    dw, dh = w // 20, h // 20
    covered = 0
    for j in range(dh):
        for i in range(dw):
            sx = _nearest_texel((np.float32(i) + np.float32(0.5)) / np.float32(dw), w)
            sy = _nearest_texel((np.float32(j) + np.float32(0.5)) / np.float32(dh), h)
            covered += bool((image[sy, sx, :3] > 0).all())
    return covered, dw * dh


def _host_quotient_is(m, covered, total):
    """cf_model_requires_fill_in answers (float)covered / (float)total < ratio from the host's copy of the counts"""
    if total == 0:
        return not m.requires_fill_in(np.float32(np.inf))   # 0 / 0: no ratio is above it
    q = np.float32(covered) / np.float32(total)
    return (not m.requires_fill_in(float(q))) and m.requires_fill_in(float(np.nextafter(q, np.float32(2))))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("which,flags,do_fuse", CASES)
def test_fill_in_inside_the_chain(shape, which, flags, do_fuse):
    from co_fusion_amd import api, model as M
    cam, frame, maps = _scene(shape)
    case = sc.Case("fill", shape, cam, [maps[which], maps["other"]], {"f": frame}, [], max_surfels=1 << 15)
    ctx = api.Context(shape[0], shape[1], cam.fx, cam.fy, cam.cx, cam.cy, max_models=8)
    dev = lambda a: ctx.to_device(np.array(a))
    fr = dict(rgba=dev(frame.rgba), mask=dev(frame.mask), depth=dev(frame.depth), depth_filt=dev(frame.depth_filt))
    chain = [M.Model(ctx, case.max_surfels) for _ in case.maps]
    twins = [M.Model(ctx, case.max_surfels) for _ in case.maps]
    try:
        for ms in (chain, twins):
            for m, s in zip(ms, case.maps):
                m.upload_map(s)
        untouched = [chain[1].buffer(k).copy() for k in (8, 9, 10)]
        surf = maps[which]
        for rep in range(2):
            what = f"{shape} {which} {flags} fuse {do_fuse}, call {rep}"
            items = [sc.Item(0, "f", common.perturbed_pose(1), TIME + rep, do_fuse=do_fuse), sc.Item(1, "f", common.perturbed_pose(2), TIME + rep, do_fuse=do_fuse)]
            asked = dict(_item(chain[0], items[0], fr), fill_in=1, passthrough_geom=flags[0], passthrough_rgb=flags[1])
            M.frame_passes(ctx, [asked, _item(chain[1], items[1], fr)], sc.DEPTH_CUTOFF, case.outlier, case.time_delta)
            for it in items:
                _per_model(twins[it.model], it, fr, case)
            twins[0].prefetch_fill_ratio()
            twins[0].perform_fill_in(fr["rgba"], fr["depth_filt"], bool(flags[0]), bool(flags[1]))
            for k in range(4, 11):
                _same(chain[0].buffer(k), twins[0].buffer(k), f"{what}: buffer {k}")
            for k in range(4, 8):
                _same(chain[1].buffer(k), twins[1].buffer(k), f"{what}: buffer {k} of the model that did not ask")
            for k, before in zip((8, 9, 10), untouched):
                _same(chain[1].buffer(k), before, f"{what}: fill map {k} of the model that did not ask")
            assert chain[1].fill_counts_device() is None
            got, want = chain[0].fill_counts_device(), twins[0].fill_counts_device()
            assert got is not None and want is not None
            covered, total = int(want[0]), int(want[1])
            assert (int(got[0]), int(got[1])) == (covered, total), f"{what}: device counts {got} != {want}"
            assert total == (shape[0] // 20) * (shape[1] // 20)
            assert chain[0].requires_fill_in(0.75) == twins[0].requires_fill_in(0.75), what
            assert _host_quotient_is(chain[0], covered, total) and _host_quotient_is(twins[0], covered, total), f"{what}: host counts"
            if not do_fuse:
                r = sc.oracle_item(case, items[0], surf)
                assert _sampled_count(r.splat[0], shape) == (covered, total), f"{what}: counts against the oracle's prediction"
            if which == "empty":
                assert covered == 0 and not chain[0].buffer(4).any()
            if which == "full" and not do_fuse:
                assert covered == total
            if shape == (16, 4):
                assert (covered, total) == (0, 0)
    finally:
        for m in chain + twins:
            m.close()
        ctx.close()
