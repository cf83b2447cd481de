"""GPU suite: the first launch of a tracking call (so3_prealign_kernel, csrc/track_so3_dev.h) on crafted image pairs.

Every case of tests/so3_cases.py goes through cf_so3_prealign_step -- the production launch on its own: 16 workgroups per system on
one XCD, meeting at the context's sync blocks -- and is compared with orc_so3_prealign_state, the loop of the oracle's tracking
function and the seeding behind it, BIT FOR BIT (NaN equal to NaN).  What the cases cover is asserted on the CPU
(tests/test_cpu_so3_cases.py); a failing case's name says which branch of the loop is wrong.

Besides the words the loop computes, every launch is checked for what the kernel does around it: the state hand-over (every word the
pinned host state held arrives in the device state, which the entry pre-fills with a pattern), the ICP / RGB statistics left alone,
the whole-image screen box, no fault, the hot block, and every word of every sync block zero again.  Batches are launched three times
on the same context with nothing reset in between, with and without the pre-alignment in turn, and every model of a batch is compared
with the same case launched alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import common
import orc
import so3_cases as sc
from co_fusion_amd import api
from gn_compare import expected_hot, raw, same, show

pytestmark = pytest.mark.gpu

OUTPUT = ("resultRt", "krkInv", "kt", "lastRGBError", "level_done", "residual")
SO3_STATS = ("so3_iterations", "last_so3_error", "last_so3_count")
HANDED = ("intr", "width", "height", "icp", "rgb", "rgbOnly", "icpWeight", "Rprev", "tprev", "Rprev_inv", "Rcurr", "tcurr", "solves", "pose_inv")
OTHER_STATS = ("last_icp_error", "last_icp_count", "last_rgb_error", "last_rgb_count", "lastA", "lastb")
FILL = 0xA5                          # what cf_so3_prealign_step fills the device states with before the launch
MODES = [(1, 2), (1, 0), (0, 2), (0, 0)]          # (do_so3, first_level): the schedule with and without the pyramid
MODE_IDS = ["so3-pyramid", "so3-level0", "plain-pyramid", "plain-level0"]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(160, 120, 132.0, 132.0, 79.5, 59.5, max_models=16)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def state_in(name, shape):
    """what the pinned host state of a tracker holds when its tracking call is enqueued, as bytes of api.GnState: the case's camera and
    size, distinct poses, and in every word the launch must overwrite a value it never produces"""
    c = sc.case(name, shape)
    seed = sc.CONTENT.index(name) * len(sc.SHAPES) + sc.SHAPES.index(shape)
    P, Q = common.perturbed_pose(100 + seed), common.perturbed_pose(200 + seed, trans=0.02, rot_deg=2.0)
    s = api.GnState()
    s.intr = api.Cam(c.intr.fx, c.intr.fy, c.intr.cx, c.intr.cy)
    s.width, s.height = shape
    s.icp, s.rgb, s.rgbOnly, s.icpWeight = 1, 1 + seed % 2, seed % 3 == 0, 10.0 + seed
    f = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1).tolist()
    s.Rprev[:] = f(P[:3, :3]); s.tprev[:] = f(P[:3, 3]); s.Rprev_inv[:] = f(P[:3, :3].T)
    s.Rcurr[:] = f(Q[:3, :3]); s.tcurr[:] = f(Q[:3, 3])
    s.pose_inv[:] = f(orc.inverse_pose(Q))
    s.solves = 7 + seed
    # overwritten by the launch
    s.resultRt[:] = np.arange(16, dtype=np.float64).tolist()
    s.krkInv[:] = [float(v) for v in range(20, 29)]; s.kt[:] = [30.0, 31.0, 32.0]
    s.lastRGBError, s.level_done = 1.5, 1
    s.residual[:] = [3.0, 4.0]; s.cull_z[:] = [1.0, 2.0]
    s.stats.so3_iterations, s.stats.last_so3_error, s.stats.last_so3_count = 5, 6.0, 7.0
    s.stats.cull_box[:] = [9, 9, 9, 9]
    s.stats.fault = 0
    # left alone by the launch
    s.stats.last_icp_error, s.stats.last_icp_count, s.stats.last_rgb_error, s.stats.last_rgb_count = 0.25 + seed, 1000.0 + seed, 0.5 + seed, 2000.0 + seed
    s.stats.lastA[:] = (np.arange(36) + 0.5 + seed).tolist(); s.stats.lastb[:] = (np.arange(6) - 0.5 - seed).tolist()
    return bytes(s)


@functools.lru_cache(maxsize=None)
def wanted(name, shape, do_so3, first_level):
    """the oracle's state after the launch"""
    c = sc.case(name, shape)
    s = api.GnState.from_buffer_copy(state_in(name, shape))
    o = orc.GnState()
    o.intr = orc.Cam(s.intr.fx, s.intr.fy, s.intr.cx, s.intr.cy)
    for k in ("width", "height", "icp", "rgb", "rgbOnly", "icpWeight", "lastRGBError", "level_done", "solves"):
        setattr(o, k, getattr(s, k))
    for k in ("Rprev", "tprev", "Rcurr", "tcurr", "resultRt", "krkInv", "kt", "residual"):
        C.memmove(getattr(o, k), getattr(s, k), C.sizeof(getattr(s, k)))
    for k in SO3_STATS:
        setattr(o.stats, k, getattr(s.stats, k))
    return orc.so3_prealign_state(o, c.last, c.next, do_so3, first_level)


class Images:
    """the level-2 images of the table on the device, uploaded once"""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, {}

    def __call__(self, c):
        if c.key not in self.held:
            self.held[c.key] = (self.ctx.to_device(c.last.copy()), self.ctx.to_device(c.next.copy()))   # (the table's arrays are read-only)
        return self.held[c.key]


@pytest.fixture(scope="module")
def images(ctx):
    return Images(ctx)


def make_system(images, c):
    g = api.So3System()
    C.memset(C.byref(g), 0x3C, C.sizeof(g))        # state_out, hot: a word the entry does not write back keeps this
    C.memset(g.sync, 0xFF, C.sizeof(g.sync))       # ... and a sync block it does not read back is not zero
    last, nxt = images(c)
    g.last_next_image, g.next_image = last.data_ptr(), nxt.data_ptr()
    g.state_in = api.GnState.from_buffer_copy(state_in(c.name, c.shape))
    return g


def check(tag, before, after, want):
    """one system after the launch: `before` / `after` api.So3System, `want` the oracle's state"""
    bad = []
    s, s0 = after.state_out, before.state_in
    for f in OUTPUT:
        if not same(getattr(s, f), getattr(want, f)):
            bad.append("%s: device %s, oracle %s" % (f, show(getattr(s, f)), show(getattr(want, f))))
    for f in SO3_STATS:
        if not same(getattr(s.stats, f), getattr(want.stats, f)):
            bad.append("stats.%s: device %s, oracle %s" % (f, getattr(s.stats, f), getattr(want.stats, f)))
    for f in HANDED:       # the hand-over: what the pinned host state held, and nothing of the fill pattern
        got = raw(getattr(s, f))
        if got != raw(getattr(s0, f)):
            bad.append("%s not handed over%s" % (f, ": the fill pattern" if got == bytes([FILL]) * len(got) else ""))
    for f in OUTPUT + ("cull_z",):
        got = raw(getattr(s, f))
        if got == bytes([FILL]) * len(got):
            bad.append("%s holds the fill pattern" % f)
    for f in OTHER_STATS:
        if raw(getattr(s.stats, f)) != raw(getattr(s0.stats, f)):
            bad.append("stats.%s changed" % f)
    if list(s.stats.cull_box) != [0, 0, s0.width - 1, s0.height - 1]:
        bad.append("cull_box %s is not the whole image" % list(s.stats.cull_box))
    if list(s.cull_z) != [float("-inf"), float("inf")]:
        bad.append("cull_z %s" % list(s.cull_z))
    if s.stats.fault != 0:
        bad.append("fault %d: the bounded wait of the meeting expired" % s.stats.fault)
    hot = np.frombuffer(bytes(after.hot), np.uint32)
    if not np.array_equal(hot, expected_hot(s)):
        bad.append("hot block is not refresh_hot of the returned state: words %s" % np.flatnonzero(hot != expected_hot(s)).tolist())
    left = np.frombuffer(bytes(after.sync), np.uint64)
    if left.any():
        bad.append("sync block not zero afterwards: words %s" % np.flatnonzero(left).tolist()[:8])
    assert not bad, "%s: %s" % (tag, "; ".join(bad))


def launch(ctx, images, cases, do_so3, first_level):
    """one launch of the cases -> (systems before, systems after)"""
    before = [make_system(images, c) for c in cases]
    after = ctx.so3_prealign_step([api.So3System.from_buffer_copy(b) for b in before], do_so3, first_level)
    return before, list(after)


def outputs(g):
    return bytes(g.state_out), bytes(g.hot), bytes(g.sync)


_alone = {}


def alone(ctx, images, c, do_so3, first_level):
    """the case in a launch of its own (n = 1), checked against the oracle, once per mode"""
    key = (c.key, do_so3, first_level)
    if key not in _alone:
        (b,), (a,) = launch(ctx, images, [c], do_so3, first_level)
        check("%s alone, do_so3 %d, first_level %d" % (c.key, do_so3, first_level), b, a, wanted(c.name, c.shape, do_so3, first_level))
        _alone[key] = outputs(a)
    return _alone[key]


@pytest.mark.parametrize("shape", sc.SHAPES, ids=["%dx%d" % s for s in sc.SHAPES])
@pytest.mark.parametrize("do_so3,first_level", MODES, ids=MODE_IDS)
def test_every_content_case_alone(ctx, images, shape, do_so3, first_level):
    for name in sc.CONTENT:
        alone(ctx, images, sc.case(name, shape), do_so3, first_level)


@pytest.mark.parametrize("do_so3,first_level", MODES, ids=MODE_IDS)
def test_every_content_case_in_full_launches(ctx, images, do_so3, first_level):
    """the 39 cases of the table dealt to launches of sixteen, in table order (shapes mixed within a launch)"""
    cases = sc.content_cases()
    for k0 in range(0, len(cases), 16):
        chunk = cases[k0:k0 + 16]
        before, after = launch(ctx, images, chunk, do_so3, first_level)
        for k, (c, b, a) in enumerate(zip(chunk, before, after)):
            check("%s in slot %d of %d, do_so3 %d, first_level %d" % (c.key, k, len(chunk), do_so3, first_level), b, a,
                  wanted(c.name, c.shape, do_so3, first_level))


@pytest.mark.parametrize("name", list(sc.BATCHES))
@pytest.mark.parametrize("do_so3,first_level", MODES, ids=MODE_IDS)
def test_batches_repeat_and_match_their_models_alone(ctx, images, name, do_so3, first_level):
    cases = sc.batch(name)
    runs = []
    for r in range(3):         # the same context, nothing reset in between: the sync blocks are as the launch before left them
        before, after = launch(ctx, images, cases, do_so3, first_level)
        for k, (c, b, a) in enumerate(zip(cases, before, after)):
            check("%s: %s in slot %d, launch %d, do_so3 %d, first_level %d" % (name, c.key, k, r, do_so3, first_level), b, a,
                  wanted(c.name, c.shape, do_so3, first_level))
        runs.append([outputs(a) for a in after])
    assert runs[0] == runs[1] == runs[2], name
    for k, c in enumerate(cases):       # no cross-talk between sync blocks (n9: models 0 and 8 meet in the same XCD's L2)
        assert runs[0][k] == alone(ctx, images, c, do_so3, first_level), "%s: %s in slot %d differs from the same case alone" % (name, c.key, k)


@pytest.mark.parametrize("name", ["n3", "n9", "n16"])
def test_with_and_without_prealignment_in_turn(ctx, images, name):
    """a launch without the pre-alignment (one workgroup per model, no meeting) directly in front of one with it, and the reverse"""
    cases = sc.batch(name)
    for r, do_so3 in enumerate((0, 1, 0, 1, 1, 0)):
        before, after = launch(ctx, images, cases, do_so3, 2)
        for k, (c, b, a) in enumerate(zip(cases, before, after)):
            check("%s: %s in slot %d, launch %d of the alternation, do_so3 %d" % (name, c.key, k, r, do_so3), b, a, wanted(c.name, c.shape, do_so3, 2))


def test_refusals(ctx, images):
    c = sc.case("rot_small", sc.SHAPES[0])
    one = make_system(images, c)
    call = lambda h, n, p, so3, lvl: ctx.lib.cf_so3_prealign_step(h, n, p, so3, lvl)
    for n in (0, 17):
        with pytest.raises(api.CofusionError):
            ctx.so3_prealign_step((api.So3System * n)(*([one] * n)), True, 2)
    assert call(ctx.h, 1, None, 1, 2) == -1
    assert call(None, 1, C.byref(one), 1, 2) == -1
    for lvl in (-1, 3):
        assert call(ctx.h, 1, C.byref(one), 1, lvl) == -1
    for field, value in (("width", 168), ("width", 0), ("height", 122), ("height", -4)):
        g = api.So3System.from_buffer_copy(one)
        setattr(g.state_in, field, value)
        assert call(ctx.h, 1, C.byref(g), 1, 2) == -1, (field, value)
    for field in ("last_next_image", "next_image"):      # null images are refused when they would be read, and only then
        g = api.So3System.from_buffer_copy(one)
        setattr(g, field, None)
        assert call(ctx.h, 1, C.byref(g), 1, 2) == -1, field
        assert call(ctx.h, 1, C.byref(g), 0, 2) == 0, field
    small = api.Context(160, 120, 132.0, 132.0, 79.5, 59.5, max_models=2)      # n is bounded by the context's sync blocks as well
    try:
        arr = (api.So3System * 3)(*([one] * 3))
        assert small.lib.cf_so3_prealign_step(small.h, 3, arr, 1, 2) == -1
        assert small.lib.cf_so3_prealign_step(small.h, 2, arr, 1, 2) == 0
    finally:
        small.close()
    # nothing was enqueued or written by a refused call: the system is as it was, and the context still runs
    assert bytes(one) == bytes(make_system(images, c))
    (b,), (a,) = launch(ctx, images, [c], 1, 2)
    check(c.key, b, a, wanted(c.name, c.shape, 1, 2))
