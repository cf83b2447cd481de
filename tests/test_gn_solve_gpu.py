"""GPU suite: the device Gauss-Newton solve (gn_solve_kernel, csrc/track_solve_dev.h) on crafted systems.

Every case of tests/solve_cases.py goes through cf_gn_solve_step -- the production kernel on its own, n systems in one launch of n
workgroups -- and is compared with orc_gn_solve_step, the algebra of one iteration as the oracle's tracking loop runs it, BIT FOR BIT
(NaN equal to NaN): the same IEEE operations in the same order is this stage's contract.  What the cases cover is asserted on the
CPU (tests/test_cpu_solve_cases.py); a failing case's name says which branch of the kernel is wrong.

Besides the state, every launch is checked for what the kernel does around the algebra: the 48 words of the hot block are
refresh_hot of the returned state, both accumulators are zero in all 64 x 32 words, the inverse pose is written by the solve that
ends a schedule and by no other, and the pinned host twin receives the mutable words if and only if the schedule ends.  Every system
is then solved a second time on what the first call returned -- the state and the accumulators as the kernel left them --, which a
kernel that left a word behind would not survive."""
import ctypes as C

import numpy as np
import pytest

import orc
import solve_cases as sc
from co_fusion_amd import api
from gn_compare import expected_hot, raw as _raw, same as _same, show as _show

pytestmark = pytest.mark.gpu

MUTABLE = ("Rprev", "tprev", "Rprev_inv", "Rcurr", "tcurr", "resultRt", "krkInv", "kt", "lastRGBError", "level_done", "solves", "residual",
           "cull_z", "pose_inv", "stats")            # OdomDev from Rprev on: what the solve writes back and publishes to the twin
CONFIG = ("intr", "width", "height", "icp", "rgb", "rgbOnly", "icpWeight")
# what the oracle's state and the device state share
SHARED = ("Rprev", "tprev", "Rcurr", "tcurr", "resultRt", "krkInv", "kt", "lastRGBError", "level_done", "solves", "residual")
STATS = ("last_icp_error", "last_icp_count", "last_rgb_error", "last_rgb_count", "lastA", "lastb")
ZERO_TOTALS = np.zeros(32, np.int64)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(160, 120, 132.0, 132.0, 79.5, 59.5)
    yield c
    c.close()


def cf_state(d):
    """state dictionary of the case table -> api.GnState"""
    s = api.GnState()
    s.intr = api.Cam(*[float(v) for v in d["intr"]])
    for k in ("width", "height", "icp", "rgb", "rgbOnly", "level_done", "solves"):
        setattr(s, k, int(d[k]))
    s.icpWeight = float(d["icpWeight"]); s.lastRGBError = float(d["lastRGBError"])
    for k, n, t in (("Rprev", 9, np.float32), ("tprev", 3, np.float32), ("Rprev_inv", 9, np.float32), ("Rcurr", 9, np.float32), ("tcurr", 3, np.float32),
                    ("resultRt", 16, np.float64), ("krkInv", 9, np.float32), ("kt", 3, np.float32), ("residual", 2, np.float32), ("pose_inv", 16, np.float32)):
        getattr(s, k)[:] = np.ascontiguousarray(d[k], t).reshape(n).tolist()
    s.cull_z[:] = [float("-inf"), float("inf")]              # (no depth culling)
    s.stats.cull_box[:] = [0, 0, int(d["width"]) - 1, int(d["height"]) - 1]
    return s


def orc_from_cf(s):
    """api.GnState -> orc.GnState (the fields the oracle keeps; its statistics are the six shared ones)"""
    o = orc.GnState()
    o.intr = orc.Cam(s.intr.fx, s.intr.fy, s.intr.cx, s.intr.cy)
    for k in ("width", "height", "icp", "rgb", "rgbOnly", "icpWeight", "lastRGBError", "level_done", "solves"):
        setattr(o, k, getattr(s, k))
    for k in ("Rprev", "tprev", "Rcurr", "tcurr", "resultRt", "krkInv", "kt", "residual"):
        C.memmove(getattr(o, k), getattr(s, k), C.sizeof(getattr(s, k)))
    for k in STATS:
        v = getattr(s.stats, k)
        if isinstance(v, C.Array):
            C.memmove(getattr(o.stats, k), v, C.sizeof(v))
        else:
            setattr(o.stats, k, v)
    return o


def make_system(state, step):
    """api.GnSystem of a state (api.GnState) and a step's sums; the twin starts as a pattern no solve produces"""
    g = api.GnSystem()
    C.memmove(g.icp_acc, step.icp.ctypes.data, 8 * 64 * 32)
    C.memmove(g.rgb_acc, step.rgb.ctypes.data, 8 * 64 * 32)
    g.state = state
    C.memset(C.byref(g.twin), 0x5A, C.sizeof(api.GnState))
    C.memset(g.hot, 0xA5, C.sizeof(g.hot))
    return g


def check(tag, before, after, want, step):
    """one solved system: `before` / `after` api.GnSystem (the entry's input and output), `want` the oracle's state"""
    bad = []
    s, s0 = after.state, before.state
    for f in SHARED:
        if not _same(getattr(s, f), getattr(want, f)):
            bad.append("%s: device %s, oracle %s" % (f, _show(getattr(s, f)), _show(getattr(want, f))))
    for f in STATS:
        if not _same(getattr(s.stats, f), getattr(want.stats, f)):
            bad.append("stats.%s: device %s, oracle %s" % (f, _show(getattr(s.stats, f)), _show(getattr(want.stats, f))))
    # what the solve must leave alone
    for f in CONFIG + ("Rprev", "tprev", "Rprev_inv", "cull_z"):
        if _raw(getattr(s, f)) != _raw(getattr(s0, f)):
            bad.append("%s changed" % f)
    for f in ("last_so3_error", "last_so3_count", "so3_iterations", "fault", "cull_box"):
        if _raw(getattr(s.stats, f)) != _raw(getattr(s0.stats, f)):
            bad.append("stats.%s changed" % f)
    if step.next_level < 0:   # the end of a schedule: the inverse of the pose the call ends with
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = np.array(s.Rcurr, np.float32).reshape(3, 3); pose[:3, 3] = np.array(s.tcurr, np.float32)
        inv = (C.c_float * 16)(*orc.inverse_pose(pose).reshape(16).tolist())
        if not _same(s.pose_inv, inv):
            bad.append("pose_inv is not the inverse of [Rcurr | tcurr]")
    elif _raw(s.pose_inv) != _raw(s0.pose_inv):
        bad.append("pose_inv written although the schedule goes on")
    if not np.array_equal(np.frombuffer(bytes(after.hot), np.uint32), expected_hot(s)):
        bad.append("hot block is not refresh_hot of the returned state: words %s"
                   % np.flatnonzero(np.frombuffer(bytes(after.hot), np.uint32) != expected_hot(s)).tolist())
    for name in ("icp_acc", "rgb_acc"):
        left = np.frombuffer(bytes(getattr(after, name)), np.int64)
        if left.any():
            bad.append("%s not zero afterwards: words %s" % (name, np.flatnonzero(left).tolist()[:8]))
    for f in CONFIG:          # configuration words of the twin are never written (the entry reads every word of state and twin back)
        if _raw(getattr(after.twin, f)) != _raw(getattr(before.twin, f)):
            bad.append("twin.%s written" % f)
    for f in MUTABLE:
        got, pub, old = _raw(getattr(after.twin, f)), _raw(getattr(s, f)), _raw(getattr(before.twin, f))
        if step.next_level < 0 and got != pub:
            bad.append("twin.%s does not hold the published word" % f)
        if step.next_level >= 0 and got != old:
            bad.append("twin.%s written although the schedule goes on" % f)
    assert not bad, "%s: %s" % (tag, "; ".join(bad))


def launch(ctx, systems, step):
    arr = (api.GnSystem * len(systems))(*systems)
    return ctx.gn_solve_step(arr, step.next_level, step.last_of_level, step.icp_fix)


def run_single_step_cases(ctx, cases, width=16):
    """the one-step cases, `width` per launch among those that share (next_level, last_of_level, format); then every returned system
    once more as it stands: accumulators as the kernel left them, the state fed back"""
    groups = {}
    for c in cases:
        st, = c.steps
        groups.setdefault((st.next_level, st.last_of_level, st.icp_fix), []).append(c)
    results = {}
    for key, members in groups.items():
        for k0 in range(0, len(members), width):
            chunk = members[k0:k0 + width]
            step = chunk[0].steps[0]
            before = [make_system(cf_state(c.state), c.steps[0]) for c in chunk]
            after = launch(ctx, before, step)
            for c, b, a in zip(chunk, before, after):
                check("%s [%s]" % (c.name, c.aims), b, a, sc.reference(c.name)[0][0], step)
                results[c.name] = bytes(a.state)
            again_in = [api.GnSystem.from_buffer_copy(a) for a in after]
            again = launch(ctx, again_in, step)
            for c, b, a in zip(chunk, again_in, again):
                want, _ = orc.gn_solve_step(orc_from_cf(b.state), ZERO_TOTALS, ZERO_TOTALS, step.next_level, step.last_of_level, step.icp_fix)
                check("%s, solved again on the returned state and accumulators" % c.name, b, a, want, step)
    return results


# How the table is dealt to the tests below: the pivots family has a test of its own, every other one-step case goes with its family,
# every case of several steps is a sequence.  Derived from the table, so that a new case or family cannot be left out.
PIVOTS = [c.name for c in sc.family("pivots")]
BY_FAMILY = {}
for _c in sc.cases().values():
    if len(_c.steps) == 1 and _c.family != "pivots":
        BY_FAMILY.setdefault(_c.family, []).append(_c.name)
SEQUENCES = [c.name for c in sc.cases().values() if len(c.steps) > 1]


def test_every_case_of_the_table_is_sent():
    sent = PIVOTS + [n for names in BY_FAMILY.values() for n in names] + SEQUENCES
    assert len(sent) == len(set(sent)) and set(sent) == set(sc.cases()), set(sc.cases()) ^ set(sent)
    assert set(BY_FAMILY) | {"pivots", "chain"} == {c.family for c in sc.cases().values()}


@pytest.mark.parametrize("family", list(BY_FAMILY))
def test_family_matches_the_oracle_bit_for_bit(ctx, family):
    done = run_single_step_cases(ctx, [sc.cases()[n] for n in BY_FAMILY[family]])
    assert sorted(done) == sorted(BY_FAMILY[family])


def test_pivots_sixteen_per_launch_and_slot_independence(ctx):
    """720 pivot orders, 16 workgroups per launch (the blockIdx.x indexing of the kernel's arguments); then the first sixteen in
    reversed order, one launch of one and one of seven: a result does not depend on its slot or on its neighbours"""
    cases = [sc.cases()[n] for n in PIVOTS]
    assert len(cases) == 720
    first = run_single_step_cases(ctx, cases)
    assert len(first) == 720
    for chunk in (cases[:16][::-1], cases[5:6], cases[20:27]):
        again = run_single_step_cases(ctx, chunk, width=len(chunk))
        for c in chunk:
            assert again[c.name] == first[c.name], c.name


@pytest.mark.parametrize("name", SEQUENCES)
def test_sequences_feed_the_state_back(ctx, name):
    """the stop rule's four solves and the 19 solves of a 4 / 5 / 10 schedule: every step starts from the state the DEVICE returned"""
    c = sc.cases()[name]
    state = cf_state(c.state)
    for k, (step, (want, _)) in enumerate(zip(c.steps, sc.reference(name))):
        before = make_system(state, step)
        after, = launch(ctx, [before], step)
        check("%s step %d [%s]" % (name, k, c.aims), before, after, want, step)
        state = api.GnState.from_buffer_copy(after.state)


def test_refusals(ctx):
    c = sc.family("ties")[0]
    one = make_system(cf_state(c.state), c.steps[0])
    for n in (0, 17):
        with pytest.raises(api.CofusionError):
            ctx.gn_solve_step((api.GnSystem * n)(*([one] * n)), 2, False)
    assert ctx.lib.cf_gn_solve_step(ctx.h, 1, None, 2, 0, 32) == -1
    assert ctx.lib.cf_gn_solve_step(None, 1, C.byref(one), 2, 0, 32) == -1
    for bad in (dict(next_level=3), dict(next_level=-2), dict(icp_fix=12)):
        kw = dict(next_level=2, icp_fix=32); kw.update(bad)
        assert ctx.lib.cf_gn_solve_step(ctx.h, 1, C.byref(one), kw["next_level"], 0, kw["icp_fix"]) == -1
    # nothing was enqueued or written: the system is as it was, and the context still solves
    assert bytes(one) == bytes(make_system(cf_state(c.state), c.steps[0]))
    after, = launch(ctx, [one], c.steps[0])
    check(c.name, one, after, sc.reference(c.name)[0][0], c.steps[0])
