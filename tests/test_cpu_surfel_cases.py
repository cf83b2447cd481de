"""CPU suite: the cases of tests/surfel_cases.py hold the edges they were built for -- asserted from the CPU oracle alone (its traced
fuse and clean), so that a case which silently stops taking a branch fails here and not unnoticed on the GPU -- and the ctypes mirrors of
cf_model_pass / cf_model_preindex have the layout of the header."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import surfel_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AT_LEAST = 8


def _fused(name):
    case, res = sc.get(name), sc.oracle(name)
    return [(k, q, case.calls[k][q], r) for k, call in enumerate(res) for q, r in call.items() if case.calls[k][q].do_fuse]


@pytest.mark.parametrize("name", sc.NAMES)
def test_shapes_counts_and_capacity(name):
    case = sc.get(name)
    w, h = case.shape
    assert case.shape in (sc.A, sc.B) and w % 16 == 0 and h % 4 == 0           # what cf_create accepts
    assert sc.B[0] % 32 and (sc.B[0] * sc.B[1]) % 256 and (sc.B[0] * sc.B[1]) % sc.SCAN_ITEMS
    for k, q, it, r in _fused(name):
        # the clean stage stages the map and a quarter image of new surfels: cf_models_frame_passes refuses a model that cannot hold them
        assert r.map_fused.shape[0] + (w // 2) * (h // 2) <= case.max_surfels + w * h // 4 + 64
        assert r.map.shape[0] <= case.max_surfels and r.fresh.shape[0] <= (w // 2) * (h // 2)
        assert np.count_nonzero(r.index[0]) > 0 or r.map_fused.shape[0] == 0
    for call in case.calls:
        assert len({it.model for it in call}) == len(call)                      # a model appears once per call


def test_one_model_is_a_plain_frame():
    (_, _, it, r), = _fused("one_model")
    code = r.pix_trace[..., 0]
    assert np.count_nonzero(code == 5) > 500 and np.count_nonzero(code == 4) >= AT_LEAST and np.count_nonzero(r.splat[0][..., 3]) > 2000


def test_five_models():
    case, res = sc.get("five_models"), sc.oracle("five_models")[0]
    call = case.calls[0]
    assert len(call) == 5 and len({m.shape[0] for m in case.maps}) == 5
    assert {it.time % 2 for it in call if it.do_fuse} == {0, 1}                 # both parities in one association launch
    empty = [q for q, it in enumerate(call) if case.maps[it.model].shape[0] == 0]
    assert len(empty) == 1 and call[empty[0]].do_fuse
    r = res[empty[0]]
    assert r.fresh.shape[0] >= AT_LEAST and r.map.shape[0] == r.fresh.shape[0] and not np.count_nonzero(r.pix_trace[..., 0] == 5)
    idle = [q for q, it in enumerate(call) if not it.do_fuse]
    assert len(idle) == 1 and res[idle[0]].index is None and np.count_nonzero(res[idle[0]].splat[0][..., 3]) > 50
    assert np.array_equal(res[idle[0]].map, case.maps[call[idle[0]].model])
    for q, it in enumerate(call):
        if it.do_fuse and q not in empty:
            assert np.count_nonzero(res[q].pix_trace[..., 0] == 5) >= AT_LEAST      # every model with a map merges ...
            assert res[q].fresh.shape[0] > 0                                        # ... and appends


@pytest.mark.parametrize("name,n", [("sixteen_models", 16), ("seventeen_models", 17)])
def test_batch_sizes(name, n):
    case, res = sc.get(name), sc.oracle(name)[0]
    assert sc.K_SURF_BATCH == 16
    src = open(os.path.join(ROOT, "co_fusion_amd", "csrc", "cf_kernels.h")).read()
    assert "constexpr int kSurfBatch = 16;" in src
    assert len(case.calls[0]) == n and (n > sc.K_SURF_BATCH) == (name == "seventeen_models")
    assert all(it.do_fuse for it in case.calls[0]) and {it.time % 2 for it in case.calls[0]} == {0, 1}
    assert max(m.shape[0] for m in case.maps) < 256                            # tiny: one workgroup and seven of padding per model
    assert all(r.fresh.shape[0] > 0 for r in res.values()) and sum(np.count_nonzero(r.upd_trace[:, 0]) > 0 for r in res.values()) >= n // 2


@pytest.mark.parametrize("name", ["two_frames", "two_frames_reinit"])
def test_two_frames(name):
    case, res = sc.get(name), sc.oracle(name)
    assert len(case.calls) == 2 and [it.model for it in case.calls[0]] == [it.model for it in case.calls[1]]
    assert {it.time % 2 for it in case.calls[0]} != {it.time % 2 for it in case.calls[1]}   # the second association visits other pixels
    for q, r in res[0].items():
        # what a compaction that left its flags set, or an update that left its owner slot set, would act on in the second call
        assert r.fresh.shape[0] > 0 and np.count_nonzero(r.upd_trace[:, 0]) >= AT_LEAST
        r2 = res[1][q]
        if case.between and case.calls[0][q].model == case.between[1][0][1]:
            continue                                                           # (this model's map is replaced between the calls)
        n_old = r.upd_trace.shape[0]
        survived = np.nonzero(r.clean_trace[:n_old, 5])[0]                     # clean compacts: id k of the second call was id survived[k]
        merged_then = r.upd_trace[survived, 0] != 0
        untouched_now = r2.upd_trace[:len(survived), 0] == 0
        assert np.count_nonzero(merged_then & untouched_now) >= AT_LEAST       # merged in the first call, unclaimed in the second
    assert bool(case.between) == (name == "two_frames_reinit")
    if case.between:
        (_, model, frame, time), = case.between[1]
        q = [it.model for it in case.calls[1]].index(model)
        assert res[1][q].map_fused.shape[0] > 10 * res[0][q].map.shape[0]      # the bootstrap of a whole frame replaced the object's map


def test_clean_branches():
    case = sc.get("clean_branches")
    (_, _, it, r), _ = _fused("clean_branches")                # (the first model; the second one: the next test)
    w, h = case.shape
    tr, g = r.clean_trace, case.note["groups"]
    window, cnt, zc, viol, foreign, kept, old, outdated = (tr[:, k] for k in range(8))
    assert case.time_delta < 30 and all(len(v) >= AT_LEAST for k, v in g.items() if k != "corner")

    def rows(name):
        return np.array(g[name])
    a = rows("old_unconfident")
    assert (old[a] == 1).all() and (outdated[a] == 0).all() and (kept[a] == 0).all() and (cnt[a] <= 8).all() and (zc[a] <= 4).all()
    assert np.count_nonzero(window[a]) >= 4 and np.count_nonzero(window[a] == 0) >= 4
    a = rows("outdated")
    assert (outdated[a] == 1).all() and (old[a] == 1).all() and (kept[a] == 1).all()         # kept although old and unconfident
    a = rows("stacked")
    assert (cnt[a] > 8).all() and (zc[a] <= 4).all() and (old[a] == 0).all() and (kept[a] == 0).all()
    a = rows("z_count")
    assert (zc[a] > 4).all() and (cnt[a] <= 8).all() and (old[a] == 0).all() and (kept[a] == 0).all()
    a = rows("violation")
    assert (viol[a] > 0).all() and (foreign[a] == 0).all() and (kept[a] == 1).all() and (cnt[a] <= 8).all() and (zc[a] <= 4).all()
    a = rows("violation_foreign")
    assert (viol[a] > 0).all() and (foreign[a] == 1).all() and (kept[a] == 1).all()
    # the factors really lowered the confidences: the kept surfels come out in input order
    kept_ids = np.nonzero(kept)[0]
    out_of = {int(i): k for k, i in enumerate(kept_ids)}
    f_alone = [r.map[out_of[i], 3] / r.map_fused[i, 3] for i in g["violation"]]
    f_both = [r.map[out_of[i], 3] / r.map_fused[i, 3] for i in g["violation_foreign"]]
    assert max(f_alone) < 0.95 and max(f_both) < 0.95 * (0.5 + 0.5 * (1 - case.outlier / 10.0)) + 1e-3
    for name in ("behind", "outside"):
        a = rows(name)
        assert (window[a] == 0).all() and (kept[a] == 1).all()
    # within one pixel of every border: the 4x4 patch the kernel stages starts at floor(x - 1.5) and is clamped there
    t_inv = np.linalg.inv(np.asarray(it.pose, np.float64))
    p = r.map_fused[:, 0:3].astype(np.float64) @ t_inv[:3, :3].T + t_inv[:3, 3]
    x = case.cam.fx * p[:, 0] / p[:, 2] + case.cam.cx; y = case.cam.fy * p[:, 1] / p[:, 2] + case.cam.cy
    n_old = r.map_fused.shape[0]
    win = window[:n_old] == 1
    for side, sel in (("left", x < 1), ("right", x > w - 1), ("top", y < 1), ("bottom", y > h - 1)):
        ids = np.nonzero(win & sel & (x > 0.05) & (x < w - 0.05) & (y > 0.05) & (y < h - 0.05))[0]
        assert len(ids) >= AT_LEAST, side
        x0, y0 = np.floor(x[ids] - 1.5), np.floor(y[ids] - 1.5)
        clamped = {"left": x0 < 0, "right": x0 + 3 > w - 1, "top": y0 < 0, "bottom": y0 + 3 > h - 1}[side]
        assert clamped.all(), side
    assert all(window[i] == 1 for i in g["corner"])


def test_clean_thresholds_and_borders_that_decide():
    """the second model of clean_branches: surfels whose count / zCount is exactly at and exactly under the thresholds, and border surfels
    removed with count == 9 of which at least one qualifying sample lies outside the image -- a clamped fetch that returned anything
    else would keep them"""
    case = sc.get("clean_branches")
    r = sc.oracle("clean_branches")[0][1]
    w, h = case.shape
    tr, sites = r.clean_trace, case.note["sites"]
    cnt, zc, kept, old = tr[:, 1], tr[:, 2], tr[:, 5], tr[:, 6]
    for group, col, target, keeps in (("count_9", cnt, 9, 0), ("count_8", cnt, 8, 1), ("z_count_5", zc, 5, 0), ("z_count_4", zc, 4, 1)):
        ids = np.array([s["id"] for s in sites[group]])
        assert len(ids) >= AT_LEAST, group
        assert (col[ids] == target).all() and (kept[ids] == keeps).all() and (old[ids] == 0).all(), group
        other = zc if col is cnt else cnt
        assert (other[ids] == 0).all(), group
    for side in ("left", "right", "top", "bottom"):
        ss = sites[side]
        assert len(ss) >= AT_LEAST, side
        ids = np.array([s["id"] for s in ss])
        assert (cnt[ids] == 9).all() and (zc[ids] == 0).all() and (kept[ids] == 0).all() and (old[ids] == 0).all(), side
        assert all(s["outside"] >= 1 for s in ss), side
        on = {"left": lambda s: s["px"] == 0, "right": lambda s: s["px"] == w - 1, "top": lambda s: s["py"] == 0,
              "bottom": lambda s: s["py"] == h - 1}[side]
        assert all(on(s) for s in ss)
        # the designer's model of the window is the oracle's at these sites: its count of samples outside the image can be relied on
        for s in ss:
            conf, n_out = sc.design_conf(s["px"], s["py"], w, h, "count", 9)
            assert sc.window_count(s["px"], s["py"], w, h, conf, "count") == (9, s["outside"]) and n_out == s["outside"]
    assert {s["outside"] for s in sites["left"]} != {s["outside"] for s in sites["right"]}      # the sides clamp different samples


def test_fuse_branches():
    case, res = sc.get("fuse_branches"), sc.oracle("fuse_branches")[0]
    w, h = case.shape
    r0, r1 = res[0], res[1]
    code = r0.pix_trace[..., 0]
    for c, why in ((1, "mask"), (2, "a zero depth neighbour"), (3, "beyond fuse_max_depth"), (5, "merge")):
        assert np.count_nonzero(code == c) >= AT_LEAST, why
    assert (r0.pix_trace[..., 0][code == 3] == 3).all() and case.calls[0][0].fuse_max_depth < sc.get("fuse_branches").frames["f"].depth.max()
    assert np.count_nonzero(r0.upd_trace[:, 0] == 1) >= AT_LEAST                 # averaged
    assert np.count_nonzero(r0.upd_trace[:, 0] == 2) >= AT_LEAST                 # the measurement's radius rejected
    twice = np.nonzero(r0.upd_trace[:, 1] >= 2)[0]
    assert len(twice) >= AT_LEAST
    # ... and the pixel with the smaller column-major rank is the one whose record went in: its confidence is the map's plus that pixel's
    best = r0.pix_trace[..., 1]
    for sid in twice[:AT_LEAST]:
        ys, xs = np.nonzero((code == 5) & (best == sid))
        assert len(ys) >= 2 and len(set(xs * h + ys)) == len(ys)
    # duplicated surfels: equal z in the index pass, the lower id holds the texel
    idx = r0.index_first[0]
    dup_of = case.note["dup_of"]
    held = 0
    for k, a in enumerate(dup_of):
        b = w * h + k
        assert np.array_equal(case.maps[0][a, 0:3], case.maps[0][b, 0:3]) and a < b
        assert not (idx == b).any()
        held += int((idx == a).any())
    assert held >= AT_LEAST
    # model 1: window samples of different outer iterations at bit-equal distance
    ties = r1.pix_trace[..., 3]
    assert np.count_nonzero(ties) >= AT_LEAST and set(np.nonzero(ties)[1]) == {case.note["tie_column"]}
    assert np.array_equal(np.asarray(case.calls[0][1].pose), np.eye(4, dtype=np.float32))


def test_long_map_count_arithmetic():
    case = sc.get("long_map")
    (_, _, it, r), = _fused("long_map")
    w, h = case.shape
    n = case.maps[0].shape[0]
    assert case.shape == sc.A and n >= sc.SCAN_ITEMS * 257 + 5 and n % 8 and n % sc.SCAN_ITEMS
    bound = n + (w // 2) * (h // 2)                                            # what the clean stage stages and compacts
    blocks = -(-bound // sc.SCAN_ITEMS)
    assert blocks - 1 > 256                                                    # the last scan workgroup adds more than 256 block sums
    assert bound >= 131072 and -(-4 * bound // 64) >= 4 * 8 * 256              # clean_kernel's XCD-ordered runs (64-thread workgroups, runs of 256)
    assert bound % sc.SCAN_ITEMS and r.map.shape[0] % sc.SCAN_ITEMS and r.map.shape[0] % 8
    kept = r.clean_trace[:, 5]
    assert kept.shape[0] == n + r.fresh.shape[0] and r.fresh.shape[0] > 0
    per_block = np.add.reduceat(kept, np.arange(0, kept.shape[0], sc.SCAN_ITEMS))
    assert len(per_block) == blocks and per_block[256] > 0 and per_block[257] > 0    # a base that forgets block 256 moves the tail
    assert (per_block < sc.SCAN_ITEMS).all() and (per_block[:-1] > 0).all()          # every block compacts: no block is kept whole
    assert n - np.count_nonzero(kept[:n]) > 10000
    idx = r.index_first[0]
    assert n / np.count_nonzero(idx) > 100                                     # many surfels per pixel
    assert np.count_nonzero(r.upd_trace[:, 0]) > 500


def test_struct_mirrors_match_the_header(tmp_path):
    from co_fusion_amd import model as M
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler (the build of the oracle needs one too)"
    fields = {"cf_model_pass": [f[0] for f in M.ModelPass._fields_], "cf_model_preindex": [f[0] for f in M.ModelPreindex._fields_]}
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"cofusion_hip.h\"\nint main(void) {\n"
    for s, fs in fields.items():
        src += f'  printf("{s} %zu\\n", sizeof({s}));\n'
        for f in fs:
            src += f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));\n'
    src += "  return 0;\n}\n"
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = str(tmp_path / "layout")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    for s, mirror in (("cf_model_pass", M.ModelPass), ("cf_model_preindex", M.ModelPreindex)):
        assert int(got[s]) == C.sizeof(mirror), s
        for f in fields[s]:
            assert int(got[f"{s}.{f}"]) == getattr(mirror, f).offset, f"{s}.{f}"
    # every member of the header's structs is mirrored
    import re
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cofusion_hip.h")).read(), flags=re.S)
    for s in fields:
        m = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % s, hdr)
        assert m, s
        names = re.findall(r"\*?\s*\*?(\w+)\s*[,;]", m.group(1))
        assert sorted(names) == sorted(fields[s]), (s, names)
