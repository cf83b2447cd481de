"""GPU suite: re-detection of inactive object models end to end (CoFusion::setRedetection) through the facade, at 160x128
with label masks on the device.  Scenes: synth.Scene(n_obj=2); its second object (label 2, mask value 80) is the one that leaves.

  parked    the object stands still from frame 4 on, is missing from the scene in frames 6-8 and is back from frame 9
  moved     the same, but it comes back 0.5 m from where it stood
  dropout   the plain scene (both objects moving), the object's mask value zeroed in frame 7 only

The returning object carries its old mask value (80), or -- as a segmentation that numbers its instances anew would give it -- another
one (120).  With re-detection OFF a deactivated model's mask value stays mapped to the dead id for the rest of the run, so only a new value
can spawn a model again: the on / off pair that shows the feature is run with the new value."""
import warnings

import numpy as np
import pytest

from co_fusion_amd import synth

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

W, H = 160, 128
FRAMES, FROZEN_FROM, HIDDEN, BACK = 14, 4, (6, 7, 8), 9
KW = dict(max_surfels=1 << 18, conf_global_init=0.5, model_spawn_offset=2, enable_multiple_models=1)   # (tests/test_facade_masks_gpu.py)
RD = dict(keep_min_surfels=64, keep_conf_threshold=0.3)   # small images: small models are kept
VALUE = 80


class Parked(synth.Scene):
    """object 2 frozen at its pose of frame FROZEN_FROM; from BACK on displaced by `shift` (world)"""

    def __init__(self, seed=1234, shift=None):
        super().__init__(n_obj=2, seed=seed)
        self.shift = shift

    def object_pose(self, i, t):
        T = super().object_pose(i, min(t, FROZEN_FROM) if i == 1 else t)
        if i == 1 and t >= BACK and self.shift is not None:
            T = T.copy()
            T[:3, 3] += self.shift
        return T

    def render(self, cam, t, noise=True, hidden=False):
        if not hidden:
            return super().render(cam, t, noise)
        keep = self.objects
        self.objects = keep[:1]            # a copy of the scene without the object
        try:
            return super().render(cam, t, noise)
        finally:
            self.objects = keep


_FRAMES = {}


def frames(kind, seed=1234, value_back=VALUE, hide=True, dist=0.5):
    """[(depth, rgb, mask)] of a scenario, rendered once per module; dist: how far a "moved" object comes back from where it stood (m)"""
    key = (kind, seed, value_back, hide, dist)
    if key in _FRAMES:
        return _FRAMES[key]
    cam = synth.Camera.scaled(W, H)
    out = []
    if kind == "dropout":
        sc = synth.Scene(n_obj=2, seed=seed)
        for t in range(FRAMES):
            d, rgb, lab, _ = sc.render(cam, t, noise=True)
            gt = (lab * 40).astype(np.uint8)
            if t == 7:
                gt[gt == VALUE] = 0
            out.append((d, rgb, gt))
    else:
        shift = None
        if kind == "moved":   # 0.5 m sideways, towards the middle of the view
            x = Parked(seed).object_pose(1, FROZEN_FROM)[0, 3]
            shift = np.array([-dist if x > 0 else dist, 0.0, 0.0])
        sc = Parked(seed, shift)
        for t in range(FRAMES):
            d, rgb, lab, _ = sc.render(cam, t, noise=True, hidden=hide and t in HIDDEN)
            gt = (lab * 40).astype(np.uint8)
            if t >= BACK:
                assert np.count_nonzero(gt == VALUE) >= 2 * 256, "the returning object must be large enough to propose a label"
                gt[gt == VALUE] = value_back
            out.append((d, rgb, gt))
    _FRAMES[key] = out
    return out


def _cf(on, **rd):
    from co_fusion_amd import facade
    cam = synth.Camera.scaled(W, H)
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, **KW)
    if on:
        cf.set_redetection(True, **{**RD, **rd})
    return cf


def _feed(cf, fr, t):
    import torch
    d, rgb, gt = fr
    cf.process_frame_device(torch.from_numpy(d).cuda(), torch.from_numpy(synth.rgb_to_rgba(rgb)).cuda(), timestamp=t,
                            mask=torch.from_numpy(gt).cuda())


def _snap(cf, maps=False):
    infos = [cf.model_info(i) for i in range(cf.num_models)]
    s = dict(ids=[m["id"] for m in infos], counts=[m["count"] for m in infos], poses=[m["pose"].copy() for m in infos],
             confs=[m["conf_threshold"] for m in infos], inactive=cf.num_inactive_models, stats=cf.redetect_stats())
    if maps:
        s["maps"] = [cf.model_download(i) for i in range(cf.num_models)]
    return s


def _id_of_value(cf, gt, value):
    """the model id the label image gives the pixels of a mask value"""
    ids = cf.mask()[gt == value]
    assert ids.size
    return int(np.bincount(ids).argmax())


_RUNS = {}


def run(kind, on, value_back=VALUE, hide=True, dist=0.5):
    """a whole scenario through one instance, once per module: per frame the snapshot, the id the object's pixels carry, and -- at frame 5
    and in the frame of a reactivation -- the object's map"""
    key = (kind, on, value_back, hide, dist)
    if key in _RUNS:
        return _RUNS[key]
    fr = frames(kind, value_back=value_back, hide=hide, dist=dist)
    cf = _cf(on)
    rec = []
    for t in range(FRAMES):
        _feed(cf, fr[t], t)
        s = _snap(cf)
        v = value_back if (kind != "dropout" and t >= BACK) else VALUE
        s["obj_id"] = _id_of_value(cf, fr[t][2], v) if np.any(fr[t][2] == v) else None
        if s["obj_id"] in s["ids"] and (t == 5 or (rec and s["stats"]["reactivations"] > rec[-1]["stats"]["reactivations"])):
            s["obj_map"] = cf.model_download(s["ids"].index(s["obj_id"]))
        if rec and s["stats"]["attempts"] > rec[-1]["stats"]["attempts"]:
            s["last"] = cf.redetect_last()
            print(f"{kind} on={on} value={value_back} frame {t}: {s['last']}")
        rec.append(s)
    cf.close()
    _RUNS[key] = rec
    return rec


def _world_point(snap, idx, c):
    """G * M^-1 applied to the model-frame point c (the convention of the pose log)"""
    G = snap["poses"][0].astype(np.float64); M = snap["poses"][idx].astype(np.float64)
    return (G @ np.linalg.inv(M) @ np.append(c, 1.0))[:3]


@pytest.mark.parametrize("value_back", [VALUE, 120])
def test_parked_object_resumes_its_old_model(value_back):
    rec = run("parked", True, value_back)
    old = rec[5]["obj_id"]
    assert old not in (None, 0) and old in rec[5]["ids"], "the object must have a model of its own before it leaves"
    assert rec[5]["inactive"] == 0 and rec[6]["inactive"] == 1 and old not in rec[6]["ids"], "deactivated in the first frame without its label"
    assert all(old not in rec[t]["ids"] for t in HIDDEN)
    back = next(t for t in range(BACK, FRAMES) if rec[t]["stats"]["reactivations"])
    assert back <= BACK + 1
    s = rec[back]
    assert s["stats"] == dict(attempts=1, reactivations=1, last_id=old)
    assert s["ids"][-1] == old and s["obj_id"] == old and s["inactive"] == 0, "the old id, at the end of the list; the label image carries it"
    assert s["last"]["winner"] == 0 and s["last"]["candidates"][0]["eligible"] and s["last"]["candidates"][0]["id"] == old
    # in the frame of its reactivation the map is what it was when the model was deactivated, byte for byte
    assert s["obj_map"].shape == rec[5]["obj_map"].shape and s["obj_map"].tobytes() == rec[5]["obj_map"].tobytes()
    assert max(s["ids"]) == max(rec[5]["ids"]), "no id was consumed"
    for t in range(back, FRAMES):
        assert old in rec[t]["ids"] and rec[t]["obj_id"] == old, f"frame {t}: the model stays"
        assert rec[t]["stats"]["reactivations"] == 1


def test_exported_segmentation_carries_the_old_id(tmp_path):
    """the label image is rewritten before the frame's Segmentation<n>.png is written: the file of the reactivation frame shows the old id"""
    from co_fusion_amd import masks
    fr = frames("parked")
    old = run("parked", True)[5]["obj_id"]
    cf = _cf(True)
    cf.set_export_segmentation(str(tmp_path) + "/")
    for t in range(BACK + 1):
        _feed(cf, fr[t], t)
    assert cf.redetect_stats()["reactivations"] == 1
    cf.close()
    png = masks.read_mask(str(tmp_path / f"Segmentation{BACK + 1}.png"))   # (frame t is tick t + 1)
    ids = png[fr[BACK][2] == VALUE]
    assert ids.size and np.all(ids == old)
    assert not np.any(png > max(run("parked", True)[5]["ids"])), "the provisional label is nowhere in the file"


def test_without_redetection_the_object_gets_a_new_id():
    """the same frames with re-detection off: the returning object is spawned under another id (what fails without the feature is the
    assertion above; this is its other half)"""
    rec = run("parked", False, 120)
    old = rec[5]["obj_id"]
    assert old in rec[5]["ids"] and old not in rec[6]["ids"]
    assert rec[6]["inactive"] == 0, "a small model is not kept under the default thresholds"
    new = rec[-1]["obj_id"]
    assert new not in (None, 0, old) and new in rec[-1]["ids"] and old not in rec[-1]["ids"]
    assert rec[-1]["stats"] == dict(attempts=0, reactivations=0, last_id=-1)


def test_drift_of_the_parked_object_is_bounded_by_continuous_tracking():
    """e = how far the object's world position G M^-1 c (c: the centroid of its map at frame 5) has moved between frame 5 and the last
    frame; the truth is 0.  e_r: hidden for three frames and re-detected; e_c: never hidden, tracked throughout (the parent's behaviour).
    Bound: e_r <= 2 e_c + 1e-3 m."""
    errs = {}
    for name, rec in (("redetected", run("parked", True, VALUE)), ("continuous", run("parked", True, VALUE, hide=False))):
        old = rec[5]["obj_id"]
        c = rec[5]["obj_map"][:, :3].astype(np.float64).mean(axis=0)
        p5 = _world_point(rec[5], rec[5]["ids"].index(old), c)
        pl = _world_point(rec[-1], rec[-1]["ids"].index(old), c)
        errs[name] = float(np.linalg.norm(pl - p5))
    print(f"drift of the parked object over frames 5..{FRAMES - 1}: re-detected {errs['redetected']:.6f} m, continuous {errs['continuous']:.6f} m")
    assert run("parked", True, VALUE, hide=False)[-1]["stats"]["attempts"] == 0
    assert errs["redetected"] <= 2 * errs["continuous"] + 1e-3, errs


def test_one_frame_dropout_of_a_moving_object():
    rec = run("dropout", True)
    old = rec[6]["obj_id"]
    assert old in rec[6]["ids"] and old not in rec[7]["ids"] and rec[7]["inactive"] == 1
    back = next(t for t in range(8, FRAMES) if rec[t]["stats"]["reactivations"])
    assert back in (8, 9)
    assert rec[back]["ids"][-1] == old and rec[back]["obj_id"] == old
    for t in range(back, FRAMES):
        assert old in rec[t]["ids"] and rec[t]["stats"]["reactivations"] == 1
    assert rec[-1]["stats"]["last_id"] == old and max(rec[-1]["ids"]) == max(rec[6]["ids"])


@pytest.mark.parametrize("dist", [0.5, 0.3])
def test_an_object_that_moved_away_is_spawned_anew(dist):
    """0.5 m: the kept map explains nothing of the new label.  0.3 m (three times the gate): the strongest false candidate that agrees
    with the frame anywhere -- the figure the default min_cover was placed against"""
    rec = run("moved", True, dist=dist)
    old = rec[5]["obj_id"]
    assert rec[6]["inactive"] == 1 and old not in rec[6]["ids"]
    st = rec[-1]["stats"]
    assert st["attempts"] >= 1 and st["reactivations"] == 0 and st["last_id"] == -1
    new = rec[-1]["obj_id"]
    assert new not in (None, 0, old) and new in rec[-1]["ids"] and old not in rec[-1]["ids"]
    assert rec[-1]["inactive"] >= 1, "the rejected candidate is still kept"
    first = next(s["last"] for s in rec if "last" in s)
    assert first["winner"] == -1 and not any(c["eligible"] for c in first["candidates"])


def test_idle_redetection_changes_nothing():
    """switched on against off over the frames before any deactivation: masks, model lists, poses, counts and maps byte for byte"""
    fr = frames("parked")
    a, b = _cf(True), _cf(False)
    for t in range(HIDDEN[0]):
        _feed(a, fr[t], t); _feed(b, fr[t], t)
        x, y = _snap(a, maps=True), _snap(b, maps=True)
        assert x["ids"] == y["ids"] and x["counts"] == y["counts"] and x["confs"] == y["confs"], f"frame {t}"
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x["poses"], y["poses"])), f"frame {t}: poses"
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x["maps"], y["maps"])), f"frame {t}: maps"
        if t > 0:
            assert np.array_equal(a.mask(), b.mask()), f"frame {t}: label image"
    assert len(x["ids"]) == 3 and x["stats"]["attempts"] == 0
    a.close(); b.close()


def test_group_sequences_equal_single_handles():
    import torch
    from co_fusion_amd import facade
    seeds = (1234, 1234 + 17)
    runs = [frames("parked", seed=s) for s in seeds]
    cam = synth.Camera.scaled(W, H)
    group = facade.CoFusionGroup(2, W, H, cam.fx, cam.fy, cam.cx, cam.cy, **KW)
    singles = [_cf(True) for _ in seeds]
    for q in group.sequences:
        q.set_redetection(True, **RD)
    for t in range(FRAMES):
        dts = [torch.from_numpy(r[t][0]).cuda() for r in runs]
        cts = [torch.from_numpy(synth.rgb_to_rgba(r[t][1])).cuda() for r in runs]
        mts = [torch.from_numpy(r[t][2]).cuda() for r in runs]
        group.process_frames_device(dts, cts, timestamp=t, masks=mts)
        for s, q in enumerate(singles):
            q.process_frame_device(dts[s], cts[s], timestamp=t, mask=mts[s])
        for s, (a, b) in enumerate(zip(group.sequences, singles)):
            x, y = _snap(a), _snap(b)
            assert x["ids"] == y["ids"] and x["counts"] == y["counts"] and x["inactive"] == y["inactive"], f"frame {t} sequence {s}"
            assert x["stats"] == y["stats"], f"frame {t} sequence {s}: {x['stats']} vs {y['stats']}"
            assert all(p.tobytes() == r.tobytes() for p, r in zip(x["poses"], y["poses"])), f"frame {t} sequence {s}: poses"
    assert singles[0].redetect_stats()["reactivations"] == 1
    group.close()
    for q in singles:
        q.close()


def test_model_parallel_instances_are_refused():
    from co_fusion_amd import facade
    cam = synth.Camera.scaled(W, H)
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, rank=0, world=2, **KW)
    with pytest.raises(facade.CoFusionError, match="world == 1"):
        cf.set_redetection(True)
    cf.set_redetection(False)   # switching it off is always possible
    cf.close()
