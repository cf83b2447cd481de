"""GPU suite: the re-detection search end to end (CoFusion::setRedetectionSearch, DESIGN.md 4.13 "Search") through the facade, at 160x128
with label masks on the device.  The scenes are those of tests/test_redetect_facade_gpu.py, built here: synth.Scene(n_obj=2), whose
second object (label 2, mask value 80) stands still from frame 4 on, is missing from the scene in frames 6-8 and is back from frame 9
under ANOTHER mask value (120), as a segmentation that numbers its instances anew would give it --

  parked     where it stood
  moved      0.3 m or 0.5 m sideways from where it stood (three and five times the static hypothesis's gate)
  stranger   at the moved place, but another object: the same shape, another base colour

An instance runs with re-detection off, with the static pass only ("static"), or with the search behind it ("search")."""
import warnings

import numpy as np
import pytest

from co_fusion_amd import synth

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

W, H = 160, 128
FRAMES, FROZEN_FROM, HIDDEN, BACK = 14, 4, (6, 7, 8), 9
KW = dict(max_surfels=1 << 18, conf_global_init=0.5, model_spawn_offset=2, enable_multiple_models=1, enable_pose_logging=1)
RD = dict(keep_min_surfels=64, keep_conf_threshold=0.3)   # small images: small models are kept
VALUE, VALUE_BACK = 80, 120
STRANGER_BASE = np.array([0.15, 0.55, 1.0])   # (the scene's bases are drawn from [0.45, 1.0]^3)


class Returning(synth.Scene):
    """object 2 frozen at its pose of frame FROZEN_FROM; from BACK on displaced by `shift` (world) and, as a stranger, recoloured"""

    def __init__(self, seed=1234, shift=None, stranger=False):
        super().__init__(n_obj=2, seed=seed)
        self.shift, self.stranger = shift, stranger

    def object_pose(self, i, t):
        T = super().object_pose(i, min(t, FROZEN_FROM) if i == 1 else t)
        if i == 1 and t >= BACK and self.shift is not None:
            T = T.copy()
            T[:3, 3] += self.shift
        return T

    def render(self, cam, t, noise=True, hidden=False):
        keep = self.objects
        if hidden:
            self.objects = keep[:1]            # a copy of the scene without the object
        elif self.stranger and t >= BACK:
            self.objects = [keep[0], dict(keep[1], base=STRANGER_BASE, seed=keep[1]["seed"] + 50)]
        try:
            return super().render(cam, t, noise)
        finally:
            self.objects = keep


def shift_of(dist, seed=1234):
    """`dist` m sideways, towards the middle of the view"""
    if not dist:
        return None
    x = Returning(seed).object_pose(1, FROZEN_FROM)[0, 3]
    return np.array([-dist if x > 0 else dist, 0.0, 0.0])


_FRAMES = {}


def frames(dist=0.0, stranger=False, hide=True, seed=1234):
    """[(depth, rgb, mask)] of a scenario, rendered once per module"""
    key = (dist, stranger, hide, seed)
    if key in _FRAMES:
        return _FRAMES[key]
    cam = synth.Camera.scaled(W, H)
    sc = Returning(seed, shift_of(dist, seed), stranger)
    out = []
    for t in range(FRAMES):
        d, rgb, lab, _ = sc.render(cam, t, noise=True, hidden=hide and t in HIDDEN)
        gt = (lab * 40).astype(np.uint8)
        if t >= BACK and hide:
            assert np.count_nonzero(gt == VALUE) >= 2 * 256, "the returning object must be large enough to propose a label"
            gt[gt == VALUE] = VALUE_BACK
        out.append((d, rgb, gt))
    _FRAMES[key] = out
    return out


def make(mode, **search):
    """mode: "off", "static" (setRedetection only) or "search" (setRedetectionSearch behind it)"""
    from co_fusion_amd import facade
    cam = synth.Camera.scaled(W, H)
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, **KW)
    if mode != "off":
        cf.set_redetection(True, **RD)
    if mode == "search":
        cf.set_redetection_search(True, **search)
    return cf


def feed(cf, fr, t):
    import torch
    d, rgb, gt = fr
    cf.process_frame_device(torch.from_numpy(d).cuda(), torch.from_numpy(synth.rgb_to_rgba(rgb)).cuda(), timestamp=t, mask=torch.from_numpy(gt).cuda())


def snap(cf, maps=False):
    infos = [cf.model_info(i) for i in range(cf.num_models)]
    s = dict(ids=[m["id"] for m in infos], counts=[m["count"] for m in infos], poses=[m["pose"].copy() for m in infos],
             confs=[m["conf_threshold"] for m in infos], inactive=cf.num_inactive_models, stats=cf.redetect_stats())
    if maps:
        s["maps"] = [cf.model_download(i) for i in range(cf.num_models)]
    return s


_RUNS = {}


def run(mode, dist=0.0, stranger=False, hide=True, poses_to=None, **search):
    """a whole scenario through one instance, once per module: per frame the snapshot, the id the object's pixels carry, the object's
    map at frame 5 and in the frame of a reactivation, and the records of every attempt"""
    key = (mode, dist, stranger, hide, tuple(sorted(search.items())))
    if key in _RUNS and poses_to is None:
        return _RUNS[key]
    fr = frames(dist, stranger, hide)
    cf = make(mode, **search)
    rec = []
    for t in range(FRAMES):
        feed(cf, fr[t], t)
        s = snap(cf)
        v = VALUE_BACK if (t >= BACK and hide) else VALUE
        px = cf.mask()[fr[t][2] == v]
        s["obj_id"] = int(np.bincount(px).argmax()) if px.size else None
        if s["obj_id"] in s["ids"] and (t == 5 or (rec and s["stats"]["reactivations"] > rec[-1]["stats"]["reactivations"])):
            s["obj_map"] = cf.model_download(s["ids"].index(s["obj_id"]))
        if rec and s["stats"]["attempts"] > rec[-1]["stats"]["attempts"]:
            s["last"] = cf.redetect_last()
            s["search"] = cf.redetect_search_last()
            print(f"{mode} dist={dist} stranger={stranger} frame {t}: static {s['last']}\n    search {s['search']}")
        rec.append(s)
    if poses_to is not None:
        cf.export_poses(poses_to)
    cf.close()
    _RUNS[key] = rec
    return rec


def world_point(s, idx, c):
    """G * M^-1 applied to the model-frame point c (the convention of the pose log)"""
    G = s["poses"][0].astype(np.float64); M = s["poses"][idx].astype(np.float64)
    return (G @ np.linalg.inv(M) @ np.append(c, 1.0))[:3]


@pytest.mark.parametrize("dist", [0.3, 0.5])
def test_an_object_that_returns_moved_resumes_its_old_model(dist):
    rec = run("search", dist)
    old = rec[5]["obj_id"]
    assert old not in (None, 0) and old in rec[5]["ids"], "the object must have a model of its own before it leaves"
    assert rec[6]["inactive"] == 1 and all(old not in rec[t]["ids"] for t in HIDDEN)
    back = next((t for t in range(BACK, FRAMES) if rec[t]["stats"]["reactivations"]), None)
    assert back is not None and back <= BACK + 1, "reactivated in the frame its label appears"
    s = rec[back]
    assert s["stats"]["reactivations"] == 1 and s["stats"]["last_id"] == old
    assert s["ids"][-1] == old and s["obj_id"] == old and s["inactive"] == 0, "the old id, at the end of the list; the label image carries it"
    assert s["last"]["winner"] == -1 and not any(c["eligible"] for c in s["last"]["candidates"]), "the static hypothesis explains nothing there"
    q = s["search"]
    assert q["winner"] == 0 and q["attempts"] >= 1
    c = q["candidates"][0]
    assert c["id"] == old and c["registered"] and c["converged"] and c["eligible"] and 1 <= c["iterations"] <= 10
    assert c["first_inliers"] >= 6 and c["last_inliers"] >= c["first_inliers"] // 2
    assert abs(c["moved"] - dist) <= 0.05, "the registration carried the map about as far as the object went"
    # old map, count, confidence threshold: in the frame of its reactivation the map is what it was when the model was deactivated
    i5, ib = rec[5]["ids"].index(old), s["ids"].index(old)
    assert s["obj_map"].shape == rec[5]["obj_map"].shape and s["obj_map"].tobytes() == rec[5]["obj_map"].tobytes()
    assert s["counts"][ib] == rec[5]["counts"][i5] and s["confs"][ib] == rec[5]["confs"][i5]
    assert max(s["ids"]) == max(rec[5]["ids"]), "no id was consumed"
    for t in range(back, FRAMES):
        assert old in rec[t]["ids"] and rec[t]["obj_id"] == old, f"frame {t}: the model stays"
        assert rec[t]["stats"]["reactivations"] == 1


def test_the_pose_log_continues(tmp_path):
    """the old model's pose log: its entries from before it left, then those from its return on, in ONE file under the old id"""
    rec = run("search", 0.3, poses_to=str(tmp_path) + "/")
    old = rec[5]["obj_id"]
    log = np.loadtxt(tmp_path / f"poses-{old}.txt", ndmin=2)
    stamps = [int(v) for v in log[:, 0]]          # (frame t is fed with timestamp t)
    back = next(t for t in range(BACK, FRAMES) if rec[t]["stats"]["reactivations"])
    assert any(t <= 5 for t in stamps) and not any(t in HIDDEN for t in stamps), stamps
    assert [t for t in stamps if t > HIDDEN[-1]] == list(range(back, FRAMES)), stamps
    assert not any((tmp_path / f"poses-{i}.txt").exists() for i in range(max(rec[5]["ids"]) + 1, 10)), "no other object was ever logged"


@pytest.mark.parametrize("dist", [0.3, 0.5])
def test_without_the_search_the_same_frames_spawn_a_new_id(dist):
    """the other half of the pair: the static pass alone tries the object where it stood and spawns"""
    rec = run("static", dist)
    old = rec[5]["obj_id"]
    assert rec[6]["inactive"] == 1 and old not in rec[6]["ids"]
    st = rec[-1]["stats"]
    assert st["attempts"] >= 1 and st["reactivations"] == 0 and st["last_id"] == -1
    new = rec[-1]["obj_id"]
    assert new not in (None, 0, old) and new in rec[-1]["ids"] and old not in rec[-1]["ids"]
    first = next(s for s in rec if "last" in s)
    assert first["last"]["winner"] == -1 and first["search"] == dict(winner=-1, attempts=0, candidates=[]), "the search reports nothing when it is off"


def test_drift_after_reactivation_is_bounded_by_continuous_tracking():
    """e = the error of the object's world position G M^-1 c (c: the centroid of its map at frame 5) at the last frame against the truth
    (where it was at frame 5, plus the shift).  e_r: hidden for three frames, back 0.3 m away and found by the search; e_c: never hidden,
    never moved, tracked throughout.  Bound: e_r <= 2 e_c + 1e-3 m, the bound of the static pass's drift test."""
    errs = {}
    for name, dist, rec in (("searched", 0.3, run("search", 0.3)), ("continuous", 0.0, run("search", 0.0, hide=False))):
        old = rec[5]["obj_id"]
        c = rec[5]["obj_map"][:, :3].astype(np.float64).mean(axis=0)
        p5 = world_point(rec[5], rec[5]["ids"].index(old), c)
        pl = world_point(rec[-1], rec[-1]["ids"].index(old), c)
        truth = p5 + (shift_of(dist) if dist else 0.0)
        errs[name] = float(np.linalg.norm(pl - truth))
    print(f"world-point error at frame {FRAMES - 1}: searched {errs['searched']:.6f} m, continuous {errs['continuous']:.6f} m")
    assert run("search", 0.0, hide=False)[-1]["stats"]["attempts"] == 0
    assert errs["searched"] <= 2 * errs["continuous"] + 1e-3, errs


def test_a_stranger_of_the_same_shape_is_spawned_anew():
    rec = run("search", 0.3, stranger=True)
    old = rec[5]["obj_id"]
    assert rec[6]["inactive"] == 1
    st = rec[-1]["stats"]
    assert st["attempts"] >= 1 and st["reactivations"] == 0
    new = rec[-1]["obj_id"]
    assert new not in (None, 0, old) and new in rec[-1]["ids"] and old not in rec[-1]["ids"]
    assert rec[-1]["inactive"] >= 1, "the rejected candidate is still kept"
    first = next(s for s in rec if "search" in s)
    c = first["search"]["candidates"][0]
    true = next(s for s in run("search", 0.3) if "search" in s)["search"]["candidates"][0]
    print(f"colour similarity: the returning object {true['colour']:.4f}, the stranger {c['colour']:.4f}")
    assert first["search"]["winner"] == -1 and not c["registered"], "refused by its colours, before any registration"
    assert c["colour"] < true["colour"]


def test_a_parked_object_goes_through_the_static_path():
    """with the search on, an object that returns where it stood is the static pass's: its record and the maps equal, byte for byte, those
    of an instance that has no search -- and the search never ran"""
    fr = frames(0.0)
    a, b = make("search"), make("static")
    for t in range(FRAMES):
        feed(a, fr[t], t); feed(b, fr[t], t)
        x, y = snap(a, maps=True), snap(b, maps=True)
        assert x["ids"] == y["ids"] and x["counts"] == y["counts"] and x["confs"] == y["confs"] and x["stats"] == y["stats"], f"frame {t}"
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x["poses"], y["poses"])), f"frame {t}: poses"
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x["maps"], y["maps"])), f"frame {t}: maps"
        assert a.redetect_last() == b.redetect_last(), f"frame {t}"
        assert np.array_equal(a.mask(), b.mask()), f"frame {t}: label image"
    assert x["stats"]["reactivations"] == 1 and a.redetect_last()["winner"] == 0
    assert a.redetect_search_last() == dict(winner=-1, attempts=0, candidates=[])
    a.close(); b.close()


def test_an_idle_search_changes_nothing():
    """switched on against re-detection off over the frames before any deactivation: snapshot for snapshot"""
    fr = frames(0.3)
    a, b = make("search"), make("off")
    for t in range(HIDDEN[0]):
        feed(a, fr[t], t); feed(b, fr[t], t)
        x, y = snap(a, maps=True), snap(b, maps=True)
        assert x["ids"] == y["ids"] and x["counts"] == y["counts"] and x["confs"] == y["confs"], f"frame {t}"
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x["poses"], y["poses"])), f"frame {t}: poses"
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x["maps"], y["maps"])), f"frame {t}: maps"
        if t > 0:
            assert np.array_equal(a.mask(), b.mask()), f"frame {t}: label image"
    assert len(x["ids"]) == 3 and x["stats"]["attempts"] == 0 and a.redetect_search_last()["attempts"] == 0
    a.close(); b.close()


def test_model_parallel_instances_and_a_search_without_redetection_are_refused():
    from co_fusion_amd import facade
    cam = synth.Camera.scaled(W, H)
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, rank=0, world=2, **KW)
    with pytest.raises(facade.CoFusionError, match="world == 1"):
        cf.set_redetection_search(True)
    cf.set_redetection_search(False)   # switching it off is always possible
    cf.close()
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, **KW)
    with pytest.raises(facade.CoFusionError, match="setRedetection"):
        cf.set_redetection_search(True)
    cf.set_redetection(True, **RD)
    cf.set_redetection_search(True, iterations=3, min_colour=0.25, max_registered=1)
    with pytest.raises(facade.CoFusionError):
        cf.set_redetection_search(True, iterations=101)
    cf.close()
