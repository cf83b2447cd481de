"""GPU parity of the facade's device-mask entries (cofusion_process_frame_device_masked, cofusion_group_process_frames_device_masked):
frames AND their label masks resident in device memory, the mask branch of the segmentation as kernels on a side lane -- against the
oracle's restatement of CoFusion::processFrame with ground-truth masks, free running: model list, label mask, counts, poses, confidence
thresholds and surfels bit for bit, every frame, through a spawn and a deactivation."""
import warnings

import numpy as np
import pytest

import orc_multi as om
from co_fusion_amd import synth

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

W, H = 160, 128
FRAMES, GONE_FROM = 10, 7   # from frame GONE_FROM on the masks lack the second object's label: its model is deactivated
KW = dict(max_surfels=1 << 18, conf_global_init=0.5, model_spawn_offset=2, enable_multiple_models=1)


def _frames(seed=None):
    cam = synth.Camera.scaled(W, H)
    sc = synth.Scene(n_obj=2) if seed is None else synth.Scene(n_obj=2, seed=seed)   # (no seed: the scene of test_facade_multi_model_matches_oracle)
    out = []
    for t in range(FRAMES):
        d, rgb, lab, _ = sc.render(cam, t, noise=True)
        gt = (lab * 40).astype(np.uint8)
        if t >= GONE_FROM:
            gt[gt == 80] = 0
        out.append((d, rgb, gt))
    return cam, out


_REF = {}


def _reference():
    """the oracle's run, once for the module: per frame the model list (id, count, pose, confidence threshold, surfels) and the label mask"""
    if not _REF:
        cam, frames = _frames()
        ref = om.MultiPipeline(cam, conf_global=0.5, spawn_offset=2)
        snaps = []
        for d, rgb, gt in frames:
            ref.process_frame(d, synth.rgb_to_rgba(rgb), gt_mask=gt)
            snaps.append(dict(mask=ref.mask.copy(),
                              models=[dict(id=m.id, pose=m.pose.copy(), conf=np.float32(m.conf_threshold), surfels=m.surfels.copy()) for m in ref.models]))
        _REF.update(cam=cam, frames=frames, snaps=snaps)
    return _REF


def _same(a, b, what):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    assert a.tobytes() == b.tobytes(), f"{what}: {np.count_nonzero(a.view(np.uint8) != b.view(np.uint8))} bytes differ"


@pytest.mark.parametrize("complete", [0, 1])
def test_device_masks_match_the_oracle(complete):
    import torch
    from co_fusion_amd import facade
    R = _reference()
    cam = R["cam"]
    counts = [len(s["models"]) for s in R["snaps"]]
    assert max(counts) == 3, "both objects must have been spawned"
    assert counts[GONE_FROM - 1] == 3 and counts[GONE_FROM] == 2, "the model whose label left the masks must be deactivated"
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, device_frames_complete=complete, **KW)
    for t, ((d, rgb, gt), snap) in enumerate(zip(R["frames"], R["snaps"])):
        dt = torch.from_numpy(d).cuda(); ct = torch.from_numpy(synth.rgb_to_rgba(rgb)).cuda(); mt = torch.from_numpy(gt).cuda()
        torch.cuda.synchronize()   # (device_frames_complete = 1: the buffers are complete at call time)
        cf.process_frame_device(dt, ct, timestamp=t, mask=mt)
        assert cf.num_models == len(snap["models"]), f"frame {t}: model count {cf.num_models} vs {len(snap['models'])}"
        if t > 0:
            _same(cf.mask(), snap["mask"], f"frame {t}: label mask")
        for i, m in enumerate(snap["models"]):
            info = cf.model_info(i)
            assert info["id"] == m["id"], f"frame {t} model {i}: id"
            assert info["count"] == m["surfels"].shape[0], f"frame {t} model {i}: count {info['count']} vs {m['surfels'].shape[0]}"
            _same(info["pose"], m["pose"], f"frame {t} model {i}: pose")
            _same(np.float32(info["conf_threshold"]), m["conf"], f"frame {t} model {i}: confidence threshold")
            _same(cf.model_download(i), m["surfels"], f"frame {t} model {i}: surfels")
    cf.close()


def test_masked_group_equals_single_handles():
    """three sequences through the masked group entry -- the middle one WITHOUT a mask (motion segmentation) -- against three handles of
    their own fed through the single entry"""
    import torch
    from co_fusion_amd import facade
    S = 3
    runs = [_frames(seed=1234 + 17 * s) for s in range(S)]
    cam = runs[0][0]
    group = facade.CoFusionGroup(S, W, H, cam.fx, cam.fy, cam.cx, cam.cy, **KW)
    singles = [facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, **KW) for _ in range(S)]
    most = 0
    for t in range(FRAMES):
        dts = [torch.from_numpy(r[1][t][0]).cuda() for r in runs]
        cts = [torch.from_numpy(synth.rgb_to_rgba(r[1][t][1])).cuda() for r in runs]
        mts = [None if s == 1 else torch.from_numpy(runs[s][1][t][2]).cuda() for s in range(S)]
        group.process_frames_device(dts, cts, timestamp=t, masks=mts)
        for s in range(S):
            singles[s].process_frame_device(dts[s], cts[s], timestamp=t, mask=mts[s])
        for s, (a, b) in enumerate(zip(group.sequences, singles)):
            assert a.num_models == b.num_models, f"frame {t} sequence {s}: {a.num_models} vs {b.num_models} models"
            if t > 0:
                assert np.array_equal(a.mask(), b.mask()), f"frame {t} sequence {s}: label mask"
            for i in range(b.num_models):
                x, y = a.model_info(i), b.model_info(i)
                assert x["id"] == y["id"] and x["count"] == y["count"], f"frame {t} sequence {s} model {i}: id / count"
                assert x["pose"].tobytes() == y["pose"].tobytes(), f"frame {t} sequence {s} model {i}: pose"
                assert x["conf_threshold"] == y["conf_threshold"]
                assert a.model_download(i).tobytes() == b.model_download(i).tobytes(), f"frame {t} sequence {s} model {i}: surfels"
        most = max(most, singles[0].num_models, singles[2].num_models)
    assert most >= 2, "no object model was spawned from the masks"
    group.close()
    for q in singles:
        q.close()


def test_device_masks_are_refused_for_model_parallel_instances():
    import torch
    from co_fusion_amd import facade
    cam = synth.Camera.scaled(W, H)
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, rank=0, world=2, **KW)
    d = torch.zeros((H, W), dtype=torch.float32, device="cuda"); c = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    m = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    with pytest.raises(facade.CoFusionError, match="world == 1"):
        cf.process_frame_device(d, c, mask=m)
    with pytest.raises(facade.CoFusionError, match="16-byte aligned|contiguous"):
        facade._check_mask_tensor(torch.zeros((H, W + 1), dtype=torch.uint8, device="cuda")[:, 1:], d)
    cf.close()
