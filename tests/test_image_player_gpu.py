"""GPU suite: the image player end to end (images.ImageSequencePlayer, host/ImagePlayer.cpp over csrc/image_decode.hip).  A directory
played through the player must deliver the serial reader's frames byte for byte and leave the CoFusion instance exactly where
images.ImageSequenceReader + process_frame (the host entry) leaves it: same model list, surfel counts and pose bits after every frame,
for any number of workers."""
import os

import numpy as np
import pytest

import klg_player_cases as kc
from co_fusion_amd import synth

pytestmark = pytest.mark.gpu

W, H, FRAMES = 160, 128, 6
CAM = synth.Camera.scaled(W, H)
OPTS = dict(max_surfels=1 << 17, conf_global_init=0.5, model_spawn_offset=2, enable_multiple_models=1)


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    from co_fusion_amd import facade, images
    return facade, images


@pytest.fixture(scope="module")
def scene_dir(mods, tmp_path_factory):
    """the synthetic scene with one moving object: PNG colour (a filter type per frame, several IDATs), ZIP EXR depth with B, G, R
    planes, PNG label masks; numbered from 1"""
    _, im = mods
    d = tmp_path_factory.mktemp("images")
    sc = synth.Scene(n_obj=1)
    for t in range(FRAMES):
        depth, rgb, lab, _ = sc.render(CAM, t, noise=True)
        depth = np.nan_to_num(depth).astype(np.float32)
        im.write_png(str(d / f"Color{t + 1:04d}.png"), np.ascontiguousarray(rgb, np.uint8), filters=(t % 5,), idat_chunks=2)
        im.write_exr(str(d / f"Depth{t + 1:04d}.exr"), {"B": depth, "G": depth * 2, "R": depth * 0}, compression=im.EXR_ZIP)
        im.write_png(str(d / f"Mask{t + 1:04d}.png"), (lab * 40).astype(np.uint8), filters=(2,))
    return str(d)


class _View:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(int(ptr), False), version=2)


def _download(cf, ptrs, h, w):
    import torch
    ts, dptr, cptr, mptr = ptrs
    assert cf.abi.cf_synchronize(cf._ctx()) == 0   # with device_frames_complete = 0 the frame is ordered on the context's stream
    get = lambda p, shape, t: torch.as_tensor(_View(p, shape, t), device=cf.device).cpu().numpy()
    return ts, get(dptr, (h, w), "<f4"), get(cptr, (h, w, 4), "|u1"), (None if not mptr else get(mptr, (h, w), "|u1"))


def _same_frames(got, want):
    assert len(got) == len(want)
    for k, ((ts, d, c, m), (ts0, d0, c0, m0)) in enumerate(zip(got, want)):
        assert ts == ts0 and d.tobytes() == d0.tobytes(), f"frame {k}: timestamp / depth"
        assert np.array_equal(c[..., :3], c0) and (c[..., 3] == 255).all(), f"frame {k}: colour"
        assert (m is None and m0 is None) or np.array_equal(m, m0), f"frame {k}: mask"


def _state(cf):
    return [(m["id"], m["count"], m["pose"].tobytes()) for m in (cf.model_info(i) for i in range(cf.num_models))]


@pytest.fixture(scope="module")
def baseline(mods, scene_dir):
    """the serial reader into the host entry, masks included"""
    facade, im = mods
    cf = facade.CoFusion(W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy, **OPTS)
    frames, states = [], []
    with im.ImageSequenceReader(scene_dir) as r:
        assert (r.width, r.height, r.num_frames, r.start_index, r.has_masks) == (W, H, FRAMES, 1, True)
        for ts, depth, rgb, mask in r:
            cf.process_frame(depth, rgb, mask=mask, timestamp=ts)
            frames.append((ts, depth, rgb, mask))
            states.append(_state(cf))
    cf.close()
    print("models per frame:", [len(s) for s in states])
    return frames, states


@pytest.mark.parametrize("workers", [1, 3])
def test_player_leaves_the_instance_where_the_reader_does(mods, scene_dir, baseline, workers):
    facade, im = mods
    for complete in (0, 1):
        cf = facade.CoFusion(W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy, device_frames_complete=complete, **OPTS)
        player = im.ImageSequencePlayer(cf, scene_dir, workers=workers)
        assert (player.num_frames, player.has_masks, player.max_masks) == (FRAMES, True, FRAMES)
        states = []
        while player.process():
            states.append(_state(cf))
        assert not player.process()
        t = player.times()
        assert t["inflate"] > 0 and t["unfilter"] > 0 and t["read"] > 0 and t["parse"] > 0
        player.close()
        cf.close()
        assert len(states) == FRAMES
        for k, (a, b) in enumerate(zip(states, baseline[1])):
            assert [m[0] for m in a] == [m[0] for m in b], f"frame {k}: model list"
            assert [m[1] for m in a] == [m[1] for m in b], f"frame {k}: surfel counts"
            assert [m[2] for m in a] == [m[2] for m in b], f"frame {k}: pose bits"


@pytest.mark.parametrize("workers", [1, 3])
def test_player_frames_are_the_readers_frames_and_rewind_replays_them(mods, scene_dir, baseline, workers):
    facade, im = mods
    cf = facade.CoFusion(W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy, max_surfels=1 << 12, enable_multiple_models=0)
    player = im.ImageSequencePlayer(cf, scene_dir, workers=workers)
    for _ in range(2):
        _same_frames([_download(cf, p, H, W) for p in player], baseline[0])
        player.rewind()
    _same_frames([_download(cf, next(player), H, W) for _ in range(2)], baseline[0][:2])
    player.rewind()   # with frames submitted ahead
    player.set_limits(4)
    _same_frames([_download(cf, p, H, W) for p in player], baseline[0][:4])
    player.close()
    cf.close()


def test_jpeg_colour_with_png_depth_and_flipped_channels(mods, tmp_path):
    facade, im = mods
    stream, ref = kc.fixture("restart_64x48_420")   # (an instance's width is a multiple of 16)
    mm = np.random.default_rng(6).integers(0, 65536, ref.shape[:2]).astype(np.uint16)
    mm.reshape(-1)[:5] = [0, 1, 255, 256, 65535]
    ddata = im.png_bytes(mm, filters=(4, 3, 1), idat_chunks=2)
    for i in range(3):
        (tmp_path / f"Color{i:04d}.jpg").write_bytes(bytes(stream))
        (tmp_path / f"Depth{i:04d}.png").write_bytes(ddata)
    h, w = ref.shape[:2]
    cam = synth.Camera.scaled(w, h)
    cf = facade.CoFusion(w, h, cam.fx, cam.fy, cam.cx, cam.cy, max_surfels=1 << 12, enable_multiple_models=0, device_frames_complete=1)
    for flip in (False, True):
        with im.ImageSequenceReader(str(tmp_path), flip_colors=flip, depth_scale=0.0002) as r:
            want = list(r)
        assert np.array_equal(want[0][2], ref[..., ::-1] if flip else ref)
        assert want[0][1].tobytes() == (mm.astype(np.float32) * np.float32(0.0002)).tobytes()
        with im.ImageSequencePlayer(cf, str(tmp_path), flip_colors=flip, depth_scale=0.0002, workers=2) as player:
            _same_frames([_download(cf, p, h, w) for p in player], want)
    cf.close()


def test_a_corrupt_frame_and_refusals(mods, scene_dir, baseline, tmp_path):
    facade, im = mods
    import shutil
    d = tmp_path / "bad"
    shutil.copytree(scene_dir, d)
    data = (d / "Color0004.png").read_bytes()
    (d / "Color0004.png").write_bytes(data[:len(data) // 2])
    cf = facade.CoFusion(W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy, max_surfels=1 << 12, enable_multiple_models=0)
    player = im.ImageSequencePlayer(cf, str(d), workers=3)
    _same_frames([_download(cf, next(player), H, W) for _ in range(3)], baseline[0][:3])
    with pytest.raises(im.ImageError, match="frame 3: .*Color0004.png: "):
        next(player)
    assert list(player) == []
    player.close()
    cf.close()
    small = facade.CoFusion(64, 48, 50.0, 50.0, 32.0, 24.0, max_surfels=1 << 12, enable_multiple_models=0)
    with pytest.raises(im.ImageError, match="160 x 128"):
        im.ImageSequencePlayer(small, scene_dir)
    small.close()
    g = facade.CoFusionGroup(2, W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy, **OPTS)
    with pytest.raises(im.ImageError, match="lock-step"):
        im.ImageSequencePlayer(g.sequences[0], scene_dir)
    g.close()


def test_masks_ending_at_frame_4_and_the_model_parallel_refusal(mods, scene_dir, baseline):
    """max_masks = 4: frames 0..3 go through the masked device entry, frames 4 and 5 -- inside a set that has masks -- through the
    plain one, and the instance ends where the host entry with the same masks ends"""
    facade, im = mods
    want = facade.CoFusion(W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy, **OPTS)
    states = []
    for k, (ts, depth, rgb, mask) in enumerate(baseline[0]):
        want.process_frame(depth, rgb, mask=mask if k < 4 else None, timestamp=ts)
        states.append(_state(want))
    want.close()
    for workers in (1, 3):
        cf = facade.CoFusion(W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy, **OPTS)
        with im.ImageSequencePlayer(cf, scene_dir, workers=workers, max_masks=4) as player:
            assert (player.has_masks, player.max_masks) == (True, 4)
            got = [_download(cf, p, H, W) for p in player]
            assert [g[3] is not None for g in got] == [True] * 4 + [False] * 2
            _same_frames(got, [(ts, d, c, m if k < 4 else None) for k, (ts, d, c, m) in enumerate(baseline[0])])
            player.rewind()
            played = []
            while player.process():
                played.append(_state(cf))
        cf.close()
        assert played == states
    par = facade.CoFusion(W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy, rank=0, world=2, **OPTS)
    with pytest.raises(im.ImageError, match="world > 1"):
        im.ImageSequencePlayer(par, scene_dir)
    par.close()

