"""GPU suite: the .klg log player end to end (klg.KlgPlayer, host/KlgPlayer.cpp over csrc/frame_decode.hip).  A log played through the
player must leave the CoFusion instance exactly where today's path -- klg.KlgReader + process_frame -- leaves it: same model list,
surfel counts and pose bits after every frame, for any number of workers and both meanings of device_frames_complete."""
import os
import subprocess
import sys

import numpy as np
import pytest

import klg_player_cases as kc
from co_fusion_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES = 160, 128, 8
CAM = synth.Camera.scaled(W, H)
OPTS = dict(max_surfels=1 << 17, conf_global_init=0.5, model_spawn_offset=2, enable_multiple_models=1)


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    from co_fusion_amd import facade, klg
    return facade, klg


def _frames(refused=None):
    """the synthetic scene with one moving object as a log: zlib depth, JPEG 4:2:0 colour (the committed encodes of the scene's frames)"""
    sc = synth.Scene(n_obj=1)
    out = []
    for t in range(FRAMES):
        d = sc.render(CAM, t, noise=True)[0]
        mm = np.rint(d * np.float32(1000.0)).astype(np.uint16)
        jb = kc.scene_jpeg(t)
        out.append((t * 33333, mm, "zlib", kc.wide_quant(jb) if t == refused else jb))
    return out


@pytest.fixture(scope="module")
def logs(tmp_path_factory):
    d = tmp_path_factory.mktemp("player")
    return kc.write_log(d / "scene.klg", _frames()), kc.write_log(d / "refused.klg", _frames(refused=3))


def _state(cf):
    out = []
    for i in range(cf.num_models):
        m = cf.model_info(i)
        out.append((m["id"], m["count"], m["pose"].tobytes()))
    return out


@pytest.fixture(scope="module")
def baseline(mods, logs):
    """(a) today's path: the serial reader into process_frame"""
    facade, klg = mods
    cf = facade.CoFusion(W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy, **OPTS)
    states = []
    for ts, depth, rgb in klg.KlgReader(logs[0], W, H):
        cf.process_frame(depth, rgb, timestamp=ts)
        states.append(_state(cf))
    cf.close()
    assert len(states) == FRAMES
    print("models per frame:", [len(s) for s in states])
    return states


def _play(mods, path, workers, complete):
    facade, klg = mods
    cf = facade.CoFusion(W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy, device_frames_complete=complete, **OPTS)
    player = klg.KlgPlayer(cf, path, workers=workers)
    assert player.num_frames == FRAMES
    states = []
    while player.process():
        states.append(_state(cf))
    assert not player.process()
    player.close()
    cf.close()
    return states


def _same(got, want):
    assert len(got) == len(want)
    for t, (a, b) in enumerate(zip(got, want)):
        assert [m[0] for m in a] == [m[0] for m in b], f"frame {t}: model list"
        assert [m[1] for m in a] == [m[1] for m in b], f"frame {t}: surfel counts"
        assert [m[2] for m in a] == [m[2] for m in b], f"frame {t}: pose bits"


@pytest.mark.parametrize("complete", [0, 1])
@pytest.mark.parametrize("workers", [1, 4])
def test_player_leaves_the_instance_where_the_reader_does(mods, logs, baseline, workers, complete):
    _same(_play(mods, logs[0], workers, complete), baseline)


def test_a_refused_frame_plays_through_the_host_decoder(mods, logs, baseline):
    """frame 3 carries 16-bit quantisation tables: the front end refuses it, the player decodes it on the host and uploads RGB"""
    _, klg = mods
    kinds = [k for _, _, k, _ in klg.KlgPrefetcher(logs[1], W, H, workers=2)]
    assert kinds == [klg.COLOR_JPEG] * 3 + [klg.COLOR_DECODED] + [klg.COLOR_JPEG] * 4
    _same(_play(mods, logs[1], 4, 0), baseline)


def test_player_frames_are_the_readers_frames(mods, tmp_path):
    """the frames themselves, on a log of every frame kind (zlib and raw depth holding 0, 1, 999, 1000, 32768, 65535; JPEG and raw
    colour), both flip_colors values, twice (rewind): depth bit for bit, colour byte for byte"""
    import torch
    facade, klg = mods
    w, h = 64, 48
    path = kc.write_log(tmp_path / "mixed.klg", kc.mixed_log_frames())
    cam = synth.Camera.scaled(w, h)
    for complete in (0, 1):
        cf = facade.CoFusion(w, h, cam.fx, cam.fy, cam.cx, cam.cy, max_surfels=1 << 12, enable_multiple_models=0, device_frames_complete=complete)
        for flip in (False, True):
            want = list(klg.KlgReader(path, w, h, flip_colors=flip))
            player = klg.KlgPlayer(cf, path, flip_colors=flip, workers=3)
            for _ in range(2):
                got = []
                for ts, dptr, cptr in player:
                    if not complete:
                        assert cf.abi.cf_synchronize(cf._ctx()) == 0   # the frame is ordered on the context's stream
                    d = torch.as_tensor(_View(dptr, (h, w), "<f4"), device=cf.device).cpu().numpy()
                    c = torch.as_tensor(_View(cptr, (h, w, 4), "|u1"), device=cf.device).cpu().numpy()
                    got.append((ts, d, c))
                assert len(got) == len(want) == 8
                for k, ((ts, d, c), (ts0, d0, c0)) in enumerate(zip(got, want)):
                    assert ts == ts0 and d.tobytes() == d0.tobytes(), f"frame {k}: timestamp / depth"
                    assert np.array_equal(c[..., :3], c0) and (c[..., 3] == 255).all(), f"frame {k}: colour"
                player.rewind()
            player.close()
        cf.close()


class _View:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(int(ptr), False), version=2)


def test_player_is_refused_for_a_group_sequence(mods, logs):
    facade, klg = mods
    g = facade.CoFusionGroup(2, W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy, **OPTS)
    with pytest.raises(klg.KlgError, match="lock-step"):
        klg.KlgPlayer(g.sequences[0], logs[0])
    g.close()


def test_run_klg_with_the_player_writes_the_same_pose_files(logs, tmp_path):
    outs = []
    for extra in ([], ["--player", "--workers", "3"]):
        out = tmp_path / ("player" if extra else "reader")
        cmd = [sys.executable, os.path.join(ROOT, "tools", "run_klg.py"), str(logs[0]), str(out), "--width", str(W), "--height", str(H),
               "--fx", str(CAM.fx), "--fy", str(CAM.fy), "--cx", str(CAM.cx), "--cy", str(CAM.cy), "--max-surfels", str(1 << 17)] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"{FRAMES} frames of {FRAMES}" in r.stdout, r.stdout
        outs.append({f: (out / f).read_bytes() for f in sorted(os.listdir(out)) if f.startswith("poses-")})
    assert outs[0] and outs[0].keys() == outs[1].keys()
    for f in outs[0]:
        assert outs[0][f] == outs[1][f], f"{f} differs"
