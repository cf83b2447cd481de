"""GPU test of `tools/run_klg.py <directory>`: a Co-Fusion-style image set (Color####.png, 16-bit Depth####.png in millimetres,
Mask####.png, numbered from 1) through the tool -- the serial image reader and the host entry, then --player: worker threads, frames
finished on the device, the masked device entry -- exports the pose files of a run that is fed the same arrays directly."""
import os
import subprocess
import sys

import numpy as np
import pytest

from co_fusion_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 160, 128
FRAMES = 25   # the default spawn offset lets the first object in at frame 22


def test_run_klg_plays_an_image_directory(tmp_path):
    from co_fusion_amd import facade, images
    cam = synth.Camera.scaled(W, H)
    sc = synth.Scene(n_obj=2)
    d = tmp_path / "set"; d.mkdir()
    frames = []
    for t in range(FRAMES):
        depth, rgb, lab, _ = sc.render(cam, t, noise=True)
        mm = np.clip(np.round(np.nan_to_num(depth) * 1000.0), 0, 65535).astype(np.uint16)
        mask = (lab * 40).astype(np.uint8)
        images.write_png(str(d / f"Color{t + 1:04d}.png"), np.ascontiguousarray(rgb, np.uint8), filters=(t % 5,))
        images.write_png(str(d / f"Depth{t + 1:04d}.png"), mm, filters=(4,), idat_chunks=3)
        images.write_png(str(d / f"Mask{t + 1:04d}.png"), mask, filters=(2,))
        ts = int(np.float32(t) * np.float32(1000.0) / np.float32(24.0))
        frames.append((ts, mm.astype(np.float32) * np.float32(0.001), np.ascontiguousarray(rgb, np.uint8), mask))
    out = tmp_path / "tool"; out.mkdir()
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_klg.py"), str(d), str(out), "--fx", str(cam.fx), "--fy", str(cam.fy),
           "--cx", str(cam.cx), "--cy", str(cam.cy), "--max-surfels", str(1 << 18), "--depth-scale", "0.001"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{FRAMES} frames of {FRAMES}" in r.stdout and "2 active models" in r.stdout, r.stdout
    ref = tmp_path / "direct"; ref.mkdir()
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, max_surfels=1 << 18, enable_multiple_models=1, enable_pose_logging=1, reloc=0)
    for ts, depth, rgb, mask in frames:
        cf.process_frame(depth, rgb, mask=mask, timestamp=ts)
    assert cf.export_poses(str(ref) + "/") >= 1
    cf.close()
    poses = [{f: open(p / f, "rb").read() for f in sorted(os.listdir(p)) if f.startswith("poses-")} for p in (out, ref)]
    assert len(poses[0]) >= 1 and poses[0] == poses[1], "the tool's run differs from a run fed the same arrays"
    played = tmp_path / "player"; played.mkdir()
    cmd[3] = str(played)
    r = subprocess.run(cmd + ["--player", "--workers", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{FRAMES} frames of {FRAMES}" in r.stdout and "image player, 2 workers" in r.stdout, r.stdout
    assert {f: open(played / f, "rb").read() for f in sorted(os.listdir(played)) if f.startswith("poses-")} == poses[0], "serial reader and player disagree"
