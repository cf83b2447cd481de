"""GPU test of `tools/run_klg.py --mask-dir`: a short log with per-frame PGM label masks through the serial reader (host entry) and
through --player (player iteration + the masked device entry) -- both spawn the objects from the masks and export the same poses."""
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


def test_run_klg_feeds_pgm_masks(tmp_path):
    from co_fusion_amd import klg, masks
    cam = synth.Camera.scaled(W, H)
    sc = synth.Scene(n_obj=2)
    log = tmp_path / "seq.klg"
    mdir = tmp_path / "masks"; mdir.mkdir()
    with klg.KlgWriter(log, W, H) as wr:
        for t in range(FRAMES):
            d, rgb, lab, _ = sc.render(cam, t, noise=True)
            wr.write(33333 * t, d, rgb)
            with open(masks.mask_path(str(mdir), t + 1, "M", 3), "wb") as f:   # numbering from 1, as the reference's datasets
                f.write(b"P5\n%d %d\n255\n" % (W, H) + (lab * 40).astype(np.uint8).tobytes())
    outs = []
    for extra in ([], ["--player", "--workers", "2"]):
        out = tmp_path / ("player" if extra else "serial"); out.mkdir()
        cmd = [sys.executable, os.path.join(ROOT, "tools", "run_klg.py"), str(log), str(out), "--width", str(W), "--height", str(H),
               "--fx", str(cam.fx), "--fy", str(cam.fy), "--cx", str(cam.cx), "--cy", str(cam.cy), "--max-surfels", str(1 << 18),
               "--mask-dir", str(mdir), "--mask-prefix", "M", "--index-width", "3"] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"{FRAMES} frames of {FRAMES}" in r.stdout and "2 active models" in r.stdout, r.stdout   # (one object so far)
        outs.append({f: open(out / f, "rb").read() for f in sorted(os.listdir(out)) if f.startswith("poses-")})
    assert len(outs[0]) >= 1 and outs[0] == outs[1], "serial reader and player disagree"
