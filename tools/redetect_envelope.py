#!/usr/bin/env python3
"""The envelope of the re-detection search's registration (DESIGN.md 4.13 "Search", limits), measured with the numpy statement
tests/redetect_search_ref.py -- no GPU: a 0.30 x 0.24 x 0.20 m box at 160x128 (fx = 128), mapped from a random orientation with the
faces then in view (2 mm noise), comes back 0.3 m sideways, turned by the row's angle about a random axis (3 mm depth noise).  Seed and
loop as the frame loop runs them; a draw counts when the result is within 50 mm and 10 degrees of the truth -- half the tracker's gates.

    python tools/redetect_envelope.py [--draws 32] [--angles 0 10 20 30 40]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import redetect_ref            # noqa: E402
import redetect_search_cases as sc   # noqa: E402
import redetect_search_ref as ref    # noqa: E402

SIZE = (160, 128)


def draw(rng, angle):
    axis = rng.normal(size=3)
    R_old = sc.rot(rng.normal(size=3), rng.uniform(0.0, 180.0))
    T_old = sc.rigid(R_old, [-0.15, 0.0, 1.5])
    T_true = sc.rigid(sc.rot(axis, angle) @ R_old, [0.15, 0.0, 1.5])
    m = sc.box_map(T_old, sc.BOX_HALF, rng)
    depth, label, rgba = sc.raycast_box(SIZE, T_true, sc.BOX_HALF, rng)
    cam = sc.cam_of(SIZE)
    fm, _ = ref.frame_moments(depth, label, rgba, sc.L, cam, sc.CUTOFF)
    fbar, dhat = ref.frame_centroid(fm)
    pose = np.linalg.inv(T_old).astype(np.float32)
    mm, _ = ref.model_moments(m, sc.THETA, pose, np.asarray(dhat, np.float32))
    seed = ref.seed(redetect_ref.inv44f(pose), mm, fbar)
    if seed is None:
        return None
    reg = ref.register(m, sc.THETA, seed, depth, label, sc.L, cam, sc.CUTOFF, sc.TOL_BOX, np.asarray(fbar, np.float32))
    T = reg["cam_from_model"].astype(np.float64)
    D = T[:3, :3] @ T_true[:3, :3].T
    ang = float(np.degrees(np.arccos(np.clip((np.trace(D) - 1.0) / 2.0, -1.0, 1.0))))
    return dict(ok=bool(reg["ok"]), dist=float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])), angle=ang, faces=int(len(m) > 0), iterations=reg["iterations"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--angles", type=float, nargs="*", default=[0, 10, 20, 30, 40])
    a = ap.parse_args()
    out = {}
    for angle in a.angles:
        rng = np.random.default_rng(1000 + int(angle))
        rows = [draw(rng, angle) for _ in range(a.draws)]
        good = [r for r in rows if r and r["ok"] and r["dist"] <= 0.05 and r["angle"] <= 10.0]
        miss = [r for r in rows if r not in good and r]
        out[str(angle)] = dict(good=len(good), draws=a.draws, failed=sum(1 for r in rows if not r or not r["ok"]),
                               miss_angle=[round(r["angle"], 1) for r in miss], miss_dist_mm=[round(r["dist"] * 1e3, 1) for r in miss],
                               good_dist_mm_max=round(max([r["dist"] for r in good], default=0.0) * 1e3, 2),
                               good_angle_max=round(max([r["angle"] for r in good], default=0.0), 2))
        print(f"turned {angle:g} deg: {len(good)}/{a.draws} within 50 mm and 10 deg", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
