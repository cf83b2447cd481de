#!/usr/bin/env python3
"""Micro-benchmark of the deformation-graph loop closure (csrc/deform.hip, cofusion_deform_background).  Prints one JSON
line and writes it to profiles/loop_bench.json:

  * every stage's time by in-stream events (medians of --iters) for 40 / 200 / 1024 nodes with 100 constraints (50 + 50 pins): sample,
    weights (upload included), assemble (residual rows + normal equations), iterate (assemble + band Cholesky + substitutions + update +
    new residual; its read-back included), the keyframe-pose pass over 64 poses;
  * the map pass at 10^5 and 10^6 surfels over 200 and 1024 nodes, with its bytes (48 B read + 32 B written per surfel) and their share
    of the 8 TB/s peak;
  * wall time of cofusion_deform_background on a fused 640x480 map (an accepted correction, and one the 0.06 gate turns away) beside
    the wall time of a plain frame of the same sequence.

    python tools/loop_bench.py [--iters 30] [--no-frames]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_BPS = 8e12


def median_ms(torch, fn, iters, before=None):
    ms = []
    for i in range(iters + 3):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def stages(torch, iters):
    import deform_cases as dc
    from co_fusion_amd import api, deform
    ctx = api.Context(640, 480, 528.0, 528.0, 320.0, 240.0, max_models=2, max_surfels=1 << 16)
    d = deform.Deform(ctx)
    out = {}
    for n in (40, 200, 1024):
        nodes = dc.make_nodes(n)
        src, dst, tm = dc.constraints("shift", nodes)
        surfels = dc.make_map(4 * n, 4, seed=1)
        dev = ctx.to_device(surfels)
        poses = ctx.to_device(np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (64, 1)))
        times = ctx.to_device(np.linspace(0, float(nodes[-1, 3]), 64).astype(np.int32))
        row = {}
        row["sample_ms"] = median_ms(torch, lambda: d.sample(dev, 4), iters)
        d.set_nodes(nodes)
        row["weights_ms"] = median_ms(torch, lambda: d.weights(src, dst, tm), iters)
        row["assemble_ms"] = median_ms(torch, d.assemble, iters)
        reset = lambda: d.set_nodes(nodes) or d.weights(src, dst, tm)
        row["iterate_ms"] = median_ms(torch, d.iterate, iters, before=reset)
        reset()
        t0 = time.perf_counter(); res = d.optimise(); row["optimise_wall_ms"] = (time.perf_counter() - t0) * 1e3
        row["optimise"] = {k: (bool(v) if isinstance(v, bool) else float(v)) for k, v in res.items()}
        row["poses_ms"] = median_ms(torch, lambda: d.apply_poses(poses, times), iters)
        out[str(n)] = row
    apply = {}
    for n in (200, 1024):
        nodes = dc.make_nodes(n)
        d.set_nodes(nodes, dc.bent_params(n))
        for s in (100_000, 1_000_000):
            m = dc.make_map(s, max(s // int(nodes[-1, 3]), 1), seed=2)
            dev = ctx.to_device(m)
            ms = median_ms(torch, lambda: d.apply(dev), iters)
            apply[f"{n}_nodes_{s}_surfels"] = dict(ms=ms, bytes=80 * s, share_of_peak=80 * s / (ms * 1e-3) / PEAK_BPS)
    d.close(); ctx.close()
    return dict(stages=out, apply=apply)


def frames(torch):
    import ferns_scene as fs
    from co_fusion_amd import facade
    c = fs.CAM
    cf = facade.CoFusion(fs.W, fs.H, c.fx, c.fy, c.cx, c.cy, enable_multiple_models=0, max_models=2, max_surfels=1 << 20)
    try:
        wall = []
        for i, t in enumerate(range(0, 30, 3)):
            dpt, rgb, gt = fs.view(t)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            cf.process_frame(dpt, rgb, timestamp=i, in_pose=gt)
            torch.cuda.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
        m = cf.model_download(0)
        pick = np.linspace(0, len(m) - 1, 50).astype(np.int64)
        src, tm = m[pick, :3].copy(), m[pick, 6].copy()
        out = dict(surfels=int(len(m)), plain_frame_wall_ms=float(np.median(wall[2:])))
        for name, shift in (("turned_away", 0.01), ("accepted", 0.07)):
            t0 = time.perf_counter()
            res = cf.deform_background(src, src + np.float32([shift, 0, 0]), tm, sample_rate=2500)
            out[name] = dict(wall_ms=(time.perf_counter() - t0) * 1e3, nodes=res["nodes"], accepted=res["accepted"], iterations=res["iterations"])
        return out
    finally:
        cf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-frames", action="store_true")
    a = ap.parse_args()
    import torch
    out = stages(torch, a.iters)
    if not a.no_frames:
        out["deform_background"] = frames(torch)
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "loop_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
