#!/usr/bin/env python3
"""Micro-benchmark of the fern keyframe database (csrc/ferns.hip), one JSON line:

  * microseconds of the encode, search and append launches at database sizes 0, 1000 and 10000 keyframes of 500 ferns at 640x480,
    by in-stream events around each single launch, median of --iters (>= 200); the append is a real one (its threshold is below every
    dissimilarity, so the copy of the 130 KB slot happens);
  * the scan's bytes / time: code rows (512 B) + good count + time read and co[] written per keyframe, against the 8 TB/s peak;
  * frames/s of the objects4 workload of bench.py (same frames, same pre-roll) in ONE process: as bench.py runs it, with reloc = 1,
    and with reloc = 1 and the relocalisation switch on.

    python tools/ferns_bench.py [--iters 200] [--steps 300] [--no-frames] [--no-kernels]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_us(torch, fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)


def kernels(torch, iters):
    from co_fusion_amd import api, ferns, synth
    cam = synth.Camera.scaled(640, 480)
    d, rgb, _, _ = synth.Scene(n_obj=0).render(cam, 0, noise=False)
    v4, n4, img = synth.ideal_prediction(cam, d, rgb)
    ctx = api.Context(640, 480, cam.fx, cam.fy, cam.cx, cam.cy, max_models=1, max_surfels=1024)
    dv = tuple(ctx.to_device(a) for a in (v4, n4, img))
    pose = np.eye(4, dtype=np.float32)
    out = {}
    for K in (0, 1000, 10000):
        f = ferns.Ferns(ctx, n_ferns=500, capacity=K + iters + 16, max_depth_mm=5000, seed=1)
        for i in range(K):
            f.add(*dv, pose, i, -1.0)
        assert f.count()[0] == K
        f.encode(*dv)
        enc = median_us(torch, lambda: f.encode(*dv), iters)
        sea = median_us(torch, lambda: f.search(1 << 30, 0), iters)
        scan_bytes = K * (512 + 4 + 4 + 4)
        app = median_us(torch, lambda: f.append(pose, 0, -1.0), iters)   # (the database grows by iters + 10 keyframes meanwhile)
        out[str(K)] = dict(encode_us=round(enc, 2), search_us=round(sea, 2), append_us=round(app, 2), scan_bytes=scan_bytes,
                           scan_gb_s=round(scan_bytes / (sea * 1e-6) / 1e9, 2) if K else 0.0,
                           scan_fraction_of_8tb_s=round(scan_bytes / (sea * 1e-6) / 8e12, 5) if K else 0.0)
        f.close()
    ctx.close()
    return out


def frames(torch, steps, warmup):
    import bench
    from co_fusion_amd import facade
    wl = bench.WORKLOADS["objects4"]
    W, H = wl["size"]
    n_frames, n_obj = 16, wl["n_obj"]
    cam, fr = bench.make_stream(W, H, n_frames, n_obj=n_obj, seed=1234)
    dev = torch.device("cuda", 0)
    resident = [dict(depth=torch.from_numpy(f["depth"]).to(dev), rgba=torch.from_numpy(f["rgba"]).to(dev)) for f in fr]
    P = 24 * n_obj + 30
    out = {}
    for name, kw, on in (("as_bench", {}, False), ("reloc", dict(reloc=1), False), ("relocalisation_on", dict(reloc=1), True)):
        cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, enable_multiple_models=1, device_frames_complete=1, **kw)
        if on:
            cf.set_relocalisation(True)
        for i in range(P):   # the pre-roll of bench.py: ground-truth masks until the object models exist
            f = fr[bench.frame_index(i, n_frames)]
            cf.process_frame(f["depth"], f["rgb"], mask=(f["label"] * 40).astype(np.uint8), timestamp=i)
        def run(lo, hi):
            for i in range(lo, hi):
                r = resident[bench.frame_index(i, n_frames)]
                cf.process_frame_device(r["depth"], r["rgba"], timestamp=i)
        run(P, P + warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(P + warmup, P + warmup + steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[name] = dict(frames_per_s=round(steps / dt, 1), models=cf.num_models, lost=bool(cf.lost))
        if on:
            out[name]["stats"] = cf.reloc_stats()
        cf.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--no-frames", action="store_true", help="skip the objects4 frames/s legs")
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-launch times (e.g. under a kernel trace of the frame legs)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ferns_bench.py needs a GPU")
    res = dict(tool="ferns_bench", n_ferns=500, size=[640, 480], iters=max(200, a.iters))
    if not a.no_kernels:
        res["kernels"] = kernels(torch, max(200, a.iters))
    if not a.no_frames:
        res["objects4"] = frames(torch, a.steps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
