#!/usr/bin/env python3
"""Micro-benchmark of the re-detection of inactive models (csrc/redetect.hip, CoFusion::redetectModels).  Prints one JSON
line and writes it to profiles/redetect_bench.json:

  * device time of cf_redetect_score's launches (the counters' fill, the score, the finishing launch: device events inside the call,
    cf_redetect_timing) for 1 / 4 / 8 candidate maps of about 10^5 and 10^6 surfels at 640x480, and of the relabel launch (in-stream
    events), medians of --iters; the score's streamed bytes (16 B per surfel) over its time;
  * wall time of a frame in which a kept model is reactivated against a frame in which a model is spawned, on the same stream: the
    objects4 frames of bench.py with ground-truth masks on the device, one object's mask value withheld for three frames at a time
    and given back -- with re-detection on (the old value: a reactivation) and off (a new value: a spawn) --, and of the frames around;
  * frames/s of the objects4 workload of bench.py (same frames, same pre-roll) with re-detection off and on, legs alternated.

  * the search behind the static pass (csrc/redetect_search.hip, CoFusion::setRedetectionSearch): device time of its three launches
    (frame moments; model moments of 1 / 8 candidates; one registration step) for maps of about 10^5 and 10^6 surfels, the wall time
    of one iteration of cf_redetect_register -- launch, read-back, host wait and solve: the per-iteration wait --, and the wall time of
    a whole frame in which an object that came back 0.3 m away is found by the search against the same frame spawning a model.

    python tools/redetect_bench.py [--iters 100] [--steps 300] [--cycles 8] [--no-frames] [--no-kernels] [--no-search]
    python tools/redetect_bench.py --only-search      (measures the search leg alone and adds it to the file of --out)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480
NEW_LABEL = 7


def kernels(torch, iters):
    from co_fusion_amd import api, model, redetect, synth
    cam = synth.Camera.scaled(W, H)
    depth, _, label, _ = synth.Scene(n_obj=2).render(cam, 0, noise=True)
    lab = np.where(label == 1, np.uint8(NEW_LABEL), np.uint8(0))
    # a map of the whole frame: every valid pixel back-projected, repeated with a sub-pixel jitter up to the wanted size
    v, u = np.nonzero(depth > 0)
    rng = np.random.default_rng(5)

    def surfels(n):
        k = rng.integers(0, v.size, size=n)
        z = depth[v[k], u[k]].astype(np.float32)
        s = np.zeros((n, 12), np.float32)
        s[:, 0] = (u[k] + rng.random(n).astype(np.float32) - np.float32(cam.cx)) * z / np.float32(cam.fx)
        s[:, 1] = (v[k] + rng.random(n).astype(np.float32) - np.float32(cam.cy)) * z / np.float32(cam.fy)
        s[:, 2] = z
        s[:, 3] = 1.0
        return s

    ctx = api.Context(W, H, cam.fx, cam.fy, cam.cx, cam.cy, max_models=2, max_surfels=1 << 20)
    dd, dl = ctx.to_device(depth), ctx.to_device(lab)
    models = [model.Model(ctx, 1 << 20) for _ in range(8)]
    out = {}
    redetect.timing(ctx, True)
    for n in (100_000, 1_000_000):
        for m in models:
            m.upload_map(surfels(n))
        for c in (1, 4, 8):
            cands = [(m, np.eye(4, dtype=np.float32), 0.5) for m in models[:c]]
            ms = []
            for i in range(iters + 5):
                counts, px = redetect.score(ctx, cands, dd, dl, (cam.fx, cam.fy, cam.cx, cam.cy), NEW_LABEL, 20.0, 0.10)
                if i >= 5:
                    ms.append(redetect.timing(ctx, True))
            us = float(np.median(ms) * 1e3)
            out[f"{c}x{n}"] = dict(score_us=round(us, 2), surfels=c * n, streamed_bytes=c * n * 16, gb_per_s=round(c * n * 16 / (us * 1e-6) / 1e9, 1),
                                   agree_on_label=counts[0]["agree_on_label"], covered=counts[0]["covered"], label_pixels=px)
    flat = dl.reshape(-1).clone()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for k, (a, b) in enumerate(ev):   # (7 -> 9 -> 7 ...: every launch rewrites the labelled pixels)
        a.record(); redetect.relabel(ctx, flat, NEW_LABEL if k % 2 == 0 else 9, 9 if k % 2 == 0 else NEW_LABEL); b.record()
    torch.cuda.synchronize()
    out["relabel_us"] = round(float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3), 2)
    for m in models:
        m.close()
    ctx.close()
    return out


def _stream(torch):
    import bench
    wl = bench.WORKLOADS["objects4"]
    n_frames, n_obj = 16, wl["n_obj"]
    cam, fr = bench.make_stream(W, H, n_frames, n_obj=n_obj, seed=1234)
    dev = torch.device("cuda", 0)
    resident = [dict(depth=torch.from_numpy(f["depth"]).to(dev), rgba=torch.from_numpy(f["rgba"]).to(dev)) for f in fr]
    return bench, cam, fr, resident, n_frames, n_obj


def reactivation_frames(torch, cycles):
    """the objects4 frames with their ground-truth masks on the device; the mask value of object 2 is withheld for three frames of every
    twelve.  on: it returns under its old value and the kept model is reactivated; off: under a fresh value, and a model is spawned."""
    from co_fusion_amd import facade
    bench, cam, fr, resident, n_frames, n_obj = _stream(torch)
    P = 24 * n_obj + 30
    out = {}
    for name, on in (("spawn", False), ("reactivation", True)):
        cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, enable_multiple_models=1, model_spawn_offset=2)
        if on:
            cf.set_redetection(True)
        value = 80
        event_ms, other_ms, events = [], [], 0
        for i in range(P + 12 * cycles):
            k = bench.frame_index(i, n_frames)
            gt = (fr[k]["label"] * 40).astype(np.uint8)
            phase = (i - P) % 12 if i >= P else -1
            if 0 <= phase < 3:
                gt[gt == 80] = 0
            elif phase == 3 and not on:
                value = 80 + 1 + (i - P) // 12          # (a mapped value cannot spawn again with re-detection off)
            if value != 80:
                gt[gt == 80] = value
            mt = torch.from_numpy(gt).to(resident[k]["depth"].device)
            before = (cf.num_models, cf.redetect_stats()["reactivations"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cf.process_frame_device(resident[k]["depth"], resident[k]["rgba"], timestamp=i, mask=mt)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if i < P:
                continue
            happened = cf.redetect_stats()["reactivations"] > before[1] if on else cf.num_models > before[0]
            if happened:
                event_ms.append(dt); events += 1
            elif phase > 4:
                other_ms.append(dt)
        out[name] = dict(frames=events, median_ms=round(float(np.median(event_ms)), 3) if event_ms else None,
                         other_frames_median_ms=round(float(np.median(other_ms)), 3), models=cf.num_models, inactive=cf.num_inactive_models,
                         stats=cf.redetect_stats())
        cf.close()
    return out


def objects4(torch, steps, warmup):
    from co_fusion_amd import facade
    bench, cam, fr, resident, n_frames, n_obj = _stream(torch)
    P = 24 * n_obj + 30
    out = {"off": [], "on": []}
    for name in ("off", "on", "off", "on"):
        cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, enable_multiple_models=1, device_frames_complete=1)
        if name == "on":
            cf.set_redetection(True)
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
        out[name].append(dict(frames_per_s=round(steps / (time.perf_counter() - t0), 1), models=cf.num_models, inactive=cf.num_inactive_models,
                              stats=cf.redetect_stats()))
        cf.close()
    return out


def search_kernels(torch, iters):
    """the three launches of the search by device events (cf_redetect_timing covers them), and the registration loop in wall time"""
    from co_fusion_amd import api, model, redetect, synth
    cam = synth.Camera.scaled(W, H)
    depth, rgb, label, _ = synth.Scene(n_obj=2).render(cam, 0, noise=True)
    lab = np.where(label == 2, np.uint8(NEW_LABEL), np.uint8(0))
    v, u = np.nonzero((label == 2) & (depth > 0))
    rng = np.random.default_rng(5)
    camt = (cam.fx, cam.fy, cam.cx, cam.cy)

    def surfels(n):   # the labelled object's pixels back-projected with a sub-pixel jitter, normals along the viewing ray
        k = rng.integers(0, v.size, size=n)
        z = depth[v[k], u[k]].astype(np.float32)
        s = np.zeros((n, 12), np.float32)
        s[:, 0] = (u[k] + rng.random(n).astype(np.float32) - np.float32(cam.cx)) * z / np.float32(cam.fx)
        s[:, 1] = (v[k] + rng.random(n).astype(np.float32) - np.float32(cam.cy)) * z / np.float32(cam.fy)
        s[:, 2] = z
        s[:, 3] = 1.0
        s[:, 4] = 0x804020
        s[:, 8:11] = s[:, :3] / np.linalg.norm(s[:, :3], axis=1, keepdims=True)
        return s

    ctx = api.Context(W, H, cam.fx, cam.fy, cam.cx, cam.cy, max_models=2, max_surfels=1 << 20)
    dd, dl, dc = ctx.to_device(depth), ctx.to_device(lab), ctx.to_device(synth.rgb_to_rgba(rgb))
    models = [model.Model(ctx, 1 << 20) for _ in range(8)]
    redetect.timing(ctx, True)
    out = {}
    ms = []
    for i in range(iters + 5):
        fm, _ = redetect.frame_moments(ctx, dd, dl, dc, camt, NEW_LABEL, 20.0)
        if i >= 5:
            ms.append(redetect.timing(ctx, True))
    out["frame_moments_us"] = round(float(np.median(ms) * 1e3), 2)
    centre = np.array([fm[1 + a] / 65536.0 / fm[0] for a in range(3)], np.float32)
    dhat = centre / np.linalg.norm(centre)
    shifted = np.eye(4, dtype=np.float32); shifted[0, 3] = 0.02   # the loop starts 2 cm off and has something to do
    for n in (100_000, 1_000_000):
        for m in models:
            m.upload_map(surfels(n))
        row = dict(surfels=n)
        for c in (1, 8):
            cands = [(m, np.eye(4, dtype=np.float32), 0.5) for m in models[:c]]
            ms = []
            for i in range(iters + 5):
                mm, _ = redetect.model_moments(ctx, cands, dhat)
                if i >= 5:
                    ms.append(redetect.timing(ctx, True))
            row[f"model_moments_{c}_us"] = round(float(np.median(ms) * 1e3), 2)
        ms, wall = [], []
        for i in range(iters + 5):
            sums = redetect.register_step(ctx, models[0], 0.5, shifted, dd, dl, camt, NEW_LABEL, 20.0, 0.10, centre)
            if i >= 5:
                ms.append(redetect.timing(ctx, True))
        for i in range(iters + 5):   # ONE iteration per call: launch, read-back, host wait, solve -- what every iteration of the loop costs
            t0 = time.perf_counter()
            r = redetect.register(ctx, models[0], 0.5, shifted, dd, dl, camt, NEW_LABEL, 20.0, 0.10, centre, iterations=1)
            if i >= 5:
                wall.append((time.perf_counter() - t0) * 1e6)
        row.update(register_step_us=round(float(np.median(ms) * 1e3), 2), step_inliers=int(sums[28]), front_facing=int(mm[0][0]),
                   register_wall_per_iteration_us=round(float(np.median(wall)), 1), register_ok=bool(r["ok"]))
        out[str(n)] = row
    for m in models:
        m.close()
    ctx.close()
    return out


def searched_frames(torch, repeats):
    """synth.Scene(n_obj=2) at 640x480: its second object stands still from frame 4 on, is gone in frames 6-8 and is back in frame 9,
    0.3 m from where it stood, under a new mask value.  spawn: re-detection off; searched: the static pass fails, the search finds it."""
    from co_fusion_amd import facade, synth

    class Returning(synth.Scene):
        def object_pose(self, i, t):
            T = super().object_pose(i, min(t, 4) if i == 1 else t).copy()
            if i == 1 and t >= 9:
                T[0, 3] += -0.3 if T[0, 3] > 0 else 0.3
            return T

    cam = synth.Camera.scaled(W, H)
    sc = Returning(n_obj=2)
    fr = []
    for t in range(11):
        keep = sc.objects
        if t in (6, 7, 8):
            sc.objects = keep[:1]
        d, rgb, lab, _ = sc.render(cam, t, noise=True)
        sc.objects = keep
        gt = (lab * 40).astype(np.uint8)
        if t >= 9:
            gt[gt == 80] = 120
        fr.append((torch.from_numpy(d).cuda(), torch.from_numpy(synth.rgb_to_rgba(rgb)).cuda(), torch.from_numpy(gt).cuda()))
    out = {}
    for name in ("spawn", "searched"):
        ev, other, last = [], [], None
        for _ in range(repeats):
            cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, enable_multiple_models=1, model_spawn_offset=2, conf_global_init=0.5)
            if name == "searched":
                cf.set_redetection(True, keep_min_surfels=64)
                cf.set_redetection_search(True)
            for t, (d, c, m) in enumerate(fr):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cf.process_frame_device(d, c, timestamp=t, mask=m)
                torch.cuda.synchronize()
                (ev if t == 9 else other).append((time.perf_counter() - t0) * 1e3) if t >= 5 else None
            last = dict(models=cf.num_models, inactive=cf.num_inactive_models, stats=cf.redetect_stats(), search=cf.redetect_search_last())
            cf.close()
        out[name] = dict(frames=len(ev), median_ms=round(float(np.median(ev)), 3), other_frames_median_ms=round(float(np.median(other)), 3), last=last)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--cycles", type=int, default=8, help="withhold-and-return cycles of the reactivation / spawn frame legs")
    ap.add_argument("--no-frames", action="store_true", help="skip the frame legs")
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-launch times")
    ap.add_argument("--no-search", action="store_true", help="skip the legs of the search behind the static pass")
    ap.add_argument("--only-search", action="store_true", help="the search legs alone, added to the file of --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redetect_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("redetect_bench.py needs a GPU")
    res = dict(tool="redetect_bench", size=[W, H], iters=a.iters)
    if a.only_search:
        if a.out and os.path.exists(a.out):
            res = json.loads(open(a.out).read())
        a.no_kernels = a.no_frames = True
    if not a.no_search:
        res["search"] = dict(iters=a.iters, kernels=search_kernels(torch, a.iters), frame_ms=searched_frames(torch, max(a.cycles // 2, 3)))
    if not a.no_kernels:
        res["kernels"] = kernels(torch, a.iters)
    if not a.no_frames:
        res["frame_ms"] = reactivation_frames(torch, a.cycles)
        res["objects4"] = objects4(torch, a.steps, a.warmup)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
