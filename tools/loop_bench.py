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

With --seam, the legs of the fern seam (cofusion_set_loop_closure) instead, merged into the same file under "seam": the gate launch and
the closure launch at 500 ferns and 640x480, cf_ferns_find_frame's wall time beside cf_ferns_relocalise's on the same state, frames/s of
bench.py's objects4 workload with loop closure on against relocalisation alone and against off (alternated --rounds times in one
process; the price of the per-frame wait in microseconds beside the relocalisation leg's own spread), and the wall time of the frame
that closes the loop in the scenario of tests/test_loop_closure_gpu.py.

With --local, the built legs of local loop closure, merged into the same file under "local" (medians of 20 by in-stream events): the
inactive prediction and the depth synthesis of a 640x480 map of 307 200 surfels, and assemble / iterate of a graph object sized for 1536
constraints at 768 + 768 constraints for 40 / 200 / 1024 nodes, beside the same object's and the 128-capacity object's figures at 100
constraints; the model-to-model tracker (preparation through cf_odom_init_icp_maps + the Gauss-Newton loop) on two views of the room of
the smoke test at 640x480, and the constraint launch + the wait on its record.  (The frame loop is not built: no closing frame, no
objects4 leg.)

With --relative, the step with relative constraints, merged into the same file under "relative" (medians of --iters by in-stream
events, read-back included): assemble and iterate at 40 / 200 / 1024 nodes with the 100 shift constraints and 0 / 16 / 128 stored pairs
between the newest and the oldest nodes, on an object with the ring enabled, beside iterate on an object without it (0 pairs launches
the same kernels: the two must agree within the run-to-run spread, which the repeated "plain" figure shows), and the launch
Y = L^-1 U^T on its own (cf_deform_bench_relative_y on the state an iteration left).  The other kernels' own times come from a kernel
trace of this leg taken in a run of its own.

    python tools/loop_bench.py [--iters 30] [--no-frames]
    python tools/loop_bench.py --relative
    python tools/loop_bench.py --local
    python tools/loop_bench.py --seam [--steps 300] [--warmup 30] [--rounds 3] [--min-age 30]
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


def relative_legs(torch, iters):
    import deform_cases as dc
    import deform_rel_cases as rc
    from co_fusion_amd import api, deform
    ctx = api.Context(640, 480, 528.0, 528.0, 320.0, 240.0, max_models=2, max_surfels=1 << 16)
    plain, d = deform.Deform(ctx), deform.Deform(ctx)
    d.enable_relative()
    out = {}
    for n in (40, 200, 1024):
        nodes = dc.make_nodes(n)
        src, dst, tm = dc.constraints("shift", nodes)
        row = {}
        for name, obj, pairs in (("plain", plain, None), ("0_pairs", d, 0), ("16_pairs", d, 16), ("128_pairs", d, 128), ("plain_again", plain, None)):
            def reset():
                obj.set_nodes(nodes); obj.weights(src, dst, tm)
                if pairs is not None:
                    obj.set_relative(rc.pairs_between(nodes, np.arange(n - 8, n), np.arange(8), pairs))
            reset()
            row[name + "_assemble_ms"] = median_ms(torch, obj.assemble, iters)
            row[name + "_iterate_ms"] = median_ms(torch, obj.iterate, iters, before=reset)
            reset()
            step = obj.iterate()
            row[name + "_step"] = dict(error=float(step["error"]), failed=bool(step["failed"]))
            if pairs:   # the Y launch on its own, on the factor and the rows that step left
                row[name + "_y_launch_ms"] = median_ms(torch, obj.bench_relative_y, iters)
        out[str(n)] = row
    plain.close(); d.close(); ctx.close()
    return out


def local_legs(torch, iters=20):
    import deform_cases as dc
    import local_loop_cases as lc
    from co_fusion_amd import api, deform, model as M
    ctx = api.Context(640, 480, 528.0, 528.0, 320.0, 240.0, max_models=2, max_surfels=1 << 19)
    out = {}
    # a wall of one surfel per texel, every second one inactive
    rng = np.random.default_rng(5)
    wall = lc.layer(rng, 640, 480, 2.0, np.where(np.arange(640 * 480) % 2 == 0, 50, 130), -1.2, 1.2, -0.9, 0.9, radius=0.004)
    m = M.Model(ctx, 1 << 19)
    m.upload_map(wall)
    pose = np.eye(4, dtype=np.float32)
    depth = ctx.empty((480, 640))
    m.combined_predict(pose, 20.0, 10.0, 140, 140, 40)
    out["active_prediction_ms"] = median_ms(torch, lambda: m.combined_predict(pose, 20.0, 10.0, 140, 140, 40), iters)
    out["inactive_prediction_ms"] = median_ms(torch, lambda: m.predict_inactive(pose, 20.0, 10.0, 100, 40), iters)
    out["inactive_covered"] = m.inactive_covered()
    out["depth_synthesis_ms"] = median_ms(torch, lambda: m.synthesize_depth(pose, 20.0, 10.0, 140, 100, 65535, depth), iters)
    out["surfels"] = int(len(wall))
    m.close()
    out.update(local_tracker(torch, ctx, iters))
    small, big = deform.Deform(ctx), deform.Deform(ctx, deform.MAX_CONSTRAINTS_SIZED)
    graph = {}
    for n in (40, 200, 1024):
        nodes = dc.make_nodes(n)
        row = {}
        for name, d, cons, ldt in (("100_cap128", small, dc.constraints("shift", nodes), None), ("100_cap1536", big, dc.constraints("shift", nodes), None),
                                   ("1536_cap1536", big, lc.big_constraints(nodes), 0)):
            src, dst, tm = cons
            d.set_nodes(nodes)
            row[name + "_weights_ms"] = median_ms(torch, lambda: d.weights(src, dst, tm), iters)
            row[name + "_assemble_ms"] = median_ms(torch, lambda: d.assemble(ldt), iters)
            reset = lambda: d.set_nodes(nodes) or d.weights(src, dst, tm)
            row[name + "_iterate_ms"] = median_ms(torch, lambda: d.iterate(ldt), iters, before=reset)
        graph[str(n)] = row
    out["graph"] = graph
    small.close(); big.close(); ctx.close()
    return out


def local_scenario(torch):
    """wall time of the frames of tests/test_local_loop_closure_gpu.py up to its first closure, by what the local branch did in them"""
    import local_loop_scene as sc
    import test_local_loop_closure_gpu as t
    from co_fusion_amd import facade
    views = sc.make_views()
    cf = facade.CoFusion(**t.KW)
    try:
        cf.set_local_loop_closure(True, sample_rate=sc.RATE)
        rows = []
        for k in range(t.MAX_FRAMES):
            d, rgb = views(k)
            before = cf.local_loop_stats()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            cf.process_frame(d, rgb, timestamp=k, in_pose=sc.yaw_pose(sc.DRIFT * sc.TURN_DEG * k))
            torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3
            after = cf.local_loop_stats()
            kind = ("closing" if after["deforms"] > before["deforms"] else "skipped_by_gate" if after["skipped_by_gate"] > before["skipped_by_gate"] else
                    "tracker_rejected" if after["examined"] > before["examined"] else "not_examined")
            rows.append((kind, ms))
            if kind == "closing":
                break
        out = {k: dict(frames=sum(1 for a, _ in rows if a == k), median_wall_ms=float(np.median([m for a, m in rows if a == k])))
               for k in ("not_examined", "skipped_by_gate", "tracker_rejected", "closing") if any(a == k for a, _ in rows)}
        st = cf.local_loop_stats(); st["last_est_pose"] = st["last_est_pose"].tolist()
        out["stats"] = st; out["surfels"] = cf.model_info(0)["count"]
        return out
    finally:
        cf.close()


def local_objects4(torch, steps, warmup, rounds):
    """frames/s of bench.py's objects4 workload in ONE process, the legs alternated `rounds` times: with the relocalisation switch and a
    time_delta of 100 ticks, and with local loop closure on top (every measured frame examined: the pre-roll and the warm-up are longer
    than time_delta)"""
    import bench
    from co_fusion_amd import facade
    wl = bench.WORKLOADS["objects4"]
    W, H = wl["size"]
    n_frames, n_obj = 16, wl["n_obj"]
    cam, fr = bench.make_stream(W, H, n_frames, n_obj=n_obj, seed=1234)
    dev = torch.device("cuda", 0)
    resident = [dict(depth=torch.from_numpy(f["depth"]).to(dev), rgba=torch.from_numpy(f["rgba"]).to(dev)) for f in fr]
    P = 24 * n_obj + 30
    legs = (("relocalisation_on", False), ("local_loop_closure_on", True))
    out = {name: dict(frames_per_s=[]) for name, _ in legs}
    for _ in range(rounds):
        for name, local in legs:
            cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, enable_multiple_models=1, device_frames_complete=1, reloc=1, time_delta=100)
            cf.set_relocalisation(True, min_age=30)
            if local:
                cf.set_local_loop_closure(True)
            for i in range(P):   # the pre-roll of bench.py: ground-truth masks until the object models exist
                f = fr[bench.frame_index(i, n_frames)]
                cf.process_frame(f["depth"], f["rgb"], mask=(f["label"] * 40).astype(np.uint8), timestamp=i)
            def run(lo, hi):
                for i in range(lo, hi):
                    r = resident[bench.frame_index(i, n_frames)]
                    cf.process_frame_device(r["depth"], r["rgba"], timestamp=i)
            run(P, P + warmup)
            torch.cuda.synchronize()
            e0 = cf.local_loop_stats()["examined"]
            t0 = time.perf_counter()
            run(P + warmup, P + warmup + steps)
            torch.cuda.synchronize()
            out[name]["frames_per_s"].append(round(steps / (time.perf_counter() - t0), 1))
            if local:
                st = cf.local_loop_stats(); st["last_est_pose"] = st["last_est_pose"].tolist()
                out[name]["stats"] = st; out[name]["examined_in_measured_frames"] = st["examined"] - e0
            cf.close()
    med = {k: float(np.median(v["frames_per_s"])) for k, v in out.items()}
    out["per_frame_price_us_vs_relocalisation_on"] = round((1.0 / med["local_loop_closure_on"] - 1.0 / med["relocalisation_on"]) * 1e6, 1)
    out["relocalisation_on_spread_us"] = round((1.0 / min(out["relocalisation_on"]["frames_per_s"]) - 1.0 / max(out["relocalisation_on"]["frames_per_s"])) * 1e6, 1)
    return out


def local_tracker(torch, ctx, iters):
    """the model-to-model tracker in the reference's call order, and the constraint launch behind it with the wait on its record"""
    import common
    from co_fusion_amd import api, local_loop, synth
    fp = common.frame_pair(640, 480, noise=True)
    v4b, n4b, imgb = synth.ideal_prediction(fp["cam"], fp["d1"], fp["rgb1"])
    cam = fp["cam"]
    c2 = api.Context(640, 480, cam.fx, cam.fy, cam.cx, cam.cy)
    g, l = api.Odometry(c2), local_loop.LocalLoop(c2)
    d = c2.to_device
    pose = common.perturbed_pose(2)
    dev = dict(v4=d(fp["v4"]), n4=d(fp["n4"]), img=d(fp["img"]), v4b=d(np.float32(v4b)), n4b=d(np.float32(n4b)), imgb=d(imgb))
    old_time = d(np.full((480, 640), 7, np.uint16))

    def prepare():
        g.init_icp_model(dev["v4"], dev["n4"], pose)
        g.init_rgb_model(dev["img"])
        g.init_icp_maps(dev["v4b"], dev["n4b"])
        g.init_rgb(dev["imgb"])

    def track():
        prepare()
        return g.track(pose[:3, 3], pose[:3, :3], rgb_only=False, icp_weight=10.0, pyramid=True, fast_odom=False, so3=False)

    def constraints():
        l.constraints_async(dev["v4b"], old_time, pose, 9, 20.0, True, odom=g, cov_thresh=1.0, icp_count_thresh=1000, icp_err_thresh=1.0)
        return l.wait()

    out = dict(tracker_preparation_ms=median_ms(torch, prepare, iters), tracker_preparation_and_loop_ms=median_ms(torch, track, iters))
    track()
    out["constraints_launch_and_wait_ms"] = median_ms(torch, constraints, iters)
    rec = constraints()
    out["constraints"] = dict(accepted=rec["accepted"], n_constraints=rec["n_constraints"])
    l.close(); g.close(); c2.close()
    return out


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


def seam_kernels(torch, iters):
    """the fern side of the seam at 500 ferns, 640x480 (the room of tests/ferns_scene.py, query 94 against keyframe 2): the gate launch
    and the closure launch by in-stream events, cf_ferns_find_frame's wall time against cf_ferns_relocalise's on the same state"""
    import ferns_scene as fs
    from co_fusion_amd import api, ferns
    c = fs.CAM
    ctx = api.Context(fs.W, fs.H, c.fx, c.fy, c.cx, c.cy, max_models=1, max_surfels=1024)
    f = ferns.Ferns(ctx, n_ferns=500, capacity=8, max_depth_mm=5000, photo_threshold=115.0, seed=7)
    try:
        for i, t in enumerate(fs.KEYFRAME_TIMES):
            f.add(*(ctx.to_device(a) for a in fs.maps(t)), fs.view(t)[2], 1 + i, -1.0)
        f.encode(*(ctx.to_device(a) for a in fs.maps(fs.QUERY_TIME)))
        curr = fs.view(fs.QUERY_TIME)[2]
        f.search(1000, 300)
        gate_ms = median_ms(torch, lambda: (f.gate_async(), f.gate_wait()), iters)
        f.gate_async(); g = f.gate_wait()
        res, cl = f.find_frame(curr, 1000, 300, lost=False)
        close_ms = median_ms(torch, lambda: f.constraints(res["keyframe"], curr, res["pose"], res["icp_error"], res["icp_count"], False, 1000), iters)
        wall = dict(find_frame=[], relocalise=[])
        for _ in range(iters + 3):
            f.search(1000, 300); f.gate_async(); f.gate_wait()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            f.find_frame(curr, 1000, 300, lost=False)
            wall["find_frame"].append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            f.relocalise(curr, 1000, 300, lost=False)   # (its own search included: one launch)
            wall["relocalise"].append((time.perf_counter() - t0) * 1e3)
        return dict(gate_launch_and_wait_ms=gate_ms, closure_launch_and_read_ms=close_ms, overlap=float(g["overlap"]), accepted=bool(cl["accepted"]),
                    n_constraints=cl["n_constraints"], find_frame_wall_ms=float(np.median(wall["find_frame"][3:])),
                    relocalise_wall_ms=float(np.median(wall["relocalise"][3:])))
    finally:
        f.close(); ctx.close()


def seam_objects4(torch, steps, warmup, rounds, min_age):
    """frames/s of bench.py's objects4 workload in ONE process, the legs alternated `rounds` times: as bench.py runs it, with the
    relocalisation switch on, and with loop closure on top (every measured frame gated: min_age ticks are over before the warm-up ends)"""
    import bench
    from co_fusion_amd import facade
    wl = bench.WORKLOADS["objects4"]
    W, H = wl["size"]
    n_frames, n_obj = 16, wl["n_obj"]
    cam, fr = bench.make_stream(W, H, n_frames, n_obj=n_obj, seed=1234)
    dev = torch.device("cuda", 0)
    resident = [dict(depth=torch.from_numpy(f["depth"]).to(dev), rgba=torch.from_numpy(f["rgba"]).to(dev)) for f in fr]
    P = 24 * n_obj + 30
    legs = (("off", {}, 0), ("relocalisation_on", dict(reloc=1), 1), ("loop_closure_on", dict(reloc=1, time_delta=200), 2))
    out = {name: dict(frames_per_s=[]) for name, _, _ in legs}
    for _ in range(rounds):
        for name, kw, level in legs:
            cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, enable_multiple_models=1, device_frames_complete=1, **kw)
            if level >= 1:
                cf.set_relocalisation(True, min_age=min_age)
            if level >= 2:
                cf.set_loop_closure(True)
            for i in range(P):   # the pre-roll of bench.py: ground-truth masks until the object models exist
                f = fr[bench.frame_index(i, n_frames)]
                cf.process_frame(f["depth"], f["rgb"], mask=(f["label"] * 40).astype(np.uint8), timestamp=i)
            def run(lo, hi):
                for i in range(lo, hi):
                    r = resident[bench.frame_index(i, n_frames)]
                    cf.process_frame_device(r["depth"], r["rgba"], timestamp=i)
            run(P, P + warmup)
            torch.cuda.synchronize()
            g0 = cf.loop_stats()["gated"] if level >= 2 else 0
            t0 = time.perf_counter()
            run(P + warmup, P + warmup + steps)
            torch.cuda.synchronize()
            out[name]["frames_per_s"].append(round(steps / (time.perf_counter() - t0), 1))
            if level >= 2:
                out[name]["stats"] = cf.loop_stats(); out[name]["gated_in_measured_frames"] = out[name]["stats"]["gated"] - g0
            cf.close()
    med = {k: float(np.median(v["frames_per_s"])) for k, v in out.items()}
    out["per_frame_price_us_vs_relocalisation_on"] = round((1.0 / med["loop_closure_on"] - 1.0 / med["relocalisation_on"]) * 1e6, 1)
    out["relocalisation_on_spread_us"] = round((1.0 / min(out["relocalisation_on"]["frames_per_s"]) - 1.0 / max(out["relocalisation_on"]["frames_per_s"])) * 1e6, 1)
    return out


def seam_scenario(torch):
    """wall time of the frame that closes the loop in the scenario of tests/test_loop_closure_gpu.py, beside the plain frames before it"""
    import test_loop_closure_gpu as sc
    from co_fusion_amd import facade, synth
    scene = synth.Scene(n_obj=0, seed=1234)
    scene.camera_pose = lambda t: sc.yaw_pose(sc.TURN_DEG * t)
    cam, cache = synth.Camera(), {}
    cf = facade.CoFusion(reloc=1, enable_multiple_models=0, max_models=2, max_surfels=1 << 22, time_delta=sc.TIME_DELTA)
    try:
        cf.set_relocalisation(True, min_age=sc.MIN_AGE, seed=3)
        cf.set_loop_closure(True, sample_rate=sc.RATE)
        rows = []
        for k in range(sc.LAST + 1):
            if k % 120 not in cache:
                cache[k % 120] = scene.render(cam, k % 120, noise=False)[:2]
            d, rgb = cache[k % 120]
            before = cf.loop_stats()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            cf.process_frame(d, rgb, timestamp=k, in_pose=sc.yaw_pose(sc.DRIFT * sc.TURN_DEG * k))
            torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3
            after = cf.loop_stats()
            kind = ("closing" if after["accepted"] > before["accepted"] else "graph_rejected" if after["optimised"] > before["optimised"] else
                    "fern_rejected" if after["candidates"] > before["candidates"] else "gated" if after["gated"] > before["gated"] else "plain")
            rows.append((kind, ms))
            if kind == "closing":
                break
        out = {k: dict(frames=sum(1 for a, _ in rows if a == k), median_wall_ms=float(np.median([m for a, m in rows if a == k])))
               for k in ("plain", "gated", "fern_rejected", "graph_rejected", "closing") if any(a == k for a, _ in rows)}
        out["stats"] = cf.loop_stats(); out["surfels"] = cf.model_info(0)["count"]
        return out
    finally:
        cf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-frames", action="store_true")
    ap.add_argument("--seam", action="store_true", help="only the legs of the fern seam (written to the 'seam' entry of profiles/loop_bench.json)")
    ap.add_argument("--local", action="store_true", help="only the legs of local loop closure (the 'local' entry of profiles/loop_bench.json)")
    ap.add_argument("--relative", action="store_true", help="only the step with relative constraints (the 'relative' entry of profiles/loop_bench.json)")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-age", type=int, default=30)
    a = ap.parse_args()
    import torch
    path = os.path.join(ROOT, "profiles", "loop_bench.json")
    if a.relative:
        out = json.load(open(path)) if os.path.exists(path) else {}
        out["relative"] = relative_legs(torch, a.iters)
        print(json.dumps(out["relative"]))
        with open(path, "w") as f:
            f.write(json.dumps(out) + "\n")
        return
    if a.local:
        out = json.load(open(path)) if os.path.exists(path) else {}
        out["local"] = local_legs(torch)
        out["local"]["scenario"] = local_scenario(torch)
        if not a.no_frames:
            out["local"]["objects4"] = local_objects4(torch, a.steps, a.warmup, a.rounds)
        print(json.dumps(out["local"]))
        with open(path, "w") as f:
            f.write(json.dumps(out) + "\n")
        return
    if a.seam:
        out = json.load(open(path)) if os.path.exists(path) else {}
        out["seam"] = dict(kernels=seam_kernels(torch, a.iters), scenario=seam_scenario(torch))
        if not a.no_frames:
            out["seam"]["objects4"] = seam_objects4(torch, a.steps, a.warmup, a.rounds, a.min_age)
        line = json.dumps(out)
        print(json.dumps(out["seam"]))
        with open(path, "w") as f:
            f.write(line + "\n")
        return
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
