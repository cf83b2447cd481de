#!/usr/bin/env python3
"""What the label-mask branch costs per frame, three ways, on the stream of bench.py's objects4-gt workload (640x480, 4 objects):

  a  host entry, host masks            cofusion_process_frame(mask=...)            frame AND mask uploaded / visited on the host
  b  device entry, device masks        cofusion_process_frame_device_masked        frame and mask resident in HBM, mask kernels on a lane
  c  device entry, motion CRF          cofusion_process_frame_device               for scale: the other segmentation branch
  h  host entry, host loops kept       the same call as a with CF_MASKS_HOST=1     (diagnostics switch: the route before the mask kernels)

Every leg has an instance of its own, pre-rolled with ground-truth masks through the host entry until the object models exist (bench.py's
pre-roll); then the legs are ALTERNATED --rounds times in one process, --steps timed frames each after --warmup untimed ones.  One JSON
line: per leg the median ms/frame with min and max over the rounds, and whether legs a and b ended in the same state (they are fed
the same frames and masks: the digests must agree).  --legs a: only that leg (an older build of the libraries, loaded with CF_LIB_DIR,
has no masked device entry)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--preroll", type=int, default=24 * 4 + 30)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mask_bench.py needs a GPU: the hot path has no CPU fallback")
    import bench
    from co_fusion_amd import facade
    W, H, n_obj = 640, 480, 4
    cam, frames = bench.make_stream(W, H, a.frames, n_obj=n_obj, seed=1234)
    masks = [(f["label"] * 40).astype(np.uint8) for f in frames]
    dev = torch.device("cuda", 0)
    resident = [dict(depth=torch.from_numpy(f["depth"]).to(dev), rgba=torch.from_numpy(f["rgba"]).to(dev), mask=torch.from_numpy(m).to(dev))
                for f, m in zip(frames, masks)]
    torch.cuda.synchronize()
    legs = [x for x in a.legs.split(",") if x]
    inst, pos = {}, {}
    for leg in legs:
        if leg == "h":
            os.environ["CF_MASKS_HOST"] = "1"   # (read when the instance is created)
        cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, enable_multiple_models=1, device_frames_complete=1)
        os.environ.pop("CF_MASKS_HOST", None)
        for i in range(a.preroll):
            k = bench.frame_index(i, a.frames)
            cf.process_frame(frames[k]["depth"], frames[k]["rgb"], mask=masks[k], timestamp=i)
        inst[leg], pos[leg] = cf, a.preroll

    def step(leg, i):
        k = bench.frame_index(i, a.frames)
        cf = inst[leg]
        if leg in ("a", "h"):
            cf.process_frame(frames[k]["depth"], frames[k]["rgb"], mask=masks[k], timestamp=i)
        elif leg == "b":
            cf.process_frame_device(resident[k]["depth"], resident[k]["rgba"], timestamp=i, mask=resident[k]["mask"])
        else:
            cf.process_frame_device(resident[k]["depth"], resident[k]["rgba"], timestamp=i)

    ms = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg in legs:
            i0 = pos[leg]
            for i in range(i0, i0 + a.warmup):
                step(leg, i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(i0 + a.warmup, i0 + a.warmup + a.steps):
                step(leg, i)
            torch.cuda.synchronize()
            ms[leg].append((time.perf_counter() - t0) * 1e3 / a.steps)
            pos[leg] = i0 + a.warmup + a.steps
    out = dict(tool="mask_bench", size=[W, H], objects=n_obj, steps=a.steps, warmup=a.warmup, rounds=a.rounds, preroll=a.preroll,
               lib_dir=os.environ.get("CF_LIB_DIR", "co_fusion_amd/lib"),
               ms_per_frame={leg: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), rounds=[round(x, 4) for x in v])
                             for leg, v in ms.items()},
               models={leg: inst[leg].num_models for leg in legs})
    if "a" in inst and "b" in inst:
        out["legs_a_b_same_state"] = bench.state_digest(inst["a"]) == bench.state_digest(inst["b"])
    print(json.dumps(out), flush=True)
    for cf in inst.values():
        cf.close()


if __name__ == "__main__":
    main()
