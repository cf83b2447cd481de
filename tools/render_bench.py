#!/usr/bin/env python
"""Time the scene renderer (csrc/render.hip) on the bench.py `objects4` workload: 640x480, the pre-roll played with ground-truth masks
until the object models exist, a few more frames, then the maps of all active models rendered from the current camera:

  one colour output (640x480) | three colour outputs from one rasterisation | one colour output at 1280x960

Device-event times (median of --reps) are printed as one JSON line.  The renders run on the downloaded maps uploaded into a context of
their own (same kernels, same surfels and poses as the facade's models).  For kernel times, run the script under
`rocprofv3 --kernel-trace --stats`: the frame loop's own splat_raster_kernel / splat_resolve_kernel are in the same trace
(--frames-played in the line says how many frames they ran for)."""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preroll", type=int, default=24 * 4 + 30, help="frames with ground-truth masks (bench.py's objects4 pre-roll)")
    ap.add_argument("--frames", type=int, default=10, help="frames after the pre-roll")
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    warnings.filterwarnings("ignore", category=RuntimeWarning)
    import numpy as np
    import torch
    import bench
    from co_fusion_amd import api, facade, model as M, render as R

    W, H = 640, 480
    cam, frames = bench.make_stream(W, H, 16, n_obj=4)
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, enable_multiple_models=1)
    played = 0
    for i in range(a.preroll + a.frames):
        f = frames[bench.frame_index(i, 16)]
        cf.process_frame(f["depth"], f["rgb"], mask=(f["label"] * 40).astype(np.uint8), timestamp=i)
        played += 1
    torch.cuda.synchronize()
    n = cf.num_models
    infos = [cf.model_info(i) for i in range(n)]
    maps = [cf.model_download(i) for i in range(n)]

    ctx = api.Context(W, H, cam.fx, cam.fy, cam.cx, cam.cy)
    rnd = R.Renderer(ctx, 2 * W, 2 * H)
    models, items = [], []
    glob_pose = infos[0]["pose"]
    for i, (info, S) in enumerate(zip(infos, maps)):
        m = M.Model(ctx, max(len(S), 1))
        m.upload_map(S)
        models.append(m)
        ptr, _ = m.tensor(11)
        Tp = np.eye(4, dtype=np.float32) if i == 0 else (glob_pose.astype(np.float64) @ np.linalg.inv(info["pose"].astype(np.float64)))
        items.append(R.make_item(ptr, len(S), Tp, info["conf_threshold"], info["id"], R.COLOUR if i == 0 else R.LABEL))
    v1 = R.make_view(glob_pose, cam.fx, cam.fy, cam.cx, cam.cy, W, H, tick=cf.tick)
    v2 = R.make_view(glob_pose, 2 * cam.fx, 2 * cam.fy, 2 * cam.cx, 2 * cam.cy, 2 * W, 2 * H, tick=cf.tick)

    def timed(view, modes):
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rnd.render(view, items, modes)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(ts))

    timed(v1, (R.ITEM_MODE,))   # warm-up
    line = dict(metric="render_us", workload="objects4", models=n, surfels=int(sum(len(S) for S in maps)), frames_played=played,
                reps=a.reps, one_output_640x480=timed(v1, (R.ITEM_MODE,)),
                three_outputs_640x480=timed(v1, (R.ITEM_MODE, R.NORMALS, R.COLOUR)), one_output_1280x960=timed(v2, (R.ITEM_MODE,)))
    print(json.dumps(line), flush=True)
    for m in models:
        m.close()
    rnd.close(); ctx.close(); cf.close()


if __name__ == "__main__":
    main()
