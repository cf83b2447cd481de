#!/usr/bin/env python3
"""Benchmark of the image player (images.ImageSequencePlayer: host/ImagePlayer.cpp + csrc/image_decode.hip) beside the serial reader,
one JSON line.  Writes bench.py's `klg_input` stream -- the configs[2] synthetic stream, 60 frames at 640x480 -- as a directory of PNG
colour (filter type 4, "Paeth", on every row, zlib level 6) and ZIP-compressed OpenEXR depth (one f32 channel), and plays it from
frame 0 through the same CoFusion configuration three ways in ONE process:

  reader    images.ImageSequenceReader + process_frame: everything on the calling thread
  ceiling   the same frames decoded beforehand and resident on the device, through process_frame_device
  player_N  images.ImageSequencePlayer with N = 1, 2, 4, 8 workers

Every leg is timed whole (for the player that includes opening it) and from its 11th frame on (`steady`).  The legs are alternated
(--repeats rounds), so the spread between the repeated legs is in the line beside their medians: the player counts as faster than the
reader only where the gap exceeds the reader's own spread.  Also: the decode-only rate, the workers' time per frame split into
read / inflate (zlib's inflate() alone) / unfilter / parse (cofusion_image_player_times) -- the number that says whether PNG
unfiltering is worth moving to the device --, and the two kernels' durations per frame from device events
(cf_frame_decoder_image_timing) over one pass of the set.

    python tools/image_bench.py [--frames 60] [--repeats 3] [--workers 1,2,4,8]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workers", default="1,2,4,8")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("image_bench.py needs a GPU")
    import bench
    from co_fusion_amd import facade, images
    wl = bench.WORKLOADS["objects4"]
    W, H = wl["size"]
    F = a.frames
    SKIP = 10   # frames left out of the `steady` figure
    assert F > 2 * SKIP
    workers = [int(w) for w in a.workers.split(",")]
    cam, frames = bench.make_stream(W, H, 16, n_obj=wl["n_obj"], seed=1234)
    d = tempfile.mkdtemp(prefix="image_bench_")
    nbytes = 0
    for t in range(F):
        fr = frames[bench.frame_index(t, len(frames))]
        images.write_png(os.path.join(d, f"Color{t:04d}.png"), np.ascontiguousarray(fr["rgb"], np.uint8), filters=(4,))
        images.write_exr(os.path.join(d, f"Depth{t:04d}.exr"), {"Z": np.nan_to_num(np.ascontiguousarray(fr["depth"], np.float32))}, compression=images.EXR_ZIP)
        nbytes += os.path.getsize(os.path.join(d, f"Color{t:04d}.png")) + os.path.getsize(os.path.join(d, f"Depth{t:04d}.exr"))
    dev = torch.device("cuda", 0)
    res = dict(tool="image_bench", size=[W, H], frames=F, repeats=a.repeats, bytes_per_frame=int(nbytes / F),
               set="configs[2] synthetic stream as Color####.png (RGB, Paeth rows, zlib 6) + Depth####.exr (ZIP, one FLOAT channel)")
    try:
        def timed(fn):
            t0 = time.perf_counter(); fn(); return 1e3 * (time.perf_counter() - t0) / F
        dec = dict(reader_ms_per_frame=round(min(timed(lambda: [None for _ in images.ImageSequenceReader(d)]) for _ in range(2)), 4))
        res["decode_only"] = dec

        resident = []
        for ts, depth, rgb, _ in images.ImageSequenceReader(d):
            rgba = np.full((H, W, 4), 255, np.uint8); rgba[..., :3] = rgb
            resident.append((ts, torch.from_numpy(depth).to(dev), torch.from_numpy(rgba).to(dev)))
        torch.cuda.synchronize()

        def make(**kw):
            return facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, max_surfels=1 << 21, enable_multiple_models=1, **kw)

        def leg_reader():
            g = make()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k, (ts, depth, rgb, _) in enumerate(images.ImageSequenceReader(d)):
                g.process_frame(depth, rgb, timestamp=ts)
                if k == SKIP - 1:
                    t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            n = g.num_models; g.close()
            return F / (t2 - t0), (F - SKIP) / (t2 - t1), n, None

        def leg_ceiling():
            g = make(device_frames_complete=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k, (ts, dd, c) in enumerate(resident):
                g.process_frame_device(dd, c, timestamp=ts)
                if k == SKIP - 1:
                    t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            n = g.num_models; g.close()
            return F / (t2 - t0), (F - SKIP) / (t2 - t1), n, None

        def leg_player(w):
            g = make(device_frames_complete=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = images.ImageSequencePlayer(g, d, workers=w)   # (opening it -- directory scan, pinned slots, threads -- is part of playing)
            played = p.play(SKIP)
            t1 = time.perf_counter()
            played += p.play()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert played == F
            split = p.times()
            p.close()
            n = g.num_models; g.close()
            return F / (t2 - t0), (F - SKIP) / (t2 - t1), n, split

        legs = [("reader", leg_reader), ("ceiling", leg_ceiling)] + [(f"player_{w}", (lambda w=w: leg_player(w))) for w in workers]
        for _, fn in legs[:2]:
            fn()   # warm-up: code objects loaded, allocator primed
        runs = {name: [] for name, _ in legs}
        steady = {name: [] for name, _ in legs}
        models, splits = {}, {}
        for _ in range(a.repeats):   # alternated: reader, ceiling, players, reader, ...
            for name, fn in legs:
                fps, fps_steady, n, split = fn()
                runs[name].append(round(fps, 2)); steady[name].append(round(fps_steady, 2)); models[name] = n
                if split:
                    splits.setdefault(name, []).append(split)
        res["frames_per_s"] = {name: dict(median=round(float(np.median(v)), 2), runs=v, spread=round(max(v) - min(v), 2),
                                          steady_median=round(float(np.median(steady[name])), 2), steady_runs=steady[name]) for name, v in runs.items()}
        res["active_models_at_end"] = models
        med = {k: v["median"] for k, v in res["frames_per_s"].items()}
        res["player_over_reader"] = {k: round(med[k] / med["reader"], 3) for k in med if k.startswith("player")}
        res["player_over_ceiling"] = {k: round(med[k] / med["ceiling"], 3) for k in med if k.startswith("player")}
        res["player_minus_reader_over_reader_spread"] = {k: round((med[k] - med["reader"]) / max(res["frames_per_s"]["reader"]["spread"], 1e-9), 1)
                                                         for k in med if k.startswith("player")}
        # the workers' time per frame (all workers summed, so it does not shrink with their number), median over the repeats
        res["worker_ms_per_frame"] = {name: {k: round(1e3 * float(np.median([s[k] for s in v])) / F, 4) for k in ("read", "inflate", "unfilter", "parse")}
                                      for name, v in splits.items()}

        # ---- the two kernels, by device events around every launch of one pass over the set ----
        from co_fusion_amd import api
        ctx = api.Context(W, H, cam.fx, cam.fy, cam.cx, cam.cy, max_models=1, max_surfels=1024)
        fd = api.FrameDecoder(ctx, W, H, slots=2)
        fd.enable_images()
        fd.timing(True)
        t_submit = []
        for t in range(F):
            planes = [(ext, open(os.path.join(d, f"{pre}{t:04d}{ext}"), "rb").read()) for pre, ext in (("Color", ".png"), ("Depth", ".exr"))]
            t0 = time.perf_counter()
            desc = fd.submit_image_files(t & 1, planes[0], planes[1])
            fd.acquire(t & 1, complete=True)
            t_submit.append(1e3 * (time.perf_counter() - t0))
        exr_ms, exr_n, fin_ms, fin_n = fd.image_timing()
        fd.timing(False)
        res["kernels"] = dict(exr_depth_us=round(1e3 * exr_ms / exr_n, 2), png_finish_us=round(1e3 * fin_ms / fin_n, 2), frames=int(exr_n),
                              exr_blocks=int(desc.exr_blocks), exr_bytes=int(desc.exr_line_bytes) * H, png_scanline_bytes=(1 + 3 * W) * H,
                              decode_submit_complete_ms_median=round(float(np.median(t_submit)), 4),
                              note="decode_submit_complete: host parsers on the calling thread + copies + both kernels + the event pairs, host clock")
        fd.close(); ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
