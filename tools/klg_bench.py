#!/usr/bin/env python3
"""Benchmark of the .klg log player (klg.KlgPlayer: host/KlgPlayer.cpp + csrc/frame_decode.hip) beside today's serial reader, one JSON
line.  Writes the log of bench.py's `klg_input` leg -- the configs[2] synthetic stream, 60 frames, quality-90 4:2:0 JPEG colour, zlib
level 6 depth -- and plays it from frame 0 through the same CoFusion configuration three ways in ONE process:

  reader    klg.KlgReader + process_frame: the serial path (what `klg_input` of bench.py measures)
  ceiling   the same frames decoded beforehand and resident on the device, through process_frame_device
  player_N  klg.KlgPlayer with N = 1, 2, 4, 8 workers

Every leg is timed whole (for the player that includes opening it: index walk, pinned slots, threads, and the first frame's decode,
which nothing can hide) and from its 11th frame on (`steady`).  The legs are alternated (reader, ceiling, players; --repeats rounds), so the spread between the repeated legs is in the line
beside their medians.  Also: the decode-only rates (reader; prefetcher alone per worker count) and the two kernels' durations from
device events.  Needs Pillow for the JPEG encoder.

    python tools/klg_bench.py [--frames 60] [--repeats 3] [--workers 1,2,4,8]
"""
import argparse
import io
import json
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_log(path, frames, n, bench):
    from PIL import Image
    nbytes = 4
    with open(path, "wb") as f:
        f.write(struct.pack("<i", n))
        for t in range(n):
            fr = frames[bench.frame_index(t, len(frames))]
            mm = np.rint(fr["depth"] * np.float32(1000.0)).astype(np.uint16)
            zd = zlib.compress(mm.tobytes(), 6)
            buf = io.BytesIO()
            Image.fromarray(fr["rgb"]).save(buf, format="JPEG", quality=90, subsampling=2)
            jb = buf.getvalue()
            f.write(struct.pack("<qii", t * 33333, len(zd), len(jb))); f.write(zd); f.write(jb)
            nbytes += 16 + len(zd) + len(jb)
    return nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workers", default="1,2,4,8")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("klg_bench.py needs a GPU")
    import bench
    from co_fusion_amd import facade, klg
    wl = bench.WORKLOADS["objects4"]
    W, H = wl["size"]
    F = a.frames
    SKIP = 10   # frames left out of the `steady` figure
    assert F > 2 * SKIP
    workers = [int(w) for w in a.workers.split(",")]
    cam, frames = bench.make_stream(W, H, 16, n_obj=wl["n_obj"], seed=1234)
    path = os.path.join(tempfile.gettempdir(), f"klg_bench_{os.getpid()}.klg")
    nbytes = write_log(path, frames, F, bench)
    dev = torch.device("cuda", 0)
    res = dict(tool="klg_bench", size=[W, H], frames=F, repeats=a.repeats, log_bytes_per_frame=int(nbytes / F),
               log="configs[2] synthetic stream, zlib(uint16 mm) level 6 + JPEG quality 90 4:2:0 (the log of bench.py's klg_input leg)")
    try:
        # ---- decode only ----
        def timed(fn):
            t0 = time.perf_counter(); fn(); return 1e3 * (time.perf_counter() - t0) / F
        dec = dict(reader_ms_per_frame=round(min(timed(lambda: [None for _ in klg.KlgReader(path, W, H)]) for _ in range(2)), 4))
        for w in workers:
            def run():
                p = klg.KlgPrefetcher(path, W, H, workers=w, slots=min(16, w + 3))
                while p.lib.cofusion_klg_prefetch_next(p.h, None, None, None) == 0:   # (no copies out of the slots)
                    pass
                p.close()
            dec[f"prefetch_{w}_ms_per_frame"] = round(min(timed(run) for _ in range(2)), 4)
        res["decode_only"] = dec

        # ---- the frames of the ceiling leg: decoded once, resident ----
        resident = []
        for ts, depth, rgb in klg.KlgReader(path, W, H):
            rgba = np.full((H, W, 4), 255, np.uint8); rgba[..., :3] = rgb
            resident.append((ts, torch.from_numpy(depth).to(dev), torch.from_numpy(rgba).to(dev)))
        torch.cuda.synchronize()

        def make(**kw):
            return facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, max_surfels=1 << 21, enable_multiple_models=1, **kw)

        def leg_reader():
            g = make()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k, (ts, depth, rgb) in enumerate(klg.KlgReader(path, W, H)):
                g.process_frame(depth, rgb, timestamp=ts)
                if k == SKIP - 1:
                    t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            n = g.num_models; g.close()
            return F / (t2 - t0), (F - SKIP) / (t2 - t1), n

        def leg_ceiling():
            g = make(device_frames_complete=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k, (ts, d, c) in enumerate(resident):
                g.process_frame_device(d, c, timestamp=ts)
                if k == SKIP - 1:
                    t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            n = g.num_models; g.close()
            return F / (t2 - t0), (F - SKIP) / (t2 - t1), n

        def leg_player(w):
            g = make(device_frames_complete=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = klg.KlgPlayer(g, path, workers=w)   # (opening it -- index walk, pinned slots, threads -- is part of playing a log)
            played = p.play(SKIP)
            t1 = time.perf_counter()
            played += p.play()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert played == F
            p.close()
            n = g.num_models; g.close()
            return F / (t2 - t0), (F - SKIP) / (t2 - t1), n

        legs = [("reader", leg_reader), ("ceiling", leg_ceiling)] + [(f"player_{w}", (lambda w=w: leg_player(w))) for w in workers]
        for _, fn in legs[:2]:
            fn()   # warm-up: code objects loaded, allocator primed
        runs = {name: [] for name, _ in legs}
        steady = {name: [] for name, _ in legs}
        models = {}
        for _ in range(a.repeats):   # alternated: reader, ceiling, players, reader, ...
            for name, fn in legs:
                fps, fps_steady, n = fn()
                runs[name].append(round(fps, 2)); steady[name].append(round(fps_steady, 2)); models[name] = n
        res["frames_per_s"] = {name: dict(median=round(float(np.median(v)), 2), runs=v, spread=round(max(v) - min(v), 2),
                                          steady_median=round(float(np.median(steady[name])), 2), steady_runs=steady[name]) for name, v in runs.items()}
        res["active_models_at_end"] = models
        med = {k: v["median"] for k, v in res["frames_per_s"].items()}
        res["player_over_reader"] = {k: round(med[k] / med["reader"], 3) for k in med if k.startswith("player")}
        res["player_over_ceiling"] = {k: round(med[k] / med["ceiling"], 3) for k in med if k.startswith("player")}
        sm = {k: v["steady_median"] for k, v in res["frames_per_s"].items()}
        res["player_over_ceiling_steady"] = {k: round(sm[k] / sm["ceiling"], 3) for k in sm if k.startswith("player")}

        # ---- the two kernels, by device events around every launch of one pass over the log ----
        from co_fusion_amd import api
        ctx = api.Context(W, H, cam.fx, cam.fy, cam.cx, cam.cy, max_models=1, max_surfels=1024)
        fd = api.FrameDecoder(ctx, W, H, slots=2)
        fd.timing(True)
        t_copy = []
        for k, (ts, mm, kind, colour) in enumerate(klg.KlgPrefetcher(path, W, H, workers=4)):
            fd.fill(k & 1, W, H, mm, kind, colour)
            t0 = time.perf_counter()
            fd.submit(k & 1, W, H, kind)
            fd.acquire(k & 1, complete=True)
            t_copy.append(1e3 * (time.perf_counter() - t0))
        idct_ms, finish_ms, n = fd.timing(False)
        res["kernels"] = dict(jpeg_idct_us=round(1e3 * idct_ms / n, 2), jpeg_finish_us=round(1e3 * finish_ms / n, 2), frames=int(n),
                              submit_to_complete_ms_median=round(float(np.median(t_copy)), 4),
                              note="submit_to_complete: copies (depth 0.6 MB + header and coefficients ~0.9 MB) + both kernels + the event pairs, host clock")
        fd.close(); ctx.close()
    finally:
        os.remove(path)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
