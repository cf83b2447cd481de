#!/usr/bin/env python
"""Run a .klg RGB-D log through the hot path and export the reference's outputs (what `CoFusion -l <log> -exportdir <dir>`
does head-less, GUI/MainController.cpp):

    python tools/run_klg.py seq.klg out/ [--static] [--width 640 --height 480 --fx 528 --fy 528 --cx 320 --cy 240]
                            [--frames N] [--flip-colors] [--export-segmentation]
                            [--export-labels] [--export-normals] [--export-viewport] [--player [--workers N]]
                            [--mask-dir DIR [--mask-prefix Mask --index-width 4]]

Writes out/poses-<id>.txt, out/cloud-<id>.ply (and out/Segmentation<tick>.png, out/Labels<tick>.png, out/Normals<tick>.png,
out/Viewport<tick>.png: the reference's -el / -en / -ev views of every frame) and prints frames/s.  --player reads the log ahead on
worker threads and finishes the frames on the device (klg.KlgPlayer) instead of decoding each frame in front of its processing: the
same frames, the same outputs.  --mask-dir feeds the reference's pre-processed segmentation (one label mask per frame, <prefix><index>.pgm,
binary PGM with maxval <= 255; the numbering starts at 0 or 1, whichever file exists) instead of running the motion segmentation: with the
serial reader through the host entry, with --player through player iteration and the masked device entry (mask uploaded, frame on the
device).  A frame without a mask file runs the motion segmentation."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log"); ap.add_argument("outdir")
    ap.add_argument("--static", action="store_true", help="single static model (-static)")
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--fx", type=float, default=528.0); ap.add_argument("--fy", type=float, default=528.0)
    ap.add_argument("--cx", type=float, default=320.0); ap.add_argument("--cy", type=float, default=240.0)
    ap.add_argument("--frames", type=int, default=-1)
    ap.add_argument("--flip-colors", action="store_true")
    ap.add_argument("--export-segmentation", action="store_true")
    ap.add_argument("--export-labels", action="store_true", help="Labels<n>.png: background in colour, objects in label colour (-el)")
    ap.add_argument("--export-normals", action="store_true", help="Normals<n>.png (-en)")
    ap.add_argument("--export-viewport", action="store_true", help="Viewport<n>.png: every model in colour (-ev)")
    ap.add_argument("--max-surfels", type=int, default=3072 * 3072)
    ap.add_argument("--relocalise", action="store_true", help="failure detection (-rl) with the fern keyframe database: a lost camera recovers")
    ap.add_argument("--fern-threshold", type=float, default=0.3095, help="a frame becomes a keyframe when it differs more than this from every keyframe")
    ap.add_argument("--photo-threshold", type=float, default=115.0)
    ap.add_argument("--fern-min-age", type=int, default=300, help="ticks a keyframe must be old to be matched")
    ap.add_argument("--fern-seed", type=int, default=0)
    ap.add_argument("--player", action="store_true", help="threaded prefetch + JPEG finished on the device (default: the serial reader)")
    ap.add_argument("--workers", type=int, default=4, help="host threads of --player (1..16)")
    ap.add_argument("--mask-dir", default=None, help="directory of per-frame label masks (binary PGM)")
    ap.add_argument("--mask-prefix", default="Mask")
    ap.add_argument("--index-width", type=int, default=4)
    a = ap.parse_args()
    from co_fusion_amd import facade, klg
    os.makedirs(a.outdir, exist_ok=True)
    prefix = a.outdir.rstrip("/") + "/"
    log = None if a.player else klg.KlgReader(a.log, a.width, a.height, flip_colors=a.flip_colors)
    cf = facade.CoFusion(a.width, a.height, a.fx, a.fy, a.cx, a.cy, max_surfels=a.max_surfels, enable_multiple_models=int(not a.static),
                         enable_pose_logging=1, reloc=int(a.relocalise))
    if a.relocalise:
        cf.set_relocalisation(True, fern_threshold=a.fern_threshold, photo_threshold=a.photo_threshold, min_age=a.fern_min_age, seed=a.fern_seed)
    if a.export_segmentation and not a.static:
        cf.set_export_segmentation(prefix)
    if a.export_labels or a.export_normals or a.export_viewport:
        cf.set_export_views(prefix, labels=a.export_labels, normals=a.export_normals, viewport=a.export_viewport)
    n, t0 = 0, time.perf_counter()
    mask_of = None
    if a.mask_dir:
        from co_fusion_amd import masks
        if a.static:
            raise SystemExit("--mask-dir needs the multi-model mode (no --static)")
        start = 0 if os.path.exists(masks.mask_path(a.mask_dir, 0, a.mask_prefix, a.index_width)) else 1

        def mask_of(i):
            path = masks.mask_path(a.mask_dir, i + start, a.mask_prefix, a.index_width)
            if not os.path.exists(path):
                return None
            m = masks.read_pgm(path)
            if m.shape != (a.height, a.width):
                raise SystemExit(f"{path}: {m.shape[1]}x{m.shape[0]}, the log is {a.width}x{a.height}")
            return m
    if a.player and mask_of:
        import torch
        log = klg.KlgPlayer(cf, a.log, flip_colors=a.flip_colors, workers=a.workers)
        log.set_limits(frame_limit=a.frames if a.frames > 0 else -1)
        for ts, depth_ptr, rgba_ptr in log:
            m = mask_of(n)
            mt = None if m is None else torch.from_numpy(m).cuda()   # (consumed in stream order: device_frames_complete = 0)
            cf.process_frame_device_ptr(depth_ptr, rgba_ptr, None if mt is None else mt.data_ptr(), timestamp=ts)
            n += 1
        log.close()
    elif a.player:
        log = klg.KlgPlayer(cf, a.log, flip_colors=a.flip_colors, workers=a.workers)
        log.set_limits(frame_limit=a.frames if a.frames > 0 else -1)
        n = log.play()
        log.close()
    else:
        for ts, depth, rgb in log:
            cf.process_frame(depth, rgb, mask=mask_of(n) if mask_of else None, timestamp=ts)
            n += 1
            if 0 < a.frames <= n:
                break
    dt = time.perf_counter() - t0
    how = f"log player, {a.workers} workers" if a.player else "incl. log decoding and upload"
    print(f"{n} frames of {log.num_frames} in {dt:.2f} s ({n / dt:.1f} frames/s {how}), {cf.num_models} active models")
    if a.relocalise:
        print(f"relocalisation: {cf.reloc_stats()}, lost at the end: {cf.lost}")
    print(f"exported {cf.export_poses(prefix)} pose file(s), {cf.save_ply(prefix)} PLY cloud(s) to {prefix}")
    cf.close()


if __name__ == "__main__":
    main()
