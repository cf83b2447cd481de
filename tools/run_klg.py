#!/usr/bin/env python
"""Run a .klg RGB-D log through the hot path and export the reference's outputs (what `CoFusion -l <log> -exportdir <dir>`
does head-less, GUI/MainController.cpp):

    python tools/run_klg.py seq.klg out/ [--static] [--width 640 --height 480 --fx 528 --fy 528 --cx 320 --cy 240]
                            [--frames N] [--flip-colors] [--export-segmentation]
                            [--export-labels] [--export-normals] [--export-viewport] [--export-async [--export-workers N]]
                            [--player [--workers N]]
                            [--mask-dir DIR [--mask-prefix Mask --index-width 4]]
                            [--redetect [--redetect-fit F --redetect-cover C --redetect-tol T]] [--redetect-search]

Writes out/poses-<id>.txt, out/cloud-<id>.ply (and out/Segmentation<tick>.png, out/Labels<tick>.png, out/Normals<tick>.png,
out/Viewport<tick>.png: the reference's -el / -en / -ev views of every frame) and prints frames/s.  --export-async encodes those PNGs on
the device and writes them from --export-workers threads (the same names and pixels; flushed before the rate is reported).  --player reads the log ahead on
worker threads and finishes the frames on the device (klg.KlgPlayer) instead of decoding each frame in front of its processing: the
same frames, the same outputs.  --mask-dir feeds the reference's pre-processed segmentation (one label mask per frame, <prefix><index>.pgm,
binary PGM with maxval <= 255; the numbering starts at 0 or 1, whichever file exists) instead of running the motion segmentation: with the
serial reader through the host entry, with --player through player iteration and the masked device entry (mask uploaded, frame on the
device).  A frame without a mask file runs the motion segmentation.  Masks may be .pgm or 8-bit grey .png files.

The positional `log` may also be a DIRECTORY of image files as the reference's `-dir` reads them (co_fusion_amd/images.py:
colour <prefix><index>.jpg/.png/.ppm, depth .exr/.png, masks .png/.pgm):

    python tools/run_klg.py car4/ out/ [--depth-dir DIR --mask-dir DIR] [--color-prefix Color --depth-prefix Depth --mask-prefix Mask]
                            [--index-width 4] [--start-index N] [--depth-scale 0.001]

The frame size is the first colour file's (--width / --height are ignored); the files are read by the serial reader
(images.ImageSequenceReader) and the frames go through the host entry, masks included where the set has them.  With --player worker
threads read, inflate and unfilter ahead and the device finishes the frames (images.ImageSequencePlayer): the same frames, the same
outputs."""
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
    ap.add_argument("--export-async", action="store_true", help="the per-frame PNG exports through the device encoder and writer threads")
    ap.add_argument("--export-workers", type=int, default=2, help="writer threads of --export-async (1..8)")
    ap.add_argument("--export-mesh", action="store_true", help="mesh-<id>.ply per model at the end of the run: a triangle mesh of the confident "
                                                               "surfels, extracted on the device (DESIGN.md 4.15)")
    ap.add_argument("--mesh-voxel", type=float, default=0.0, help="voxel size of --export-mesh in metres (default 0: each model's mean confident "
                                                                  "surfel radius; far below the radius the mesh gets holes)")
    ap.add_argument("--max-surfels", type=int, default=3072 * 3072)
    ap.add_argument("--relocalise", action="store_true", help="failure detection (-rl) with the fern keyframe database: a lost camera recovers")
    ap.add_argument("--fern-threshold", type=float, default=0.3095, help="a frame becomes a keyframe when it differs more than this from every keyframe")
    ap.add_argument("--photo-threshold", type=float, default=115.0)
    ap.add_argument("--fern-min-age", type=int, default=300, help="ticks a keyframe must be old to be matched")
    ap.add_argument("--fern-seed", type=int, default=0)
    ap.add_argument("--close-loops", action="store_true", help="global loop closure: a view that returns with drift corrects the background map "
                                                                "(implies --relocalise)")
    ap.add_argument("--loop-sample-rate", type=int, default=25000, help="every N-th surfel of the background map is a node of the deformation graph")
    ap.add_argument("--close-local-loops", action="store_true", help="local loop closure: the active view of the background map is registered onto "
                                                                      "the inactive one in every frame (a second tracking loop per frame); needs no --relocalise")
    ap.add_argument("--local-sample-rate", type=int, default=5000, help="every N-th surfel is a node of the local deformation graph")
    ap.add_argument("--relative-constraints", action="store_true", help="an accepted local closure leaves pairs behind that every later global "
                                                                         "closure keeps together (with --close-loops and --close-local-loops)")
    ap.add_argument("--time-delta", type=int, default=0, help="ticks after which an unseen surfel is inactive (0: never; ElasticFusion's 200 with "
                                                              "--close-loops)")
    ap.add_argument("--redetect", action="store_true", help="an object that is labelled again resumes its kept inactive model (old id and map) "
                                                            "where that explains the frame, instead of a new model")
    ap.add_argument("--redetect-search", action="store_true", help="implies --redetect: an object that comes back somewhere else is looked for by "
                    "registration -- colour gate, then point-to-plane onto the new label's pixels (DESIGN.md 4.13, Search)")
    ap.add_argument("--redetect-fit", type=float, default=-1.0, help="least agree_on_label / (agree + seen_through) of a candidate (default 0.5)")
    ap.add_argument("--redetect-cover", type=float, default=-1.0, help="least share of the new label's pixels a candidate must explain (default 0.044)")
    ap.add_argument("--redetect-tol", type=float, default=-1.0, help="depth agreement in metres (default 0.10, the tracker's gate)")
    ap.add_argument("--player", action="store_true", help="threaded prefetch + JPEG finished on the device (default: the serial reader)")
    ap.add_argument("--workers", type=int, default=4, help="host threads of --player (1..16)")
    ap.add_argument("--mask-dir", default=None, help="directory of per-frame label masks (binary PGM or 8-bit grey PNG)")
    ap.add_argument("--depth-dir", default=None, help="image directory: where the depth files are (default: the colour directory)")
    ap.add_argument("--color-prefix", default=None, help="image directory: colour files are <prefix><index>.jpg/.png/.ppm")
    ap.add_argument("--depth-prefix", default=None, help="image directory: depth files are <prefix><index>.exr/.png")
    ap.add_argument("--start-index", type=int, default=-1, help="image directory: index of the first frame (default: 0 or 1, whichever exists)")
    ap.add_argument("--depth-scale", type=float, default=0.0,
                    help="image directory, 16-bit PNG depth: metres per unit (default: the reference's 0.0006; 0.001 for millimetre data, "
                         "0.0002 for TUM's 5000 units per metre)")
    ap.add_argument("--mask-prefix", default="Mask")
    ap.add_argument("--index-width", type=int, default=4)
    a = ap.parse_args()
    from co_fusion_amd import facade, klg
    os.makedirs(a.outdir, exist_ok=True)
    prefix = a.outdir.rstrip("/") + "/"
    images_dir = os.path.isdir(a.log)
    if images_dir:
        from co_fusion_amd import images
        # No prefix given: all three go in empty, and the reader applies the reference's rule ("Color" / "Depth" / "Mask" where the
        # directories overlap, every file of its own directory otherwise).  Any prefix given: all three as given (--mask-prefix
        # defaults to "Mask").
        given = a.color_prefix is not None or a.depth_prefix is not None or a.mask_prefix != "Mask"
        prefixes = (a.color_prefix or "", a.depth_prefix or "", a.mask_prefix) if given else ("", "", "")
        where = (a.log, a.depth_dir or "", a.mask_dir or "") + prefixes
        how_read = dict(index_width=a.index_width, start_index=a.start_index, flip_colors=a.flip_colors, depth_scale=a.depth_scale)
        log = images.ImageSequenceReader(*where, **how_read)   # (with --player: the directory rules and the frame size)
        a.width, a.height = log.width, log.height
        if log.has_masks and a.static:
            raise SystemExit("a dataset with masks needs the multi-model mode (no --static)")
    else:
        log = None if a.player else klg.KlgReader(a.log, a.width, a.height, flip_colors=a.flip_colors)
    a.relocalise = a.relocalise or a.close_loops
    time_delta = a.time_delta if a.time_delta > 0 else 200 if a.close_loops or a.close_local_loops else 0
    cf = facade.CoFusion(a.width, a.height, a.fx, a.fy, a.cx, a.cy, max_surfels=a.max_surfels, enable_multiple_models=int(not a.static),
                         enable_pose_logging=1, reloc=int(a.relocalise), time_delta=time_delta)
    if a.relocalise:
        cf.set_relocalisation(True, fern_threshold=a.fern_threshold, photo_threshold=a.photo_threshold, min_age=a.fern_min_age, seed=a.fern_seed)
    if a.close_loops:
        cf.set_loop_closure(True, sample_rate=a.loop_sample_rate)
    if a.close_local_loops:
        cf.set_local_loop_closure(True, sample_rate=a.local_sample_rate)
    if a.relative_constraints:
        cf.set_relative_constraints(True)
    a.redetect = a.redetect or a.redetect_search
    if a.redetect:
        if a.static:
            raise SystemExit("--redetect needs the multi-model mode (no --static)")
        cf.set_redetection(True, min_fit=a.redetect_fit, min_cover=a.redetect_cover, depth_tol=a.redetect_tol)   # (negative: the defaults)
        if a.redetect_search:
            cf.set_redetection_search(True)
    if a.export_segmentation and not a.static:
        cf.set_export_segmentation(prefix)
    if a.export_labels or a.export_normals or a.export_viewport:
        cf.set_export_views(prefix, labels=a.export_labels, normals=a.export_normals, viewport=a.export_viewport)
    if a.export_async:
        cf.set_export_async(True, workers=a.export_workers)
    n, t0 = 0, time.perf_counter()
    mask_of = None
    if a.mask_dir and not images_dir:
        from co_fusion_amd import masks
        if a.static:
            raise SystemExit("--mask-dir needs the multi-model mode (no --static)")
        def find(i):
            pgm = masks.mask_path(a.mask_dir, i, a.mask_prefix, a.index_width)
            return next((p for p in (pgm, pgm[:-4] + ".png") if os.path.exists(p)), None)

        start = 0 if find(0) else 1

        def mask_of(i):
            path = find(i + start)
            if path is None:
                return None
            m = masks.read_mask(path)
            if m.shape != (a.height, a.width):
                raise SystemExit(f"{path}: {m.shape[1]}x{m.shape[0]}, the log is {a.width}x{a.height}")
            return m
    if a.player and images_dir:
        log.close()
        log = images.ImageSequencePlayer(cf, *where, workers=a.workers, **how_read)
        log.set_limits(frame_limit=a.frames if a.frames > 0 else -1)
        n = log.play()
        log.close()
    elif a.player and mask_of:
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
    elif images_dir:
        for ts, depth, rgb, mask in log:
            cf.process_frame(depth, rgb, mask=mask, timestamp=ts)
            n += 1
            if 0 < a.frames <= n:
                break
    else:
        for ts, depth, rgb in log:
            cf.process_frame(depth, rgb, mask=mask_of(n) if mask_of else None, timestamp=ts)
            n += 1
            if 0 < a.frames <= n:
                break
    if a.export_async:
        cf.export_flush()   # the rate below includes every file
    dt = time.perf_counter() - t0
    how = f"{'image' if images_dir else 'log'} player, {a.workers} workers" if a.player else ("incl. file decoding and upload" if images_dir else "incl. log decoding and upload")
    print(f"{n} frames of {log.num_frames} in {dt:.2f} s ({n / dt:.1f} frames/s {how}), {cf.num_models} active models")
    if a.relocalise:
        print(f"relocalisation: {cf.reloc_stats()}, lost at the end: {cf.lost}")
    if a.close_loops:
        print(f"loop closure: {cf.loop_stats()}")
    if a.close_local_loops:
        print(f"local loop closure: {cf.local_loop_stats()}")
    if a.relative_constraints:
        print(f"relative constraints: {cf.relative_stats()}")
    if a.redetect:
        print(f"re-detection: {cf.redetect_stats()}, {cf.num_inactive_models} inactive model(s) kept")
        if a.redetect_search:
            print(f"re-detection search: {cf.redetect_search_last()['attempts']} frame(s) searched")
    if a.export_async:
        s = cf.export_stats()
        print(f"asynchronous exports: {s['images']} files, {s['bytes']} bytes, {s['stalls']} submits waited for a slot")
    print(f"exported {cf.export_poses(prefix)} pose file(s), {cf.save_ply(prefix)} PLY cloud(s) to {prefix}")
    if a.export_mesh:
        print(f"exported {cf.save_mesh(prefix, a.mesh_voxel)} PLY mesh(es) to {prefix}")
    cf.close()


if __name__ == "__main__":
    main()
