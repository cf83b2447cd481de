#!/usr/bin/env python3
"""What the per-frame exports cost, on the stream of bench.py's objects4 workload (640x480, 4 objects, device-resident frames, motion
segmentation) after its pre-roll.  Legs:

  none      no export: the ceiling
  sync      the synchronous exports (read-back, zlib and fwrite on the frame thread)
  async1 / async2 / async4   CoFusion::setExportAsync with 1 / 2 / 4 writer threads (device PNG encoder)

each for `seg` (Segmentation<n>.png alone) and `all` (plus Labels / Normals / Viewport).  Every leg has an instance of its own; the
legs are ALTERNATED --rounds times in one process, --steps timed frames each after --warmup untimed ones, the asynchronous legs
flushed inside the timed section.  Files go to a temporary directory that is emptied after every section and removed at the end.
One JSON line: per leg frames/s (median, min, max over the rounds), its fraction of the ceiling, bytes per image by kind, stalls, and
the encoding kernel's time per image from device events (a separate short pass with the encoder's timing mode on).
--legs none,sync: only those (an older build of the libraries, loaded with CF_LIB_DIR, has no asynchronous entry).
--r-sweep: instead, the kernel time and file size of one Segmentation, Labels and Viewport image at rows_per_band 2 / 4 / 8 / 16."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KINDS = ("Segmentation", "Labels", "Normals", "Viewport")


class _ContextView:
    """the facade instance's cf_ctx for api.PngEncoder (borrowed: never destroyed here)"""

    def __init__(self, cf, device):
        from co_fusion_amd import api, lib
        self.lib, self.device, self._err = lib.load(), device, api.CofusionError
        self.h = C.c_void_p(cf.lib.cofusion_context(cf.h))

    def _check(self, rc):
        if rc != 0:
            raise self._err(f"cofusion_hip error {rc}: {self.lib.cf_last_error(self.h).decode()}")


def r_sweep(cf, dev, reps):
    import torch
    import png_encode_ref as ref
    from co_fusion_amd import api
    ctx = _ContextView(cf, dev)
    images = dict(Segmentation=(torch.from_numpy(cf.mask()).to(dev), ref.CF_PNG_LABELS),
                  Labels=(cf.render(background_mode=2, object_mode=4, as_torch=True).clone(), 0),
                  Viewport=(cf.render(background_mode=2, object_mode=2, as_torch=True).clone(), 0))
    out = {}
    for R in (2, 4, 8, 16):
        enc = api.PngEncoder(ctx, 640, 480, slots=2, rows_per_band=R)
        row = {}
        for name, (img, flags) in images.items():
            for s in (0, 1):
                enc.submit(s, img, flags)
            enc.timing(True)
            us = []
            for _ in range(3):
                for i in range(reps):
                    enc.submit(i & 1, img, flags)
                ms, n = enc.timing(True)
                us.append(ms * 1e3 / n)
            st, bands = enc.acquire(0)
            row[name] = dict(kernel_us=round(statistics.median(us), 2), kernel_us_min=round(min(us), 2), kernel_us_max=round(max(us), 2),
                             idat_bytes=sum(len(b) for b, _, _ in bands) + 8, stored_bands=sum(len(b) == n + 5 for b, _, n in bands), bands=len(bands))
        enc.close()
        out[str(R)] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="none,sync,async1,async2,async4")
    ap.add_argument("--kinds", default="seg,all")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--preroll", type=int, default=24 * 4 + 30)
    ap.add_argument("--r-sweep", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("export_bench.py needs a GPU: the hot path has no CPU fallback")
    import numpy as np
    import bench
    from co_fusion_amd import facade
    W, H, n_obj = 640, 480, 4
    cam, frames = bench.make_stream(W, H, a.frames, n_obj=n_obj, seed=1234)
    masks = [(f["label"] * 40).astype(np.uint8) for f in frames]
    dev = torch.device("cuda", 0)
    resident = [dict(depth=torch.from_numpy(f["depth"]).to(dev), rgba=torch.from_numpy(f["rgba"]).to(dev)) for f in frames]
    torch.cuda.synchronize()

    def instance():
        cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, enable_multiple_models=1, device_frames_complete=1)
        for i in range(a.preroll):
            k = bench.frame_index(i, a.frames)
            cf.process_frame(frames[k]["depth"], frames[k]["rgb"], mask=masks[k], timestamp=i)
        return cf

    if a.r_sweep:
        cf = instance()
        out = dict(tool="export_bench", mode="r_sweep", size=[W, H], objects=n_obj, reps=50, rows_per_band=r_sweep(cf, dev, 50))
        print(json.dumps(out), flush=True)
        cf.close()
        return

    tmp = tempfile.mkdtemp(prefix="export_bench_")
    legs = [(leg, kind) for kind in a.kinds.split(",") for leg in a.legs.split(",") if leg and kind and not (leg == "none" and kind != a.kinds.split(",")[0])]
    inst, pos, dirs = {}, {}, {}
    try:
        for key in legs:
            leg, kind = key
            cf = instance()
            d = os.path.join(tmp, f"{leg}_{kind}") + "/"
            os.makedirs(d)
            if leg != "none":
                cf.set_export_segmentation(d)
                if kind == "all":
                    cf.set_export_views(d, labels=True, normals=True, viewport=True)
            if leg.startswith("async"):
                cf.set_export_async(True, workers=int(leg[5:]), slots=a.slots)
            inst[key], pos[key], dirs[key] = cf, a.preroll, d

        def run(key, n):
            cf = inst[key]
            for i in range(pos[key], pos[key] + n):
                k = bench.frame_index(i, a.frames)
                cf.process_frame_device(resident[k]["depth"], resident[k]["rgba"], timestamp=i)
            pos[key] += n
            if key[0].startswith("async"):
                cf.export_flush()
            torch.cuda.synchronize()

        def sizes(key, into):
            for f in os.listdir(dirs[key]):
                kind = next(k for k in KINDS if f.startswith(k))
                into.setdefault(kind, []).append(os.path.getsize(dirs[key] + f))
                os.remove(dirs[key] + f)

        fps = {key: [] for key in legs}
        file_bytes = {key: {} for key in legs}
        stalls = {key: 0 for key in legs}
        for _ in range(a.rounds):
            for key in legs:
                run(key, a.warmup)
                sizes(key, {})
                before = inst[key].export_stats()["stalls"] if key[0].startswith("async") else 0
                t0 = time.perf_counter()
                run(key, a.steps)
                fps[key].append(a.steps / (time.perf_counter() - t0))
                if key[0].startswith("async"):
                    stalls[key] += inst[key].export_stats()["stalls"] - before
                sizes(key, file_bytes[key])
        device = {}
        for key in legs:   # the encoder's timing mode, outside the timed sections
            if key[0].startswith("async"):
                inst[key].export_stats(timing=True)
                run(key, 20)
                s = inst[key].export_stats(timing=False)
                device[key] = round(s["device_ms"] * 1e3 / max(1, s["device_images"]), 2)
                sizes(key, {})
        ceiling = statistics.median(fps[legs[0]]) if legs[0][0] == "none" else None
        out = dict(tool="export_bench", size=[W, H], objects=n_obj, steps=a.steps, warmup=a.warmup, rounds=a.rounds, slots=a.slots,
                   lib_dir=os.path.relpath(os.environ.get("CF_LIB_DIR") or os.path.join(ROOT, "co_fusion_amd", "lib"), ROOT), legs={})
        for key in legs:
            v = fps[key]
            e = dict(fps_median=round(statistics.median(v), 2), fps_min=round(min(v), 2), fps_max=round(max(v), 2), rounds=[round(x, 2) for x in v],
                     bytes_per_image={k: int(statistics.mean(b)) for k, b in sorted(file_bytes[key].items())},
                     files_per_round=sum(len(b) for b in file_bytes[key].values()) // a.rounds)
            if ceiling:
                e["fraction_of_ceiling"] = round(statistics.median(v) / ceiling, 4)
            if key[0].startswith("async"):
                e["stalls"] = stalls[key]
                e["encoder_kernel_us_per_image"] = device[key]
            out["legs"][f"{key[0]}/{key[1]}"] = e
        print(json.dumps(out), flush=True)
    finally:
        for cf in inst.values():
            cf.close()
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
