#!/usr/bin/env python
"""Time the mesh export (csrc/mesh.hip).  One JSON line, also saved as profiles/mesh_bench.json:

  stages     per-stage device-event times (cf_mesh_timing, median of --reps) for a sphere of 10^5 and of 10^6 surfels seen from outside,
             each at the default voxel (the mean confident radius, grown until the grid fits max_voxels) and at twice that; grid size,
             vertex and triangle counts; the accumulation's (surfel, sample) pairs -- recounted with torch from the same rule, 5 integer
             atomics of 8 bytes each -- over its time: the achieved atomic bytes per second; the extraction's bytes per second against
             the grid's footprint (64 bytes per sample: every array of the mesher is touched at least once)
  atomics    tools/microbench/atomic_u64_rate (when it has been built): the chip-wide rate of no-return 64-bit integer atomic adds next
             to f32 atomic adds from the same program, and the float figure MI355X_MICROARCH.md quotes (1.3 TB/s of added bytes)
  save_mesh  wall time of a whole save_mesh on a fused objects4 run (bench.py's stream, ground-truth masks): first call (creates the
             mesher) and a second one
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GUIDE_FLOAT_ATOMIC_TBPS = 1.3


def sphere(n, R=1.0, centre=(0.0, 0.0, 2.0), seed=3):
    import numpy as np
    rng = np.random.default_rng(seed)
    k = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * k / n)
    th = np.pi * (1 + 5 ** 0.5) * k
    d = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    s = np.zeros((n, 12), np.float32)
    s[:, 0:3] = np.asarray(centre) + R * d
    s[:, 3] = rng.uniform(11, 40, n)
    s[:, 4] = rng.integers(0, 1 << 24, n).astype(np.float32)
    s[:, 6] = 1; s[:, 7] = 2
    s[:, 8:11] = -d                      # stored normals point away from the observer
    s[:, 11] = 2.0 * R / np.sqrt(n)      # discs that tile the sphere
    return s


def count_pairs(S, grid, thr, trunc=3.0, support=4.0, cap=100.0, chunk=2048):
    """(surfel, sample) pairs the accumulation adds, recounted with torch from the support rule (a count: last-bit differences of the
    arithmetic move a pair in or out at the rim only)"""
    import torch
    v = float(grid.voxel)
    o = torch.tensor(list(grid.origin), device=S.device)
    dims = torch.tensor(list(grid.dims), device=S.device)
    tau = trunc * v
    total = 0
    rho_all = S[:, 11].clamp(1.5 * v, support * v)
    B = int(torch.ceil(2 * (tau + rho_all.max()) / v).item()) + 2
    r = torch.arange(B, device=S.device)
    off = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), dim=-1).reshape(-1, 3)
    for a in range(0, len(S), chunk):
        s = S[a:a + chunk]
        p, n, rho = s[:, 0:3], -s[:, 8:11], rho_all[a:a + chunk]
        lo = torch.floor((p - (tau + rho)[:, None] - o) / v).clamp(min=0).long()
        idx = lo[:, None, :] + off[None]
        inside = (idx < dims).all(dim=-1)
        e = o + idx.float() * v - p[:, None, :]
        d = (n[:, None, :] * e).sum(-1)
        t2 = ((e * e).sum(-1) - d * d).clamp(min=0)
        w = s[:, 3].clamp(max=cap)[:, None] * (1 - t2 / (rho * rho)[:, None])
        ok = inside & (d.abs() <= tau) & (t2 <= (rho * rho)[:, None]) & (s[:, 3] > thr)[:, None] & (torch.round(w * 4096) > 0)
        total += int(ok.sum().item())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--max-voxels", type=int, default=1 << 24)
    ap.add_argument("--preroll", type=int, default=24 * 4 + 30, help="objects4 frames with ground-truth masks before save_mesh (0: skip that leg)")
    ap.add_argument("--atomic-bench", default=os.path.join(ROOT, "tools", "microbench", "atomic_u64_rate"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    a = ap.parse_args()
    warnings.filterwarnings("ignore", category=RuntimeWarning)
    import numpy as np
    import torch
    from co_fusion_amd import api, facade, mesh, model

    thr = 10.0
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = api.Context(64, 48, 60.0, 60.0, 32.0, 24.0, max_models=2, max_surfels=max(sizes))
    ms = mesh.Mesher(ctx, a.max_voxels)
    stages = []
    for n in sizes:
        host = sphere(n)
        S = ctx.to_device(host)
        m = model.Model(ctx, n)
        m.upload_map(host)
        g0 = ms.default_grid(m, thr, 0.0)
        for mult in (1.0, 2.0):
            grid = g0 if mult == 1.0 else ms.default_grid(m, thr, g0.voxel * mult)
            acc_ms, ext_ms = [], []
            for _ in range(a.reps + 1):     # (the first one warms up)
                ms.accumulate(grid, thr, surfels=S)
                nv, nt = ms.extract(1.0)
                t = ms.timing()
                acc_ms.append(t[0]); ext_ms.append(t[1])
            acc, ext = float(np.median(acc_ms[1:])), float(np.median(ext_ms[1:]))
            pairs = count_pairs(S, grid, thr)
            stages.append(dict(surfels=n, voxel=float(grid.voxel), grid=list(grid.dims), samples=grid.samples, vertices=nv, triangles=nt,
                               accumulate_ms=acc, extract_ms=ext, pairs=pairs, atomic_bytes=pairs * 40,
                               accumulate_atomic_GBps=pairs * 40 / (acc * 1e-3) / 1e9,
                               extract_grid_footprint_GBps=grid.samples * 64 / (ext * 1e-3) / 1e9))
        m.close()
        del S
    ms.close(); ctx.close()

    atomics = dict(guide_float_atomic_TBps=GUIDE_FLOAT_ATOMIC_TBPS,
                   remark="the guide's figure is for float atomics; the 64-bit integer rate had not been measured before")
    if os.path.exists(a.atomic_bench):
        out = subprocess.run([a.atomic_bench], capture_output=True, text=True, timeout=300)
        try:
            atomics["measured"] = json.loads(out.stdout.strip().splitlines()[-1])
        except Exception:
            atomics["measured"] = "failed: " + (out.stdout + out.stderr)[-300:]
    else:
        atomics["measured"] = "not measured (tools/microbench/atomic_u64_rate is not built)"

    save = None
    if a.preroll > 0:
        import bench
        W, H = 640, 480
        cam, frames = bench.make_stream(W, H, 16, n_obj=4)
        cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, enable_multiple_models=1)
        for i in range(a.preroll):
            f = frames[bench.frame_index(i, 16)]
            cf.process_frame(f["depth"], f["rgb"], mask=(f["label"] * 40).astype(np.uint8), timestamp=i)
        torch.cuda.synchronize()
        cf.set_mesh_max_voxels(a.max_voxels)
        with tempfile.TemporaryDirectory() as d:
            walls = []
            for _ in range(2):
                t0 = time.perf_counter()
                files = cf.save_mesh(d + os.sep)
                walls.append((time.perf_counter() - t0) * 1e3)
            sizes = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        counts = [tuple(len(x) for x in cf.model_mesh(i)) for i in range(cf.num_models)]
        save = dict(workload="objects4", frames_played=a.preroll, models=cf.num_models, files=files, surfels=[cf.model_info(i)["count"] for i in range(cf.num_models)],
                    vertices=[c[0] for c in counts], triangles=[c[1] for c in counts], file_bytes=sizes, first_call_ms=walls[0], second_call_ms=walls[1])
        cf.close()

    line = dict(metric="mesh_export", reps=a.reps, max_voxels=a.max_voxels, stages=stages, atomics=atomics, save_mesh=save)
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
