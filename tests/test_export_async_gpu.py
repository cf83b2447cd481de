"""GPU tests of the asynchronous per-frame exports (CoFusion::setExportAsync: device PNG encoder + writer threads)
against the synchronous exports: the same file names, every file decodes to the same pixels, and the frame loop -- poses, model lists,
surfels -- is what it is without them.  Back-pressure (two slots, one writer) loses nothing; a prefix that cannot be written raises
from the frame loop or the flush and leaves the instance destroyable; tools/run_klg.py --export-async writes what the synchronous
flags write."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import png_encode_ref as ref
from co_fusion_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 160, 128
FRAMES = 8
ROWS_PER_BAND = 2   # ExportWriter::kDefaultRowsPerBand
KW = dict(max_surfels=1 << 18, conf_global_init=0.5, model_spawn_offset=2, enable_multiple_models=1)


def _pixels(path):
    data = open(path, "rb").read()
    try:
        from PIL import Image
    except ImportError:
        return ref.decode(data)
    return np.asarray(Image.open(io.BytesIO(data)))


def _state(cf):
    out = []
    for i in range(cf.num_models):
        info = cf.model_info(i)
        out.append((info["id"], info["count"], info["pose"].tobytes(), cf.model_download(i).tobytes()))
    return out


def _instance(cam, out, **async_kw):
    from co_fusion_amd import facade
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, **KW)
    cf.set_export_views(out, labels=True, normals=True, viewport=True)
    cf.set_export_segmentation(out)
    if async_kw:
        cf.set_export_async(True, **async_kw)
    return cf


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    cam = synth.Camera.scaled(W, H)
    sc = synth.Scene(n_obj=2)
    dirs = {k: str(tmp_path_factory.mktemp(k)) + "/" for k in ("sync", "async", "tight")}
    inst = dict(sync=_instance(cam, dirs["sync"]), **{"async": _instance(cam, dirs["async"], workers=2, slots=8)},
                tight=_instance(cam, dirs["tight"], workers=1, slots=2))
    diffs, max_models = [], 0
    for t in range(FRAMES):
        d, rgb, lab, _ = sc.render(cam, t, noise=True)
        gt = (lab * 40).astype(np.uint8)
        for cf in inst.values():
            cf.process_frame(d, rgb, mask=gt, timestamp=t)
        want = _state(inst["sync"])
        for k in ("async", "tight"):
            if _state(inst[k]) != want or inst[k].mask().tobytes() != inst["sync"].mask().tobytes():
                diffs.append(f"frame {t}: {k} differs from the synchronous run")
        max_models = max(max_models, inst["sync"].num_models)
    inst["async"].export_flush()
    inst["tight"].export_flush()
    listed = {k: sorted(os.listdir(v)) for k, v in dirs.items()}   # (before anything is closed: flush alone has finished the files)
    stats = {k: inst[k].export_stats() for k in ("async", "tight")}
    yield dict(dirs=dirs, listed=listed, stats=stats, diffs=diffs, max_models=max_models)
    for cf in inst.values():
        cf.close()


def test_exporting_does_not_perturb_the_frame_loop(runs):
    assert runs["max_models"] >= 2, "no object model was spawned"
    assert not runs["diffs"], runs["diffs"]


def test_same_file_names_after_flush(runs):
    names = runs["listed"]["sync"]
    for kind in ("Labels", "Normals", "Viewport"):
        assert sum(n.startswith(kind) for n in names) == FRAMES, names
    assert sum(n.startswith("Segmentation") for n in names) >= FRAMES - 1, names
    assert runs["listed"]["async"] == names and runs["listed"]["tight"] == names


@pytest.mark.parametrize("which", ["async", "tight"])
def test_every_file_decodes_to_the_synchronous_pixels(runs, which):
    for name in runs["listed"]["sync"]:
        want = _pixels(runs["dirs"]["sync"] + name)
        got = _pixels(runs["dirs"][which] + name)
        assert got.shape == want.shape == ((H, W) if name.startswith("Segmentation") else (H, W, 4)), name
        assert np.array_equal(got, want), name
    # ... and they are this encoder's files: the reference's statement of the format gives the same bytes
    name = runs["listed"]["sync"][-1]
    px = _pixels(runs["dirs"]["sync"] + name)
    assert open(runs["dirs"][which] + name, "rb").read() == ref.encode(px, 4 if px.ndim == 3 else 1, ROWS_PER_BAND, 0)[0]


def test_back_pressure_stalls_and_loses_nothing(runs):
    n = len(runs["listed"]["sync"])
    for k in ("async", "tight"):
        s = runs["stats"][k]
        assert s["images"] == n and s["bytes"] == sum(os.path.getsize(runs["dirs"][k] + f) for f in runs["listed"][k]), (k, s)
    assert runs["stats"]["tight"]["stalls"] > 0, runs["stats"]["tight"]


def test_a_prefix_that_cannot_be_written_raises_and_nothing_crashes(tmp_path):
    from co_fusion_amd import facade
    cam = synth.Camera.scaled(W, H)
    sc = synth.Scene(n_obj=2)
    cf = facade.CoFusion(W, H, cam.fx, cam.fy, cam.cx, cam.cy, **KW)
    cf.set_export_views(str(tmp_path / "no_such_directory") + "/", labels=True)
    cf.set_export_async(True, workers=1, slots=2)
    with pytest.raises(facade.CoFusionError, match="no_such_directory"):
        for t in range(3):
            d, rgb, lab, _ = sc.render(cam, t, noise=True)
            cf.process_frame(d, rgb, timestamp=t)
        cf.export_flush()
    with pytest.raises(facade.CoFusionError):
        cf.set_export_async(True, workers=9)
    with pytest.raises(facade.CoFusionError):
        cf.set_export_async(True, slots=1)
    # the instance goes on: a writable prefix from here on, and a clean end
    good = str(tmp_path) + "/"
    try:
        cf.export_flush()
    except facade.CoFusionError:
        pass   # (a file of the frames above that failed after the first report)
    cf.set_export_views(good, labels=True)
    cf.set_export_async(True, workers=1, slots=2)
    d, rgb, lab, _ = sc.render(cam, 3, noise=True)
    cf.process_frame(d, rgb, timestamp=3)
    cf.export_flush()
    assert [f for f in os.listdir(good) if f.startswith("Labels")], os.listdir(good)
    cf.close()


def test_run_klg_export_async_writes_what_the_synchronous_flags_write(tmp_path):
    from co_fusion_amd import klg
    cam = synth.Camera.scaled(W, H)
    sc = synth.Scene(n_obj=2)
    log = tmp_path / "seq.klg"
    with klg.KlgWriter(log, W, H) as wr:
        for t in range(6):
            d, rgb, lab, _ = sc.render(cam, t, noise=True)
            wr.write(33333 * t, d, rgb)
    outs = []
    for extra in ([], ["--export-async", "--export-workers", "1"]):
        out = tmp_path / ("async" if extra else "sync"); out.mkdir()
        cmd = [sys.executable, os.path.join(ROOT, "tools", "run_klg.py"), str(log), str(out), "--width", str(W), "--height", str(H),
               "--fx", str(cam.fx), "--fy", str(cam.fy), "--cx", str(cam.cx), "--cy", str(cam.cy), "--max-surfels", str(1 << 18),
               "--export-segmentation", "--export-labels"] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "6 frames of 6" in r.stdout and (not extra or "asynchronous exports:" in r.stdout), r.stdout
        outs.append({f: _pixels(out / f) for f in sorted(os.listdir(out)) if f.endswith(".png")})
    assert sum(f.startswith("Labels") for f in outs[0]) == 6 and any(f.startswith("Segmentation") for f in outs[0]), sorted(outs[0])
    assert sorted(outs[0]) == sorted(outs[1])
    for f in outs[0]:
        assert np.array_equal(outs[0][f], outs[1][f]), f
