"""CPU suite: the host half of the .klg log player -- the JPEG decoder split at the coefficient boundary
(host/Jpeg.cpp: front end + host back end) and the threaded prefetcher (host/KlgPrefetch.cpp).  Every comparison is byte equality
with klg.KlgReader, today's serial reader, and with libjpeg's pixels stored in tests/golden/klg_player."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import klg_player_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def klg():
    import __graft_entry__ as g
    g.build()
    from co_fusion_amd import klg as k
    return k


def _reader_colour(klg, tmp_path, stream, W, H, flip=False):
    """the colour klg.KlgReader delivers for a one-frame log holding this JPEG"""
    p = kc.write_log(tmp_path / "one.klg", [(7, np.zeros((H, W), np.uint16), "raw", stream)])
    r = klg.KlgReader(p, W, H, flip_colors=flip)
    _, _, c = next(iter(r))
    r.close()
    return c


@pytest.mark.parametrize("name", kc.FIXTURES)
def test_front_end_plus_host_back_end_is_the_reader_and_libjpeg(klg, tmp_path, name):
    stream, ref = kc.fixture(name)
    H, W = ref.shape[:2]
    rc, hd, coef = klg.jpeg_front(stream, W, H)
    assert rc == 0
    assert (hd.width, hd.height, hd.ncomp) == (W, H, 1 if name.startswith("grey") else 3)
    mx, my = -(-W // (8 * hd.hmax)), -(-H // (8 * hd.vmax))
    first = 0
    for c in range(hd.ncomp):   # the block grid: mx*h x my*v blocks per component, planar
        cc = hd.comp[c]
        assert (cc.bw, cc.bh, cc.first) == (mx * cc.h, my * cc.v, first)
        first += cc.bw * cc.bh
    assert hd.total_blocks == first == coef.shape[0] <= klg.jpeg_max_blocks(W, H)
    rgb = klg.jpeg_finish_host(hd, coef)
    assert np.array_equal(rgb, ref), "front end + host back end differs from libjpeg"
    assert np.array_equal(_reader_colour(klg, tmp_path, stream, W, H)[..., ::-1], rgb), "differs from the serial reader"
    assert np.array_equal(_reader_colour(klg, tmp_path, stream, W, H, flip=True), rgb)


def test_front_end_refuses_what_the_device_path_does_not_promise(klg, tmp_path):
    stream, ref = kc.fixture("edge_104x72_420")
    H, W = ref.shape[:2]
    wide = kc.wide_quant(stream)
    assert wide != stream
    rc, _, _ = klg.jpeg_front(wide, W, H)
    assert rc == 1, "a 16-bit quantisation table must be refused"
    assert np.array_equal(_reader_colour(klg, tmp_path, wide, W, H)[..., ::-1], ref), "the reader still plays it, to the same pixels"
    over = kc.dc_overflow_stream(64, 48)
    rc, _, _ = klg.jpeg_front(over, 64, 48)
    assert rc == 1, "a DC predictor outside int16 must be refused"
    c = _reader_colour(klg, tmp_path, over, 64, 48)   # ... and the reader plays it: white once the predictor has saturated the IDCT
    assert c.shape == (48, 64, 3) and (c[8:] == 255).all()
    with pytest.raises(klg.KlgError):
        klg.jpeg_front(stream[:200], W, H)


@pytest.fixture(scope="module")
def mixed(klg, tmp_path_factory):
    """the 8-frame 64x48 log of every frame kind, and what the serial reader makes of it"""
    d = tmp_path_factory.mktemp("mixed")
    frames = kc.mixed_log_frames()
    path = kc.write_log(d / "mixed.klg", frames)
    r = klg.KlgReader(path, 64, 48)
    want = [(ts, dep.copy(), rgb.copy()) for ts, dep, rgb in r]
    r.close()
    assert len(want) == 8
    return path, frames, want


def _colour_of(klg, kind, colour, H, W):
    """what the device would make of a prefetched frame, computed on the host: the reader's channel order (flip_colors off)"""
    if kind == klg.COLOR_JPEG:
        return klg.jpeg_finish_host(*colour)[..., ::-1]
    if kind == klg.COLOR_DECODED:
        return colour[..., ::-1]
    if kind == klg.COLOR_RAW:
        return colour
    return np.zeros((H, W, 3), np.uint8)


def _check_frames(klg, got, frames, want):
    assert len(got) == len(want)
    for k, ((ts, mm, kind, colour), (_, mm0, _, _), (ts0, dep0, rgb0)) in enumerate(zip(got, frames, want)):
        assert ts == ts0, f"frame {k}: timestamp (order)"
        assert np.array_equal(mm, mm0), f"frame {k}: u16 depth"
        assert np.array_equal(mm.astype(np.float32) * np.float32(0.001), dep0), f"frame {k}: depth in metres"
        assert np.array_equal(_colour_of(klg, kind, colour, 48, 64), rgb0), f"frame {k}: colour"


@pytest.mark.parametrize("workers", [1, 3, 8])
def test_prefetcher_delivers_the_readers_frames_in_order(klg, mixed, workers):
    path, frames, want = mixed
    p = klg.KlgPrefetcher(path, 64, 48, workers=workers, slots=4)
    assert p.num_frames == 8
    got = list(p)
    kinds = [g[2] for g in got]
    assert klg.COLOR_JPEG in kinds and klg.COLOR_RAW in kinds
    _check_frames(klg, got, frames, want)
    p.rewind()   # replays identically
    _check_frames(klg, list(p), frames, want)
    p.rewind()
    first = [next(p) for _ in range(3)]
    p.rewind()   # ... also from the middle, with frames in flight
    _check_frames(klg, list(p), frames, want)
    _check_frames(klg, first, frames[:3], want[:3])
    p.close()


def test_prefetcher_falls_back_to_the_host_decoder_for_a_refused_frame(klg, tmp_path):
    stream, ref = kc.fixture("restart_64x48_420")
    mm = np.arange(64 * 48, dtype=np.uint16).reshape(48, 64)
    path = kc.write_log(tmp_path / "wide.klg", [(1, mm, "zlib", stream), (2, mm, "raw", kc.wide_quant(stream)), (3, mm, "zlib", stream)])
    got = list(klg.KlgPrefetcher(path, 64, 48, workers=2, slots=3))
    assert [g[2] for g in got] == [klg.COLOR_JPEG, klg.COLOR_DECODED, klg.COLOR_JPEG]
    for g in got:
        assert np.array_equal(_colour_of(klg, g[2], g[3], 48, 64)[..., ::-1], ref)


def test_truncated_log_plays_up_to_the_broken_frame_and_names_it(klg, mixed, tmp_path):
    _, frames, want = mixed
    path = kc.write_log(tmp_path / "cut.klg", frames, truncate_at=5)
    for workers in (1, 8):
        p = klg.KlgPrefetcher(path, 64, 48, workers=workers, slots=4)
        assert p.num_frames == 8
        got = [next(p) for _ in range(5)]
        _check_frames(klg, got, frames[:5], want[:5])
        with pytest.raises(klg.KlgError, match="frame 5"):
            next(p)
        p.close()
    with pytest.raises(klg.KlgError):
        klg.KlgPrefetcher(tmp_path / "missing.klg", 64, 48)


def test_closing_with_workers_mid_frame_returns(klg, mixed):
    """eight workers read ahead while the owner takes one frame and closes: run in a child process so that a hang cannot take the
    suite with it"""
    path, _, _ = mixed
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from co_fusion_amd import klg\n"
            "p = klg.KlgPrefetcher(%r, 64, 48, workers=8, slots=10)\n"
            "ts = next(p)[0]\n"
            "p.close()\n"
            "print('closed', ts)\n") % (ROOT, str(path))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "closed 1000" in r.stdout, r.stdout + r.stderr


def _have_sanitizer(tmp_path, flag):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = tmp_path / "probe"
    r = subprocess.run(["g++", flag, str(src), "-o", str(exe)], capture_output=True)
    return r.returncode == 0 and subprocess.run([str(exe)], capture_output=True).returncode == 0


@pytest.mark.parametrize("flag", ["-fsanitize=thread", "-fsanitize=address,undefined"])
def test_prefetcher_is_clean_under_the_sanitizers(mixed, tmp_path, flag):
    """tests/native/klg_prefetch_check.cpp: a program of its own (no HIP, no Python) that links KlgIO.cpp, Jpeg.cpp and the prefetcher,
    plays the mixed log with 8 workers against the serial reader, rewinds mid-way and closes with frames in flight"""
    if not shutil.which("g++") or not _have_sanitizer(tmp_path, flag):
        pytest.skip(f"g++ {flag} is not available on this machine")
    path, _, _ = mixed
    host = os.path.join(ROOT, "co_fusion_amd", "host")
    exe = str(tmp_path / "klg_prefetch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", flag, "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "klg_prefetch_check.cpp"), os.path.join(host, "KlgPrefetch.cpp"),
                           os.path.join(host, "KlgIO.cpp"), os.path.join(host, "Jpeg.cpp"), "-lz", "-o", exe])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1:exitcode=67", UBSAN_OPTIONS="halt_on_error=1:exitcode=68")
    r = subprocess.run([exe, str(path), "64", "48", "8"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "frames ok" in r.stdout, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
