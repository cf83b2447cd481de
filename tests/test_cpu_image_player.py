"""CPU suite: the host half of the image player (co_fusion_amd/host/ImagePlayer.cpp: ImagePrefetcher) -- worker threads decode the
frames of a directory ahead into slot memory; delivered in order and finished by the host statements of the device's kernels they must
equal the serial reader's frames (ImageSequenceReader) byte for byte, with any number of workers, after a rewind, and up to a
corrupt frame."""
import os

import numpy as np
import pytest

import image_cases as ic
import klg_player_cases as kc

W, H, FRAMES = 24, 16, 7


@pytest.fixture(scope="module")
def im():
    import __graft_entry__ as g
    g.build()
    from co_fusion_amd import images
    return images


def write_set(im, d, frames=FRAMES, kinds=("png", "exr", "png"), seed=0, w=W, h=H):
    """Color / Depth / Mask files of `frames` frames, numbered from 1; colour types and filters vary from frame to frame"""
    rng = np.random.default_rng(seed)
    os.makedirs(d, exist_ok=True)
    for i in range(frames):
        idx = f"{i + 1:04d}"
        rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        depth = (1.0 + rng.random((h, w)) + i).astype(np.float32)
        mask = rng.integers(0, 4, (h, w)).astype(np.uint8)
        if kinds[0] == "png":
            img = [rgb, np.dstack([rgb, rgb[..., :1]]), rgb[..., 0]][i % 3]   # RGB, RGBA, grey
            im.write_png(os.path.join(d, f"Color{idx}.png"), img, filters=(i % 5, (i + 2) % 5), idat_chunks=1 + i % 3)
        else:
            im.write_ppm(os.path.join(d, f"Color{idx}.ppm"), rgb)
        if kinds[1] == "exr":
            planes = {"B": depth, "G": depth * 2, "R": depth * 3} if i % 2 else {"Z": depth.astype(np.float16)}
            im.write_exr(os.path.join(d, f"Depth{idx}.exr"), planes, compression=[im.EXR_ZIP, im.EXR_ZIPS, im.EXR_NONE][i % 3])
        else:
            im.write_png(os.path.join(d, f"Depth{idx}.png"), np.round(depth * 1000).astype(np.uint16), filters=(4, 1))
        if kinds[2] == "png":
            im.write_png(os.path.join(d, f"Mask{idx}.png"), mask, filters=(2,))
        elif kinds[2] == "pgm":
            with open(os.path.join(d, f"Mask{idx}.pgm"), "wb") as f:
                f.write(im.pgm_bytes(mask))


def serial(im, d, **kw):
    with im.ImageSequenceReader(d, **kw) as r:
        return list(r)


def same(got, want):
    assert len(got) == len(want)
    for (ts, depth, rgba, mask), (wts, wdepth, wrgb, wmask) in zip(got, want):
        assert ts == wts and depth.tobytes() == wdepth.tobytes()
        assert np.array_equal(rgba[..., :3], wrgb) and (rgba[..., 3] == 255).all()
        assert (mask is None and wmask is None) or np.array_equal(mask, wmask)


@pytest.mark.parametrize("workers", [1, 3])
@pytest.mark.parametrize("kinds", [("png", "exr", "png"), ("ppm", "png", "pgm"), ("png", "png", None)])
def test_prefetched_frames_equal_the_serial_readers(im, tmp_path, kinds, workers):
    d = str(tmp_path / "set")
    write_set(im, d, kinds=kinds)
    for kw in ({}, {"flip_colors": True, "depth_scale": 0.001, "rate_hz": 30.0}):
        want = serial(im, d, **kw)
        assert len(want) == FRAMES and (want[0][3] is None) == (kinds[2] is None)
        p = im.ImagePrefetcher(d, workers=workers, slots=4, **kw)
        assert (p.width, p.height, p.num_frames) == (W, H, FRAMES)
        same(list(p), want)
        p.rewind()
        same([next(p) for _ in range(3)], want[:3])
        p.rewind()   # with frames in flight and a slot held
        same(list(p), want)
        p.close()


def test_jpeg_colour_directory(im, tmp_path):
    stream, ref = kc.fixture("edge_104x72_420")
    mm = ic.golden("depth_104x72_idat5")
    d = tmp_path / "jpg"
    d.mkdir()
    for i in range(3):
        (d / f"Color{i:04d}.jpg").write_bytes(bytes(stream))
        (d / f"Depth{i:04d}.png").write_bytes(mm[0])
    want = serial(im, str(d), depth_scale=0.0002)
    assert np.array_equal(want[0][2], ref) and want[0][1].tobytes() == (mm[1].astype(np.float32) * np.float32(0.0002)).tobytes()
    p = im.ImagePrefetcher(str(d), workers=2, depth_scale=0.0002)
    same(list(p), want)
    p.close()


def test_a_corrupt_frame_fails_at_its_position_and_names_the_file(im, tmp_path):
    d = str(tmp_path / "set")
    write_set(im, d)
    want = serial(im, d)
    bad = os.path.join(d, "Depth0004.exr")
    data = open(bad, "rb").read()
    open(bad, "wb").write(data[:-10])   # the last block runs past the end of the file
    for workers in (1, 3):
        p = im.ImagePrefetcher(d, workers=workers)
        same([next(p) for _ in range(3)], want[:3])
        with pytest.raises(im.ImageError, match="frame 3: .*Depth0004.exr: "):
            next(p)
        assert list(p) == [], "nothing is played behind a frame that failed"
        p.rewind()
        same([next(p) for _ in range(3)], want[:3])
        p.close()
    with pytest.raises(im.ImageError, match="mask frames"):
        os.remove(os.path.join(d, "Mask0007.png"))
        im.ImagePrefetcher(d)


def test_masks_for_the_first_frames_only(im, tmp_path):
    """the reference's `index < maxMasks` (ImageLogReader.cpp:269).  Its own count rule keeps maxMasks at the frame count, so the
    branch is reached through the max_masks option: masks end at frame 4, the mask files of the later frames are never opened"""
    d = str(tmp_path / "set")
    write_set(im, d)
    full = serial(im, d)
    open(os.path.join(d, "Mask0006.png"), "wb").write(b"not a PNG")   # frame 5: beyond max_masks, must not be read
    want = serial(im, d, max_masks=4)
    assert [w[3] is not None for w in want] == [True] * 4 + [False] * 3
    for a, b in zip(want, full):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
        assert a[3] is None or np.array_equal(a[3], b[3])
    with im.ImageSequenceReader(d, max_masks=4) as r:
        assert (r.has_masks, r.max_masks) == (True, 4)
    with im.ImageSequenceReader(d, max_masks=99) as r:
        assert r.max_masks == FRAMES
    for workers in (1, 3):
        p = im.ImagePrefetcher(d, workers=workers, max_masks=4)
        assert p.max_masks == 4
        same(list(p), want)
        p.close()
    with pytest.raises(im.ImageError, match="Mask0006.png: "):
        serial(im, d)

