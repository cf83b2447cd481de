"""CPU suite: the host parsers of image-sequence datasets (co_fusion_amd/host/ImageIO.cpp) -- PNG, OpenEXR, PPM, the directory rules
of the reference's ImageLogReader and the serial reader.  Fixtures: tests/golden/image_seq (PNG expectations are PIL's decode; the
OpenEXR ones are the writer's input plus the numpy restatement in image_cases.py, for want of an independent decoder)."""
import os
import struct
import zlib

import numpy as np
import pytest

import image_cases as ic


@pytest.fixture(scope="module")
def im():
    import __graft_entry__ as g
    g.build()
    from co_fusion_amd import images
    return images


def test_fixtures_are_what_the_writers_produce(im):
    """the committed files are reproducible from the case tables (the writers are deterministic: numpy + zlib)"""
    for name in list(ic.PNG_CASES)[:6] + ["depth_104x72_idat5"]:
        assert ic.png_make(name)[0] == ic.golden(name)[0], name
    for name in ic.EXR_CASES:
        assert ic.exr_make(name)[0] == ic.golden(name)[0], name


@pytest.mark.parametrize("name", sorted(ic.PNG_CASES))
def test_png_scanlines_and_finish_match_pil(im, name):
    data, want = ic.golden(name)
    role = ic.png_role(name)
    info, scan, pal = im.decode_png(data, role)
    kind, W, H, filters, idat = ic.PNG_CASES[name]
    assert (info.width, info.height) == (W, H) and scan.shape == (H, 1 + info.bpp * W)
    assert [int(f) for f in scan[:, 0]] == [filters[y % len(filters)] for y in range(H)], "the filter bytes stay in the scanlines"
    assert data.count(b"IDAT") >= idat
    # the unfiltered scanlines, byte for byte, in file layout (16-bit samples big-endian)
    if role == ic.ROLE_DEPTH:
        assert scan[:, 1:].tobytes() == want.astype(">u2").tobytes()
        for scale in (im.DEFAULT_DEPTH_SCALE, 0.001, 0.0002):
            got = im.png_finish_host(info, scan, None, role, depth_scale=scale)
            assert got.tobytes() == (want.astype(np.float32) * np.float32(scale)).tobytes()
    elif role == ic.ROLE_MASK:
        assert np.array_equal(scan[:, 1:], want)
        assert np.array_equal(im.png_finish_host(info, scan, None, role), want)
    else:
        pix = scan[:, 1:].reshape(H, W, info.bpp)
        rgb = pal[pix[..., 0]] if kind == "pal" else (np.repeat(pix, 3, 2) if info.bpp == 1 else pix[..., :3])
        assert np.array_equal(rgb, want)
        for flip in (False, True):
            assert np.array_equal(im.png_finish_host(info, scan, pal, role, flip_colors=flip), ic.rgba_of(want, flip))


@pytest.mark.parametrize("name", sorted(ic.EXR_CASES))
def test_exr_blocks_and_finish(im, name):
    data, want = ic.golden(name)
    W, H, dtype, names, comp, noise = ic.EXR_CASES[name]
    assert ic.exr_decode_numpy(data).tobytes() == want.tobytes(), "the numpy restatement against the writer's input"
    info, raw, blocks = im.decode_exr(data)
    size = np.dtype(dtype).itemsize
    assert (info.width, info.height, info.compression) == (W, H, comp)
    assert info.lines_per_block == (16 if comp == ic.EXR_ZIP else 1) and info.blocks == len(blocks) == -(-H // info.lines_per_block)
    assert info.line_bytes == W * size * len(names) and info.chan_half == int(size == 2) and info.chan_offset == 0   # B sorts first
    table = ic.exr_blocks_numpy(data)
    for b, (first, stored, full, at) in zip(blocks, table):
        assert (b["first_line"], b["offset"], b["bytes"], b["stored_raw"]) == (first, first * info.line_bytes, full, int(stored == full))
        payload = data[at:at + stored]
        assert raw[b["offset"]:b["offset"] + full].tobytes() == (payload if stored == full else zlib.decompress(payload))
    if noise == "all":
        assert blocks["stored_raw"].all()
    if noise == "head":
        assert list(blocks["stored_raw"]) == [1, 0, 0], "a file that mixes raw and compressed blocks"
    if name == "zip_half_bgr_40x37":
        assert blocks[-1]["bytes"] == 5 * info.line_bytes, "the last ZIP block has 5 lines"
    if name == "zip_f32_z_640x16":
        assert len(blocks) == 1 and blocks[0]["bytes"] == 40960 and not blocks[0]["stored_raw"]
    assert im.exr_finish_host(info, raw, blocks).tobytes() == want.tobytes()


def test_exr_channel_choice(im):
    rng = np.random.default_rng(5)
    p = {n: rng.random((5, 6)).astype(np.float32) for n in "ABGRZ"}
    pick = lambda names: im.exr_finish_host(*im.decode_exr(im.exr_bytes({n: p[n] for n in names}, compression=im.EXR_ZIPS)))
    assert np.array_equal(pick("A"), p["A"]), "one channel of any name"
    assert np.array_equal(pick("BGR"), p["B"]) and np.array_equal(pick("ABGR"), p["B"]), "B of a file with B, G, R"
    mixed = {"B": p["B"].astype(np.float16), "G": p["G"], "R": p["R"], "A": p["A"].astype(np.float16)}
    info, raw, blocks = im.decode_exr(im.exr_bytes(mixed, compression=im.EXR_ZIP))
    assert info.chan_half == 1 and info.chan_offset == 6 * 2 and info.line_bytes == 6 * (2 + 2 + 4 + 4)
    assert np.array_equal(im.exr_finish_host(info, raw, blocks), mixed["B"].astype(np.float32))
    with pytest.raises(im.ImageError, match="no depth channel.*G, Z"):
        pick("GZ")


def test_half_to_float_every_finite_and_infinite_value(im):
    bits = np.arange(1 << 16, dtype=np.uint16)
    bits = bits[(bits & 0x7c00) != 0x7c00]   # NaN payloads are no part of what is promised
    bits = np.concatenate([bits, np.array([0x7c00, 0xfc00], np.uint16)])
    plane = np.resize(bits, (251, 256)).view(np.float16)
    got = im.exr_finish_host(*im.decode_exr(im.exr_bytes({"Z": plane}, compression=im.EXR_NONE)))
    assert got.tobytes() == plane.astype(np.float32).tobytes()


def _png_parts(data):
    """[(offset of the chunk, kind)] of a PNG"""
    pos, out = 8, []
    while pos < len(data):
        n, = struct.unpack_from(">I", data, pos)
        out.append((pos, data[pos + 4:pos + 8]))
        pos += 12 + n
    return out


def test_png_refusals_name_the_reason(im):
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (5, 6, 3)).astype(np.uint8)
    grey = rgb[..., 0]
    cases = [
        (im.png_bytes(rgb, interlace=1), ic.ROLE_COLOR, "Adam7"),
        (im.png_bytes(rgb.astype(np.uint16) * 257), ic.ROLE_COLOR, "16-bit colour"),
        (im.png_bytes(rgb), ic.ROLE_MASK, "colour masks"),
        (im.png_bytes(rgb), ic.ROLE_DEPTH, "16-bit grey"),
        (im.png_bytes(grey), ic.ROLE_DEPTH, "16-bit grey"),
        (im.png_bytes(grey.astype(np.uint16)), ic.ROLE_MASK, "8-bit grey"),
        (b"\x89PNG\r\n\x1a\n" + im.png_chunk(b"IHDR", struct.pack(">IIBBBBB", 6, 5, 4, 0, 0, 0, 0)) + im.png_chunk(b"IEND"), ic.ROLE_MASK, "sub-byte"),
        (b"\x89PNG\r\n\x1a\n" + im.png_chunk(b"IHDR", struct.pack(">IIBBBBB", 6, 5, 2, 3, 0, 0, 0)) + im.png_chunk(b"IEND"), ic.ROLE_COLOR, "sub-byte"),
        (b"JFIF" * 10, ic.ROLE_COLOR, "signature"),
        (im.png_bytes(grey, palette=np.zeros((3, 3), np.uint8)), ic.ROLE_COLOR, "palette index"),
    ]
    for data, role, pattern in cases:
        with pytest.raises(im.ImageError, match=pattern):
            im.decode_png(data, role)
    with pytest.raises(im.ImageError, match="Mask0007.png: .*Adam7"):
        im.decode_png(im.png_bytes(grey, interlace=1), ic.ROLE_MASK, name="Mask0007.png")
    good = im.png_bytes(rgb, filters=(4,), idat_chunks=2)
    parts = _png_parts(good)
    assert [k for _, k in parts] == [b"IHDR", b"IDAT", b"IDAT", b"IEND"]
    # truncation at every chunk boundary, inside every chunk header and inside every body
    for at, _ in parts:
        for cut in (at, at + 3, at + 8, at + 9):
            if cut < len(good):
                with pytest.raises(im.ImageError, match="truncated|IDAT|zlib"):
                    im.decode_png(good[:cut], ic.ROLE_COLOR)
    # a flipped bit in every critical chunk: the CRC names the chunk
    for at, kind in parts[:3]:
        bad = bytearray(good)
        bad[at + 9] ^= 0x10
        with pytest.raises(im.ImageError, match="CRC mismatch in chunk '%s'" % kind.decode()):
            im.decode_png(bytes(bad), ic.ROLE_COLOR)
    # a damaged Adler-32 under a correct CRC
    scan = im.png_filter_rows(rgb.reshape(5, -1), 3, (0,)).tobytes()
    z = bytearray(zlib.compress(scan))
    z[-1] ^= 1
    bad = good[:parts[1][0]] + im.png_chunk(b"IDAT", bytes(z)) + im.png_chunk(b"IEND")
    with pytest.raises(im.ImageError, match="Adler"):
        im.decode_png(bad, ic.ROLE_COLOR)
    # a stream of the wrong length, a row with filter type 5, an unknown critical chunk (an ancillary one is skipped)
    for rows, pattern in ((scan[:-1], "truncated|expected"), (scan + b"\0", "more pixels"), (b"\x05" + scan[1:], "filter type 5")):
        bad = good[:parts[1][0]] + im.png_chunk(b"IDAT", zlib.compress(rows)) + im.png_chunk(b"IEND")
        with pytest.raises(im.ImageError, match=pattern):
            im.decode_png(bad, ic.ROLE_COLOR)
    with pytest.raises(im.ImageError, match="unknown critical chunk 'ABCD'"):
        im.decode_png(im.png_bytes(rgb, extra_chunks=[(b"ABCD", b"xy")]), ic.ROLE_COLOR)
    info, scan2, _ = im.decode_png(im.png_bytes(rgb, extra_chunks=[(b"tRNS", b"\0\0\0\0\0\0"), (b"teXt", b"k\0v")]), ic.ROLE_COLOR)
    assert np.array_equal(scan2[:, 1:].reshape(5, 6, 3), rgb)


def test_exr_refusals_name_the_reason(im):
    z = np.linspace(0.5, 2.0, 40 * 20, dtype=np.float32).reshape(20, 40)
    box = struct.pack("<iiii", 0, 0, 39, 19)
    cases = [
        (im.exr_bytes({"Z": z}, version_flags=0x200), "tiled"),
        (im.exr_bytes({"Z": z}, extra_attrs=[("tiles", "tiledesc", struct.pack("<IIB", 32, 32, 0))]), "tiled"),
        (im.exr_bytes({"Z": z}, version_flags=0x1000), "multipart"),
        (im.exr_bytes({"Z": z}, version_flags=0x800), "deep"),
        (im.exr_bytes({"Z": z}, compression_code=4), "PIZ"),
        (im.exr_bytes({"Z": z}, compression_code=5), "PXR24"),
        (im.exr_bytes({"Z": z}, compression_code=6), "B44"),
        (im.exr_bytes({"Z": z}, compression_code=8), "DWAA"),
        (im.exr_bytes({"Z": z}, compression_code=1), "RLE"),
        (im.exr_bytes({"Z": z}, line_order=1), "line order"),
        (im.exr_bytes({"Z": z}, data_window=(2, 0, 39, 19)), "dataWindow"),
        (b"\x00" * 64, "magic"),
    ]
    good = im.exr_bytes({"Z": z}, compression=im.EXR_ZIP)
    uint = good.replace(b"Z\0" + struct.pack("<i", 2), b"Z\0" + struct.pack("<i", 0), 1)
    sub = good.replace(b"Z\0" + struct.pack("<iB3xii", 2, 0, 1, 1), b"Z\0" + struct.pack("<iB3xii", 2, 0, 2, 1), 1)
    cases += [(uint, "UINT"), (sub, "subsampled")]
    for data, pattern in cases:
        with pytest.raises(im.ImageError, match=pattern):
            im.decode_exr(data)
    with pytest.raises(im.ImageError, match="Depth0003.exr: .*PIZ"):
        im.decode_exr(cases[4][0], name="Depth0003.exr")
    # the offset table: an entry outside the file, an entry that points at the wrong block
    W, H, chans, line_bytes, blocks = ic._exr_parse(good)
    at_table = blocks[0][3] - 8 - 8 * len(blocks)
    assert struct.unpack_from("<Q", good, at_table)[0] == blocks[0][3] - 8
    for value, pattern in ((len(good) + 5, "outside the file"), (len(good) - 4, "outside the file"), (blocks[1][3] - 8, "starts at line 16")):
        bad = good[:at_table] + struct.pack("<Q", value) + good[at_table + 8:]
        with pytest.raises(im.ImageError, match=pattern):
            im.decode_exr(bad)
    # truncation: in the header, in the offset table, at every block boundary and inside every block
    cuts = [4, 9, 40, at_table - 1, at_table + 3] + [c for _, size, _, at in blocks for c in (at - 8, at - 3, at, at + size // 2, at + size - 1)]
    for cut in cuts:
        with pytest.raises(im.ImageError, match="truncated|outside the file|magic"):
            im.decode_exr(good[:cut])
    # a damaged deflate stream inside a block
    bad = bytearray(good)
    bad[blocks[0][3] + blocks[0][1] - 1] ^= 1
    with pytest.raises(im.ImageError, match="block 0: .*(Adler|zlib)"):
        im.decode_exr(bytes(bad))


def test_ppm(im):
    rgb = np.random.default_rng(2).integers(0, 256, (7, 13, 3)).astype(np.uint8)
    assert np.array_equal(im.decode_ppm(im.ppm_bytes(rgb)), rgb)
    assert np.array_equal(im.decode_ppm(im.ppm_bytes(rgb, comment="made here")), rgb)
    assert np.array_equal(im.decode_ppm(b"P6 13\t7\r\n255 " + rgb.tobytes()), rgb)
    for data, pattern in ((b"P5\n13 7\n255\n" + rgb.tobytes(), "magic"), (b"P6\n13 7\n65535\n" + rgb.tobytes() * 2, "maxval"),
                          (im.ppm_bytes(rgb)[:-1], "bytes of pixels"), (b"P6\n13", "truncated header"), (b"P6\n13 x 255\n", "decimal")):
        with pytest.raises(im.ImageError, match=pattern):
            im.decode_ppm(data)


def test_read_mask_dispatches_on_the_extension(im, tmp_path):
    from co_fusion_amd import masks
    m = np.random.default_rng(3).integers(0, 5, (7, 13)).astype(np.uint8)
    im.write_png(str(tmp_path / "Mask0000.png"), m, filters=(3,))
    (tmp_path / "Mask0001.pgm").write_bytes(im.pgm_bytes(m))
    assert np.array_equal(masks.read_mask(str(tmp_path / "Mask0000.png")), m)
    assert np.array_equal(masks.read_mask(str(tmp_path / "Mask0001.pgm")), m)
    with pytest.raises(ValueError):
        masks.read_mask(str(tmp_path / "Mask0002.jpg"))


# ---- the directory rules and the serial reader ----
W, H = 24, 16


def _frames(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        depth = (1.0 + rng.random((H, W)) + i).astype(np.float32)
        mask = rng.integers(0, 4, (H, W)).astype(np.uint8)
        out.append((rgb, depth, mask))
    return out


def _write_set(im, d, frames, start=0, masks=None, depth="exr", color="png", width=4):
    os.makedirs(d, exist_ok=True)
    for i, (rgb, depth_m, mask) in enumerate(frames):
        idx = f"{i + start:0{width}d}"
        if color == "png":
            im.write_png(os.path.join(d, f"Color{idx}.png"), rgb, filters=(i % 5,))
        else:
            im.write_ppm(os.path.join(d, f"Color{idx}.ppm"), rgb)
        if depth == "exr":
            im.write_exr(os.path.join(d, f"Depth{idx}.exr"), {"B": depth_m, "G": depth_m * 2, "R": depth_m * 3}, compression=im.EXR_ZIP)
        else:
            im.write_png(os.path.join(d, f"Depth{idx}.png"), np.round(depth_m * 1000).astype(np.uint16), filters=(4,))
        if masks is None or i < masks:
            im.write_png(os.path.join(d, f"Mask{idx}.png"), mask, filters=(2,))


def test_serial_reader_on_a_co_fusion_style_directory(im, tmp_path):
    frames = _frames(5)
    d = str(tmp_path / "set")
    _write_set(im, d, frames, start=1)
    with im.ImageSequenceReader(d) as r:
        assert (r.width, r.height, r.num_frames, r.start_index, r.has_masks, r.max_masks) == (W, H, 5, 1, True, 5)
        for rounds in range(2):
            got = list(r)
            assert len(got) == 5
            for i, ((ts, depth, rgb, mask), (wrgb, wdepth, wmask)) in enumerate(zip(got, frames)):
                assert ts == int(np.float32(i) * np.float32(1000.0) / np.float32(24.0))   # ImageLogReader.cpp:275 in f32
                assert np.array_equal(rgb, wrgb) and depth.tobytes() == wdepth.tobytes() and np.array_equal(mask, wmask)
            r.rewind()
    assert [int(np.float32(i) * np.float32(1000.0) / np.float32(24.0)) for i in (1, 2, 3)] == [41, 83, 125]
    with im.ImageSequenceReader(d, flip_colors=True, rate_hz=30.0) as r:
        ts, depth, rgb, mask = list(r)[4]
        assert np.array_equal(rgb, frames[4][0][..., ::-1]) and ts == int(np.float32(4) * np.float32(1000.0) / np.float32(30.0))


def test_serial_reader_png_depth_ppm_colour_and_depth_scale(im, tmp_path):
    frames = _frames(3, seed=4)
    d = str(tmp_path / "tum")
    _write_set(im, d, frames, masks=0, depth="png", color="ppm")
    for scale, used in ((0.0, np.float32(0.0006)), (0.001, np.float32(0.001)), (0.0002, np.float32(0.0002))):
        with im.ImageSequenceReader(d, depth_scale=scale) as r:
            assert not r.has_masks and r.start_index == 0
            for (ts, depth, rgb, mask), (wrgb, wdepth, _) in zip(r, frames):
                mm = np.round(wdepth * 1000).astype(np.uint16)
                assert mask is None and np.array_equal(rgb, wrgb) and depth.tobytes() == (mm.astype(np.float32) * used).tobytes()


def test_directory_rules(im, tmp_path):
    frames = _frames(4, seed=7)
    # masks must match the colour count
    d = str(tmp_path / "short")
    _write_set(im, d, frames, masks=3)
    with pytest.raises(im.ImageError, match=r"colour frames \(4\) != mask frames \(3\)"):
        im.ImageSequenceReader(d)
    os.remove(os.path.join(d, "Depth0003.exr"))
    with pytest.raises(im.ImageError, match=r"colour frames \(4\) != depth frames \(3\)"):
        im.ImageSequenceReader(d)
    # mixed extensions of one role
    d = str(tmp_path / "mixed")
    _write_set(im, d, frames, masks=0)
    im.write_ppm(os.path.join(d, "Color0009.ppm"), frames[0][0])
    with pytest.raises(im.ImageError, match="same extension"):
        im.ImageSequenceReader(d)
    # no file with index 0 or 1
    d = str(tmp_path / "late")
    _write_set(im, d, frames, start=2, masks=0)
    with pytest.raises(im.ImageError, match="start index"):
        im.ImageSequenceReader(d)
    with im.ImageSequenceReader(d, start_index=2) as r:
        assert r.start_index == 2 and np.array_equal(next(r)[2], frames[0][0])
    # separate directories with their own prefixes and index width; masks stop after max_masks frames
    c, dd, m = (str(tmp_path / n) for n in ("c", "d", "m"))
    for p in (c, dd, m):
        os.makedirs(p)
    for i, (rgb, depth, mask) in enumerate(frames):
        im.write_png(os.path.join(c, f"rgb_{i:06d}.png"), rgb)
        im.write_exr(os.path.join(dd, f"z_{i:06d}.exr"), {"Z": depth}, compression=im.EXR_ZIPS)
        im.write_png(os.path.join(m, f"seg_{i:06d}.png"), mask)
    with im.ImageSequenceReader(c, dd, m, "rgb_", "z_", "seg_", index_width=6) as r:
        assert r.num_frames == 4 and r.max_masks == 4
        assert all(np.array_equal(mk, f[2]) and dp.tobytes() == f[1].tobytes() for (_, dp, _, mk), f in zip(r, frames))
    # a corrupt frame fails at its position and names the file
    bad = os.path.join(c, "rgb_000002.png")
    data = bytearray(open(bad, "rb").read())
    data[40] ^= 0xff
    open(bad, "wb").write(bytes(data))
    with im.ImageSequenceReader(c, dd, m, "rgb_", "z_", "seg_", index_width=6) as r:
        assert np.array_equal(next(r)[2], frames[0][0]) and np.array_equal(next(r)[2], frames[1][0])
        with pytest.raises(im.ImageError, match="rgb_000002.png: "):
            next(r)
