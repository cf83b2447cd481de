"""GPU suite: the image entries of cf_frame_decoder (csrc/image_decode.hip) -- exr_depth_kernel (ZIP predictor scan, interleave,
channel pick, HALF -> f32) and png_finish_kernel (scanlines -> RGBA8 / f32 depth / u8 mask).  Integer work plus one f32 product: every
comparison is byte equality with the fixture arrays of tests/golden/image_seq (PIL's decode of the PNGs; the writer's input and the
numpy restatement for OpenEXR) and with the host statements of the kernels."""
import numpy as np
import pytest

import image_cases as ic
import klg_player_cases as kc

pytestmark = pytest.mark.gpu

MAX_W, MAX_H = 640, 77


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from co_fusion_amd import api, images, klg
    ctx = api.Context(64, 48, 50.0, 50.0, 32.0, 24.0)
    dec = api.FrameDecoder(ctx, MAX_W, MAX_H, slots=3)
    dec.enable_images()
    yield api, images, klg, ctx, dec
    dec.close()
    ctx.close()


def _out(dec, s, complete=True):
    d, c = dec.acquire(s, complete=complete)
    m = dec.acquire_mask(s, complete=complete)
    if not complete:
        dec.ctx.synchronize()
    return d.cpu().numpy(), c.cpu().numpy(), (None if m is None else m.cpu().numpy())


BLACK = lambda H, W: ic.rgba_of(np.zeros((H, W, 3), np.uint8))
SIZES = ["1x1", "13x7_mixed", "104x72_idat5"]


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("kind", ["rgb", "rgba", "grey", "pal"])
def test_png_frames_match_pil(env, kind, size, flip):
    """colour of every accepted type beside 16-bit depth (0, 1, 255, 256, 65535 among the samples) and an 8-bit mask: widths 1, 13
    (rows that start at every byte alignment, pixel groups that straddle row ends) and 104, one workgroup and several"""
    api, im, klg, ctx, dec = env
    (cdata, rgb), (ddata, mm), (mdata, mask) = (ic.golden(f"{k}_{size}") for k in (kind, "depth", "mask"))
    for s, scale in ((0, None), (1, 0.001)):
        dec.submit_image_files(s, (".png", cdata), (".png", ddata), (".png", mdata), flip_colors=flip, depth_scale=scale)
        d, c, m = _out(dec, s)
        assert np.array_equal(c, ic.rgba_of(rgb, flip)), "RGBA differs from PIL's decode"
        assert d.tobytes() == (mm.astype(np.float32) * np.float32(im.DEFAULT_DEPTH_SCALE if scale is None else scale)).tobytes()
        assert np.array_equal(m, mask)


@pytest.mark.parametrize("f", range(5))
def test_png_every_filter_type(env, f):
    api, im, klg, ctx, dec = env
    (cdata, rgb), (ddata, mm) = ic.golden(f"rgb_13x7_f{f}"), ic.golden(f"depth_13x7_f{f}")
    dec.submit_image_files(2, (".png", cdata), (".png", ddata))
    d, c, m = _out(dec, 2)
    assert m is None, "a frame without a mask file has no mask"
    assert np.array_equal(c, ic.rgba_of(rgb)) and d.tobytes() == (mm.astype(np.float32) * np.float32(0.0006)).tobytes()


@pytest.mark.parametrize("name", sorted(ic.EXR_CASES))
def test_exr_depth_is_passed_on_bit_for_bit(env, name):
    """HALF and FLOAT, one channel and B of B, G, R; block starts at every alignment (13 x 7 HALF: 26-byte lines), a short last block
    (40 x 37), a 40 KB block (640 x 16: the scan's carry through ten steps), blocks stored raw and a file that mixes both kinds"""
    api, im, klg, ctx, dec = env
    data, want = ic.golden(name)
    H, W = want.shape
    desc = dec.submit_image_files(0, None, (".exr", data))
    d, c, m = _out(dec, 0)
    assert d.tobytes() == want.tobytes(), "depth differs from the plane the file holds"
    assert np.array_equal(c, BLACK(H, W)) and m is None
    info, raw, blocks = im.decode_exr(data)
    assert (desc.exr_blocks, desc.exr_line_bytes, desc.exr_chan_half) == (info.blocks, info.line_bytes, info.chan_half)
    assert d.tobytes() == im.exr_finish_host(info, raw, blocks).tobytes()
    _, v = dec.image_slot(0)
    assert v["depth"][:raw.size].tobytes() == raw.tobytes(), "the scan runs on the device's copy: the staging keeps the file's bytes"


def test_klg_frames_between_png_frames_share_the_slots(env):
    """PNG frame, .klg frame, PNG frame through the same slot, then all three slots in flight at once, acquired in stream order"""
    api, im, klg, ctx, dec = env
    (cdata, rgb), (ddata, mm), (mdata, mask) = (ic.golden(f"{k}_104x72_idat5") for k in ("rgba", "depth", "mask"))
    stream, ref = kc.fixture("odd_101x77_422")
    Hk, Wk = ref.shape[:2]
    _, hd, coef = klg.jpeg_front(stream, Wk, Hk)
    kmm = np.random.default_rng(4).integers(0, 65536, (Hk, Wk)).astype(np.uint16)
    png_depth = (mm.astype(np.float32) * np.float32(0.0006)).tobytes()

    def png(s, with_mask=True):
        dec.submit_image_files(s, (".png", cdata), (".png", ddata), (".png", mdata) if with_mask else None)

    def check_png(out, with_mask=True):
        d, c, m = out
        assert np.array_equal(c, ic.rgba_of(rgb)) and d.tobytes() == png_depth
        assert np.array_equal(m, mask) if with_mask else m is None

    def check_klg(d, c):
        assert np.array_equal(c, ic.rgba_of(ref, True)) and d.tobytes() == (kmm.astype(np.float32) * np.float32(0.001)).tobytes()

    png(0)
    check_png(_out(dec, 0))
    dec.fill(0, Wk, Hk, kmm, klg.COLOR_JPEG, (hd, coef))
    dec.submit(0, Wk, Hk, klg.COLOR_JPEG)
    d, c = dec.acquire(0)
    check_klg(d.cpu().numpy(), c.cpu().numpy())
    assert dec.acquire_mask(0) is None, "a .klg frame has no mask: the PNG frame's mask before it in this slot is not handed out"
    png(0, with_mask=False)
    check_png(_out(dec, 0), with_mask=False)
    png(1)
    dec.fill(2, Wk, Hk, kmm, klg.COLOR_JPEG, (hd, coef))
    dec.submit(2, Wk, Hk, klg.COLOR_JPEG)
    png(0)
    outs = [_out(dec, s, complete=False) for s in (1, 0)]
    d, c = dec.acquire(2, complete=False)
    assert dec.acquire_mask(2, complete=False) is None
    ctx.synchronize()
    check_klg(d.cpu().numpy(), c.cpu().numpy())
    for o in outs:
        check_png(o)


@pytest.mark.parametrize("flip", [False, True])
def test_jpeg_colour_beside_png_depth_and_ppm_colour_beside_exr(env, flip):
    api, im, klg, ctx, dec = env
    stream, ref = kc.fixture("edge_104x72_420")
    ddata, mm = ic.golden("depth_104x72_idat5")
    dec.submit_image_files(0, (".jpg", stream), (".png", ddata), flip_colors=flip, depth_scale=0.0002)
    d, c, m = _out(dec, 0)
    assert np.array_equal(c, ic.rgba_of(ref, flip)), "a JPEG file's R, G, B unless flip_colors"
    assert d.tobytes() == (mm.astype(np.float32) * np.float32(0.0002)).tobytes() and m is None
    edata, want = ic.golden("zip_half_bgr_40x37")
    rng = np.random.default_rng(8)
    rgb, mask = rng.integers(0, 256, (37, 40, 3)).astype(np.uint8), rng.integers(0, 9, (37, 40)).astype(np.uint8)
    dec.submit_image_files(1, (".ppm", im.ppm_bytes(rgb)), (".exr", edata), (".pgm", im.pgm_bytes(mask)), flip_colors=flip)
    d, c, m = _out(dec, 1)
    assert np.array_equal(c, ic.rgba_of(rgb, flip)) and d.tobytes() == want.tobytes() and np.array_equal(m, mask)


def test_refusals_launch_nothing(env):
    api, im, klg, ctx, dec = env
    plain = api.FrameDecoder(ctx, 16, 16, slots=2)
    with pytest.raises(api.CofusionError, match="not enabled"):   # a decoder without the image staging
        plain.submit_images(0, im.ImageDesc(width=8, height=8))
    with pytest.raises(api.CofusionError, match="not enabled"):
        plain.image_slot(0)
    plain.close()
    data, want = ic.golden("zip_f32_bgr_40x37")
    desc = dec.submit_image_files(0, None, (".exr", data))
    good = _out(dec, 0)[0]
    _, v = dec.image_slot(0)
    for row, col, value in ((1, 0, 5), (2, 1, 1 << 30), (0, 3, 16), (1, 2, 7)):   # a block's offset, bytes, first_line, stored_raw
        keep = int(v["blocks"][row, col])
        v["blocks"][row, col] = value
        with pytest.raises(api.CofusionError, match="block table"):
            dec.submit_images(0, desc)
        v["blocks"][row, col] = keep
    for field, value in (("exr_line_bytes", desc.exr_line_bytes + 2), ("exr_chan_offset", desc.exr_line_bytes), ("exr_blocks", 4),
                         ("exr_lines_per_block", 8), ("width", MAX_W + 1), ("depth_kind", 7), ("color_kind", im.IMAGE_EXR)):
        keep = getattr(desc, field)
        setattr(desc, field, value)
        with pytest.raises(api.CofusionError):
            dec.submit_images(0, desc)
        setattr(desc, field, keep)
    dec.submit_images(0, desc)
    assert _out(dec, 0)[0].tobytes() == good.tobytes() == want.tobytes(), "the frame is intact after the refused submits"
    with pytest.raises(api.CofusionError, match="differ in size"):
        dec.submit_image_files(0, (".png", ic.golden("rgb_13x7_mixed")[0]), (".png", ic.golden("depth_1x1")[0]))
    with pytest.raises(api.CofusionError, match="Adam7"):
        dec.submit_image_files(0, (".png", im.png_bytes(np.zeros((4, 4, 3), np.uint8), interlace=1)), None)


def test_timing_mode_measures_the_two_image_kernels(env):
    """cf_frame_decoder_timing switches the event pairs on for both kinds of frame: image frames are counted by
    cf_frame_decoder_image_timing per kernel (an EXR frame without colour and mask still runs png_finish_kernel for the black colour
    plane), .klg frames by cf_frame_decoder_timing alone; the frames stay what they are"""
    api, im, klg, ctx, dec = env
    (cdata, rgb), (ddata, mm), (mdata, mask) = (ic.golden(f"{k}_104x72_idat5") for k in ("rgb", "depth", "mask"))
    edata, want = ic.golden("zip_f32_z_640x16")
    stream, ref = kc.fixture("odd_101x77_422")
    Hk, Wk = ref.shape[:2]
    _, hd, coef = klg.jpeg_front(stream, Wk, Hk)
    dec.timing(True)
    dec.image_timing()
    for k in range(4):   # slots reused while their events are pending: harvested at the next submit
        dec.submit_image_files(k % 2, (".png", cdata), (".png", ddata), (".png", mdata))
    dec.submit_image_files(2, None, (".exr", edata))
    dec.submit_image_files(2, None, (".exr", edata))
    dec.fill(0, Wk, Hk, np.zeros((Hk, Wk), np.uint16), klg.COLOR_JPEG, (hd, coef))
    dec.submit(0, Wk, Hk, klg.COLOR_JPEG)
    d, c, m = _out(dec, 1)
    assert np.array_equal(c, ic.rgba_of(rgb)) and np.array_equal(m, mask)
    assert _out(dec, 2)[0].tobytes() == want.tobytes()
    exr_ms, exr_n, fin_ms, fin_n = dec.image_timing()
    idct_ms, finish_ms, n = dec.timing(False)
    print(f"exr_depth_kernel {1e3 * exr_ms / exr_n:.1f} us (640x16), png_finish_kernel {1e3 * fin_ms / fin_n:.1f} us per frame")
    assert (exr_n, fin_n, n) == (2, 6, 1)
    assert 0 < exr_ms < 50 and 0 < fin_ms < 50 and idct_ms > 0 and finish_ms > 0
    assert dec.image_timing() == (0.0, 0, 0.0, 0), "reading resets the sums"
    dec.submit_image_files(0, (".png", cdata), (".png", ddata))   # timing off: nothing is recorded
    _out(dec, 0)
    assert dec.image_timing()[1::2] == (0, 0)

