"""GPU suite: cf_frame_decoder (csrc/frame_decode.hip) -- the device half of the .klg log player.  Two kernels finish a frame whose
depth was inflated and whose JPEG was entropy-decoded on the host: dequantisation + islow IDCT, then chroma upsampling + colour
conversion + u16 mm -> f32 metres.  Integer arithmetic: every comparison is byte equality with the host decoder (host/Jpeg.cpp,
host/KlgIO.cpp), itself pinned to libjpeg by tests/test_cpu_klg_player.py."""
import zlib

import numpy as np
import pytest

import klg_player_cases as kc

pytestmark = pytest.mark.gpu

MAX_W, MAX_H = 104, 77


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from co_fusion_amd import api, klg
    ctx = api.Context(64, 48, 50.0, 50.0, 32.0, 24.0)
    dec = api.FrameDecoder(ctx, MAX_W, MAX_H, slots=3)
    yield api, klg, ctx, dec
    dec.close()
    ctx.close()


def _mm(rng, W, H):
    mm = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    mm.reshape(-1)[:6] = [0, 1, 999, 1000, 32768, 65535][:min(6, W * H)]
    return mm


def _run(dec, slot, W, H, mm, kind, colour, flip, complete=True):
    dec.fill(slot, W, H, mm, kind, colour)
    dec.submit(slot, W, H, kind, flip_colors=flip)
    d, c = dec.acquire(slot, complete=complete)
    if not complete:
        dec.ctx.synchronize()
    return d.cpu().numpy(), c.cpu().numpy()


def _rgba(rgb, reverse):
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = rgb[..., ::-1] if reverse else rgb
    return out


def _metres(mm):
    return mm.astype(np.float32) * np.float32(0.001)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", kc.FIXTURES)
def test_fixtures_decode_like_the_host_decoder(env, name, flip):
    api, klg, ctx, dec = env
    stream, ref = kc.fixture(name)
    H, W = ref.shape[:2]
    rc, hd, coef = klg.jpeg_front(stream, W, H)
    assert rc == 0
    host = klg.jpeg_finish_host(hd, coef)
    assert np.array_equal(host, ref)
    mm = _mm(np.random.default_rng(3), W, H)
    d, c = _run(dec, 0, W, H, mm, klg.COLOR_JPEG, (hd, coef), flip)
    assert np.array_equal(c, _rgba(host, reverse=not flip)), "RGBA differs from the host decoder"   # KlgLogReader: reversed unless flip_colors
    assert d.tobytes() == _metres(mm).tobytes()


# sampling-factor pairs the fixtures cannot reach: replication for both chroma planes; luma 4x1; fancy h2v2 for one chroma plane and
# replication (2x1 under a 2x2 luma is no case of the fancy filters) for the other
SAMPLINGS = {"1x2": [(1, 2), (1, 1), (1, 1)], "4x1": [(4, 1), (1, 1), (1, 1)], "2x2+2x1": [(2, 2), (2, 1), (1, 1)],
             "420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)], "444": [(1, 1), (1, 1), (1, 1)], "grey": [(1, 1)]}


@pytest.mark.parametrize("kind", ["dc", "mixed", "extreme"])
@pytest.mark.parametrize("size", [(8, 8), (24, 40), (101, 77)])
@pytest.mark.parametrize("sampling", sorted(SAMPLINGS))
def test_random_coefficients_against_the_host_back_end(env, sampling, size, kind):
    """no encoder needed: int16 coefficients anywhere in the range the front end hands over (all of int16, 8-bit tables)"""
    api, klg, ctx, dec = env
    W, H = size
    rng = np.random.default_rng(zlib.crc32(repr((sampling, size, kind)).encode()))
    nc = len(SAMPLINGS[sampling])
    qt = np.full((nc, 64), 255) if kind == "extreme" else rng.integers(1, 256 if kind == "mixed" else 17, (nc, 64))
    hd = klg.jpeg_header(W, H, SAMPLINGS[sampling], qt)
    coef = kc.random_coef(rng, hd.total_blocks, kind)
    if kind == "dc":
        assert not coef[:, 1:].any()
    host = klg.jpeg_finish_host(hd, coef)
    if kind == "extreme":   # both clamps of the IDCT fire in the host result (a plane value outside 0..255 is cut to the bound)
        assert (host == 0).any() and (host == 255).any(), "the extreme case does not reach the clamps"
    for flip in (False, True):
        mm = _mm(rng, W, H)
        d, c = _run(dec, int(flip), W, H, mm, klg.COLOR_JPEG, (hd, coef), flip)
        assert np.array_equal(c, _rgba(host, reverse=not flip))
        assert d.tobytes() == _metres(mm).tobytes()


def test_both_colour_clamps_fire(env):
    """4:4:4 at the range's extremes: the planes come from one-component decodes of each component's coefficients, the colour
    conversion is restated here WITHOUT its clamp -- values below 0 and above 255 must occur, and the device must equal the host."""
    api, klg, ctx, dec = env
    W, H = 24, 40
    rng = np.random.default_rng(77)
    hd = klg.jpeg_header(W, H, SAMPLINGS["444"], np.full((3, 64), 255))
    coef = kc.random_coef(rng, hd.total_blocks, "extreme")
    per = hd.total_blocks // 3
    g1 = klg.jpeg_header(W, H, [(1, 1)], np.full((1, 64), 255))
    Y, Cb, Cr = [klg.jpeg_finish_host(g1, coef[k * per:(k + 1) * per])[..., 0].astype(np.int64) for k in range(3)]
    assert Y.min() == 0 and Y.max() == 255, "IDCT clamps"
    cb, cr = Cb - 128, Cr - 128
    r = Y + ((91881 * cr + 32768) >> 16)
    g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    for ch in (r, g, b):
        assert ch.min() < 0 and ch.max() > 255, "the colour clamps do not fire"
    host = klg.jpeg_finish_host(hd, coef)
    assert np.array_equal(host, np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8))
    _, c = _run(dec, 2, W, H, _mm(rng, W, H), klg.COLOR_JPEG, (hd, coef), True)
    assert np.array_equal(c, _rgba(host, reverse=False))


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (101, 77), (104, 72)])
def test_depth_and_raw_colour(env, size):
    """u16 millimetres -> f32(u16) * f32(0.001), one multiply, bit for bit (0, 1, 999, 1000, 32768, 65535 and a ramp); raw colour with
    the reader's flip rule (reversed only WITH flip_colors), a host-decoded JPEG with the JPEG's rule, no colour block -> black"""
    api, klg, ctx, dec = env
    W, H = size
    rng = np.random.default_rng(W * 1000 + H)
    ramp = (np.arange(W * H, dtype=np.uint64) * 65535 // max(W * H - 1, 1)).astype(np.uint16).reshape(H, W)
    for mm in (_mm(rng, W, H), ramp):
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for flip in (False, True):
            d, c = _run(dec, 0, W, H, mm, klg.COLOR_RAW, rgb, flip)
            assert d.tobytes() == _metres(mm).tobytes()
            assert np.array_equal(c, _rgba(rgb, reverse=flip))
            d, c = _run(dec, 1, W, H, mm, klg.COLOR_DECODED, rgb, flip)
            assert np.array_equal(c, _rgba(rgb, reverse=not flip)) and d.tobytes() == _metres(mm).tobytes()
        d, c = _run(dec, 2, W, H, mm, klg.COLOR_NONE, None, False)
        assert np.array_equal(c, _rgba(np.zeros((H, W, 3), np.uint8), False)) and d.tobytes() == _metres(mm).tobytes()


def test_slots_rotate(env):
    """two frames submitted back to back into different slots, acquired in order; then the first slot takes a third frame while the
    second frame's output stays what it was"""
    api, klg, ctx, dec = env
    names = ["edge_104x72_420", "odd_101x77_422", "grey_64x48"]
    want, sizes = [], []
    rng = np.random.default_rng(9)
    for s, name in zip((0, 1), names):
        stream, ref = kc.fixture(name)
        H, W = ref.shape[:2]
        _, hd, coef = klg.jpeg_front(stream, W, H)
        mm = _mm(rng, W, H)
        dec.fill(s, W, H, mm, klg.COLOR_JPEG, (hd, coef))
        dec.submit(s, W, H, klg.COLOR_JPEG)
        want.append((_rgba(ref, True), _metres(mm)))
    outs = [dec.acquire(s, complete=(s == 0)) for s in (0, 1)]   # slot 1 in stream order on the context's stream
    ctx.synchronize()
    for (d, c), (wc, wd) in zip(outs, want):
        assert np.array_equal(c.cpu().numpy(), wc) and d.cpu().numpy().tobytes() == wd.tobytes()
    stream, ref = kc.fixture(names[2])
    H, W = ref.shape[:2]
    _, hd, coef = klg.jpeg_front(stream, W, H)
    mm = _mm(rng, W, H)
    d, c = _run(dec, 0, W, H, mm, klg.COLOR_JPEG, (hd, coef), False)
    assert np.array_equal(c, _rgba(ref, True)) and d.tobytes() == _metres(mm).tobytes()
    d1, c1 = dec.acquire(1)
    assert np.array_equal(c1.cpu().numpy(), want[1][0]) and d1.cpu().numpy().tobytes() == want[1][1].tobytes()


def test_maximum_size_then_a_smaller_frame_and_refusals(env):
    api, klg, ctx, _ = env
    dec = api.FrameDecoder(ctx, 101, 77, slots=2)
    for name in ("odd_101x77_420", "mcu_16x16_420", "odd_101x77_422"):
        stream, ref = kc.fixture(name)
        H, W = ref.shape[:2]
        _, hd, coef = klg.jpeg_front(stream, W, H)
        d, c = _run(dec, 1, W, H, np.zeros((H, W), np.uint16), klg.COLOR_JPEG, (hd, coef), False)
        assert np.array_equal(c, _rgba(ref, True)) and not d.any()
    with pytest.raises(api.CofusionError):   # larger than the decoder
        dec.submit(0, 104, 72, klg.COLOR_RAW)
    stream, ref = kc.fixture("mcu_16x16_420")
    _, hd, coef = klg.jpeg_front(stream, 16, 16)
    dec.fill(0, 16, 16, np.zeros((16, 16), np.uint16), klg.COLOR_JPEG, (hd, coef))
    with pytest.raises(api.CofusionError):   # a header that does not describe the frame: nothing is launched
        dec.submit(0, 24, 16, klg.COLOR_JPEG)
    with pytest.raises(api.CofusionError):
        dec.acquire(0)
    dec.close()
    with pytest.raises(api.CofusionError):
        api.FrameDecoder(ctx, 0, 16)
