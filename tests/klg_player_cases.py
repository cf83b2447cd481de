"""Shared inputs of the log player's tests (test_cpu_klg_player.py, test_frame_decode_gpu.py, test_klg_player_gpu.py): the committed
JPEG fixtures (tests/golden/klg_player, written by tools/make_klg_player_fixtures.py), crafted streams the JPEG front end must
refuse, hand-built .klg logs and coefficient-level cases.  Nothing here needs Pillow or a GPU."""
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "klg_player")
FIXTURES = ["mcu_16x16_420", "edge_104x72_420", "odd_101x77_420", "odd_101x77_422", "edge_104x72_444", "grey_64x48", "restart_64x48_420"]


def fixture(name):
    """(JPEG stream, the RGB libjpeg decodes it to)"""
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read(), np.load(os.path.join(GOLDEN, name + ".npy"))


def scene_jpeg(t):
    with open(os.path.join(GOLDEN, f"scene_160x128_{t}.jpg"), "rb") as f:
        return f.read()


def _segments(stream):
    """(marker, start of the marker, end of the segment) of the header segments up to SOS"""
    pos = 2
    while pos + 4 <= len(stream):
        assert stream[pos] == 0xFF
        m = stream[pos + 1]
        ln = struct.unpack_from(">H", stream, pos + 2)[0]
        yield m, pos, pos + 2 + ln
        if m == 0xDA:
            return
        pos += 2 + ln


def wide_quant(stream):
    """the same picture with its quantisation tables rewritten as 16-bit entries (pq = 1): a stream the front end refuses and the
    host decoder decodes to the same pixels"""
    out, last = bytearray(stream[:2]), 2
    for m, a, b in _segments(stream):
        out += stream[last:a]
        last = b
        if m != 0xDB:
            out += stream[a:b]
            continue
        body, p = bytearray(), a + 4
        while p < b:
            pq, tq = stream[p] >> 4, stream[p] & 15
            assert pq == 0
            body.append(0x10 | tq)
            for v in stream[p + 1:p + 65]:
                body += struct.pack(">H", v)
            p += 65
        out += b"\xff\xdb" + struct.pack(">H", len(body) + 2) + body
    return bytes(out + stream[last:])


def dc_overflow_stream(width=64, height=48):
    """A grey baseline JPEG written by hand whose every block adds +2047 to the DC predictor: it passes 32767 at the 17th block.  One
    DC code (category 11) and one AC code (end of block), one bit each; quantisation table of ones."""
    assert width % 8 == 0 and height % 8 == 0 and (width // 8) * (height // 8) > 17
    s = bytearray(b"\xff\xd8")
    s += b"\xff\xdb" + struct.pack(">H", 67) + b"\x00" + bytes([1] * 64)
    s += b"\xff\xc0" + struct.pack(">HBHHB", 11, 8, height, width, 1) + bytes([1, 0x11, 0])
    for tc, sym in ((0, 11), (1, 0)):
        s += b"\xff\xc4" + struct.pack(">H", 2 + 1 + 16 + 1) + bytes([tc << 4]) + bytes([1] + [0] * 15) + bytes([sym])
    s += b"\xff\xda" + struct.pack(">HB", 8, 1) + bytes([1, 0x00, 0, 63, 0])
    bits = ("0" + "1" * 11 + "0") * ((width // 8) * (height // 8))
    bits += "1" * (-len(bits) % 8)
    for i in range(0, len(bits), 8):
        b = int(bits[i:i + 8], 2)
        s.append(b)
        if b == 0xFF:
            s.append(0)
    return bytes(s + b"\xff\xd9")


def write_log(path, frames, truncate_at=None):
    """frames: [(timestamp, depth_mm u16 [H, W], 'zlib' | 'raw', colour bytes or b'')].  truncate_at = k: the file ends in the middle of
    frame k's depth block."""
    blob = bytearray(struct.pack("<i", len(frames)))
    for k, (ts, mm, how, colour) in enumerate(frames):
        d = mm.tobytes() if how == "raw" else zlib.compress(mm.tobytes(), 6)
        assert how == "raw" or len(d) != mm.nbytes
        blob += struct.pack("<qii", ts, len(d), len(colour))
        if truncate_at == k:
            blob += d[:len(d) // 2]
            break
        blob += d + colour
    with open(path, "wb") as f:
        f.write(blob)
    return path


def mixed_log_frames(n=8, W=64, H=48, seed=5):
    """n frames of every kind the reader knows: zlib and raw depth; JPEG (4:2:0 with restart markers, grey) and raw colour"""
    rng = np.random.default_rng(seed)
    jpegs = [fixture("restart_64x48_420")[0], fixture("grey_64x48")[0]]
    out = []
    for t in range(n):
        mm = (rng.integers(0, 5000, (H, W)) * (rng.random((H, W)) > 0.1)).astype(np.uint16)
        mm[0, :6] = [0, 1, 999, 1000, 32768, 65535]
        colour = jpegs[(t // 2) % 2] if t % 2 == 0 else rng.integers(0, 256, (H, W, 3), dtype=np.uint8).tobytes()
        out.append((1000 + 33333 * t, mm, "zlib" if t % 3 else "raw", colour))
    return out


def random_coef(rng, total_blocks, kind):
    """int16 [total_blocks, 64] quantised coefficients: 'dc' only the DC term, 'mixed' a decaying spectrum as a picture has, 'extreme'
    blocks at the ends of the int16 range (with a table of 255s both IDCT clamps and both colour clamps fire)"""
    c = np.zeros((total_blocks, 64), np.int64)
    if kind == "dc":
        c[:, 0] = rng.integers(-1100, 1100, total_blocks)
    elif kind == "mixed":
        scale = 600.0 / (1.0 + np.arange(64)) ** 1.2
        c = np.rint(rng.normal(size=(total_blocks, 64)) * scale)
        c[:, 0] = rng.integers(-1024, 1024, total_blocks)
        c[rng.random((total_blocks, 64)) < 0.5] = 0
    elif kind == "extreme":
        # by block: 0 -- no DC, a few AC terms at the ends of int16 (a wave far beyond the pixel range: both clamps inside one block);
        # 1 / 2 -- the DC term at either end (a block of 0s, a block of 255s); 3 -- small terms, which a table of 255s still saturates
        pick = np.arange(total_blocks) % 4
        hot = rng.random((total_blocks, 64)) < 0.1
        hot[:, 1] = True
        hot[:, 0] = False
        ends = rng.choice(np.array([-32768, 32767]), (total_blocks, 64))
        c[pick == 0] = np.where(hot, ends, 0)[pick == 0]
        c[pick == 1, 0] = -32768
        c[pick == 2, 0] = 32767
        c[pick == 3] = rng.integers(-255, 256, (total_blocks, 64))[pick == 3]
    else:
        raise ValueError(kind)
    return np.clip(c, -32768, 32767).astype(np.int16)
