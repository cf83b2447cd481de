"""The PNG stream format of the device exporter restated in numpy / Python: the yardstick of
csrc/png_encode.hip and host/ExportWriter.cpp.  encode() returns the file and a trace (per band its kind and bit length, per row its
filter, every token); assemble() builds the file from a band table the way the host writer does.  Nothing here is shared with the
product code."""
import struct
import zlib

import numpy as np

CF_PNG_LABELS = 1

_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]


def length_code(n):
    """RFC 1951 3.2.5: (index 0..28 of the length symbol 257 + index, number of extra bits, their value)"""
    for k in range(28, -1, -1):
        if n >= _LEN_BASE[k]:
            assert n - _LEN_BASE[k] < (1 << _LEN_EXTRA[k]) or (_LEN_EXTRA[k] == 0 and n == _LEN_BASE[k])
            return k, _LEN_EXTRA[k], n - _LEN_BASE[k]
    raise ValueError(n)


class _Bits:
    def __init__(self):
        self.bits = []

    def lsb(self, value, n):          # extra bits and header fields: least significant bit first
        self.bits += [(value >> i) & 1 for i in range(n)]

    def huff(self, code, n):          # Huffman codes: most significant bit first
        self.bits += [(code >> i) & 1 for i in range(n - 1, -1, -1)]

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def _fixed_symbol(bits, sym):
    if sym < 144:
        bits.huff(0x30 + sym, 8)
    elif sym < 256:
        bits.huff(0x190 + sym - 144, 9)
    elif sym < 280:
        bits.huff(sym - 256, 7)
    else:
        bits.huff(0xC0 + sym - 280, 8)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def filter_rows(img, channels):
    """img u8 [h, w * channels] -> (list of (type, filtered bytes u8)): per row the type of the smallest sum of |int8|, ties lowest"""
    h, rb = img.shape
    bpp = channels
    out = []
    zero = np.zeros(rb, np.int32)
    for y in range(h):
        x = img[y].astype(np.int32)
        b = img[y - 1].astype(np.int32) if y else zero
        a = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        c = np.concatenate([np.zeros(bpp, np.int32), b[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        pae = np.array([_paeth(int(a[i]), int(b[i]), int(c[i])) for i in range(rb)], np.int32)
        cands = [x, x - a, x - b, x - ((a + b) >> 1), x - pae]
        best = None
        for t, f in enumerate(cands):
            f8 = (f & 255).astype(np.uint8)
            cost = int(np.abs(f8.view(np.int8).astype(np.int32)).sum())
            if best is None or cost < best[0]:
                best = (cost, t, f8)
        out.append((best[1], best[2]))
    return out


def tokens_of(S):
    """maximal runs of equal bytes -> [("lit", v)] / [("match", length)] (distance 1 always)"""
    toks = []
    i, n = 0, len(S)
    while i < n:
        j = i
        while j < n and S[j] == S[i]:
            j += 1
        v, m = int(S[i]), j - i - 1
        toks.append(("lit", v))
        while m >= 258:
            toks.append(("match", 258))
            m -= 258
        if m >= 3:
            toks.append(("match", m))
        else:
            toks += [("lit", v)] * m
        i = j
    return toks


def encode_band(S):
    """-> (bytes of the band, kind 'fixed' | 'stored', bit length of the fixed form before padding, tokens)"""
    S = bytes(S)
    toks = tokens_of(S)
    bits = _Bits()
    bits.lsb(0, 1)      # BFINAL = 0
    bits.lsb(1, 2)      # BTYPE = 01
    for kind, v in toks:
        if kind == "lit":
            _fixed_symbol(bits, v)
        else:
            k, eb, ev = length_code(v)
            _fixed_symbol(bits, 257 + k)
            bits.lsb(ev, eb)
            bits.huff(0, 5)   # distance 1
    _fixed_symbol(bits, 256)
    bits.lsb(0, 3)      # an empty stored block: BFINAL = 0, BTYPE = 00
    nbits = len(bits.bits)
    fixed = bits.bytes() + b"\x00\x00\xff\xff"
    stored = b"\x00" + struct.pack("<HH", len(S), len(S) ^ 0xFFFF) + S
    assert len(S) <= 65535
    if len(stored) < len(fixed):
        return stored, "stored", nbits, toks
    return fixed, "fixed", nbits, toks


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def assemble(width, height, channels, bands, adler):
    """bands: the encoded bands in order; adler: Adler-32 of the whole filtered stream"""
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 6 if channels == 4 else 0, 0, 0, 0)
    idat = b"\x78\x01" + b"".join(bands) + b"\x03\x00" + struct.pack(">I", adler)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b"")


def adler32_combine(a1, a2, len2):
    """Adler-32 of the concatenation from the two parts' sums and the second part's length"""
    M = 65521
    s1a, s2a = a1 & 0xFFFF, a1 >> 16
    s1b, s2b = a2 & 0xFFFF, a2 >> 16
    s1 = (s1a + s1b - 1) % M
    s2 = (s2a + s2b + (len2 % M) * ((s1a - 1) % M)) % M
    return (s2 << 16) | s1


def encode(pixels, channels, rows_per_band, flags=0):
    """pixels u8 [h, w] (channels 1) or [h, w, 4] -> (file, trace).  trace: dict(filters=[type per row], bands=[dict(kind, bits, bytes,
    tokens, stream_bytes, adler, rows)], stream=the whole filtered stream)"""
    px = np.ascontiguousarray(pixels, np.uint8)
    h, w = px.shape[:2]
    assert channels in (1, 4) and px.size == h * w * channels
    img = px.reshape(h, w * channels).copy()
    if flags & CF_PNG_LABELS:
        assert channels == 1
        img[img > 254] = 0
    assert (1 + w * channels) * rows_per_band <= 65535
    rows = filter_rows(img, channels)
    trace = dict(filters=[t for t, _ in rows], bands=[])
    bands, whole = [], b""
    for y0 in range(0, h, rows_per_band):
        part = rows[y0:y0 + rows_per_band]
        S = b"".join(bytes([t]) + f.tobytes() for t, f in part)
        data, kind, nbits, toks = encode_band(S)
        bands.append(data)
        whole += S
        trace["bands"].append(dict(kind=kind, bits=nbits, bytes=len(data), tokens=toks, stream_bytes=len(S),
                                   adler=zlib.adler32(S) & 0xFFFFFFFF, rows=len(part), stream=S))
    trace["stream"] = whole
    adler = zlib.adler32(whole) & 0xFFFFFFFF
    comb = 1
    for b in trace["bands"]:
        comb = adler32_combine(comb, b["adler"], b["stream_bytes"])
    assert comb == adler
    return assemble(w, h, channels, bands, adler), trace


def idat_of(png):
    """the concatenated IDAT payload and (width, height, bit depth, colour type)"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, ihdr = 8, b"", None
    while pos < len(png):
        n, = struct.unpack(">I", png[pos:pos + 4])
        kind, body = png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        if kind == b"IDAT":
            idat += body
        pos += 12 + n
    return idat, ihdr[:4]


def decode(png):
    """pixels of an 8-bit grey or RGBA PNG, non-interlaced (any filters): u8 [h, w] or [h, w, 4] -- a decoder for tests without PIL"""
    idat, (w, h, depth, ctype) = idat_of(png)
    assert depth == 8 and ctype in (0, 6)
    ch = 4 if ctype == 6 else 1
    raw = zlib.decompress(idat)
    rb = w * ch
    assert len(raw) == (rb + 1) * h
    out = np.zeros((h, rb), np.int32)
    for y in range(h):
        t = raw[y * (rb + 1)]
        f = np.frombuffer(raw, np.uint8, rb, y * (rb + 1) + 1).astype(np.int32)
        up = out[y - 1] if y else np.zeros(rb, np.int32)
        if t == 0:
            out[y] = f
        elif t == 2:
            out[y] = (f + up) & 255
        else:
            row = out[y]
            for i in range(rb):
                a = row[i - ch] if i >= ch else 0
                c = up[i - ch] if i >= ch else 0
                pred = a if t == 1 else ((a + up[i]) >> 1 if t == 3 else _paeth(int(a), int(up[i]), int(c)))
                row[i] = (f[i] + pred) & 255
    out = out.astype(np.uint8)
    return out.reshape(h, w, 4) if ch == 4 else out.reshape(h, w)
