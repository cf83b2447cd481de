"""CPU suite: the PNG stream format of the device exporter as tests/png_encode_ref.py states it.  Every case of the table
(tests/png_encode_cases.py) gives a valid PNG -- it opens in PIL (where installed) and in the reference's own decoder, and zlib
inflates its IDAT to the filtered stream -- and the table holds the edges of the format, asserted from the traces."""
import zlib

import numpy as np
import pytest

import png_encode_cases
import png_encode_ref as ref


@pytest.fixture(scope="module")
def encoded():
    return [(name, img, ch, R, flags) + ref.encode(img, ch, R, flags) for name, img, ch, R, flags in png_encode_cases.cases()]


def _expected(img, flags):
    want = np.array(img, np.uint8)
    if flags & ref.CF_PNG_LABELS:
        want[want > 254] = 0
    return want


def test_every_file_decodes_to_the_pixels(encoded):
    try:
        import io
        from PIL import Image
    except ImportError:
        Image = None
    for name, img, ch, R, flags, png, trace in encoded:
        want = _expected(img, flags)
        assert np.array_equal(ref.decode(png), want), name
        if Image is not None:
            im = Image.open(io.BytesIO(png))
            assert im.mode == ("RGBA" if ch == 4 else "L"), name
            assert np.array_equal(np.asarray(im), want), name


def test_idat_inflates_to_the_filtered_stream(encoded):
    for name, img, ch, R, flags, png, trace in encoded:
        idat, (w, h, depth, ctype) = ref.idat_of(png)
        assert (w, h, depth, ctype) == (img.shape[1], img.shape[0], 8, 6 if ch == 4 else 0), name
        assert idat[:2] == b"\x78\x01" and zlib.decompress(idat) == trace["stream"], name
        assert len(trace["stream"]) == (1 + img.shape[1] * ch) * img.shape[0], name
        assert sum(b["bytes"] for b in trace["bands"]) + 2 + 2 + 4 == len(idat), name


def test_the_table_holds_the_edges_of_the_format(encoded):
    filters, length_codes, remainders, literal_bits, kinds, residues = set(), set(), set(), set(), set(), set()
    partial = across_rows = False
    for name, img, ch, R, flags, png, trace in encoded:
        filters |= set(trace["filters"])
        row = 1 + img.shape[1] * ch
        for band in trace["bands"]:
            kinds.add(band["kind"])
            partial |= band["rows"] < R and img.shape[0] > R
            if band["kind"] != "fixed":
                continue   # a stored band carries no token
            residues.add(band["bits"] % 8)
            S = band["stream"]
            for kind, v in band["tokens"]:
                if kind == "match":
                    length_codes.add(ref.length_code(v)[0])
                else:
                    literal_bits.add(8 if v < 144 else 9)
            pos = 0
            while pos < len(S):           # the maximal runs of the band's stream, found here on their own
                end = pos
                while end < len(S) and S[end] == S[pos]:
                    end += 1
                m = end - pos - 1
                if m >= 258:
                    remainders.add(m % 258)
                if pos // row != (end - 1) // row:
                    across_rows = True
                pos = end
    assert filters == {0, 1, 2, 3, 4}, filters
    assert length_codes == set(range(29)), sorted(set(range(29)) - length_codes)
    assert {0, 1, 2, 3} <= remainders, remainders
    assert literal_bits == {8, 9}
    assert kinds == {"fixed", "stored"}
    assert partial and across_rows
    assert residues == set(range(8)), residues


def test_crafted_cases_are_what_their_names_say(encoded):
    by = {e[0]: e for e in encoded}
    assert by["each_filter"][6]["filters"] == [0, 1, 2, 3, 4]
    assert by["run_lengths"][6]["filters"] == [1] and by["length_codes"][6]["filters"] == [1]
    lits = [t[1] for t in by["literals_143_144"][6]["bands"][0]["tokens"] if t[0] == "lit"]
    assert 143 in lits and 144 in lits and by["literals_143_144"][6]["bands"][0]["kind"] == "fixed"
    assert all(b["kind"] == "stored" for b in by["noise_rgba_65x9"][6]["bands"])
    zero = by["zero_rgba_64x16"][6]["bands"]
    assert len(zero) == 2 and all(b["tokens"] == [("lit", 0)] + [("match", 258)] * 7 + [("match", 249)] for b in zero)
    assert by["grey_1x1"][6]["bands"][0]["kind"] == "stored"
    assert [b["rows"] for b in by["const200_grey_300x5"][6]["bands"]] == [4, 1]
    tok = by["run_lengths"][6]["bands"][0]["tokens"]
    assert tok.count(("match", 258)) == 4 and ("match", 3) in tok


def test_adler_combine_matches_zlib():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    for cut in (0, 1, 5551, 65521, 69999, 70000):
        got = ref.adler32_combine(zlib.adler32(a[:cut]), zlib.adler32(a[cut:]), len(a) - cut)
        assert got == zlib.adler32(a)
