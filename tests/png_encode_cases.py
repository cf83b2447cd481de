"""The case table of the PNG exporter's tests: (name, image, channels, rows_per_band, flags).  Images are u8 [h, w] (grey) or
[h, w, 4] (RGBA), built from fixed seeds.  tests/test_cpu_png_encode_ref.py asserts from the reference's traces that the table
holds the format's edges; tests/test_png_encode_gpu.py runs every case through the device encoder."""
import numpy as np

from png_encode_ref import CF_PNG_LABELS, _LEN_BASE


def _from_sub_stream(F):
    """the one-row grey image whose Sub-filtered bytes are F (the prefix sums mod 256)"""
    return (np.cumsum(np.asarray(F, np.int64)) & 255).astype(np.uint8).reshape(1, -1)


def _runs(lengths):
    """filtered bytes: runs of the given lengths, of 255 and 1 in turn (a literal of 9 and one of 8 bits; the type byte 1 in front of
    the first run, of 255, stays a run of its own)"""
    F = []
    for k, n in enumerate(lengths):
        F += [255 if k % 2 == 0 else 1] * n
    return F


def _label_blobs():
    rng = np.random.default_rng(5)
    img = np.zeros((12, 67), np.uint8)
    for lab, (y0, y1, x0, x1) in enumerate([(1, 6, 3, 20), (4, 11, 30, 51), (0, 3, 55, 67), (8, 12, 0, 9)], start=1):
        img[y0:y1, x0:x1] = lab
    img[6, 25:29] = 255          # rejected: written as 0 under CF_PNG_LABELS
    img[rng.integers(0, 12, 5), rng.integers(0, 67, 5)] = 255
    return img


def _each_filter():
    """five rows of 24 grey pixels, one per filter type in order: None by a tie with Up (the row above the image is zero), Sub on a
    ramp, Up on a copy of the ramp (a tie with Paeth: the lowest type takes it), Average and Paeth on rows that are their own
    predictions plus one small step"""
    w = 24
    img = np.zeros((5, w), np.int64)
    img[0] = [(1, 255, 2, 254, 3, 253)[i % 6] for i in range(w)]
    img[1] = [(7 + 10 * i) & 255 for i in range(w)]
    img[2] = img[1]
    for i in range(w):
        a = img[3, i - 1] if i else 0
        img[3, i] = (((a + img[2, i]) >> 1) + (1 if i % 5 == 0 else 0)) & 255
    for i in range(w):
        a = img[4, i - 1] if i else 0
        b = img[3, i]
        c = img[3, i - 1] if i else 0
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
        img[4, i] = (pred + (37 if i == 0 else (2 if i % 7 == 3 else 0))) & 255
    return img.astype(np.uint8)


def _literals_143_144():
    img = np.zeros((4, 40), np.uint8)
    img[1, 0] = 143
    img[3, 0] = 144
    return img


def _widest():
    rng = np.random.default_rng(9)
    img = np.zeros((2, 1280, 4), np.uint8)
    img[:, 100:400] = (40, 80, 120, 255)
    img[1, 700:760] = rng.integers(0, 256, (60, 4), dtype=np.uint8)
    img[:, 1279] = (255, 254, 253, 252)
    return img


def _residue(j):
    """one grey row of 64: j literals of 9 bits, then a run of zeros (9 j + a constant bits: j = 1..8 leave every residue mod 8)"""
    return _from_sub_stream([255 if k % 2 == 0 else 254 for k in range(j)] + [0] * (64 - j))


def cases():
    rng = np.random.default_rng(1)
    out = [
        ("grey_1x1", np.array([[7]], np.uint8), 1, 8, 0),
        ("rgba_3x2", rng.integers(0, 256, (2, 3, 4), dtype=np.uint8), 4, 8, 0),
        ("zero_rgba_64x16", np.zeros((16, 64, 4), np.uint8), 4, 8, 0),
        ("const200_grey_300x5", np.full((5, 300), 200, np.uint8), 1, 4, 0),
        ("label_blobs_67x12", _label_blobs(), 1, 5, CF_PNG_LABELS),
        ("run_lengths", _from_sub_stream(_runs([3, 4, 259, 260, 261, 262])), 1, 1, 0),
        ("length_codes", _from_sub_stream(_runs([n + 1 for n in _LEN_BASE])), 1, 1, 0),
        ("literals_143_144", _literals_143_144(), 1, 4, 0),
        ("noise_rgba_65x9", rng.integers(0, 256, (9, 65, 4), dtype=np.uint8), 4, 4, 0),
        ("each_filter", _each_filter(), 1, 2, 0),
        ("widest_rgba_1280x2", _widest(), 4, 8, 0),
    ]
    out += [("residue_%d" % j, _residue(j), 1, 1, 0) for j in range(1, 9)]
    return out
