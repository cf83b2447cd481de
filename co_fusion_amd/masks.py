"""Label masks from files: binary PGM (P5, maxval <= 255), one of the mask formats the reference accepts for its pre-processed
segmentation input (Mask####.png / .pgm).  read_mask also takes 8-bit grey PNG, through the host library's reader (images.py)."""
from __future__ import annotations

import os

import numpy as np


def parse_pgm(data: bytes) -> np.ndarray:
    """bytes of a binary PGM -> u8 [height, width].  Header tokens are separated by whitespace, `#` starts a comment that runs to the
    end of the line, exactly ONE whitespace byte follows maxval, then width * height bytes."""
    pos, tokens = 0, []
    n = len(data)
    while len(tokens) < 4:
        while pos < n and (data[pos:pos + 1].isspace() or data[pos:pos + 1] == b"#"):
            if data[pos:pos + 1] == b"#":
                while pos < n and data[pos:pos + 1] not in (b"\n", b"\r"):
                    pos += 1
            else:
                pos += 1
        start = pos
        while pos < n and not data[pos:pos + 1].isspace() and data[pos:pos + 1] != b"#":
            pos += 1
        if start == pos:
            raise ValueError("PGM: truncated header")
        tokens.append(data[start:pos])
    if tokens[0] != b"P5":
        raise ValueError(f"PGM: magic {tokens[0]!r}, only binary PGM (P5) is supported")
    try:
        width, height, maxval = (int(t) for t in tokens[1:])
    except ValueError:
        raise ValueError("PGM: width, height and maxval must be decimal numbers") from None
    if width <= 0 or height <= 0:
        raise ValueError("PGM: empty image")
    if not 0 < maxval <= 255:
        raise ValueError(f"PGM: maxval {maxval}: label masks are 8 bits (maxval <= 255)")
    if pos >= n or not data[pos:pos + 1].isspace():
        raise ValueError("PGM: no whitespace after maxval")
    pos += 1
    if n - pos < width * height:
        raise ValueError(f"PGM: {n - pos} bytes of pixels, {width * height} expected")
    return np.frombuffer(data, np.uint8, width * height, pos).reshape(height, width).copy()


def read_pgm(path: str) -> np.ndarray:
    with open(path, "rb") as f:
        return parse_pgm(f.read())


def read_mask(path: str) -> np.ndarray:
    """a label mask by its extension: .pgm (parse_pgm) or .png (8-bit grey, images.read_mask_png: the host library's PNG reader)"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".pgm":
        return read_pgm(path)
    if ext == ".png":
        from . import images
        return images.read_mask_png(path)
    raise ValueError(f"{path}: label masks are .pgm or .png files")


def mask_path(directory: str, index: int, prefix: str = "Mask", index_width: int = 4) -> str:
    """<directory>/<prefix><index, zero-padded to index_width>.pgm"""
    return os.path.join(directory, f"{prefix}{index:0{index_width}d}.pgm")
