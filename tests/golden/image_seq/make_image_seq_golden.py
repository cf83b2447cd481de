"""Regenerates the fixtures of tests/image_cases.py.  Needs PIL (the tests do not): every PNG is written by
co_fusion_amd.images.png_bytes and decoded by PIL -- the .npy beside it is PIL's answer (colour as RGB u8 [H, W, 3], depth as u16
[H, W], masks as u8 [H, W]).  OpenEXR files are written by co_fusion_amd.images.exr_bytes; no independent OpenEXR decoder was
available, so their .npy is the plane the writer was given (see README.md here).

    python tests/golden/image_seq/make_image_seq_golden.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import image_cases as ic  # noqa: E402


def main():
    for name in ic.PNG_CASES:
        data, img, pal = ic.png_make(name)
        im = Image.open(io.BytesIO(data))
        im.load()
        role = ic.png_role(name)
        if role == ic.ROLE_COLOR:
            got = np.asarray(im.convert("RGB"), np.uint8)
            want = pal[img] if pal is not None else (np.repeat(img[..., None], 3, 2) if img.ndim == 2 else img[..., :3])
        elif role == ic.ROLE_DEPTH:
            assert im.mode in ("I;16", "I;16B", "I"), im.mode
            got = np.asarray(im).astype(np.uint16)
            want = img
        else:
            assert im.mode == "L", im.mode
            got = np.asarray(im, np.uint8)
            want = img
        assert np.array_equal(got, want), f"{name}: PIL does not read back what the writer was given"
        with open(os.path.join(HERE, name + ".png"), "wb") as f:
            f.write(data)
        np.save(os.path.join(HERE, name + ".npy"), got)
    for name in ic.EXR_CASES:
        data, want = ic.exr_make(name)
        kinds = [size == full for _, size, full, _ in ic.exr_blocks_numpy(data)]
        noise = ic.EXR_CASES[name][5]
        # which blocks the file stores raw: all of a noise image, the head of a mixed one, none of the large smooth ones (a short
        # scanline of a ZIPS file may go either way: deflate's overhead can exceed what it saves)
        if noise == "all":
            assert all(kinds), (name, kinds)
        elif noise == "head":
            assert kinds == [True] + [False] * (len(kinds) - 1), (name, kinds)
        elif ic.EXR_CASES[name][4] == ic.EXR_ZIP:
            assert not any(kinds), (name, kinds)
        assert ic.exr_decode_numpy(data).tobytes() == want.tobytes(), name
        with open(os.path.join(HERE, name + ".exr"), "wb") as f:
            f.write(data)
        np.save(os.path.join(HERE, name + ".npy"), want)
    print("wrote", len(ic.PNG_CASES), "PNG and", len(ic.EXR_CASES), "OpenEXR fixtures")


if __name__ == "__main__":
    main()
