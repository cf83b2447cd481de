#!/usr/bin/env python
"""Writes the JPEG fixtures of the log player's tests (tests/golden/klg_player/): a handful of small baseline JPEG streams and, for
each, the RGB that libjpeg decodes it to (Pillow bundles libjpeg-turbo: islow IDCT, fancy upsampling), as <name>.jpg / <name>.npy.
The tests read only these files, so they do not depend on Pillow being importable.  Run once, by hand, where Pillow is installed:

    python tools/make_klg_player_fixtures.py

The pictures are procedural (smooth ramps, saturated rectangles, a little noise): the saturated patches next to dark ones drive the
IDCT's and the colour conversion's clamps, the ramps exercise the chroma filter.  Sizes: one MCU; 6.5 x 4.5 MCUs (padded right and
bottom edge); odd width and height (the fancy filter's last column ends on an even x, against an odd x for the even widths).

scene_160x128_<t>.jpg are the colour frames t = 0..7 of synth.Scene(n_obj=1) at 160 x 128 (quality 90, 4:2:0, what bench.py's
klg_input leg writes): with the depth the same scene renders, they make the short log the player's end-to-end test plays."""
import io
import os

import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "klg_player")

# name, width, height, mode, Pillow save options
CASES = [
    ("mcu_16x16_420", 16, 16, "RGB", dict(subsampling=2)),
    ("edge_104x72_420", 104, 72, "RGB", dict(subsampling=2)),
    ("odd_101x77_420", 101, 77, "RGB", dict(subsampling=2)),
    ("odd_101x77_422", 101, 77, "RGB", dict(subsampling=1)),
    ("edge_104x72_444", 104, 72, "RGB", dict(subsampling=0)),
    ("grey_64x48", 64, 48, "L", dict()),
    ("restart_64x48_420", 64, 48, "RGB", dict(subsampling=2, restart_marker_blocks=2)),
]


def picture(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 127 + 127 * np.sin(x / 5.0) * np.cos(y / 7.0)], -1)
    for k, colour in enumerate([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255), (0, 0, 0), (255, 255, 0), (255, 0, 255)]):
        x0, y0 = (k * 13) % max(w - 6, 1), (k * 11) % max(h - 5, 1)
        img[y0:y0 + 5 + k, x0:x0 + 6 + k] = colour
    img += rng.normal(0, 6, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def main():
    os.makedirs(OUT, exist_ok=True)
    for k, (name, w, h, mode, opts) in enumerate(CASES):
        rgb = picture(w, h, 100 + k)
        im = Image.fromarray(rgb).convert(mode)
        buf = io.BytesIO()
        im.save(buf, format="JPEG", quality=90, **opts)
        jb = buf.getvalue()
        ref = np.asarray(Image.open(io.BytesIO(jb)).convert("RGB"))
        assert ref.shape == (h, w, 3)
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(jb)
        np.save(os.path.join(OUT, name + ".npy"), ref)
        print(f"{name}: {len(jb)} B JPEG, {ref.nbytes} B RGB")
    from co_fusion_amd import synth
    cam, sc = synth.Camera.scaled(160, 128), synth.Scene(n_obj=1)
    for t in range(8):
        buf = io.BytesIO()
        Image.fromarray(sc.render(cam, t, noise=True)[1]).save(buf, format="JPEG", quality=90, subsampling=2)
        with open(os.path.join(OUT, f"scene_160x128_{t}.jpg"), "wb") as f:
            f.write(buf.getvalue())
        print(f"scene_160x128_{t}: {len(buf.getvalue())} B JPEG")


if __name__ == "__main__":
    main()
