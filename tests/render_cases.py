"""The case table of the scene renderer (csrc/render.hip, DESIGN.md "Scene rendering"; plain helper module, no tests in here).

A case is a list of calls on ONE render object: each call is a view, items in draw order and the outputs asked for.  The GPU side
(tests/test_render_cases_gpu.py) runs every case's calls in order on one shared 96x64 render object, so that what one call leaves behind
(ray cache, key buffer, overflow count, staging slot) meets the next, and compares every output byte for byte with the restatement
tests/render_ref.py and, under the rules below, with the independent f64 statement tests/render_oracle.py.  The CPU side
(tests/test_cpu_render_cases.py) shows from the two statements alone that they agree and that every case reaches what it `aims` at.

Views: 96x64 (6144 pixels, exactly 24 workgroups) and 83x45 (3735 pixels: odd width, partial last workgroup).  View A is fx = fy = 80,
cx = 48, cy = 32, identity pose, near 0.1, far 1000; at z = 1 a pixel is 1 / 80 m.  Every case is seeded from its name.

Selection and colour
 * conf_at_threshold: conf equal to the threshold and its two f32 neighbours, without and with UNSTABLE, all five modes at once.
 * window_boundary: tick - last_time equal to time_delta, one less, one more; WINDOW on and off.
 * times_ramp: tick 0 and 1; tick 3 with init_time 0, 2 (t == 0.5 exactly), just below 2, 3, and 5 (> tick).
 * palette_ids: ids 0, 15, 16, 17, 254 in label mode; 16 has the colour of 0 and its own label; 254 is not the empty 255.
 * item_mode_and_eight_outputs: items of all five modes; ITEM_MODE and seven fixed modes, depth and labels in one call.
 * colour_bytes: 256 surfels carry byte b, b + 85, b + 170 (mod 256) in the three channels; COLOUR returns the bytes; under WINDOW
   (every surfel outside the window) b / 4 is half-way for b % 4 == 2.
 * phong_facing: normals towards the camera, away from it, grazing; the specular term saturates on the optical axis.
Item table
 * item_table_edges: counts 0, 1, 63, 0, 0, 64, 65, 0; every item its own pose, threshold, id and mode.
 * max_items: 256 items of 1-3 surfels; items 100, 102 and 103 hold the same surfel under the same pose around the empty item 101.
 * all_empty_after_full: three empty items (no raster launch) after an ordinary call: the images are empty.
Footprints (the CPU test asserts the box sizes from the restatement's _setup)
 * narrow_boxes: boxes of 1x1, 2x2, 3x3, 5x5, 1x2, 2x1, 3x2 and 4x5 pixels (narrower than a surfel's four lanes).
 * path_switch: one fronto-parallel surfel at three offsets: boxes of 16x16 = 256 (four lanes), 16x17 and 17x17 (overflow list).
 * tile_seam: boxes of 4096 (64x64, one full tile) and 4100 (82x50, the smallest two-tile box a 96x64 view can hold) on the shared
   object.
 * tile_seam_whole_views: boxes of exactly 4097 = 241x17 and 8193 = 2731x3 pixels (two and three tiles, the seams mid-row) as whole
   views of a second, wide render object -- no box of 4097 or 8193 pixels fits into 96x64 (4097 = 17 * 241, 8193 = 3 * 2731).
 * clipped: boxes cut at each edge and corner, below 257 pixels (four lanes) and above (overflow list); again at 83x45.
 * outside_or_barely_inside: surfels wholly outside on each side; a quad that reaches in by 0.3 pixel (no box) and by 0.495 pixel (a box
   of one column, no fragment).
 * full_view: one surfel covers every pixel.
Planes and degenerates
 * near_far: a quad corner at z == near (skipped) and at near's upper neighbour (drawn); a fronto-parallel surfel at z == far (the pixel
   on the optical axis is empty) and at far's lower neighbour (covered); near = far = 0 select 0.1 and 1000.
 * degenerate: zero normal, NaN in position / normal / radius, inf position, radius 0, negative radius (drawn as |r|), a radius below
   the pixel pitch on and off a pixel centre, a plane through the camera centre (edge-on), a grazing plane, a surfel behind the camera,
   and a normal with n.x == 0, n.y == n.z (the quad's x axis has no direction: not drawn) -- between ordinary surfels.
Views
 * f64_matrix: view and model poses with rotation and tens of metres of translation; an f32 V * Tp differs.
 * odd_intrinsics: cx, cy outside the image, fx != fy, and a view with negative fy.
Sequences on one object
 * ray_cache: view A; A with only cx changed; A; A's intrinsics at 83x45; 96x64 again.
 * back_to_back: three calls with different item tables and output buffers; the GPU test enqueues all calls of a case before it reads
   any (Renderer.render does not wait), the third call reuses staging slot 0.
 * overflow_list_full: 2^18 + 2^12 + 64 surfels, all with boxes above 256 pixels.  Block 0 (40 surfels, four of them above 4096 pixels)
   is repeated exactly to 2^18 + 2^12, so whichever surfel straddles the cap of the overflow list is a copy, and copies lose every tie
   to block 0; the last 64 surfels (the last workgroup) are distinct and nearest, so a surfel the full list drops would be missed.
   Expected: the render of block 0 and the tail alone.  Two ordinary calls follow, enqueued while the first is still running: the
   overflow count has to be reset (surfels below the threshold lie in front, which a stale list entry would draw), and the second of
   them must not overwrite the staged item table of the first.

DEPTH_MEASURED is the largest relative depth difference between the restatement (f32, fixed order) and the oracle (f64) over every
unambiguous pixel of the whole table; DEPTH_BOUND = 4 x that is what both test files allow.

NOT COVERED, so that nobody takes the table for complete: views above 96x64 other than the two whole-view seams; more than 2^32 - 1
surfels and the other refusals (tests/test_render_gpu.py); non-finite confidence, colour or time fields and an infinite radius; a
non-rigid or scaled pose; three tiles inside a larger view; a list that fills while tiles of 4096 pixels are half written by several
surfels at once (which surfel straddles the cap is the hardware's choice); frame-loop lanes running beside a render.
"""
from __future__ import annotations

import dataclasses
import functools
import zlib

import numpy as np

import render_ref as rr

f32 = np.float32
UNSTABLE, WINDOW, PHONG = rr.UNSTABLE, rr.WINDOW, rr.PHONG
GREY, NORMALS, COLOUR, TIMES, LABEL, ITEM_MODE = rr.GREY, rr.NORMALS, rr.COLOUR, rr.TIMES, rr.LABEL, rr.ITEM_MODE
ALL_MODES = (GREY, NORMALS, COLOUR, TIMES, LABEL)
SIZE, SMALL = (96, 64), (83, 45)
WIDE = (2731, 17)                       # the second render object (tile_seam_whole_views)
K_BIG_AREA, K_TILE, K_BIG_CAP = 256, 4096, 1 << 18
I4 = np.eye(4, dtype=np.float32)

# measured by tests/test_cpu_render_cases.py::test_depth_bound_is_the_measured_one over the whole table (restatement against oracle,
# relative, unambiguous pixels); the bound is 4 x the measurement: the restatement is f32 in a fixed order, the factor covers later cases
DEPTH_MEASURED = 1.22e-6
DEPTH_BOUND = 4 * DEPTH_MEASURED


@dataclasses.dataclass
class Call:
    view: dict
    items: list
    modes: tuple = (ITEM_MODE,)
    depth: bool = True
    labels: bool = True
    ref_items: list = None          # what the expected images are rendered from (default: items)
    exempt: tuple = ()              # draw indices (of ref_items) put on a boundary on purpose
    drawn: tuple = ()               # hand-stated: draw indices that win at least one pixel
    not_drawn: tuple = ()           # hand-stated: draw indices that win none
    probes: tuple = ()              # hand-stated: (px, py, label) -- 255 is empty
    note: str = ""

    def outputs(self):
        return [("rgba", m) for m in self.modes] + ([("depth",)] if self.depth else []) + ([("labels",)] if self.labels else [])

    def expected_items(self):
        return self.items if self.ref_items is None else self.ref_items


@dataclasses.dataclass
class Case:
    name: str
    aims: str
    calls: list
    size: tuple = SIZE              # the render object's maximum


def view(width=96, height=64, fx=80.0, fy=80.0, cx=48.0, cy=32.0, pose=I4, **kw):
    return dict(pose=np.asarray(pose, np.float32), fx=fx, fy=fy, cx=cx, cy=cy, width=width, height=height, **kw)


def item(surfels, pose=I4, thresh=1.0, model_id=0, mode=COLOUR):
    return dict(surfels=np.asarray(surfels, np.float32).reshape(-1, 12), pose=np.asarray(pose, np.float32), thresh=thresh,
                model_id=model_id, mode=mode)


def surfel(p, n=(0, 0, -1), r=0.05, conf=5.0, colour=0x808080, init=1, last=1, unit=True):
    s = np.zeros(12, np.float32)
    n = np.asarray(n, float)
    s[:3] = p; s[3] = conf; s[4] = colour; s[6] = init; s[7] = last
    s[8:11] = n / np.linalg.norm(n) if unit else n
    s[11] = r
    return s


def at_px(v, X, Y, z, hp, **kw):
    """a fronto-parallel surfel whose centre projects to (X, Y) (pixel i's centre is i + 0.5) and whose quad reaches hp pixels to
    each side: its box holds the pixels i with X - hp - 0.51 <= i <= X + hp - 0.49"""
    return surfel(((X - v["cx"]) / v["fx"] * z, (Y - v["cy"]) / v["fy"] * z, z), kw.pop("n", (0, 0, -1)), hp * z / (abs(v["fx"]) * np.sqrt(2.0)),
                  **kw)


def boxed(v, a, b, w, h, z, L=None, **kw):
    """a fronto-parallel surfel whose box is exactly the pixels [a, a + w) x [b, b + h): the box interval is L = 2 hp + 0.02 long
    and holds floor(L) or floor(L) + 1 integers; L defaults to max(w, h) - 0.5"""
    L = (max(w, h) - 0.5) if L is None else L
    hp = (L - 0.02) / 2
    n_lo = int(np.floor(L))

    def centre(first, count):
        # interval [s, s + L] with s = first - frac: holds n_lo + 1 integers when frac <= L - n_lo, else n_lo
        frac = 0.25 if count == n_lo + 1 else 0.75
        assert count in (n_lo, n_lo + 1), (count, L)
        return first - frac + 0.51 + hp
    return at_px(v, centre(a, w), centre(b, h), z, hp, **kw)


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(ax=0.0, ay=0.0, az=0.0, t=(0, 0, 0)):
    T = np.eye(4); T[:3, :3] = rot(ax, ay, az); T[:3, 3] = t
    return T.astype(np.float32)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def scatter(rng, v, n, z=(0.8, 2.5), r_px=(2.0, 7.0), tilt=0.4, tick=30):
    """n ordinary surfels spread over the view: random depth, tilted normals, colours, times and confidences (above 1.5)"""
    S = np.zeros((n, 12), np.float32)
    zz = rng.uniform(*z, n)
    X = rng.uniform(0, v["width"], n); Y = rng.uniform(0, v["height"], n)
    S[:, 0] = (X - v["cx"]) / v["fx"] * zz; S[:, 1] = (Y - v["cy"]) / v["fy"] * zz; S[:, 2] = zz
    S[:, 3] = rng.uniform(1.5, 20.0, n)
    S[:, 4] = rng.integers(0, 1 << 24, n).astype(np.float32)
    S[:, 6] = rng.integers(1, tick + 1, n); S[:, 7] = rng.integers(1, tick + 1, n)
    nrm = rng.normal(size=(n, 3)) * tilt + np.array([0, 0, -1.0])
    S[:, 8:11] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    S[:, 11] = rng.uniform(*r_px, n) * zz / abs(v["fx"])
    return S


def row_of(v, count, z=1.0, hp=6.0, y=32.0, **kw):
    """n fronto-parallel surfels side by side in a row, apart from each other"""
    return [at_px(v, (k + 0.5) * v["width"] / count + 0.3, y + 0.3, z, hp, **kw) for k in range(count)]


RED, GREEN, BLUE = 0xFF0000, 0x00FF00, 0x0000FF


def _conf_at_threshold(name):
    v = view(tick=10)
    t = f32(10.0)
    confs = (np.nextafter(t, f32(-np.inf)), t, np.nextafter(t, f32(np.inf)))
    S = row_of(v, 3)
    for s, c, col, init in zip(S, confs, (RED, GREEN, BLUE), (2, 5, 9)):
        s[3] = c; s[4] = col; s[6] = init
    S[0][8:11] = surfel((0, 0, 1), (0.3, 0.2, -1))[8:11]
    it = [item(S, thresh=float(t), model_id=3, mode=COLOUR)]
    return [Call(dict(v, flags=0), it, ALL_MODES, drawn=(2,), not_drawn=(0, 1), note="stable only"),
            Call(dict(v, flags=UNSTABLE), it, ALL_MODES, drawn=(0, 1, 2), note="unstable too: 0 and 1 in the times colour")]


def _window_boundary(name):
    v = view(tick=20, time_delta=5)
    S = row_of(v, 3, colour=0xC8C8C8)
    for s, last in zip(S, (15, 16, 14)):          # tick - last = 5 (== delta: not dimmed), 4, 6 (dimmed)
        s[7] = last
    it = [item(S)]
    return [Call(dict(v, flags=WINDOW), it, (COLOUR, GREY), drawn=(0, 1, 2)), Call(dict(v, flags=0), it, (COLOUR, GREY), drawn=(0, 1, 2))]


def _times_ramp(name):
    v = view()
    inits = (0.0, 2.0, float(np.nextafter(f32(2.0), f32(0.0))), 3.0, 5.0, 1.0)
    S = row_of(v, 6, hp=5.0)
    for s, i in zip(S, inits):
        s[6] = i
    it = [item(S, mode=TIMES)]
    return [Call(dict(v, tick=tick), it, (ITEM_MODE,), drawn=tuple(range(6))) for tick in (0, 1, 3)]


def _palette_ids(name):
    v = view()
    ids = (0, 15, 16, 17, 254)
    S = row_of(v, 5, hp=5.0, n=(0.2, 0.1, -1))
    items = [item([s], model_id=i, mode=LABEL) for s, i in zip(S, ids)]
    probes = tuple((int((k + 0.5) * 96 / 5), 32, i) for k, i in enumerate(ids)) + ((0, 0, 255),)
    return [Call(v, items, (ITEM_MODE, LABEL), probes=probes)]


def _item_mode_and_eight_outputs(name):
    rng = _rng(name)
    v = view(tick=30, time_delta=10)
    items = [item(scatter(rng, v, 12), pose(0.02 * m, -0.03 * m, 0.01, (0.01 * m, 0, 0.02 * m)), thresh=1.0, model_id=m + 1, mode=m)
             for m in ALL_MODES]
    modes = (ITEM_MODE, GREY, NORMALS, COLOUR, TIMES, LABEL, GREY, NORMALS)
    return [Call(v, items, modes), Call(dict(v, flags=UNSTABLE | WINDOW | PHONG), items, modes)]


def _colour_bytes(name):
    v = view(tick=20, time_delta=5)
    S = []
    for b in range(256):
        col = (b << 16) | (((b + 85) & 255) << 8) | ((b + 170) & 255)
        S.append(at_px(v, (b % 16) * 6 + 3.5, (b // 16) * 4 + 2.5, 1.0 + 0.001 * b, 1.6, colour=col, last=3))
    it = [item(S)]
    return [Call(dict(v, flags=0), it, (COLOUR,), drawn=tuple(range(256))), Call(dict(v, flags=WINDOW), it, (COLOUR,), drawn=tuple(range(256)))]


def _phong_facing(name):
    v = view(cx=48.5, cy=32.5)
    S = [at_px(v, 48.5, 32.5, 1.0, 9.0, colour=0x404040),                                    # on the axis, facing: specular saturates
         surfel((-0.35, -0.2, 1.2), (0.1, 0.2, 1), 0.09, colour=0xA0A0A0),                 # facing away: flipped
         surfel((0.36, -0.2, 1.1), (1, 0.1, -0.25), 0.12, colour=0xE0E0E0),                # grazing
         surfel((-0.33, 0.21, 1.0), (-0.5, 0.3, -1), 0.1, colour=0x2060C0),
         surfel((0.33, 0.2, 0.9), (0.4, -0.4, 1), 0.09, colour=0xC06020)]                  # away and tilted
    it = [item(S, mode=COLOUR)]
    return [Call(dict(v, flags=PHONG), it, (COLOUR, GREY, LABEL), drawn=(0, 1, 2, 3, 4)), Call(dict(v, flags=0), it, (COLOUR, GREY, LABEL))]


def _item_table_edges(name):
    rng = _rng(name)
    v = view(tick=30, time_delta=10)
    counts = (0, 1, 63, 0, 0, 64, 65, 0)
    items = []
    for k, c in enumerate(counts):
        S = scatter(rng, v, c, r_px=(1.5, 4.0))
        S[: c // 3, 3] = rng.uniform(0.0, 1.0 + 0.2 * k, c // 3)          # some below the item's own threshold
        if c:                                                              # the item's first and last surfel are in plain sight
            S[0] = at_px(v, 8.3 + 11 * k, 8.3, 0.5, 3.0, conf=19.0, colour=0x203040 * k, init=3, last=25)
            S[-1] = at_px(v, 8.3 + 11 * k, 54.3, 0.5, 3.0, conf=19.0, colour=0x302010 * k, init=28, last=2)
        items.append(item(S, pose(0.01 * k, -0.02 * k, 0.03 * k, (0.02 * k, -0.01 * k, 0.03 * k)), thresh=1.0 + 0.2 * k, model_id=20 + 7 * k,
                          mode=ALL_MODES[k % 5]))
    return [Call(dict(v, flags=f), items, (ITEM_MODE, LABEL)) for f in (0, UNSTABLE)]


def _max_items(name):
    rng = _rng(name)
    v = view()
    items = []
    tie = at_px(v, 20.3, 40.3, 0.7, 6.0, colour=RED)
    for k in range(256):
        if k in (100, 102, 103):
            S = [tie]
        elif k == 101:
            S = np.zeros((0, 12), np.float32)
        else:
            S = scatter(rng, v, 1 + k % 3, z=(0.9, 2.5), r_px=(1.5, 3.5))
        items.append(item(S, I4 if 100 <= k <= 103 else pose(0, 0, 0.002 * k, (0, 0, 0.001 * k)), model_id=k % 255, mode=ALL_MODES[k % 5]))
    items[102]["surfels"][0, 4] = RED                                          # identical rows: the tie is exact in every statement
    return [Call(v, items, (ITEM_MODE, LABEL), probes=((20, 40, 100),))]


def _all_empty_after_full(name):
    rng = _rng(name)
    v = view()
    full = [item(scatter(rng, v, 40), model_id=4)]
    empty = [item(np.zeros((0, 12), np.float32), model_id=k) for k in (1, 2, 3)]
    return [Call(v, full, (COLOUR,)), Call(v, empty, (COLOUR, LABEL), probes=((0, 0, 255), (48, 32, 255), (95, 63, 255))),
            Call(v, full, (COLOUR,))]


NARROW = ((1, 1), (2, 2), (3, 3), (5, 5), (1, 2), (2, 1), (3, 2), (4, 5))


def _narrow_boxes(name):
    v = view()
    S = []
    for k, (w, h) in enumerate(NARROW):
        S.append(boxed(v, 6 + 11 * k, 10 + 5 * k, w, h, 1.0 + 0.01 * k, L=max(w, h) - (0.5 if w == h else 0.4), colour=0x102030 * (k + 1)))
    return [Call(v, [item(S)], (COLOUR,))]


PATH_SWITCH = ((16, 16), (16, 17), (17, 17))


def _path_switch(name):
    v = view()
    return [Call(v, [item([boxed(v, 30, 20, w, h, 1.0, L=16.5, colour=0x40A0F0)])], (COLOUR,), drawn=(0,)) for w, h in PATH_SWITCH]


def _tile_seam(name):
    v = view()
    one = boxed(v, 16, 0, 64, 64, 1.0, L=64.5, colour=0x30C060)                 # 64 x 64 = 4096: one full tile
    v2 = view(cx=44.0, cy=40.0)
    two = boxed(v2, 7, 14, 82, 83, 1.0, L=82.5, colour=0xC03060)                # 82 wide, rows 14.. clipped at 63: 82 x 50 = 4100
    return [Call(v, [item([one])], (COLOUR,), drawn=(0,)), Call(v2, [item([two])], (COLOUR,), drawn=(0,))]


SEAM_VIEWS = ((241, 17), (2731, 3))


def _tile_seam_whole_views(name):
    calls = []
    for W, H in SEAM_VIEWS:
        vw = view(W, H, cx=W / 2 + 0.25, cy=H / 2 + 0.25)
        big = surfel((0.013, 0.007, 1.0), (0, 0, -1), 40.0, colour=0x6030C0)
        small = at_px(vw, W - 3.2, 1.7, 0.8, 2.0, colour=0xF0F000)
        calls.append(Call(vw, [item([big, small])], (COLOUR,), drawn=(0, 1)))
    return calls


def _clipped_surfels(v, hp, z):
    W, H = v["width"], v["height"]
    xs = (1.3, W / 2 + 0.3, W - 1.3); ys = (1.3, H / 2 + 0.3, H - 1.3)
    return [at_px(v, X, Y, z + 0.01 * (3 * j + i), hp, colour=0x1F2F3F * (3 * j + i + 1)) for j, Y in enumerate(ys) for i, X in enumerate(xs)
            if (i, j) != (1, 1)]


def _clipped(name):
    calls = []
    for v in (view(), view(*SMALL, cx=41.5, cy=22.5)):
        S = _clipped_surfels(v, 5.0, 1.0) + _clipped_surfels(v, 20.0, 2.0)
        calls.append(Call(v, [item(S)], (COLOUR,), drawn=tuple(range(16))))
    return calls


def _outside_or_barely_inside(name):
    v = view()
    out = [at_px(v, -12.0, 30.3, 1.0, 6.0), at_px(v, 108.0, 30.3, 1.0, 6.0), at_px(v, 40.3, -12.0, 1.0, 6.0), at_px(v, 40.3, 76.0, 1.0, 6.0)]
    barely = [at_px(v, 0.3 - 4.0, 20.3, 1.0, 4.0), at_px(v, 0.495 - 4.0, 40.3, 1.0, 4.0)]      # the quad's right corner at x = 0.3, 0.495
    ordinary = [at_px(v, 50.3, 30.3, 1.2, 8.0, colour=RED)]
    return [Call(v, [item(out + barely + ordinary, model_id=9)], (COLOUR,), drawn=(6,), not_drawn=(0, 1, 2, 3, 4, 5))]


def _full_view(name):
    v = view()
    return [Call(v, [item([surfel((0.01, 0.02, 1.5), (0.1, -0.05, -1), 3.0, colour=0x55AA33)], model_id=7)], (COLOUR, NORMALS), drawn=(0,))]


def corner_z(s, v, M=I4):
    """the smallest quad-corner z of surfel row s as the restatement computes it: the f32 value zc for which the surfel is skipped at
    near == zc and set up at near's lower neighbour"""
    lo, hi = f32(1e-6).view(np.uint32), f32(1e6).view(np.uint32)      # positive f32 order as their bit patterns

    def ok(bits):
        with np.errstate(all="ignore"):
            return bool(rr._setup(np.asarray(s, np.float32).reshape(1, 12), np.asarray(M, np.float32), v, np.uint32(bits).view(f32))[0][0])
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = np.uint32((int(lo) + int(hi)) // 2)
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return np.uint32(hi).view(f32)


def _near_far(name):
    v = view(cx=48.5, cy=32.5)
    tilted = surfel((-0.2, 0.05, 1.0), (0.5, 0.2, -1), 0.15, colour=RED)
    other = at_px(v, 70.3, 40.3, 1.5, 6.0, colour=GREEN)
    zc = corner_z(tilted, v)
    below = np.nextafter(zc, f32(0.0))
    far = f32(4.0)
    at_far = at_px(v, 48.5, 32.5, float(far), 9.0, colour=BLUE)
    under_far = at_px(v, 48.5, 32.5, float(np.nextafter(far, f32(0.0))), 9.0, colour=BLUE)
    dflt = [surfel((0.0, 0.0, 0.15), r=0.005, colour=RED), surfel((0.05, 0.0, 0.09), r=0.002), surfel((3.0, 2.0, 999.0), r=60.0, colour=GREEN),
            surfel((-300.0, -200.0, 1001.0), r=60.0)]
    return [Call(dict(v, near=float(zc), far=10.0), [item([tilted, other], model_id=1)], (COLOUR,), exempt=(0,), drawn=(1,), not_drawn=(0,),
                 note="corner at near"),
            Call(dict(v, near=float(below), far=10.0), [item([tilted, other], model_id=1)], (COLOUR,), exempt=(0,), drawn=(0, 1),
                 note="corner at near's upper neighbour"),
            Call(dict(v, near=0.2, far=float(far)), [item([at_far, other], model_id=2)], (COLOUR,), exempt=(0,), probes=((48, 32, 255),),
                 note="z == far"),
            Call(dict(v, near=0.2, far=float(far)), [item([under_far, other], model_id=2)], (COLOUR,), exempt=(0,), probes=((48, 32, 2),),
                 note="z just below far"),
            Call(dict(v, near=0.0, far=0.0), [item(dflt, model_id=3)], (COLOUR,), drawn=(0, 2), not_drawn=(1, 3), note="defaults")]


DEGENERATE = ("zero normal", "NaN position", "NaN normal", "NaN radius", "inf position z", "inf position x", "radius 0", "negative radius",
              "sub-pixel radius off a centre", "sub-pixel radius on a centre", "edge-on", "grazing", "behind the camera", "n.x == 0, n.y == n.z")


def _degenerate(name):
    rng = _rng(name)
    v = view(cx=47.5, cy=31.5)
    nan, inf = np.nan, np.inf
    S = [surfel((-0.4, -0.3, 1.0), (0, 0, 0), 0.05, unit=False),
         surfel((nan, -0.3, 1.0)), surfel((-0.2, -0.3, 1.0), (0, nan, -1), unit=False), surfel((-0.1, -0.3, 1.0), r=nan),
         surfel((0.0, 0.0, inf)), surfel((inf, 0.1, 1.0)),
         surfel((0.1, -0.3, 1.0), r=0.0),
         at_px(v, 70.3, 8.3, 0.6, 5.0, colour=RED),
         at_px(v, 20.0, 50.0, 1.0, 0.3), at_px(v, 30.5, 50.5, 0.5, 0.3, colour=GREEN),
         surfel((0.0, 0.1, 1.0), (1, 0, 0), 0.3), surfel((0.2, 0.1, 1.0), (1, 0, 0.05), 0.2, colour=BLUE),
         surfel((0.1, 0.1, -1.0), (0, 0, 1)),
         surfel((0.3, 0.3, 1.0), (0, -1, -1), 0.08)]
    S[7][11] = -S[7][11]
    S[6][0] += 0.003                                                                    # (not through a pixel centre)
    assert len(S) == len(DEGENERATE)
    S = np.array(S + list(scatter(rng, v, 30)))
    return [Call(v, [item(S, model_id=5)], (COLOUR, NORMALS), drawn=(7, 9, 11), not_drawn=(0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 13))]


def _f64_matrix(name):
    rng = _rng(name)
    local = view()
    calls = []
    for k, (ang, t) in enumerate((((0.7, -1.1, 0.4), (31.7, -22.3, 45.1)), ((-2.1, 0.3, 1.9), (-57.9, 63.2, -38.6)))):
        Tp = pose(*ang, t)                                                              # model -> world, tens of metres away
        off = pose(0.05 * (k + 1), -0.04, 0.03, (0.03, -0.02, -0.1))                    # camera in the model's frame
        C = (Tp.astype(float) @ off.astype(float)).astype(np.float32)
        S = scatter(rng, local, 40, z=(1.0, 2.5))
        calls.append(Call(view(pose=C), [item(S, Tp, model_id=k + 1, mode=NORMALS)], (ITEM_MODE, COLOUR)))
    return calls


def _odd_intrinsics(name):
    rng = _rng(name)
    calls = []
    for kw in (dict(fx=70.0, fy=95.0, cx=-20.0, cy=90.0), dict(fx=61.0, fy=-80.0, cx=120.5, cy=-13.25),
               dict(width=83, height=45, fx=55.0, fy=-47.0, cx=41.0, cy=22.0)):
        v = view(**kw)
        calls.append(Call(v, [item(scatter(rng, v, 40), model_id=2)], (COLOUR, NORMALS)))
    return calls


def _ray_cache(name):
    rng = _rng(name)
    A = view()
    it = [item(scatter(rng, A, 40), model_id=1)]
    return [Call(v, it, (COLOUR,)) for v in (A, view(cx=51.0), A, view(*SMALL), A)]


def _back_to_back(name):
    rng = _rng(name)
    v = view()
    calls = []
    for k in range(3):
        items = [item(scatter(rng, v, 10 + 7 * k + j), pose(0, 0, 0.01 * j, (0, 0, 0.05 * j)), model_id=10 * k + j, mode=ALL_MODES[(k + j) % 5])
                 for j in range(k + 2)]
        calls.append(Call(v, items, (ITEM_MODE,)))
    return calls


OVERFLOW_BLOCK, OVERFLOW_COPIES_END, OVERFLOW_TAIL = 40, (1 << 18) + (1 << 12), 64


def _overflow_list_full(name):
    rng = _rng(name)
    v = view()
    block = []
    for k in range(OVERFLOW_BLOCK - 4):
        block.append(at_px(v, 9.3 + (k % 9) * 9.7, 9.2 + (k // 9) * 15.1, 2.0 + 0.01 * k, 8.74, colour=int(rng.integers(0, 1 << 24))))
    for k in range(4):                                                                  # 71 or 72 columns of all 64 rows: two tiles
        block.append(at_px(v, 36.3 + 8 * k, 32.3, 3.0 + 0.1 * k, 35.5, colour=int(rng.integers(0, 1 << 24))))
    block = np.array(block)
    tail = np.array([at_px(v, 6.3 + (k % 16) * 5.6, 5.2 + (k // 16) * 17.9, 1.0 + 0.005 * k, 12.0, colour=int(rng.integers(0, 1 << 24)))
                     for k in range(OVERFLOW_TAIL)])
    reps = OVERFLOW_COPIES_END // OVERFLOW_BLOCK
    S = np.concatenate([np.tile(block, (reps, 1)), tail])
    assert len(S) == OVERFLOW_COPIES_END + OVERFLOW_TAIL
    few = [item(np.concatenate([block, tail]), model_id=6)]
    A = scatter(rng, v, 30)
    A[:10, 3] = 0.5; A[:10, 2] *= 0.3; A[:10, 0:2] *= 0.3; A[:10, 11] *= 0.6         # below the threshold, in front: a stale list entry draws them
    B = [item(scatter(rng, v, 12 + 5 * j), pose(0, 0, 0.02 * j, (0, 0, 0.1 * j)), model_id=20 + j, mode=ALL_MODES[j]) for j in range(3)]
    return [Call(v, [item(S, model_id=6)], (COLOUR,), ref_items=few), Call(v, [item(A, model_id=8)], (COLOUR,), not_drawn=tuple(range(10))),
            Call(v, B, (ITEM_MODE,))]


TABLE = (
    ("conf_at_threshold", _conf_at_threshold, "conf == thresh is below; its f32 neighbours on either side; below takes the times colour"),
    ("window_boundary", _window_boundary, "tick - last_time == time_delta is inside the window; one more is dimmed"),
    ("times_ramp", _times_ramp, "tick <= 1 gives ratio 0; init_time outside [1, tick] clamps; t == 0.5 takes the upper branch"),
    ("palette_ids", _palette_ids, "ids 16 and up wrap around the 16 colours; label 254 is not the empty 255"),
    ("item_mode_and_eight_outputs", _item_mode_and_eight_outputs, "ITEM_MODE over items of all five modes, eight colour outputs at once"),
    ("colour_bytes", _colour_bytes, "every byte value decoded in every channel; the half-way values under dimming"),
    ("phong_facing", _phong_facing, "normals faced towards the light; a specular term that saturates"),
    ("item_table_edges", _item_table_edges, "empty items at the head, middle (two) and tail share base and first workgroup; 1, 63, 64, 65 surfels"),
    ("max_items", _max_items, "256 items; an exact three-way tie across an empty item goes to the first"),
    ("all_empty_after_full", _all_empty_after_full, "a call without a raster launch leaves empty images and a clear key buffer"),
    ("narrow_boxes", _narrow_boxes, "boxes narrower than the four lanes of a surfel (the fx >= w carry)"),
    ("path_switch", _path_switch, "256 pixels stay with the four lanes, 272 and 289 go to the overflow list"),
    ("tile_seam", _tile_seam, "one full tile; the smallest two-tile box of a 96x64 view, its seam mid-row"),
    ("tile_seam_whole_views", _tile_seam_whole_views, "boxes of exactly 4097 and 8193 pixels: two and three tiles, the seams mid-row"),
    ("clipped", _clipped, "boxes clipped at every edge and corner on both paths"),
    ("outside_or_barely_inside", _outside_or_barely_inside, "no box outside; a box of one column without a fragment"),
    ("full_view", _full_view, "one box of the whole view"),
    ("near_far", _near_far, "a quad corner at near and next to it; z at far and next to it; the defaults"),
    ("degenerate", _degenerate, "surfels that must not draw (or draw as |r|) between ordinary ones"),
    ("f64_matrix", _f64_matrix, "V * Tp needs f64: an f32 product gives another matrix"),
    ("odd_intrinsics", _odd_intrinsics, "principal point outside the image, fx != fy, negative fy"),
    ("ray_cache", _ray_cache, "the rays follow every one of the six key values"),
    ("back_to_back", _back_to_back, "three item tables in flight; the third reuses staging slot 0"),
    ("overflow_list_full", _overflow_list_full, "more tiles than the overflow list holds; the count is reset for the next call"),
)
NAMES = tuple(n for n, _, _ in TABLE)


@functools.lru_cache(maxsize=None)
def case(name):
    for n, make, aims in TABLE:
        if n == name:
            return Case(n, aims, make(n), WIDE if n == "tile_seam_whole_views" else SIZE)
    raise KeyError(name)


def box(call, draw_index):
    """(ok, w, h) of one surfel's box in the restatement's _setup"""
    base = 0
    V = rr.view_inverse(call.view["pose"])
    near = f32(call.view.get("near", 0.1) or 0.1)
    for it in call.expected_items():
        S = it["surfels"]
        if draw_index < base + len(S):
            with np.errstate(all="ignore"):
                ok, _, _, _, _, x_lo, x_hi, y_lo, y_hi = rr._setup(S[draw_index - base:draw_index - base + 1], rr.model_to_camera(V, it["pose"]),
                                                                   call.view, near)
            return bool(ok[0]), int(x_hi[0] - x_lo[0] + 1), int(y_hi[0] - y_lo[0] + 1), int(x_lo[0]), int(y_lo[0])
        base += len(S)
    raise IndexError(draw_index)


# ---- the expected images of a case, and the rules of a comparison with the oracle (shared by the CPU and the GPU tests)

@functools.lru_cache(maxsize=None)
def reference(name):
    """per call of the case: (the restatement's outputs, its winning draw index per pixel (-1 = empty), the oracle's Result)"""
    import render_oracle as ro
    out = []
    for c in case(name).calls:
        with np.errstate(all="ignore"):
            want = rr.render(c.view, c.expected_items(), c.outputs())
            kb, _ = rr.keys(c.view, c.expected_items())
        gid = np.where(kb == np.uint64(0xFFFFFFFFFFFFFFFF), -1, (kb & np.uint64(0xFFFFFFFF)).astype(np.int64))
        for a in want:
            a.setflags(write=False)
        out.append((want, gid, ro.render(c.view, c.expected_items(), c.modes, c.exempt)))
    return out


def against_oracle(call, outs, orc, what, bound=None):
    """the rules of the comparison with the f64 statement, off its ambiguity mask: coverage and label exact, every colour byte
    round(clamp(c) * 255) (one off only where the channel is half-way), depth within `bound` (default DEPTH_BOUND), relative.
    Returns the largest relative depth difference seen."""
    import render_oracle as ro
    bound = DEPTH_BOUND if bound is None else bound
    sure = ~orc.ambiguous
    on = sure & orc.covered
    worst = 0.0
    for o, got in zip(call.outputs(), outs):
        if o[0] == "depth":
            assert np.array_equal((got != 0)[sure], orc.covered[sure]), f"{what}: depth coverage differs from the oracle"
            if on.any():
                rel = np.abs(got[on].astype(float) - orc.depth[on]) / orc.depth[on]
                worst = float(rel.max())
                assert worst <= bound, f"{what}: depth differs from the oracle by {worst:.3g} relative (bound {bound:.3g})"
        elif o[0] == "labels":
            bad = (got.astype(np.int64) != orc.label) & sure
            assert not bad.any(), f"{what}: {np.count_nonzero(bad)} labels differ from the oracle, first at {np.argwhere(bad)[0][::-1]}"
        else:
            assert np.array_equal((got[..., 3] == 255)[sure], orc.covered[sure]), f"{what}: coverage differs from the oracle"
            assert not got[..., 3][~orc.covered & sure].any(), f"{what}: alpha of an empty pixel"
            c = orc.colours[o[1]]
            diff = np.abs(got[..., :3].astype(np.int64) - ro.to_byte(c))
            bad = ((diff > 1) | ((diff == 1) & ~ro.half_way(c))) & on[..., None]
            assert not bad.any(), (f"{what}: mode {o[1]}: {np.count_nonzero(bad)} colour bytes differ from the oracle, first at "
                                   f"{np.argwhere(bad)[0]}: {got[..., :3][bad][0]} against {c[bad][0] * 255:.5f}")
    return worst
