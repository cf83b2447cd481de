"""Named cases of the re-detection search (DESIGN.md 4.13 "Search"): small frames and crafted surfel maps, shared by
tests/test_cpu_redetect_search_ref.py (the numpy statement against the construction) and tests/test_redetect_search_gpu.py (the device
against the statement, for equality).

Two image sizes, 160x128 (fx = fy = 128) and 70x46 (fx = fy = 64, a pixel count that is no multiple of a workgroup): the focal length is
a power of two and the principal point an integer pixel, so the vertex of the principal pixel is (0, 0, d) exactly and a surfel at
(0, 0, z) lands on it without rounding -- the gate cases sit there.  Depths and tolerances of the crafted cases are binary fractions in
[1, 2), where an offset of k ulp is k * 2^-23.

  box_moved, box_turned   (a), (b): a 0.30 x 0.24 x 0.20 m box mapped with three faces in view (2 mm noise), back 0.3 m sideways (and
                          turned 10 degrees about its vertical axis); the frame is ray-cast from the box at its true pose, 3 mm noise
  plane                   (c): a single-plane map, back 0.3 m sideways
  rejects, gate_<k>       (d): every rejection of the step, the distance gate at tol +- 1 and 3 ulp
  empty                   (e): a label nobody carries, a map without surfels
  batch_1 / 3 / 9         (g): random maps of many sizes under rotated poses in one launch; batch_9 lists a map twice
  bin_edges               (h): colours on the edges of the 512 bins
(f): every case exists at both sizes."""
import numpy as np

F = np.float32
SIZES = ((160, 128), (70, 46))
L = 7                 # the new label
THETA = F(0.5)
CUTOFF = F(3.0)
TOL_GATE = F(0.125)
TOL_BOX = F(0.10)     # the tracker's gate, the default of setRedetection
ULP = F(2.0 ** -23)
GATE_K = (-3, -1, 0, 1, 3)
BOX_HALF = np.array([0.15, 0.12, 0.10])
I4 = np.eye(4, dtype=F)


def cam_of(size):
    w, h = size
    f = 128.0 if w >= 128 else 64.0
    return (F(f), F(f), F(w // 2), F(h // 2))


def colour_code(r, g, b):
    """the surfel record's colour word (encode_color): exact in f32"""
    return F((int(r) << 16) + (int(g) << 8) + int(b))


def surfel_rows(pos, normal, rgb, conf=1.0):
    pos = np.asarray(pos, F).reshape(-1, 3)
    n = pos.shape[0]
    s = np.zeros((n, 12), F)
    s[:, :3] = pos
    s[:, 3] = F(conf)
    rgb = np.broadcast_to(np.asarray(rgb, np.int64), (n, 3))
    s[:, 4] = [colour_code(*c) for c in rgb]
    s[:, 7] = 1.0
    s[:, 8:11] = np.broadcast_to(np.asarray(normal, F), (n, 3))
    s[:, 11] = 0.01
    return s


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.deg2rad(deg)
    return np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * (K @ K)


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


class Case:
    """models: surfel arrays [n, 12]; cands: (index into models, theta, static hypothesis pose model <- camera f32 4x4); truth: the true
    T(camera <- model) of candidate 0 or None; expect: what is known by construction --
    frame: (n, {bin: count}) or None; model: per candidate (n_front or None, {bin: count} or None); step: per candidate {word: value} of
    the step at the static pose, or None"""

    def __init__(self, name, size, depth, label, rgba, models, cands, tol, truth=None, frame=None, model=None, step=None):
        self.name, self.size, self.cam = name, size, cam_of(size)
        self.depth, self.label, self.rgba = depth, label, rgba
        self.models, self.cands, self.tol, self.truth = models, cands, F(tol), truth
        self.cutoff, self.new_label = CUTOFF, L
        self.expect_frame, self.expect_model, self.expect_step = frame, model or [None] * len(cands), step or [None] * len(cands)


def blank(size, wall=2.5):
    w, h = size
    rgba = np.zeros((h, w, 4), np.uint8)
    rgba[..., :3] = 90
    rgba[..., 3] = 255
    return np.full((h, w), wall, F), np.zeros((h, w), np.uint8), rgba


# ---- (a) (b) (c): a box ----
FACE_RGB = {(0, -1): (200, 60, 40), (0, 1): (200, 60, 40), (1, -1): (210, 70, 40), (1, 1): (210, 70, 40), (2, -1): (190, 50, 30), (2, 1): (190, 50, 30)}


def box_map(T_old, half, rng, step=0.01, noise=0.002):
    """surfels of the faces of the box (model frame: centred, axis aligned) that face the camera under T_old (camera <- model)"""
    out = []
    for a in range(3):
        for sgn in (-1, 1):
            n = np.zeros(3); n[a] = sgn
            c = np.zeros(3); c[a] = sgn * half[a]
            if (T_old[:3, :3] @ n) @ (T_old[:3, :3] @ c + T_old[:3, 3]) >= 0:
                continue
            o = [b for b in range(3) if b != a]
            g = [np.arange(-half[b] + step / 2, half[b], step) for b in o]
            uu, vv = np.meshgrid(g[0], g[1], indexing="ij")
            p = np.zeros((uu.size, 3))
            p[:, o[0]] = uu.ravel(); p[:, o[1]] = vv.ravel(); p[:, a] = sgn * half[a]
            p = p + n * rng.normal(0.0, noise, size=(uu.size, 1))
            out.append(surfel_rows(p, -n, FACE_RGB[(a, sgn)]))   # (stored as the maps store them: pointing away from the camera)
    return np.concatenate(out)


def raycast_box(size, T_true, half, rng, noise=0.003, rgb_of_face=FACE_RGB):
    """depth / label / rgba of the box at T_true (camera <- model) in front of a wall, rays through the integer pixel coordinates"""
    w, h = size
    fx, fy, cx, cy = (float(v) for v in cam_of(size))
    depth, label, rgba = blank(size)
    py, px = np.mgrid[0:h, 0:w]
    d = np.stack([(px - cx) / fx, (py - cy) / fy, np.ones((h, w))], -1).reshape(-1, 3)
    Rt = T_true[:3, :3].T
    o = Rt @ (-T_true[:3, 3])
    dm = d @ Rt.T
    with np.errstate(all="ignore"):
        t1 = (-half - o) / dm
        t2 = (half - o) / dm
    tn = np.minimum(t1, t2); tf = np.maximum(t1, t2)
    near = tn.max(1); far = tf.min(1)
    hit = (near < far) & (near > 0)
    axis = tn.argmax(1)
    for i in np.nonzero(hit)[0]:
        y, x = divmod(int(i), w)
        sgn = -1 if dm[i, axis[i]] > 0 else 1
        depth[y, x] = F(near[i] + rng.normal(0.0, noise))
        label[y, x] = L
        rgba[y, x, :3] = rgb_of_face[(int(axis[i]), sgn)]
    return depth, label, rgba


def _box(size, name, turn_deg, half=BOX_HALF, R_old=None):
    rng = np.random.default_rng(11 + size[0] + int(turn_deg))
    R_old = rot([0, 1, 0], 30.0) @ rot([1, 0, 0], 25.0) if R_old is None else R_old
    T_old = rigid(R_old, [-0.15, 0.0, 1.5])
    # back 0.3 m to the right, turned about its own vertical axis (through its centre)
    T_true = rigid(rot(R_old @ [0, 1, 0], turn_deg) @ R_old, [0.15, 0.0, 1.5])
    m = box_map(T_old, half, rng)
    depth, label, rgba = raycast_box(size, T_true, half, rng)
    return Case(name, size, depth, label, rgba, [m], [(0, THETA, np.linalg.inv(T_old).astype(F))], TOL_BOX, truth=T_true)


def _plane(size):
    return _box(size, "plane", 0.0, half=np.array([0.15, 0.12, 0.0005]), R_old=np.eye(3))


# ---- (d): the step's rejections ----
def on_ray(size, px, py, z, offset=(0.5, 0.5)):
    fx, fy, cx, cy = cam_of(size)
    z = F(z)
    return [(F(px) + F(offset[0]) - cx) * z / fx, (F(py) + F(offset[1]) - cy) * z / fy, z]


def _gate(size, k):
    """n surfels at (0, 0, 1.375 + k ulp), normal (0, 0, 1), the principal pixel at d = 1.5: |v - p| = 0.125 - k ulp exactly, an inlier
    iff k >= 0; J = (0, 0, 1, 0, 0, 0), r = 0.125 - k ulp: word 13 (J_z J_z) = n 2^32, word 17 (J_z r) = n (0.125 - k ulp) 2^32"""
    w, h = size
    n = 70
    depth, label, rgba = blank(size)
    depth[h // 2, w // 2] = 1.5; label[h // 2, w // 2] = L
    z = F(1.375) + F(k) * ULP
    m = surfel_rows(np.tile([0.0, 0.0, z], (n, 1)), [0, 0, 1], (10, 20, 30))
    gap = float(F(1.5) - z)
    step = {28: n, 13: n << 32, 17: n * int(gap * 2 ** 32), 27: n * int(np.rint(gap * gap * 2.0 ** 32))} if k >= 0 else {28: 0, 13: 0, 17: 0, 27: 0}
    return Case(f"gate_{k}", size, depth, label, rgba, [m], [(0, THETA, I4)], TOL_GATE, frame=(1, {colour_bin(90, 90, 90): 1}),
                model=[(n, {colour_bin(10, 20, 30): n})], step=[step])


def colour_bin(r, g, b):
    return ((r >> 5) << 6) | ((g >> 5) << 3) | (b >> 5)


def _rejects(size):
    w, h = size
    depth, label, rgba = blank(size, wall=1.0)
    label[:] = L
    col = (10, 20, 30)
    rows, n_in = [], 0

    def add(p, normal=(0, 0, 1), conf=1.0, inlier=False):
        nonlocal n_in
        rows.append(surfel_rows([p], normal, col, conf))
        n_in += 1 if inlier else 0

    for px, py in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2)):    # the four corners and the middle: in
        add(on_ray(size, px, py, 1.0), inlier=True)
    add(on_ray(size, 3, 3, 1.0), conf=np.nextafter(THETA, F(0)))                          # just below theta
    add(on_ray(size, 3, 3, 1.0), conf=THETA, inlier=True)                                 # at theta
    add(on_ray(size, 3, 3, 1.0), conf=np.nan)
    add(on_ray(size, w // 2, h // 2, -1.0))                                               # behind the camera
    add(on_ray(size, w // 2, h // 2, float(CUTOFF)))                                      # at and over the cut-off
    add(on_ray(size, w // 2, h // 2, float(CUTOFF) + 1.0))
    add(on_ray(size, 0, 3, 1.0, offset=(-0.25, 0.5)))                                     # outside each border
    add(on_ray(size, w, 3, 1.0, offset=(0.25, 0.5)))
    add(on_ray(size, 3, 0, 1.0, offset=(0.5, -0.25)))
    add(on_ray(size, 3, h, 1.0, offset=(0.5, 0.25)))
    add(on_ray(size, w, 3, 1.0, offset=(0.0, 0.5)))                                       # u exactly cols, v exactly rows
    add(on_ray(size, 3, h, 1.0, offset=(0.5, 0.0)))
    label[5, 5] = L + 1
    add(on_ray(size, 5, 5, 1.0))                                                          # on another label
    for j, bad in enumerate((0.0, np.nan, np.inf, -1.0, float(CUTOFF) + 0.5)):            # invalid depth, depth over the cut-off
        depth[7, 5 + j] = bad
        add(on_ray(size, 5 + j, 7, 1.0))
    depth[9, 5] = float(CUTOFF)                                                           # d == cutoff is valid, but 2 m away
    add(on_ray(size, 5, 9, 1.0))
    add(on_ray(size, 6, 9, 1.0), normal=(0, 0, -1))                                       # dot(n, p) < 0: seen from behind
    add([0.0, 0.0, 1.0], normal=(1, 0, 0))                                                # dot(n, p) == 0 exactly
    add([0.0, 0.0, 1.0], normal=(0, -1, 0))
    add([0.0, 0.0, 1.0], normal=(1, 0, 1), inlier=True)                                   # ... and above
    m = np.concatenate(rows)
    stable = int(np.count_nonzero(m[:, 3] >= THETA))
    n_px = w * h - 1 - 5
    return Case("rejects", size, depth, label, rgba, [m], [(0, THETA, I4)], TOL_GATE, frame=(n_px, {colour_bin(90, 90, 90): n_px}),
                model=[(None, {colour_bin(*col): stable})], step=[{28: n_in}])


# ---- (e) ----
def _empty(size):
    depth, label, rgba = blank(size)
    label[2:5, 2:5] = L + 1
    full = surfel_rows([on_ray(size, 3, 3, 1.5)] * 8, [0, 0, 1], (1, 2, 3))
    none = np.zeros((0, 12), F)
    zero = {k: 0 for k in range(29)}
    return Case("empty", size, depth, label, rgba, [none, full], [(0, THETA, I4), (1, THETA, I4)], TOL_GATE, frame=(0, {}),
                model=[(0, {}), (None, {colour_bin(1, 2, 3): 8})], step=[zero, zero])


# ---- (g) ----
def _batch(size, n_cands):
    w, h = size
    rng = np.random.default_rng(500 + w + n_cands)
    depth = rng.uniform(0.8, 2.6, size=(h, w)).astype(F)
    depth[rng.random((h, w)) < 0.1] = 0
    label = (rng.integers(0, 3, size=(h, w)) * L).astype(np.uint8)
    rgba = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
    sizes = [300, 0, 65, 1, 1000, 64, 2049, 17, 128][:n_cands]
    models, cands = [], []
    for j, n in enumerate(sizes):
        s = np.zeros((n, 12), F)
        s[:, :3] = rng.uniform([-1.5, -1.2, 0.3], [1.5, 1.2, 3.5], size=(n, 3))
        s[:, 3] = rng.uniform(0.0, 1.0, size=n)
        s[:, 4] = [colour_code(*c) for c in rng.integers(0, 256, size=(n, 3))]
        nr = rng.normal(size=(n, 3)); nr /= np.linalg.norm(nr, axis=1, keepdims=True)
        s[:, 8:11] = nr
        s[:, 11] = 0.01
        models.append(s)
        pose = rigid(rot(rng.normal(size=3), 17.0 * (j + 1)), rng.uniform(-0.2, 0.2, size=3)).astype(F)
        cands.append((j, THETA, pose))
    if n_cands == 9:   # the largest map once more, under another pose and threshold
        cands[3] = (6, F(0.25), cands[3][2])
    return Case(f"batch_{n_cands}", size, depth, label, rgba, models, cands, TOL_BOX)


# ---- (h) ----
EDGES = (0, 31, 32, 223, 224, 255)


def _bin_edges(size):
    w, h = size
    depth, label, rgba = blank(size)
    combos = [(r, g, b) for r in EDGES for g in EDGES for b in EDGES]
    want = {}
    for j, c in enumerate(combos):
        y, x = divmod(j, w - 4)
        depth[y + 2, x + 2] = 1.5; label[y + 2, x + 2] = L; rgba[y + 2, x + 2, :3] = c
        want[colour_bin(*c)] = want.get(colour_bin(*c), 0) + 1
    m = np.concatenate([surfel_rows([on_ray(size, 3, 3, 1.5)], [0, 0, 1], c) for c in combos])
    return Case("bin_edges", size, depth, label, rgba, [m], [(0, THETA, I4)], TOL_GATE, frame=(len(combos), want), model=[(len(combos), dict(want))])


BUILDERS = {
    "box_moved": lambda s: _box(s, "box_moved", 0.0), "box_turned": lambda s: _box(s, "box_turned", 10.0), "plane": _plane, "rejects": _rejects,
    **{f"gate_{k}": (lambda s, k=k: _gate(s, k)) for k in GATE_K}, "empty": _empty,
    "batch_1": lambda s: _batch(s, 1), "batch_3": lambda s: _batch(s, 3), "batch_9": lambda s: _batch(s, 9), "bin_edges": _bin_edges,
}
NAMES = tuple(BUILDERS)
REGISTERED = ("box_moved", "box_turned", "plane")   # the cases with a true pose
_CACHE = {}


def get(name, size):
    key = (name, tuple(size))
    if key not in _CACHE:
        _CACHE[key] = BUILDERS[name](tuple(size))
    return _CACHE[key]


_STATEMENT = {}
DHAT_OF_AN_EMPTY_LABEL = (0.0, 0.0, 1.0)   # (the frame loop stops before it needs one; the kernels are still compared)


def statement(case):
    """what tests/redetect_search_ref.py says about a case, computed once and shared: frame (moments, hist), centre and dhat (f32), and per
    candidate: moments, hist, T0 (the static hypothesis camera <- model), seed (or None), the step's sums at T0 and at the seed,
    the registration from the seed (or None)"""
    import redetect_ref
    import redetect_search_ref as ref
    key = (case.name, case.size)
    if key in _STATEMENT:
        return _STATEMENT[key]
    fm, fh = ref.frame_moments(case.depth, case.label, case.rgba, case.new_label, case.cam, case.cutoff)
    fbar, dhat = ref.frame_centroid(fm)
    centre = np.asarray(fbar if fbar else (0.0, 0.0, 0.0), F)
    dhat32 = np.asarray(dhat if dhat else DHAT_OF_AN_EMPTY_LABEL, F)
    out = dict(frame=(fm, fh), centre=centre, dhat=dhat32, cands=[])
    args = (case.depth, case.label, case.new_label, case.cam, case.cutoff, case.tol, centre)
    for mi, theta, pose in case.cands:
        s = case.models[mi]
        mm, mh = ref.model_moments(s, theta, pose, dhat32)
        T0 = redetect_ref.inv44f(pose)
        seed = ref.seed(T0, mm, fbar) if fbar else None
        c = dict(moments=mm, hist=mh, T0=T0, seed=seed, step_T0=ref.register_step(s, theta, T0, *args), step_seed=None, reg=None,
                 colour=ref.colour_similarity(mh, fh))
        if seed is not None:
            c["step_seed"] = ref.register_step(s, theta, seed, *args)
            c["reg"] = ref.register(s, theta, seed, *args)
        out["cands"].append(c)
    _STATEMENT[key] = out
    return out
