"""Case table of the label-mask branch of the segmentation (Segmentation.cpp:59-119; oracle: orc_segment_gt; device: cf_seg_masks).
numpy only.  One named case per branch of the reference's three loops, at the smallest sizes at which the kernels can still go wrong:

  48 x 32   (1 536 pixels)  one and a half super-blocks of the sequential chain (64 lanes x 16 pixels)
  80 x 36   (2 880 pixels)  a height that is no multiple of 16: a ragged last super-block, a last workgroup with idle threads
  160 x 128                 several workgroups and twenty super-blocks

A case is a dict: name, w, h, mask (u8 [h, w]), depth (f32 [h, w]), ids (the model list), next_id, allow_new, mapping (u8 [256], mask
value -> model id, 0 = unmapped; NOT modified by the users of the table: they pass a copy) and `expect`, the facts the case is named
for, which tests/test_cpu_mask_cases.py asserts on the oracle's result (so that a case cannot silently stop covering its edge):
  has_new, new_value (-1: none)          the spawn decision
  spc {row: superPixelCount}             selected rows
  count {label: pixels}                  pixels of selected labels in the label image
  order                                  the depth sums of the row `order` differ in bits between summation orders (see reorderings)
All depths are finite (NaN payloads are not part of the contract)."""
import numpy as np

F = np.float32
SIZES = [(48, 32), (80, 36), (160, 128)]


def mm_depth(rng, h, w):
    """sensor-like depths: f32(u16 millimetres) * 0.001f in 0.3 .. 5 m"""
    return (rng.integers(300, 5000, (h, w)).astype(np.uint16).astype(F) * F(0.001)).astype(F)


def _case(name, w, h, mask, depth, ids, next_id, allow_new, mapping, **expect):
    m = np.zeros(256, np.uint8)
    for k, v in mapping.items():
        m[k] = v
    mask = np.ascontiguousarray(mask, np.uint8)
    depth = np.ascontiguousarray(depth, F)
    assert mask.shape == (h, w) and depth.shape == (h, w) and np.isfinite(depth).all()
    return dict(name=name, w=w, h=h, mask=mask, depth=depth, ids=list(ids), next_id=int(next_id), allow_new=int(allow_new), mapping=m,
                expect=expect)


def _blocks(h, w):
    """a mask of three rectangles (values 7, 30, 20 from top to bottom: 30 comes first in raster order among the last two)"""
    mask = np.zeros((h, w), np.uint8)
    mask[2:h // 3, 3:w // 2] = 7
    mask[h // 3:h // 3 + 5, w // 4:w - 5] = 30
    mask[h // 3 + 7:h - 3, 1:w // 3] = 20
    return mask


def build():
    rng = np.random.default_rng(20240607)
    out = []
    w, h = SIZES[0]
    W1, H1 = SIZES[1]
    W2, H2 = SIZES[2]

    out.append(_case("all_zero_mask", w, h, np.zeros((h, w), np.uint8), mm_depth(rng, h, w), [0], 1, 1, {}, has_new=False, new_value=-1,
                     spc={0: w * h // 256}))

    mask = _blocks(H1, W1)
    out.append(_case("every_label_mapped", W1, H1, mask, mm_depth(rng, H1, W1), [0, 1, 2, 3], 4, 1, {7: 1, 30: 2, 20: 3},
                     has_new=False, new_value=-1))
    n20 = int((mask == 20).sum())
    out.append(_case("two_unmapped_allow_new", W1, H1, mask, mm_depth(rng, H1, W1), [0, 1], 2, 1, {7: 1}, has_new=True, new_value=30,
                     count={2: int((mask == 30).sum()), 0: int((mask == 0).sum()) + n20}))
    out.append(_case("two_unmapped_no_new", W1, H1, mask, mm_depth(rng, H1, W1), [0, 1], 2, 0, {7: 1}, has_new=False, new_value=-1,
                     count={2: 0, 0: int((mask != 7).sum())}))

    mask = _blocks(h, w); mask[0, 0] = 40; mask[h - 1, w - 9:] = 40
    out.append(_case("first_unmapped_at_index_0", w, h, mask, mm_depth(rng, h, w), [0, 1], 2, 1, {7: 1, 30: 1, 20: 1}, has_new=True,
                     new_value=40, count={2: 10}))
    mask = np.zeros((H1, W1), np.uint8); mask[4:9, 4:40] = 7; mask[H1 - 1, W1 - 1] = 40
    out.append(_case("first_unmapped_at_last_index", W1, H1, mask, mm_depth(rng, H1, W1), [0, 1], 2, 1, {7: 1}, has_new=True, new_value=40,
                     count={2: 1}, spc={2: 1}))

    mask = np.zeros((h, w), np.uint8); mask[3:20, 5:30] = 254; mask[22:30, 8:40] = 255
    out.append(_case("mask_value_255", w, h, mask, mm_depth(rng, h, w), [0, 1], 2, 1, {254: 1}, has_new=True, new_value=255,
                     count={2: 8 * 32}))
    out.append(_case("model_id_255", w, h, mask, mm_depth(rng, h, w), [0, 255], 1, 1, {254: 255, 255: 255}, has_new=False, new_value=-1,
                     count={255: 17 * 25 + 8 * 32}))

    mask = np.zeros((h, w), np.uint8); mask[3:20, 5:30] = 5
    out.append(_case("listed_model_without_pixels", w, h, mask, mm_depth(rng, h, w), [0, 1, 2], 3, 1, {5: 1, 6: 2}, has_new=False,
                     new_value=-1, spc={2: 0}, count={2: 0}))
    # a mapping that still names a model that left the list: its pixels keep the label and join row 0's statistics (modelIdToIndex defaults to 0)
    out.append(_case("mapping_to_unlisted_model", w, h, mask, mm_depth(rng, h, w), [0, 2], 3, 0, {5: 9}, has_new=False, new_value=-1,
                     count={9: 17 * 25}))

    flat = np.zeros(w * h, np.uint8)
    pos = rng.permutation(w * h)
    flat[pos[:255]] = 11; flat[pos[255:255 + 256]] = 12; flat[pos[511:511 + 257]] = 13
    out.append(_case("labels_of_255_256_257_pixels", w, h, flat.reshape(h, w), mm_depth(rng, h, w), [0, 1, 2, 3], 4, 0, {11: 1, 12: 2, 13: 3},
                     has_new=False, new_value=-1, spc={1: 0, 2: 1, 3: 1}, count={1: 255, 2: 256, 3: 257}))
    flat = np.zeros(w * h, np.uint8); flat[pos[:255]] = 11
    out.append(_case("new_label_of_255_pixels", w, h, flat.reshape(h, w), mm_depth(rng, h, w), [0], 1, 1, {}, has_new=True, new_value=11,
                     spc={1: 1}, count={1: 255}))

    flat = np.zeros(w * h, np.uint8)
    flat[np.arange(0, w * h, 16) + rng.integers(0, 16, w * h // 16)] = 5          # one pixel in every 16-pixel block
    out.append(_case("one_pixel_per_block", w, h, flat.reshape(h, w), mm_depth(rng, h, w), [0, 1], 2, 0, {5: 1}, has_new=False,
                     new_value=-1, count={1: w * h // 16}))
    flat = np.zeros(W1 * H1, np.uint8)
    flat[16 * 3:16 * 7] = 5; flat[1024:2048] = 5; flat[2048 + 16 * 50:2048 + 16 * 52] = 5   # whole blocks, one whole super-block
    out.append(_case("whole_blocks", W1, H1, flat.reshape(H1, W1), mm_depth(rng, H1, W1), [0, 1], 2, 0, {5: 1}, has_new=False, new_value=-1,
                     count={1: 64 + 1024 + 32}))
    flat = np.zeros(w * h, np.uint8)
    i, k = 3, 0
    while i + 17 < w * h:   # runs of 1, 15, 16 and 17 pixels of alternating labels, gaps of 1 and 2 pixels
        n = (1, 15, 16, 17)[k % 4]
        flat[i:i + n] = 5 + (k % 3)
        i += n + 1 + (k % 2); k += 1
    out.append(_case("run_lengths_1_15_16_17", w, h, flat.reshape(h, w), mm_depth(rng, h, w), [0, 1, 2, 3], 4, 0, {5: 1, 6: 2, 7: 3},
                     has_new=False, new_value=-1))

    def stripes(hh, ww, n):   # n + 1 mask values 1 .. n + 1 in vertical stripes, four pixels wide, on a background of zeros below
        m = ((np.arange(ww) // 4) % (n + 1) + 1).astype(np.uint8)[None, :].repeat(hh, 0)
        m[hh - 3:, :] = 0
        return m
    out.append(_case("seventeen_models_and_a_new_label", W1, H1, stripes(H1, W1, 16), mm_depth(rng, H1, W1), list(range(17)), 17, 1,
                     {v: v for v in range(1, 17)}, has_new=True, new_value=17))
    out.append(_case("eighteen_models_and_a_new_label", W1, H1, stripes(H1, W1, 17), mm_depth(rng, H1, W1), list(range(18)), 18, 1,
                     {v: v for v in range(1, 18)}, has_new=True, new_value=18))   # (more ids than a batched launch carries)

    mask = np.zeros((h, w), np.uint8); mask[2:9, 7:23] = 5; mask[12:15, 1:40] = 6
    depth = mm_depth(rng, h, w); depth[2, 7] = F(-0.0); depth[12:15, 1:40] = F(-0.0)
    out.append(_case("negative_zero_first_depth", w, h, mask, depth, [0, 1, 2], 3, 0, {5: 1, 6: 2}, has_new=False, new_value=-1))
    depth = mm_depth(rng, h, w); depth[rng.random((h, w)) < 0.3] = 0; depth[4, :] = 0
    out.append(_case("depth_zeros_inside_labels", w, h, _blocks(h, w), depth, [0, 1, 2], 3, 1, {7: 1, 30: 2}, has_new=True, new_value=20))

    for ww, hh in SIZES:   # the order cases: two big labels, sensor-like depths
        yy, xx = np.mgrid[0:hh, 0:ww]
        mask = np.where((xx * 3 + yy) % 7 < 3, 5, 0).astype(np.uint8)
        out.append(_case(f"summation_order_{ww}x{hh}", ww, hh, mask, mm_depth(rng, hh, ww), [0, 1], 2, 0, {5: 1}, has_new=False, new_value=-1,
                         order=1))
    return out


def reorderings(values):
    """f32 sums of `values` in three orders a kernel might be tempted by -- pairwise tree, sixteen blocked partials, reversed -- beside the
    specified one (sequential, from +0.0f): {"sequential", "pairwise", "blocked16", "reversed"} -> f32"""
    v = np.asarray(values, F)

    def seq(a):
        s = F(0.0)
        for x in a:
            s = F(s + x)
        return s

    def pairwise(a):
        a = list(a)
        while len(a) > 1:
            a = [F(a[i] + a[i + 1]) if i + 1 < len(a) else a[i] for i in range(0, len(a), 2)]
        return a[0] if a else F(0.0)
    parts = [seq(v[k::16]) for k in range(16)]
    return dict(sequential=seq(v), pairwise=pairwise(v), blocked16=seq(parts), reversed=seq(v[::-1]))


def parse_expected_rows(ref):
    """the oracle's rows as comparable tuples: (id, superPixelCount, bits of avgConfidence, depthMean, depthStd)"""
    b = lambda x: int(np.float32(x).view(np.uint32))
    return [(int(m["id"]), int(m["superPixelCount"]), b(m["avgConfidence"]), b(m["depthMean"]), b(m["depthStd"])) for m in ref["modelData"]]
