"""CPU suite of the label-mask branch: every case of tests/mask_cases.py through the oracle (orc_segment_gt), asserting that the case
still holds the edge it is named for, and that the order cases tell a sequential f32 sum from the re-orderings a kernel might use.
Plus the PGM reader of co_fusion_amd/masks.py."""
import numpy as np
import pytest

import mask_cases as mc
import orc_multi as om

CASES = mc.build()
_REFS = {}


def ref(case):
    if case["name"] not in _REFS:
        mapping = case["mapping"].copy()
        r = om.segment_gt(case["mask"], case["depth"], case["ids"], case["next_id"], case["allow_new"], mapping)
        new = np.flatnonzero(mapping != case["mapping"])
        r["new_value"] = int(new[0]) if len(new) else -1
        assert len(new) <= 1
        _REFS[case["name"]] = r
    return _REFS[case["name"]]


def test_the_table_names_every_branch_and_size():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert {(c["w"], c["h"]) for c in CASES} == set(mc.SIZES)
    for w, h in mc.SIZES:
        assert w % 16 == 0 and h % 4 == 0   # what a context accepts
    assert (80 * 36) % 1024 and 36 % 16     # the ragged super-block, the height no superpixel grid fits


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_holds_its_edge_on_the_oracle(case):
    r = ref(case)
    e = case["expect"]
    n = len(case["ids"])
    assert r["hasNewLabel"] == e["has_new"] and r["new_value"] == e["new_value"]
    assert len(r["modelData"]) == n + (1 if e["has_new"] else 0)
    assert [m["id"] for m in r["modelData"]] == case["ids"] + ([case["next_id"]] if e["has_new"] else [])
    for row, spc in e.get("spc", {}).items():
        assert r["modelData"][row]["superPixelCount"] == spc, (row, r["modelData"][row])
    for label, count in e.get("count", {}).items():
        assert int((r["full"] == label).sum()) == count, label
    for m in r["modelData"]:
        assert np.float32(m["avgConfidence"]) == np.float32(0.4) and np.isfinite(m["depthMean"]) and np.isfinite(m["depthStd"])
    if e["has_new"]:
        flat = case["mask"].reshape(-1)
        unmapped = np.flatnonzero((flat != 0) & (case["mapping"][flat] == 0))
        assert flat[unmapped[0]] == e["new_value"]


def test_named_edges_are_where_the_names_say():
    by = {c["name"]: c for c in CASES}
    c = by["first_unmapped_at_index_0"]; assert c["mask"].reshape(-1)[0] == 40
    c = by["first_unmapped_at_last_index"]
    flat = c["mask"].reshape(-1)
    assert flat[-1] == 40 and not (flat[:-1] == 40).any()
    c = by["two_unmapped_allow_new"]
    r = ref(c)
    assert int((c["mask"] == 20).sum()) > 0 and not (r["full"][c["mask"] == 20]).any()      # the other unmapped value became label 0 ...
    zeros = r["full"] == 0
    seq = mc.reorderings(c["depth"][zeros])["sequential"]                                   # ... and sits in the background's statistics
    assert np.float32(seq / np.float32(zeros.sum())).tobytes() == np.float32(r["modelData"][0]["depthMean"]).tobytes()
    c = by["listed_model_without_pixels"]; r = ref(c)
    assert r["modelData"][2]["depthMean"] == 0 and r["modelData"][2]["depthStd"] == 0       # 0 / 1
    c = by["negative_zero_first_depth"]; r = ref(c)
    first = np.flatnonzero(c["mask"].reshape(-1) == 5)[0]
    assert np.signbit(c["depth"].reshape(-1)[first]) and c["depth"].reshape(-1)[first] == 0
    assert r["modelData"][2]["depthMean"] == 0 and not np.signbit(np.float32(r["modelData"][2]["depthMean"]))
    c = by["one_pixel_per_block"]
    assert (c["mask"].reshape(-1, 16) == 5).sum(1).tolist() == [1] * (c["w"] * c["h"] // 16)
    c = by["whole_blocks"]
    per = (c["mask"].reshape(-1, 16) == 5).sum(1)
    assert set(per.tolist()) == {0, 16} and (c["mask"].reshape(-1)[1024:2048] == 5).all()
    c = by["run_lengths_1_15_16_17"]
    flat = np.concatenate([[0], c["mask"].reshape(-1), [0]])
    edges = np.flatnonzero(flat[1:] != flat[:-1])
    runs = {int(b - a) for a, b in zip(edges[:-1], edges[1:]) if flat[a + 1] != 0}
    assert {1, 15, 16, 17} <= runs
    c = by["depth_zeros_inside_labels"]
    assert ((c["depth"] == 0) & (c["mask"] != 0)).sum() > 10
    assert len(by["seventeen_models_and_a_new_label"]["ids"]) == 17 and len(by["eighteen_models_and_a_new_label"]["ids"]) == 18


@pytest.mark.parametrize("case", [c for c in CASES if "order" in c["expect"]], ids=lambda c: c["name"])
def test_order_cases_tell_summation_orders_apart(case):
    """a kernel that re-associates the depth sums (a tree, blocked partials, a reversed walk) cannot reproduce the oracle's depthMean"""
    r = ref(case)
    row = case["expect"]["order"]
    mine = r["full"] == (case["ids"][row] & 255)
    sums = mc.reorderings(case["depth"][mine])
    cnt = np.float32(mine.sum())
    want = np.float32(r["modelData"][row]["depthMean"]).tobytes()
    assert np.float32(sums["sequential"] / cnt).tobytes() == want
    for other in ("pairwise", "blocked16", "reversed"):
        assert np.float32(sums[other]).tobytes() != np.float32(sums["sequential"]).tobytes(), other
        assert np.float32(sums[other] / cnt).tobytes() != want, other


def test_pgm_reader(tmp_path):
    from co_fusion_amd import masks
    img = (np.arange(7 * 5) * 9 % 256).astype(np.uint8).reshape(5, 7)
    img[0, 0] = 10   # a pixel byte that is whitespace: exactly one separator byte is skipped after maxval
    assert np.array_equal(masks.parse_pgm(b"P5\n7 5\n255\n" + img.tobytes()), img)
    assert np.array_equal(masks.parse_pgm(b"P5 # binary\n# size\n7\t5 #max\n200 " + img.tobytes()), img)
    p = masks.mask_path(str(tmp_path), 12)
    assert p.endswith("Mask0012.pgm") and masks.mask_path("d", 3, "M", 2).endswith("M03.pgm")
    with open(p, "wb") as f:
        f.write(b"P5\n7 5\n255\n" + img.tobytes())
    got = masks.read_pgm(p)
    assert got.dtype == np.uint8 and got.flags.writeable and np.array_equal(got, img)
    for bad in (b"P2\n7 5\n255\n" + img.tobytes(), b"P5\n7 5\n65535\n" + img.tobytes() * 2, b"P5\n7 5\n255\n" + img.tobytes()[:-1],
                b"P5\n7 5\n", b"P5\n0 5\n255\n", b"P5\n7 x\n255\n" + img.tobytes(), b"P5\n7 5\n255"):
        with pytest.raises(ValueError):
            masks.parse_pgm(bad)
