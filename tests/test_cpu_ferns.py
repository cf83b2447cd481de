"""CPU suite of the fern keyframe relocaliser: the numpy reference agrees with itself (the literal inverted-list form of Ferns.cpp
against the vectorised scan form the GPU kernel implements), the table generator is deterministic and in range, and the libraries
export the cf_ferns_* / cofusion_*reloc* entry points with the documented signatures.  No GPU call is made."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ferns_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g
    g.build()
    from co_fusion_amd import lib as cflib
    return cflib


@pytest.mark.parametrize("n,K", [(1, 1), (7, 5), (63, 63), (64, 64), (65, 65), (500, 40), (2048, 9)])
def test_inverted_lists_equal_the_scan_form(n, K):
    rng = np.random.default_rng(n)
    table = fr.random_table(rng, n)
    if n == 1:   # the one fern sits where the base frame has depth
        ys, xs = np.nonzero(fr.reduce_maps(*fr.base_maps())[0][..., 2] > 0)
        table["x"], table["y"] = xs[0], ys[0]
    db = fr.Database(table)
    for i in range(K):
        v4, n4, rgba = fr.variant(i)
        db.add_frame(v4, n4, rgba, fr.pose_of(i), 10 + i, -1.0)
    assert len(db.frames) == K
    codes = np.stack([f.codes for f in db.frames]); good = np.array([f.good for f in db.frames]); time = np.array([f.time for f in db.frames])
    for q, qtime, min_age in ((0, 500, 300), (K // 2, 30, 5), (K + 3, 10 + K, 0), (K + 4, 0, 300)):
        v4r, _, rgb = fr.reduce_maps(*fr.variant(q))
        cl, gl = fr.codes_literal(table, v4r, rgb)
        cv, gv = fr.codes_vector(table, v4r, rgb)
        assert np.array_equal(cl, cv) and gl == gv
        m_add, co_add = db.add_minimum(cl, gl)
        m, mid, co = db.find(cl, gl, qtime, min_age)
        vco, vall, vmatch, vid = fr.search_vector(cl, gl, codes, good, time, qtime, min_age)
        assert np.array_equal(co, vco) and np.array_equal(co_add, vco)
        assert np.float32(m_add).tobytes() == np.float32(vall).tobytes()
        assert np.float32(m).tobytes() == np.float32(vmatch).tobytes() and mid == vid


def test_edge_case_codes():
    t = fr.edge_case_table()
    v4r, _, rgb = fr.reduce_maps(*fr.edge_case_maps())
    cl, gl = fr.codes_literal(t, v4r, rgb)
    cv, gv = fr.codes_vector(t, v4r, rgb)
    assert np.array_equal(cl, cv) and gl == gv == 10
    # equal is not greater (colour and depth); z == 0 and z < 0 are bad, a tiny z is good
    assert list(cl) == [0, 0b1001, 0, 0b1000, 0b0011, 255, 255, 0b1110, 0, 0, 0b1111, 0]


def test_all_bad_codes_are_never_appended_or_matched():
    t = fr.random_table(np.random.default_rng(3), 40)
    db = fr.Database(t)
    assert db.add_frame(*fr.variant(0), fr.pose_of(0), 1, -1.0)[0]
    v4, n4, rgba = (a.copy() for a in fr.base_maps())
    v4[..., 2] = 0
    ok, minimum, _ = db.add_frame(v4, n4, rgba, fr.pose_of(1), 2, -1.0)
    assert not ok and minimum == fr.FLT_MAX
    c, g = fr.codes_literal(t, *fr.reduce_maps(v4, n4, rgba)[::2])
    assert g == 0 and db.find(c, g, 1000, 0)[1] == -1


def test_photometric_check_conventions():
    t = fr.random_table(np.random.default_rng(4), 60)
    v4r, n4r, rgb = fr.reduce_maps(*fr.base_maps())
    vm, _ = fr.planar(v4r, n4r)
    I = np.eye(4, dtype=np.float32)
    # identity pose difference: every point projects where the intrinsics put it; none inside a 16x8 image from these random x, y
    err, cnt, _ = fr.photometric_check(t, vm, rgb, I, I, rgb, 1e-9, 1e-9, 3.3, 2.2, fr.MAX_DEPTH_MM)
    # (fx ~ 0: every correspondence is (3, 2) -> compared against the keyframe's pixel (3, 2))
    assert cnt > 0 and np.isfinite(err)
    err0, cnt0, _ = fr.photometric_check(t, vm, rgb, I, I, np.zeros_like(rgb), 1e-9, 1e-9, 3.3, 2.2, fr.MAX_DEPTH_MM)
    assert cnt0 == 0 and err0 == float("inf")


def test_table_generator_is_deterministic_and_in_range(libs):
    from co_fusion_amd import ferns
    a = ferns.make_table(12345, 2048, 80, 60, 5000)
    b = ferns.make_table(12345, 2048, 80, 60, 5000)
    c = ferns.make_table(12346, 2048, 80, 60, 5000)
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert a["x"].min() >= 0 and a["x"].max() < 80 and a["y"].min() >= 0 and a["y"].max() < 60
    for k in "rgb":
        assert a[k].min() >= 0 and a[k].max() <= 255
    assert a["d"].min() >= 400 and a["d"].max() <= 5000
    assert len(np.unique(a["x"])) == 80 and len(np.unique(a["y"])) == 60   # every column and row is drawn
    # the generator written down in DESIGN.md 4.8: splitmix64, six draws per fern
    s = 12345
    def draw():
        nonlocal s
        s = (s + 0x9E3779B97F4A7C15) & (2**64 - 1)
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        return z ^ (z >> 31)
    for i in range(5):
        want = (draw() % 80, draw() % 60, draw() % 256, draw() % 256, draw() % 256, 400 + draw() % 4601)
        assert tuple(int(v) for v in a[i]) == want
    lib = ferns.bind(libs.load())
    out = np.zeros(4, ferns.FERN)
    assert lib.cf_ferns_table(1, 0, 80, 60, 5000, out.ctypes.data) != 0
    assert lib.cf_ferns_table(1, 2049, 80, 60, 5000, out.ctypes.data) != 0
    assert lib.cf_ferns_table(1, 4, 80, 60, 399, out.ctypes.data) != 0


def _prototypes(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(2): (m.group(1).strip(), [a.strip() for a in m.group(3).split(",")])
            for m in re.finditer(r"^(int|void)\s+(c[of][a-z_]*(?:ferns|reloc)[a-z_]*)\s*\(([^;]*?)\)\s*;", src, flags=re.M | re.S)}


def _ctype_of(arg):
    arg = re.sub(r"\s+", " ", arg)
    if "*" in arg or "[" in arg:
        return "ptr"
    return {"int": "int", "float": "float", "uint64_t": "u64"}[arg.rsplit(" ", 1)[0].replace("const ", "")]


def test_relocalisation_entry_points_are_exported_with_the_documented_signatures(libs):
    from co_fusion_amd import ferns
    protos = _prototypes("cofusion_hip.h")
    assert set(protos) == set(ferns.SIGNATURES) and len(protos) == 12
    kind = lambda t: "ptr" if t is C.c_void_p or hasattr(t, "contents") or t is None else {C.c_int: "int", C.c_float: "float", C.c_uint64: "u64"}[t]
    for name, (ret, args) in protos.items():
        res, argtypes = ferns.SIGNATURES[name]
        assert (ret == "void") == (res is None), name
        assert [_ctype_of(a) for a in args] == [kind(t) for t in argtypes], name
    out = subprocess.check_output(["nm", "-D", "--defined-only", libs.LIB_PATH]).decode()
    exported = set(re.findall(r" T (\w+)", out))
    assert set(protos) <= exported and set(protos) <= set(libs.SYMBOLS)
    # the result / config PODs of the header and of the binding have the same size
    assert C.sizeof(ferns.FernsResult) == 104 and C.sizeof(ferns.FernsConfig) == 16 and ferns.FERN.itemsize == 24
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cofusion_hip.h")).read(), flags=re.S)
    for struct, n_members in (("cf_ferns_result", 10), ("cf_ferns_config", 4), ("cf_fern", 6)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, hdr).group(1)
        assert len(re.findall(r"\b[a-z_0-9]+(?:\[\d+\])?\s*[,;]", body)) == n_members, struct
    fac = _prototypes("cofusion.h")
    assert [_ctype_of(a) for a in fac["cofusion_set_relocalisation"][1]] == ["ptr", "int", "int", "float", "float", "int", "u64", "int"]
    assert [_ctype_of(a) for a in fac["cofusion_reloc_stats"][1]] == ["ptr"] * 5
    out = subprocess.check_output(["nm", "-D", "--defined-only", libs.HOST_LIB_PATH]).decode()
    exported = set(re.findall(r" T (\w+)", out))
    assert {"cofusion_set_relocalisation", "cofusion_reloc_stats"} <= exported
    assert {"cofusion_set_relocalisation", "cofusion_reloc_stats"} <= set(libs.HOST_SYMBOLS)
    # argument checks that need no GPU
    host = libs.load_host()
    assert host.cofusion_set_relocalisation(None, 1, 500, C.c_float(0.3095), C.c_float(115.0), 300, C.c_uint64(0), 64) != 0
    assert host.cofusion_reloc_stats(None, None, None, None, None) != 0
    lib = ferns.bind(libs.load())
    assert lib.cf_ferns_create(None, None, None, 0, None) != 0 and lib.cf_ferns_encode(None, None, None, None) != 0
    assert lib.cf_ferns_relocalise(None, None, 0, 0, 0, None) != 0 and lib.cf_ferns_count(None, None, None) != 0
