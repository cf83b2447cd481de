"""CPU suite: the re-detection search's entries exist in both libraries, its structs have the sizes the Python mirrors assume, and the
host half of a registration step (cf::redetect_register_solve: Cholesky of the damped system, Rodrigues, pose update -- no GPU in it)
equals the numpy statement BIT FOR BIT on the systems of the crafted cases: the ground under the 2 ulp bound of the GPU suite."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import redetect_search_cases as sc
import redetect_search_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = ("cf_redetect_frame_moments", "cf_redetect_model_moments", "cf_redetect_register_step", "cf_redetect_register")
HOST = ("cofusion_set_redetection_search", "cofusion_redetect_search_last")


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g
    g.build()
    from co_fusion_amd import lib as cflib
    return cflib


def test_the_new_symbols_exist_in_both_libraries(libs):
    for path, names, table in ((libs.LIB_PATH, HIP, libs.SYMBOLS), (libs.HOST_LIB_PATH, HOST, libs.HOST_SYMBOLS)):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        exported = set(re.findall(r" T (\w+)", out))
        assert set(names) <= exported, sorted(set(names) - exported)
        assert set(names) <= set(table), "listed for build()'s check"
    hdr = open(os.path.join(ROOT, "include", "cofusion_hip.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, hdr) for n in HIP)
    hdr = open(os.path.join(ROOT, "include", "cofusion.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, hdr) for n in HOST)


def test_struct_sizes(libs):
    from co_fusion_amd import facade, redetect
    assert C.sizeof(redetect.Registration) == 4 * 5 + 64 == 84
    assert C.sizeof(facade.RedetectSearchCandidate) == 18 * 4 == 72
    assert C.sizeof(redetect.Counts) == 24 and C.sizeof(facade.RedetectCandidate) == 40, "the static pass's layouts are what they were"
    assert C.sizeof(redetect.Frame) == 56 and C.sizeof(redetect.Candidate) == 80
    assert redetect.BINS == 512 == ref.BINS
    hdr = open(os.path.join(ROOT, "include", "cofusion_hip.h")).read()
    assert re.search(r"#define\s+CF_REDETECT_BINS\s+512\b", hdr)


def _solve(lib):
    f = getattr(lib, "_ZN2cf23redetect_register_solveEPKxdPKdPdS4_S4_S4_")
    f.restype = C.c_bool
    f.argtypes = [C.c_void_p, C.c_double] + [C.c_void_p] * 5
    return f


def test_host_solve_equals_the_statement_bit_for_bit(libs):
    solve = _solve(libs.load())
    n = 0
    for name in sc.REGISTERED + ("gate_0", "rejects", "empty"):
        for size in sc.SIZES:
            case = sc.get(name, size)
            st = sc.statement(case)
            c = [float(v) for v in st["centre"]]
            for cand in st["cands"]:
                for which in ("T0", "seed"):
                    if cand[which] is None:
                        continue
                    T = cand[which].reshape(4, 4).astype(np.float64)
                    R = [float(v) for v in T[:3, :3].reshape(9)]; t = [float(v) for v in T[:3, 3]]
                    sums = cand["step_" + which]
                    want = ref.solve_step(sums, c, R, t)
                    s = np.array(sums, np.int64); cc = np.array(c); Rn = np.array(R); tn = np.array(t); a = np.zeros(1); b = np.zeros(1)
                    ok = solve(s.ctypes.data, ref.LAMBDA, cc.ctypes.data, Rn.ctypes.data, tn.ctypes.data, a.ctypes.data, b.ctypes.data)
                    assert bool(ok) == (want is not None), f"{name} {size} {which}"
                    if want is not None:
                        got = np.concatenate([Rn, tn, a, b])
                        exp = np.array(want[0] + want[1] + [want[2], want[3]])
                        assert got.tobytes() == exp.tobytes(), f"{name} {size} {which}: {np.abs(got - exp).max()}"
                        n += 1
    assert n >= 12, "the box and plane systems at both sizes and both poses were solved"
