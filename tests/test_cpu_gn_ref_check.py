"""CPU suite: the host algebra of the reference-order mode (co_fusion_amd/csrc/gn_ref_host.h: the left-looking pivoted LDL^T with its
four-part in-place swap, Rodrigues, the 4x4 inverse) on the crafted systems of tests/solve_cases.py, under AddressSanitizer + UBSan,
in a stand-alone program with its own main (csrc/gn_ref_check_main.cpp, `make gn_ref_check`).  The program reads the systems from a
file and prints the results as hex words; they are compared BIT FOR BIT (NaN equal to NaN) with the oracle's statement of the same
algebra (eig_ldlt_solve_d / _f, eig_inv44d, its reference-order Rodrigues).  Nothing is loaded into python."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import orc
import solve_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(a):
    a = np.ascontiguousarray(a)
    return " ".join("%x" % int(v) for v in a.reshape(-1).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]))


def _same(got, want):
    u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return bool(np.all((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))))


def _systems3():
    """3x3 f32 analogues for the SO(3) solve: every pivot order, ties, exact zero pivots, a rank deficiency by rounding"""
    rng = np.random.default_rng(sc.SEED + 30)
    J = rng.integers(-7, 8, (6, 3)); r = rng.integers(-7, 8, 6)
    out = []
    for perm in itertools.permutations(range(3)):
        Js = J * np.array([1 << (3 * p) for p in perm])
        out.append(("perm%s" % (perm,), Js.T @ Js, Js.T @ r))
    out += [("all-equal", np.diag([8, 8, 8]), [1, -2, 3]), ("first-of-two", np.diag([1, 8, 8]), [1, -2, 3]), ("late-pair", np.diag([8, 2, 2]), [1, -2, 3]),
            ("opposite-signs", [[4, 1, 0], [1, -4, 1], [0, 1, 2]], [1, 2, 3]), ("zero", np.zeros((3, 3)), [1, 2, 3]),
            ("zero-column", [[4, 0, 2], [0, 0, 0], [2, 0, 8]], [1, 2, 3]), ("duplicated", [[4, 4, 0], [4, 4, 0], [0, 0, 1]], [8, 8, 1]),
            ("one-row", np.outer([1, 2, 4], [1, 2, 4]), [3, 6, 12])]
    K = rng.integers(-3, 4, (6, 2)) @ rng.integers(-3, 4, (2, 3))
    out.append(("rank2", K.T @ K, [1, -1, 2]))
    return [(n, np.asarray(A, np.float32), np.asarray(b, np.float32)) for n, A, b in out]


def test_reference_order_host_algebra_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtime")
    out = tmp_path / "bin"
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "co_fusion_amd", "csrc"), "gn_ref_check", f"LIBDIR={out}"])

    lines, want = [], []
    for fam in ("pivots", "ties", "zero pivots", "rotations"):
        for c in sc.family(fam):
            (state, tr), = sc.reference(c.name)
            A = np.array(state.stats.lastA).reshape(6, 6); b = np.array(state.stats.lastb)
            lines.append("L6 %s %s" % (_hex(A), _hex(b)))
            want.append((c.name, "L6", orc.eig_ldlt_solve(A, b)))
            if fam == "rotations":   # the rotation vector this system solves to, through the reference-order Rodrigues (the C library's cos / sin)
                w = np.array(tr.result[3:6])
                lines.append("R %s" % _hex(w))
                want.append((c.name, "R", orc.ref_rodrigues(w).reshape(9)))
    for n, A, b in _systems3():
        lines.append("L3 %s %s" % (_hex(A), _hex(b)))
        want.append(("3x3 " + n, "L3", orc.eig_ldlt_solve(A, b)))
    # the general 4x4 inverse: the rigid poses the levels family ends with, and general matrices (integers, all sixteen entries in
    # play, no symmetry: a transposed or misplaced cofactor changes the result), a singular one among them
    mats = [np.array(sc.reference(c.name)[0][0].resultRt).reshape(4, 4) for c in sc.family("levels")]
    rng = np.random.default_rng(sc.SEED + 31)
    mats += [rng.integers(-9, 10, (4, 4)).astype(np.float64) for _ in range(8)] + [rng.normal(size=(4, 4)) for _ in range(4)]
    mats.append(np.array([[1, 2, 3, 4], [2, 4, 6, 8], [0, 1, 0, 1], [5, 0, 0, 1]], np.float64))
    for k, M in enumerate(mats):
        lines.append("I %s" % _hex(M))
        want.append(("4x4 inverse %d" % k, "I", orc.eig_inv44(M).reshape(16)))
    src = tmp_path / "systems.txt"
    src.write_text("\n".join(lines) + "\n")

    r = subprocess.run([str(out / "gn_ref_check"), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want) and "%d systems" % len(want) in r.stderr
    bad = []
    for line, (name, tag, w) in zip(got, want):
        t, *words = line.split()
        assert t == tag, (name, line)
        g = np.array([int(x, 16) for x in words], {4: np.uint32, 8: np.uint64}[w.dtype.itemsize]).view(w.dtype)
        if not _same(g, w):
            bad.append("%s %s: checker %s, oracle %s" % (name, tag, g.tolist(), w.tolist()))
    assert not bad, "\n".join(bad[:10])
    # the table reached the branches of the 3x3 solve as well: the three transpositions of the left-looking swap
    assert len([w for w in want if w[1] == "L3"]) >= 15 and len([w for w in want if w[1] == "L6"]) > 800
