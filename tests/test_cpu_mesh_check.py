"""CPU suite: the PLY writer of the mesh export (co_fusion_amd/host/MeshPly.cpp) under AddressSanitizer + UBSan, in a stand-alone program
with its own main (host/mesh_check_main.cpp, `make mesh_check`): synthetic meshes -- none, one triangle, 10 000 random records -- are
written, read back and compared; missing arrays and an unwritable path are refused.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ply_writer_round_trips_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtime")
    out = tmp_path / "bin"
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "co_fusion_amd", "host"), "mesh_check", f"LIBDIR={out}"])
    r = subprocess.run([str(out / "mesh_check"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "3 accepted, 3 refused, 0 failed" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
