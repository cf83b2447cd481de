"""CPU suite: the PNG assembler of the asynchronous exports (co_fusion_amd/host/PngAssemble.cpp) under AddressSanitizer + UBSan, in a
stand-alone program with its own main (host/export_check_main.cpp, `make export_check`): synthetic band tables -- stored bands, one in
the fixed code, a band of 65535 bytes, partial bands -- are assembled and read back with the project's own pngDecode, and tables that
do not describe their image or reach outside their slot are refused.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_assembler_stays_inside_the_band_table_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtime")
    out = tmp_path / "bin"
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "co_fusion_amd", "host"), "export_check", f"LIBDIR={out}"])
    r = subprocess.run([str(out / "export_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "7 accepted, 17 refused, 0 failed" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
