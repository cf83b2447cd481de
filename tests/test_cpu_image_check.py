"""CPU suite: the image parsers (co_fusion_amd/host/ImageIO.cpp) under AddressSanitizer + UBSan, in a stand-alone program with its own
main (host/image_check_main.cpp, `make image_check`): the fixtures of tests/golden/image_seq, EVERY prefix truncation of each and a fixed
table of byte corruptions.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parsers_stay_inside_their_buffers_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtime")
    out = tmp_path / "bin"
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "co_fusion_amd", "host"), "image_check", f"LIBDIR={out}"])
    r = subprocess.run([str(out / "image_check"), os.path.join(ROOT, "tests", "golden", "image_seq")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "38 files" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
