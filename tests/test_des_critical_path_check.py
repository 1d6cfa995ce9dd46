"""The DES critical path fold under AddressSanitizer and UBSan on the CPU
(DESIGN.md §22): tests/cpp/des_critical_path_check.cpp, a stand-alone program
with its own main, runs dcp::fold_list (the loop isim_des_critical_path_host
runs) over the hand-derived traces of tests/golden/des_critical_path_kat.json
and their corruptions."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "istio-isotope_amd", "csrc")


def test_fold_is_clean_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "des_critical_path_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "des_critical_path_check.cpp"),
                    os.path.join(CSRC, "json.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "des_critical_path_kat.json")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
