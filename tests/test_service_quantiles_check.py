"""The per-service percentiles' host fold under AddressSanitizer and UBSan on the CPU
(DESIGN.md §28): tests/cpp/service_quantiles_check.cpp, a stand-alone program
with its own main, runs svq::fold_host (the loop isim_service_quantiles_host
runs) over the hand-derived vectors of tests/golden/service_quantiles_kat.json."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "istio-isotope_amd", "csrc")


def test_fold_is_clean_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "service_quantiles_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "service_quantiles_check.cpp"),
                    os.path.join(CSRC, "json.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "service_quantiles_kat.json")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
