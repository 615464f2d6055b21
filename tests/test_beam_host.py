"""The beam decode's host-side bookkeeping (csrc/qtx_beam.h: the reorder's chunk mapping and
region / prefix arithmetic, the argument limits; csrc/qtx_carve.h: carve_beam, the whole
workspace carved from exactly beam_ws bytes) under AddressSanitizer and UBSan:
tools/beam_host_check.cpp is a stand-alone host program (its own main, no GPU, no HIP), built
and run here.  Nothing is loaded into Python under a sanitizer."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_beam_host_bookkeeping_sanitized(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "beam_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "onnx-transformer_amd", "csrc"),
                    os.path.join(REPO, "tools", "beam_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "beam host checks ok" in r.stdout
