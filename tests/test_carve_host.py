"""The decode and scoring workspaces' carving (csrc/qtx_carve.h: carve_greedy, group_view,
carve_dfault, carve_kvfault, carve_score and their size functions) under AddressSanitizer and
UBSan: tools/carve_host_check.cpp is a stand-alone host program (its own main, no GPU, no
HIP), built and run here.  Nothing is loaded into Python under a sanitizer."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_carving_sanitized(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "carve_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "onnx-transformer_amd", "csrc"),
                    os.path.join(REPO, "tools", "carve_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "carve host checks ok" in r.stdout
