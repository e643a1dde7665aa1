"""The offset arithmetic of pm_graph_group_get_vertex_info (pm_gvi_offs.h: the
offs walk, ragged slices, the id range check, the step count) as a stand-alone
host program built with AddressSanitizer and UBSan and run on the CPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_gvi_offs_under_sanitizers(tmp_path):
    cxx = shutil.which("clang++") or shutil.which("g++") or shutil.which("c++")
    if cxx is None and Path("/opt/rocm/llvm/bin/clang++").exists():
        cxx = "/opt/rocm/llvm/bin/clang++"
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "gvi_offs_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "host" / "gvi_offs_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gvi_offs_check: ok" in r.stdout
