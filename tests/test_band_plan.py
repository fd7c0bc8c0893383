"""The piece planner of the banded long rows (csrc/band_plan.h) on the CPU: tests/cpp/test_band_plan.cpp,
a stand-alone program over the header, built with AddressSanitizer and UBSan and run on random sorted rows.  What it checks
per row is listed at its head: exact partition, no piece across a band, none empty or above segment_nnz, at most n_bands
extra slots, the same cuts whatever other rows were planned before."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_band_plan.cpp")


@pytest.fixture(scope="module")
def planner_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("band_plan") / "test_band_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sorted_rows(planner_exe, seed):
    r = subprocess.run([planner_exe, str(seed), "1500"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    fields = r.stdout.split()
    assert fields[0] == "rows" and fields[-2:] == ["failures", "0"], r.stdout
    assert int(fields[3]) > 1500 and int(fields[5]) > 0, r.stdout     # pieces were planned, and some carried a thin band along
