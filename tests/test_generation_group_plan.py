"""The ownership plan of mals_group_load_generation (csrc/generation_group_plan.h: the new bounds over the merged users, the
old owners' runs of the kept list, which run moves to which new owner) on the CPU: tests/cpp/test_generation_group_plan.cpp, a
stand-alone program over the header, built with AddressSanitizer and UBSan and run as a child process.  What it checks is
listed at its head; no device and no library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_generation_group_plan.cpp")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("generation_group_plan") / "test_generation_group_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_generation_group_plan(plan_exe, seed):
    r = subprocess.run([plan_exe, str(seed)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    fields = r.stdout.splitlines()[-1].split()
    assert fields[0] == "checks" and int(fields[1]) > 10000 and fields[2:] == ["failures", "0"], fields
