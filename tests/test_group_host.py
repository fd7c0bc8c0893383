"""The host arithmetic of a multi-GPU group (csrc/group_plan.h: owners, exchange chunks, CSR slices, owner runs, the shard
plan) and the convergence loop shared by mals_factorize and mals_group_factorize (csrc/convergence.h) on the CPU:
tests/cpp/test_group_host.cpp, a stand-alone program over the two headers, built with AddressSanitizer and UBSan and run as a
child process.  What it checks is listed at its head; the loop runs over a scripted driver, no device and no library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_group_host.cpp")


@pytest.fixture(scope="module")
def group_host_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("group_host") / "test_group_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_group_plan_and_convergence_loop(group_host_exe, seed):
    r = subprocess.run([group_host_exe, str(seed)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    fields = r.stdout.splitlines()[-1].split()
    assert fields[0] == "checks" and int(fields[1]) > 10000 and fields[2:] == ["failures", "0"], fields
