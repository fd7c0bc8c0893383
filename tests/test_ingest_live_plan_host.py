"""The host logic of mals_ingest_apply (csrc/ingest_live_plan.h: classification, the cut into runs) and the slot functions of
the id directory (csrc/ids_kernels.h, as a host compiler sees it) on the CPU: tests/cpp/test_ingest_live_plan.cpp, a
stand-alone program over those two headers alone, built with AddressSanitizer and UBSan and run as a child process.  What it
checks is listed at its head; no device and no library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ingest_live_plan.cpp")


@pytest.fixture(scope="module")
def live_plan_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ingest_live_plan") / "test_ingest_live_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_run_cutting_and_directory_slots(live_plan_exe, seed):
    r = subprocess.run([live_plan_exe, str(seed)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    fields = r.stdout.splitlines()[-1].split()
    assert fields[0] == "checks" and int(fields[1]) > 10000 and fields[2:] == ["failures", "0"], fields
