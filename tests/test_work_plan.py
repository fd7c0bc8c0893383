"""The list planner of the solve (csrc/work_plan.h) on the CPU: tests/cpp/test_work_plan.cpp, a
stand-alone program over the header, built with AddressSanitizer and UBSan and run on random row-length mixes.  What it
checks per plan is listed at its head: every row in exactly one list, the order inside the lists, the segments of a long row
and their slots, the slot groups, the counters.  The count cuts it prints tie tests/rows_cases.segment_cuts, which the
exact-rows tests depend on, to the code."""
import os
import shutil
import subprocess

import pytest

from tests import rows_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_work_plan.cpp")


@pytest.fixture(scope="module")
def planner_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("work_plan") / "test_work_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    return exe


def run(exe, seed):
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_row_mixes(planner_exe, seed):
    fields = run(planner_exe, seed)[-1].split()
    assert fields[0] == "plans" and fields[-2:] == ["failures", "0"], fields
    # 4 x 4 x 3 x 2 x 2 plans; rows went through the slot groups and through the band cuts
    assert int(fields[1]) == 192 and int(fields[3]) > 0 and int(fields[5]) > 0, fields


def test_count_cuts_match_the_python_restatement(planner_exe):
    cuts = [line.split()[1:] for line in run(planner_exe, 1) if line.startswith("cuts ")]
    assert len(cuts) >= 8
    for length, seg, *starts in ([int(x) for x in c] for c in cuts):
        assert starts == rows_cases.segment_cuts(length, seg), (length, seg)
