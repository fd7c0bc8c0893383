"""The owners of HIP events and streams (csrc/hip_buffer.h: Event, Stream, EventPair) on the CPU: tests/cpp/test_hip_owners.cpp,
a stand-alone program that instantiates them over a recording fake in place of the runtime, built with AddressSanitizer and
UBSan and run as a child process.  What it checks is listed at its head; it calls no HIP function, so it links without the HIP
runtime.  And the rule the owners exist for: events and streams are created and destroyed in csrc/ in hip_buffer.h alone."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hip_owners.cpp")
CSRC = os.path.join(ROOT, "myrrix-recommender_amd", "csrc")


@pytest.fixture(scope="module")
def hip_owners_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH") or "/opt/rocm"
    exe = str(tmp_path_factory.mktemp("hip_owners") / "test_hip_owners")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe, SRC])
    return exe


def test_event_and_stream_owners_over_a_recording_fake(hip_owners_exe):
    r = subprocess.run([hip_owners_exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    fields = r.stdout.splitlines()[-1].split()
    assert fields[0] == "checks" and int(fields[1]) > 100 and fields[2:] == ["failures", "0"], fields


def test_events_and_streams_are_created_and_destroyed_in_hip_buffer_h_alone():
    api = re.compile(r"hipEventCreate|hipEventDestroy|hipStreamCreate|hipStreamDestroy")
    # the sources: every file of csrc/ but what a build leaves there (the library names the runtime's symbols)
    files = sorted(p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p) and not p.endswith((".so", ".o", ".a")))
    assert len(files) > 30 and all(p.endswith((".h", ".hip", ".cpp", "Makefile")) for p in files), files
    found = {}
    for p in files:
        with open(p, encoding="utf-8", errors="replace") as f:
            lines = [i + 1 for i, line in enumerate(f) if api.search(line)]
        if lines:
            found[os.path.basename(p)] = lines
    assert list(found) == ["hip_buffer.h"], found
    assert len(found["hip_buffer.h"]) == 4, found   # one call each, inside the two policies
