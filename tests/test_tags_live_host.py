"""What setUserTag / setItemTag need that runs without a device: the tag hash of the C-ABI (mals_tag_id_host) against MD5 and
against the text oracle's, the tag oracle (tests/tags_live_oracle.py) on a stream whose every number is worked out by hand
below, the host cut of a tagged stream (csrc/ingest_live_plan.h) in a stand-alone program built with AddressSanitizer and
UBSan, and the argument checks of every new entry point."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from oracle import ingest_text_oracle as ito
from tests import tags_live_oracle as tlo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ingest_tag_plan.cpp")
TAGS = ["rock", "a", "", "café", "é", "\U0001F3B8", "x\U0001F3B8y", "two words", "a" * 55, "b" * 56, "c" * 64, "d" * 200]


def md5_id(b):
    v = int.from_bytes(hashlib.md5(b).digest()[:8], "big")
    return v - (1 << 64) if v >= (1 << 63) else v


@pytest.mark.parametrize("tag", TAGS)
def test_tag_id_is_the_md5_of_the_utf8_form_and_the_parsers_hash(tag):
    """ASCII, a two- and a four-byte UTF-8 character, the empty string, and lengths around MD5's 56- and 64-byte edges"""
    b = tag.encode("utf-8")
    assert pkg.tag_id(tag) == md5_id(b) == tlo.tag_id(tag) == pkg.tag_id(b)
    # ... and what the text oracle makes of the line that holds the token "<tag>"
    line = ito.java_utf8_decode(b'"' + b + b'",7,1')
    st, u, _, _, ut, _ = ito.parse_line(line, 2)
    assert st == ito.RECORD and ut and u == pkg.tag_id(tag)


def test_tag_id_arguments():
    L = _lib.load()
    out = ctypes.c_int64(5)
    assert L.mals_tag_id_host(None, 0, ctypes.byref(out)) == _lib.OK and out.value == md5_id(b"") == tlo.EMPTY_TAG_ID
    assert L.mals_tag_id_host(None, 3, ctypes.byref(out)) == _lib.INVALID_ARG
    assert L.mals_tag_id_host(b"abc", -1, ctypes.byref(out)) == _lib.INVALID_ARG
    assert L.mals_tag_id_host(b"abc", 3, None) == _lib.INVALID_ARG


class Halver:
    """the solver of A = 2 I: solveFToD(b) = b / 2"""

    def solve_ftod(self, b):
        return np.asarray(b, np.float64) / 2.0


def test_the_oracle_on_a_stream_worked_out_by_hand():
    """k = 1, X = [[1]] (user 10), Y = [[0.5]] (item 20), user 10 knows item 20, both solvers halve.  foldInWeight(e, v) for
    v > 0 and e < 1 is (1 - 1 / (1 + v)) (1 - max(0, e)).
      1. 10,"rock",1   setUserTag: the tag is a new row 1 of Y (zero).  e = 0, w = 1/2.  itemFoldIn = x / 2 = 1/2, userFoldIn =
                       y / 2 = 0: y_rock = 1/4, x_10 stays 1.  userTagIDs = {row 1}.  No known item.
      2. "rock",20,    a tag remove: ignored -- "rock" gets no row of X, lines 1 and 3 are one write call.
      3. "new",20,1    setItemTag: the tag is a new row 1 of X (zero).  e = 0, w = 1/2.  itemFoldIn = 0, userFoldIn = 1/4:
                       y_20 stays 1/2, x_new = 1/8.  itemTagIDs = {row 1}.
      4. 10,20,        removePreference: user 10's only known item goes, its row of X is zeroed, id 10 is reported.
      5. 10,"rock",3   setUserTag again: x_10 = 0, y_rock = 1/4, e = 0, w = 3/4.  itemFoldIn = 0, userFoldIn = 1/8:
                       x_10 = 3/32.  Still no known item: user 10 stays empty."""
    text = b'10,"rock",1\n"rock",20,\n"new",20,1\n10,20,\n10,"rock",3\n'
    m = tlo.TagModel([[1.0]], [[0.5]], {0: {0}}, [10], [20], Halver(), Halver())
    st, removed, statuses, tg = m.apply_text(text)
    X, Y = m.arrays()
    assert X.tolist() == [[3 / 32], [1 / 8]] and Y.tolist() == [[1 / 2], [1 / 4]]
    assert m.user_ids == [10, tlo.tag_id("new")] and m.item_ids == [20, tlo.tag_id("rock")]
    assert m.user_tag_rows == {1} and m.item_tag_rows == {1} and not any(m.known.values())
    assert st == dict(records=5, sets=3, removes=1, removes_dropped=0, sets_failed=0, new_users=1, new_items=1, write_calls=3)
    assert tg == dict(item_tag_sets=1, user_tag_sets=2, tag_removes_ignored=1, rows_marked=2)
    assert removed == [10] and statuses == [0, 0, 0]


def test_the_oracle_refuses_a_set_of_the_empty_tag_and_ignores_its_remove():
    for tok in ('""', '"a', '"é'):
        with pytest.raises(tlo.EmptyTag):
            tlo.parse_text(("1,2,1\n%s,5,1\n" % tok).encode())
        u, i, v, kd, _, _, _ = tlo.parse_text(("1,2,1\n%s,5,\n" % tok).encode())
        assert kd.tolist() == [0, 1] and np.isnan(v[1]) and u[1] == tlo.EMPTY_TAG_ID
    # a four-byte character is two chars: the tag is its lone high surrogate, not empty
    u, _, _, kd, _, _, _ = tlo.parse_text('"\U0001F3B8,5,1\n'.encode())
    assert kd.tolist() == [1] and u[0] != tlo.EMPTY_TAG_ID


@pytest.fixture(scope="module")
def tag_plan_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ingest_tag_plan") / "test_ingest_tag_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_the_cut_of_a_tagged_stream(tag_plan_exe, seed):
    r = subprocess.run([tag_plan_exe, str(seed)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    fields = r.stdout.splitlines()[-1].split()
    assert fields[0] == "checks" and int(fields[1]) > 10000 and fields[2:] == ["failures", "0"], fields


def test_null_handles_and_the_new_symbols():
    L = _lib.load()
    one = np.zeros(1, np.int64)
    p = one.ctypes.data_as(ctypes.c_void_p)
    for name in ("mals_set_user_tags", "mals_set_item_tags", "mals_group_set_user_tags", "mals_group_set_item_tags"):
        assert name in _lib.SYMBOLS
        assert getattr(L, name)(None, 1, p, p, p, p) == _lib.INVALID_ARG
    n = ctypes.c_int64(0)
    assert L.mals_get_tag_rows(None, _lib.SIDE_Y, p, 1, ctypes.byref(n)) == _lib.INVALID_ARG
    assert L.mals_ingest_apply_tag_stats(None, p) == _lib.INVALID_ARG
    assert L.mals_ingest_set_option(None, _lib.INGEST_OPT_LIVE_TAGS, 1) == _lib.INVALID_ARG
    assert _lib.INGEST_OPT_LIVE_TAGS == 7 and pkg.ingest.INGEST_OPT_LIVE_TAGS == 7
    assert L.mals_abi_version() == 5
