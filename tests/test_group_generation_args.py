"""mals_group_load_generation and its companions without a device: the argument checks that come before any group is touched,
and mals_group_generation_plan_host (csrc/generation_group_plan.h) against cases worked out by hand.  Through ctypes."""
import ctypes

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from myrrix_recommender_amd.group import generation_plan_host


def _load(struct_size=None):
    L = _lib.GenerationLoad()
    L.struct_size = ctypes.sizeof(_lib.GenerationLoad) if struct_size is None else struct_size
    L.features = 8
    return L


def test_null_group_null_load_and_struct_size_are_invalid_arg():
    lib = _lib.load()
    R = _lib.GenerationResult()
    R.struct_size = ctypes.sizeof(_lib.GenerationResult)
    good = _load()
    # a null group, whatever else is given
    assert lib.mals_group_load_generation(None, ctypes.byref(good), ctypes.byref(R)) == _lib.INVALID_ARG
    assert lib.mals_group_load_generation(None, None, None) == _lib.INVALID_ARG
    assert lib.mals_group_load_generation(None, ctypes.byref(_load(struct_size=8)), None) == _lib.INVALID_ARG
    out = np.zeros(4, dtype=np.int64)
    n = ctypes.c_int64(0)
    assert lib.mals_group_generation_get_ids(None, pkg.SIDE_X, out.ctypes.data_as(ctypes.c_void_p)) == _lib.INVALID_ARG
    assert lib.mals_group_generation_get_map(None, pkg.SIDE_Y, out.ctypes.data_as(ctypes.c_void_p)) == _lib.INVALID_ARG
    assert lib.mals_group_mark_recent(None, pkg.SIDE_X, 1, out.ctypes.data_as(ctypes.c_void_p)) == _lib.INVALID_ARG
    assert lib.mals_group_get_recent(None, pkg.SIDE_X, None, ctypes.byref(n)) == _lib.INVALID_ARG


def test_plan_host_refuses_bad_arguments():
    lib = _lib.load()
    b = np.zeros(3, dtype=np.int64)
    bp = b.ctypes.data_as(ctypes.c_void_p)
    rows = np.array([3, 2], dtype=np.int64)
    sizes = np.array([1, 1], dtype=np.int64)
    assert lib.mals_group_generation_plan_host(2, 8, 0, None, 0, None, None, None, None, None) == _lib.INVALID_ARG      # no bounds_out
    assert lib.mals_group_generation_plan_host(0, 8, 0, None, 0, None, None, None, bp, None) == _lib.INVALID_ARG        # world 0
    assert lib.mals_group_generation_plan_host(2, 8, 0, None, 2, sizes.ctypes.data_as(ctypes.c_void_p), rows.ctypes.data_as(ctypes.c_void_p),
                                               None, bp, None) == _lib.INVALID_ARG                                     # descending kept rows
    assert lib.mals_group_generation_plan_host(2, 8, 0, None, 2, None, rows.ctypes.data_as(ctypes.c_void_p), None, bp, None) == _lib.INVALID_ARG


def test_plan_host_hand_computed():
    # features = 1: a row costs its entries + 1/200.
    # (a) four new users of one entry, four kept users of one entry (two per old owner): the cut falls between them, and both
    #     old owners' kept users go to new member 1
    bounds, moves = generation_plan_host(2, 1, [0, 1, 2, 3, 4], [1, 1, 1, 1], [0, 2, 3, 5], [0, 3, 6])
    assert bounds.tolist() == [0, 4, 8]
    assert moves.tolist() == [[[0, 0], [0, 2]], [[0, 0], [0, 2]]]
    # (b) entries 2 | 2 2 2 4: half of 12 after three rows; old member 0's three kept users split 2 + 1, the user past the old
    #     bounds (a grown one) is the last rank's and stays there
    bounds, moves = generation_plan_host(2, 1, [0, 2], [2, 2, 2, 4], [0, 1, 2, 7], [0, 3, 5])
    assert bounds.tolist() == [0, 3, 5]
    assert moves.tolist() == [[[0, 2], [2, 3]], [[0, 0], [0, 1]]]
    # (c) no known items anywhere: the plan cuts by rows alone (7 merged users, 3 members: 7/3 and 14/3 round to 2 and 5)
    bounds, moves = generation_plan_host(3, 1, None, [0, 0, 0], [1, 4, 5], None, n_new=4)
    assert bounds.tolist() == [0, 2, 5, 7]
    # without old bounds every kept user is the last rank's: merged rows 4, 5, 6 -> member 1 gets the first, member 2 two
    assert moves.tolist() == [[[0, 0]] * 3, [[0, 0]] * 3, [[0, 0], [0, 1], [1, 3]]]
    # (d) an empty new model and one member: everything is its own
    bounds, moves = generation_plan_host(1, 1, [0], [5, 0, 9], [0, 1, 2], [0, 3])
    assert bounds.tolist() == [0, 3] and moves.tolist() == [[[0, 3]]]


def test_group_methods_exist():
    for name in ("load_generation", "mark_recent", "get_recent"):
        assert callable(getattr(pkg.GroupALS, name))
