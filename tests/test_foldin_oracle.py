"""tests/foldin_oracle.py pinned by hand-worked cases (CPU only): foldInWeight (ServerRecommender.java:981-994), a
three-update chain at k = 2, the partial item update on a non-finite delta (:893) and the removal rules (:1001-1074)."""
import numpy as np
import pytest

from myrrix_recommender_amd.core import HostSolver
from tests import foldin_oracle as fo


@pytest.mark.parametrize("value,estimate,expected", [
    (1.0, -1.0, 0.5), (1.0, 0.0, 0.5), (1.0, 0.5, 0.25), (1.0, 1.0, 0.0), (1.0, 2.0, 0.0),
    (0.5, 0.0, 1.0 - 1.0 / 1.5), (0.5, 0.5, (1.0 - 1.0 / 1.5) * 0.5), (0.5, 1.0, 0.0),
    (5.0, -1.0, 1.0 - 1.0 / 6.0), (5.0, 0.5, (1.0 - 1.0 / 6.0) * 0.5), (5.0, 2.0, 0.0),
    (-1.0, -1.0, 0.0), (-1.0, 0.0, 0.0), (-1.0, 0.5, -0.25), (-1.0, 1.0, -0.5), (-1.0, 2.0, -0.5),
    (-0.5, 0.5, (1.0 - 1.0 / 1.5) * -0.5), (-0.5, 2.0, -(1.0 - 1.0 / 1.5)),
    (-5.0, 0.5, (1.0 - 1.0 / 6.0) * -0.5), (-5.0, 1.0, -(1.0 - 1.0 / 6.0)), (-5.0, 0.0, 0.0),
    (0.0, -1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), (0.0, 2.0, 0.0),
])
def test_fold_in_weight(value, estimate, expected):
    assert fo.fold_in_weight(estimate, value) == expected
    assert fo.fold_in_weight(estimate, value, rate=2.0) == 2.0 * expected


def diag_solver(d):
    return HostSolver.create(np.diag(np.asarray(d, np.float64)), singularity_threshold=1e-310)


def test_three_updates_on_one_item_by_hand():
    # X^T X = diag(4, 2), Y^T Y = diag(2, 4): the solves are exact halvings / quarterings
    sx, sy = diag_solver([4.0, 2.0]), diag_solver([2.0, 4.0])
    X = np.array([[0.5, 0.0], [0.0, 0.0]], np.float32)
    Y = np.array([[1.0, 0.5]], np.float32)
    known = {}
    st = fo.set_preferences(X, Y, known, [0, 1, 0], [0, 0, 0], [1.0, 1.0, -1.0], sx, sy)
    assert st.tolist() == [0, 0, 0]
    # 1: estimate 0.5, w 0.25; itemFoldIn (0.125, 0), userFoldIn (0.5, 0.125)
    # 2: user 1 from zeros: estimate 0, w 0.5; itemFoldIn 0, userFoldIn (0.515625, 0.125)
    # 3: estimate 0.625*1.03125 + 0.03125*0.5 = 0.66015625, w = -0.330078125 (= -169/512);
    #    itemFoldIn (0.15625, 0.015625), userFoldIn (0.515625, 0.125) from Y before the update
    assert Y[0].tolist() == [16051 / 16384, 16215 / 32768]
    assert X[0].tolist() == [14903 / 32768, -41 / 4096]
    assert X[1].tolist() == [0.2578125, 0.0625]
    assert known == {0: {0}, 1: {0}}


class FixedSolver:
    """stands in for a solver whose fold-in vector is given (the loop logic alone)"""

    def __init__(self, x):
        self.x = np.asarray(x, np.float64)

    def solve_ftod(self, b):
        return self.x.copy()


def test_non_finite_item_delta_stops_the_item_loop():
    # itemFoldIn = (1, inf, 1): element 0 moves, element 1 stops the loop (checkState, :893), element 2 and x_u stay
    X = np.array([[0.5, 0.0, 0.0]], np.float32)
    Y = np.array([[1.0, 0.0, 0.0]], np.float32)
    code, why, _ = fo.update_features(X, Y, 0, 0, 1.0, FixedSolver([1.0, np.inf, 1.0]), FixedSolver([1.0, 1.0, 1.0]))
    assert (code, why) == (fo.INVALID_ARG, fo.WHY_ITEM_DELTA)
    assert Y[0].tolist() == [1.25, 0.0, 0.0] and X[0].tolist() == [0.5, 0.0, 0.0]   # w = 0.25
    # the user loop: the item row is complete, the user row stops at the NaN
    X = np.array([[0.5, 0.0, 0.0]], np.float32)
    Y = np.array([[1.0, 0.0, 0.0]], np.float32)
    code, why, _ = fo.update_features(X, Y, 0, 0, 1.0, FixedSolver([1.0, 1.0, 1.0]), FixedSolver([2.0, 4.0, np.nan]))
    assert (code, why) == (fo.INVALID_ARG, fo.WHY_USER_DELTA)
    assert Y[0].tolist() == [1.25, 0.25, 0.25] and X[0].tolist() == [1.0, 1.0, 0.0]
    # a real solver: X^T X = diag(1, 1e-300) turns x_u = (1, 3e38) into (NaN, inf) -- the loop stops at element 0
    sx, sy = diag_solver([1.0, 1e-300]), diag_solver([1.0, 1.0])
    X = np.array([[1.0, 3e38]], np.float32)
    Y = np.array([[0.25, 0.0]], np.float32)
    known = {}
    assert fo.set_preferences(X, Y, known, [0], [0], [1.0], sx, sy).tolist() == [fo.INVALID_ARG]
    assert Y[0].tolist() == [0.25, 0.0] and X[0].tolist() == [1.0, np.float32(3e38)] and known == {}


def test_xtx_without_yty_fails_before_anything_changes():
    X = np.array([[0.5, 0.5]], np.float32)
    Y = np.array([[0.5, 0.5]], np.float32)
    known = {}
    st = fo.set_preferences(X, Y, known, [0], [0], [1.0], diag_solver([1.0, 1.0]), None)
    assert st.tolist() == [fo.INVALID_ARG] and known == {}
    assert X.tolist() == [[0.5, 0.5]] and Y.tolist() == [[0.5, 0.5]]
    # no X^T X solver: only the user row moves
    st = fo.set_preferences(X, Y, known, [0], [0], [1.0], None, diag_solver([2.0, 2.0]))
    assert st.tolist() == [0] and Y.tolist() == [[0.5, 0.5]]
    assert X[0].tolist() == [0.5 + 0.25 * 0.25] * 2     # estimate 0.5, w = 0.25, userFoldIn = 0.25
    assert known == {0: {0}}


def test_removal_rules():
    X = np.ones((3, 2), np.float32)
    known = {0: {1, 2}, 1: {3}}
    removed = fo.remove_preferences(X, known, [2, 0, 0, 1, 0, 0], [1, 5, 1, 3, 2, 2])
    # user 2 unknown, item 5 unknown to 0: ignored; 1 loses its only item; 0 its two; the last pair finds no user
    assert removed == [1, 0]
    assert known == {}
    assert X[0].tolist() == [0.0, 0.0] and X[1].tolist() == [0.0, 0.0] and X[2].tolist() == [1.0, 1.0]


def test_anonymous_features_and_estimates():
    sy = diag_solver([2.0, 4.0])
    Y = np.array([[1.0, 0.5], [2.0, 4.0]], np.float32)
    acc, ok = fo.anonymous_features(Y, [-1, 0, 1], [9.0, 1.0, -1.0], sy)
    assert ok   # item 0: w = 0.5 -> (0.25, 0.0625); item 1 (value -1 at estimate 0): w = 0
    assert acc.tolist() == [0.25, 0.0625]
    assert fo.anonymous_features(Y, [-1, -1], None, sy)[1] is False
    assert fo.anonymous_features(Y, [0], None, None)[1] is False
    est, ok = fo.estimate_for_anonymous(Y, 1, [0], None, sy)
    assert ok and est == np.float32(0.25 * 2.0 + 0.0625 * 4.0)
    X = np.array([[1.0, 2.0]], np.float32)
    assert fo.estimate_preferences(X, Y, [0, -1, 0], [1, 0, -1]).tolist() == [10.0, 0.0, 0.0]
