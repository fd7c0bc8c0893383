"""tests/generation_load_oracle.py pinned by cases worked out by hand from GenerationLoader.java:49-106 (no GPU, no
library): every expected value below was written down from the Java, not produced by the oracle."""
import numpy as np

from tests import generation_load_oracle as glo


def live():
    """Users 10, 11, 12, 13 (rows 0..3), items 100, 101, 102 (rows 0..2); vectors (id, 0)."""
    return {"X": {u: (float(u), 0.0) for u in (10, 11, 12, 13)},
            "Y": {i: (float(i), 0.0) for i in (100, 101, 102)},
            "known": {10: {100, 101}, 11: {101}, 12: {102}, 13: {100, 102}},
            "item_tags": {12}, "user_tags": {102}}


def new_model(users, items, known):
    return ({u: (float(u), 1.0) for u in users}, {i: (float(i), 1.0) for i in items}, {u: set(known[u]) for u in users})


def test_overlap_nothing_recent():
    g = live()
    nx, ny, nk = new_model((11, 14), (101, 103), {11: {103}, 14: {101, 103}})
    glo.load_model(g, nx, ny, nk, set(), set(), set(), set())
    assert list(g["X"]) == [11, 14] and g["X"][11] == (11.0, 1.0)          # updated, and 10, 12, 13 pruned
    assert list(g["Y"]) == [101, 103] and g["Y"][101] == (101.0, 1.0)
    assert g["known"] == {11: {103}, 14: {101, 103}}                         # a put: 11's live set is replaced whole
    assert g["item_tags"] == set() and g["user_tags"] == set()               # live tags, not updated, not recent: gone
    d = glo.dense(g, [10, 11, 12, 13], [100, 101, 102], [11, 14], [101, 103])
    assert d["user_ids"].tolist() == [11, 14] and d["item_ids"].tolist() == [101, 103]
    assert d["user_map"].tolist() == [-1, 0, -1, -1] and d["item_map"].tolist() == [-1, 0, -1]
    assert d["known"][0].tolist() == [0, 1, 3] and d["known"][1].tolist() == [1, 0, 1]
    assert d["n_known_dropped"] == 0


def test_recent_rows_are_kept_behind_the_new_ones_in_live_order():
    g = live()
    nx, ny, nk = new_model((14, 11), (103,), {14: {103}, 11: set()})
    ru, ri = {13, 10}, {102}
    glo.load_model(g, nx, ny, nk, set(), set(), ru, ri)
    assert ru == set() and ri == set()                                       # :97-98
    assert set(g["X"]) == {10, 11, 13, 14} and g["X"][10] == (10.0, 0.0) and g["X"][13] == (13.0, 0.0)
    assert set(g["Y"]) == {102, 103} and g["Y"][102] == (102.0, 0.0)
    assert g["known"] == {14: {103}, 11: set(), 10: {100, 101}, 13: {100, 102}}
    d = glo.dense(g, [10, 11, 12, 13], [100, 101, 102], [14, 11], [103])
    assert d["user_ids"].tolist() == [14, 11, 10, 13]                        # new order, then kept in live order
    assert d["item_ids"].tolist() == [103, 102]
    assert d["user_map"].tolist() == [2, 1, -1, 3] and d["item_map"].tolist() == [-1, -1, 1]
    # the kept users' sets name pruned items 100 and 101: dropped and counted (10 loses both, 13 loses 100)
    assert d["known"][0].tolist() == [0, 1, 1, 1, 2] and d["known"][1].tolist() == [0, 1]
    assert d["n_known_dropped"] == 3
    assert d["X"][2].tolist() == [10.0, 0.0] and d["X"][1].tolist() == [11.0, 1.0]


def test_a_recent_id_the_new_model_also_has_takes_the_new_vector():
    g = live()
    nx, ny, nk = new_model((11,), (101,), {11: {101}})
    glo.load_model(g, nx, ny, nk, set(), set(), {11}, {101})
    assert g["X"] == {11: (11.0, 1.0)} and g["Y"] == {101: (101.0, 1.0)}


def test_disjoint_everything_recent_and_identical():
    g = live()
    nx, ny, nk = new_model((20, 21), (200,), {20: {200}, 21: set()})
    glo.load_model(g, nx, ny, nk, set(), set(), {10, 11, 12, 13}, {100, 101, 102})
    d = glo.dense(g, [10, 11, 12, 13], [100, 101, 102], [20, 21], [200])
    assert d["user_ids"].tolist() == [20, 21, 10, 11, 12, 13] and d["item_ids"].tolist() == [200, 100, 101, 102]
    assert d["user_map"].tolist() == [2, 3, 4, 5] and d["n_known_dropped"] == 0
    assert d["known"][0].tolist() == [0, 1, 1, 3, 4, 5, 7] and d["known"][1].tolist() == [0, 1, 2, 2, 3, 1, 3]
    g = live()                                                               # identical ids: every row updated, none kept
    nx, ny, nk = new_model((10, 11, 12, 13), (100, 101, 102), live()["known"])
    glo.load_model(g, nx, ny, nk, set(), set(), set(), set())
    d = glo.dense(g, [10, 11, 12, 13], [100, 101, 102], [10, 11, 12, 13], [100, 101, 102])
    assert d["user_map"].tolist() == [0, 1, 2, 3] and d["item_map"].tolist() == [0, 1, 2]
    assert all(v == (float(u), 1.0) for u, v in g["X"].items())


def test_keep_not_updated_keeps_every_live_row():
    g = live()
    nx, ny, nk = new_model((11, 14), (103,), {11: set(), 14: {103}})
    glo.load_model(g, nx, ny, nk, {14}, {103}, set(), set(), remove_not_updated_data=False)
    assert list(g["X"]) == [10, 11, 12, 13, 14] and g["X"][11] == (11.0, 1.0) and g["X"][12] == (12.0, 0.0)
    assert g["item_tags"] == {12, 14} and g["user_tags"] == {102, 103}
    d = glo.dense(g, [10, 11, 12, 13], [100, 101, 102], [11, 14], [103])
    assert d["user_ids"].tolist() == [11, 14, 10, 12, 13] and d["user_map"].tolist() == [2, 0, 3, 4]
    assert d["tag_users"].tolist() == [1, 3] and d["tag_items"].tolist() == [0, 3]


def test_tag_ids_updated_live_and_recent_live_and_not_recent():
    g = live()
    g["item_tags"] = {12, 13}                                                # live: 12 recent, 13 not
    g["user_tags"] = {100, 102}                                              # live: 100 recent, 102 not
    nx, ny, nk = new_model((11, 15), (101, 104), {11: set(), 15: set()})
    glo.load_model(g, nx, ny, nk, {15, 77}, {104}, {12}, {100})
    assert g["item_tags"] == {12, 15, 77} and g["user_tags"] == {100, 104}
    d = glo.dense(g, [10, 11, 12, 13], [100, 101, 102], [11, 15], [101, 104])
    assert d["user_ids"].tolist() == [11, 15, 12] and d["item_ids"].tolist() == [101, 104, 100]
    assert d["tag_users"].tolist() == [1, 2] and d["tag_items"].tolist() == [1, 2]
    assert d["n_tag_ids_without_row"] == 1                                   # 77 has no user row


def test_join_matches_the_hand_cases():
    m, c = glo.join([10, 11, 12, 13], [14, 11], [3, 0])
    assert m.tolist() == [2, 1, -1, 3] and c == {"n_merged": 4, "n_updated": 1, "n_kept": 2, "n_pruned": 1}
    m, c = glo.join([10, 11, 12, 13], [11, 14], [], keep_not_updated=True)
    assert m.tolist() == [2, 0, 3, 4] and c == {"n_merged": 5, "n_updated": 1, "n_kept": 3, "n_pruned": 0}
    m, c = glo.join([], [5, 6], [])
    assert m.tolist() == [] and c == {"n_merged": 2, "n_updated": 0, "n_kept": 0, "n_pruned": 0}
    assert glo.join([1, 1], [2], []) is None and glo.join([1], [2, 2], []) is None
    assert isinstance(m, np.ndarray)
