"""tests/ingest_live_oracle.py (the CPU restatement of ServerRecommender.ingest that the GPU tests of mals_ingest_apply
compare against) pinned by cases computed by hand.  No solver is set, so a set changes no factor (updateFeatures needs one)
and only the structure moves: rows, directories, known items, zeroed rows, counters."""
import numpy as np
import pytest

from oracle import ingest_text_oracle as ito
from tests import ingest_live_oracle as lo


def small_model():
    X = np.arange(1, 7, dtype=np.float32).reshape(3, 2)        # users 100, 200, 300 -> rows 0, 1, 2
    Y = -np.arange(1, 5, dtype=np.float32).reshape(2, 2)       # items 7, 9 -> rows 0, 1
    known = {0: {0, 1}, 1: {1}}                                # user 300 (row 2) knows nothing
    return lo.LiveModel(X, Y, known, [100, 200, 300], [7, 9])


def test_new_rows_are_numbered_in_order_of_first_appearance_among_the_sets():
    m = small_model()
    text = b"user,item,value\n500,9\n400,11,2\n500,12\n# comment\n\n400,11\r\n100,12,\n600,13,\n"
    st, removed, statuses = m.apply_text(text)
    # line 1 is the header; sets: (500,9) (400,11) (500,12) (400,11); removes: (100,12) -- item 12 has a row by then, user 100
    # does not know it: passed on, ignored -- and (600,13): neither id ever has a row: dropped
    assert st == dict(records=6, sets=4, removes=1, removes_dropped=1, sets_failed=0, new_users=2, new_items=2, write_calls=2)
    assert m.user_ids == [100, 200, 300, 500, 400] and m.item_ids == [7, 9, 11, 12]
    assert removed == [] and statuses == [0, 0, 0, 0]
    assert m.known == {0: {0, 1}, 1: {1}, 3: {1, 3}, 4: {2}}
    X, Y = m.arrays()
    assert X.shape == (5, 2) and Y.shape == (4, 2) and not X[3:].any() and not Y[2:].any()
    assert np.array_equal(X[:3], np.arange(1, 7, dtype=np.float32).reshape(3, 2))


def test_a_remove_before_the_set_that_creates_its_user():
    m = small_model()
    users = np.array([900, 900, 901], np.int64)
    items = np.array([7, 7, 7], np.int64)
    values = np.array([np.nan, 1.0, np.nan], np.float32)
    st, removed, _ = m.apply_records(users, items, values)
    # the first remove: user 900 gets its row from the LATER set of the same call, so the library passes it on (a grown user
    # without known items: ignored).  The last: user 901 never has a row: dropped.  Runs: remove, set.
    assert st == dict(records=3, sets=1, removes=1, removes_dropped=1, sets_failed=0, new_users=1, new_items=0, write_calls=2)
    assert removed == [] and m.user_ids[-1] == 900 and m.known[3] == {0}
    # in a call of its own the same remove is dropped: no set of that call creates the user
    m = small_model()
    st, _, _ = m.apply_records(users[:1], items[:1], values[:1])
    assert st["removes"] == 0 and st["removes_dropped"] == 1 and st["write_calls"] == 0 and m.user_ids == [100, 200, 300]


def test_a_user_that_is_removed_and_returns_keeps_its_row():
    m = small_model()
    st, removed, _ = m.apply_text(b"200,9,\n200,9,\n100,7,\n200,7,3.5\n100,9,\n")
    # 200 loses its only item: emptied, row 1 zeroed, reported by id; the second remove finds a user without known items;
    # 100 loses item 7, keeps 9; 200 returns: same row, zeros, knows item 7; 100 loses 9: emptied
    assert removed == [200, 100]
    assert st == dict(records=5, sets=1, removes=4, removes_dropped=0, sets_failed=0, new_users=0, new_items=0, write_calls=3)
    assert m.user_ids == [100, 200, 300] and m.known == {1: {0}}
    X, _ = m.arrays()
    assert not X[0].any() and not X[1].any() and np.array_equal(X[2], np.array([5, 6], np.float32))


def test_a_dropped_remove_cuts_no_run_and_what_is_not_served_raises():
    m = small_model()
    st, _, _ = m.apply_text(b"100,7\n999,7,\n200,7\n")
    assert st["write_calls"] == 1 and st["removes_dropped"] == 1 and st["sets"] == 2
    with pytest.raises(lo.NotServed):
        small_model().apply_text(b'100,7\n"tag",7,1\n')
    with pytest.raises(ito.TooManyBadLines):
        small_model().apply_text(b"100,7\n" + b"x\n" * 101 + b"100,9\n")
    with pytest.raises(ito.UncaughtStringIndexOutOfBounds):
        small_model().apply_text(b'100,7\n",7\n')
    u, i, v, lines, bad, header = lo.parse_text(b"a,b\n1,2\nx\n\n3,4,\n")
    assert (u.tolist(), i.tolist(), lines, bad, header) == ([1, 3], [2, 4], 5, 1, 1) and v[0] == 1.0 and np.isnan(v[1])


def test_tabs_are_delimiters_only_for_the_ingest_splitter():
    text = b"100\t7\t2\n200,9\t\n300\t 9 ,1\n"
    u, i, v, lines, bad, _ = lo.parse_text(text, tabs=True)
    assert (u.tolist(), i.tolist(), lines, bad) == ([100, 200, 300], [7, 9, 9], 3, 0) and v[0] == 2.0 and np.isnan(v[1]) and v[2] == 1.0
    # the input-file reader's comma split: line 1 is one token (unparseable on line 1: a header); line 2 has two tokens, the
    # second with a trailing tab that is trimmed as white space -- a set of 1.0, not a remove; line 3's first token holds a tab
    u, i, v, lines, bad, header = lo.parse_text(text)
    assert (u.tolist(), i.tolist(), lines, bad, header) == ([200], [9], 3, 1, 1) and v[0] == 1.0
