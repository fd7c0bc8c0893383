"""tests/popular_oracle.py pinned on the CPU: the hand-worked case, the fp32 saturation of the count, the rescorer
arithmetic of MostPopularItemsIterator, and the new entry points' NULL-handle answers (no GPU needed)."""
import ctypes

import numpy as np

from myrrix_recommender_amd import _lib
from tests import popular_oracle as po
from tests.rescorer_oracle import AffineRescorer


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# five users over six items; user 3 is an itemTag, item 4 a userTag
SETS = {0: [0, 1, 2], 1: [1, 2], 2: [2, 5, 5], 3: [0, 1, 2, 3, 4, 5], 4: [1, 4]}


def test_hand_worked_five_users():
    # without user 3: item 0 -> {0}, 1 -> {0, 1, 4}, 2 -> {0, 1, 2}, 3 -> nobody, 4 -> {4}, 5 -> {2} (repeated: once)
    counts = po.counts_from_sets(SETS, 6, item_tag_users=[3])
    assert counts.tolist() == [1, 3, 3, 0, 1, 1]
    idx, val = po.most_popular(counts, 10, user_tag_items=[4])
    assert idx.tolist() == [1, 2, 0, 5]                       # 3, 3 (ascending index), then 1, 1; item 3 has no count, 4 is a tag
    assert val.tolist() == [3.0, 3.0, 1.0, 1.0]
    idx, val = po.most_popular(counts, 3, user_tag_items=[4])
    assert idx.tolist() == [1, 2, 0]                          # the cut falls inside the tie at 1.0: the lower index wins
    lit = po.most_popular_literal(SETS, 6, 10, item_tag_users=[3], user_tag_items=[4])
    assert np.array_equal(lit[0], [1, 2, 0, 5]) and np.array_equal(bits(lit[1]), bits([3, 3, 1, 1]))
    # with user 3 counted every item gains one, item 3 becomes a candidate
    assert po.counts_from_sets(SETS, 6).tolist() == [2, 4, 4, 1, 2, 2]


def test_csr_counts_equal_set_counts():
    ptr = np.array([0, 3, 5, 8, 14, 16])
    idx = np.array([0, 1, 2, 1, 2, 5, 2, 5, 0, 1, 2, 3, 4, 5, 4, 1])     # user 2 and user 4 unsorted, user 2 repeats 5
    assert po.counts_from_csr(ptr, idx, 6, [3]).tolist() == [1, 3, 3, 0, 1, 1]
    assert po.counts_from_csr(ptr, idx, 6).tolist() == [2, 4, 4, 1, 2, 2]
    assert po.counts_from_csr(ptr, idx, 5).tolist() == [2, 4, 4, 1, 2]   # item 5 owns no row


def test_the_count_saturates_at_two_to_the_24():
    v = np.float32(2 ** 24 - 2)
    seen = []
    for _ in range(4):                                        # FastByIDFloatMap.increment(id, 1.0f), four times
        v = np.float32(v + np.float32(1.0))
        seen.append(float(v))
    assert seen == [16777215.0, 16777216.0, 16777216.0, 16777216.0]
    assert po.float_count_literal(4, start=np.float32(2 ** 24 - 2)) == np.float32(16777216.0)
    assert po.float_count([2 ** 24 - 1, 2 ** 24, 2 ** 24 + 3, 2 ** 31]).tolist() == [16777215.0, 16777216.0, 16777216.0, 16777216.0]
    for c in (0, 1, 2, 255, 1000):
        assert bits(po.float_count_literal(c)) == bits(po.float_count(c))


def test_rescorer_cases():
    counts = np.array([5, 4, 3, 2, 1, 0, 7])
    # a filter set: 6 (the best) and 1 go
    idx, val = po.most_popular(counts, 10, rescorer=AffineRescorer(filtered=[6, 1]))
    assert idx.tolist() == [0, 2, 3, 4] and val.tolist() == [5.0, 3.0, 2.0, 1.0]
    # weights that reorder across counts; item 5 has no count: its offset cannot make it a candidate
    rs = AffineRescorer(scale=[1.0, 1.0, 3.0, 1.0, 10.0, 1.0, 0.5], offset=[0.0, 0.0, 0.0, 0.25, 0.0, 100.0, 0.0])
    idx, val = po.most_popular(counts, 10, rescorer=rs)
    assert idx.tolist() == [4, 2, 0, 1, 6, 3] and val.tolist() == [10.0, 9.0, 5.0, 4.0, 3.5, 2.25]
    # the arithmetic: fp64 product, fp64 sum, then the cast -- two roundings before it
    s, o = 1.0 + 2.0 ** -30, 1e-9
    want = np.float32(np.float64(np.float64(s) * np.float64(np.float32(7.0))) + np.float64(o))
    idx, val = po.most_popular(counts, 1, rescorer=AffineRescorer(scale=s, offset=o))
    assert idx.tolist() == [6] and bits(val)[0] == bits(want)
    # an offset whose float cast is infinite skips the item, never an error
    rs = AffineRescorer(offset=[1e39, 0.0, -1e39])
    idx, val = po.most_popular(counts, 10, rescorer=rs)
    assert idx.tolist() == [6, 1, 3, 4]
    for r in (AffineRescorer(filtered=[6, 1]), rs, AffineRescorer(scale=s, offset=o)):
        sets = {u: [i for i in range(7) if counts[i] > u] for u in range(7)}
        a = po.most_popular(po.counts_from_sets(sets, 7), 10, rescorer=r)
        b = po.most_popular_literal(sets, 7, 10, rescorer=r)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def test_null_handles_are_invalid_arguments():
    L = _lib.load()
    out = (ctypes.c_int64 * 4)()
    idx = (ctypes.c_int64 * 4)()
    sc = (ctypes.c_float * 4)()
    n = ctypes.c_int32(0)
    n64 = ctypes.c_int64(0)
    assert L.mals_set_tag_users(None, 0, None, _lib.MEM_HOST) == _lib.INVALID_ARG
    assert L.mals_get_tag_user_count(None, ctypes.byref(n64)) == _lib.INVALID_ARG
    assert L.mals_most_popular_items(None, None, 4, idx, sc, ctypes.byref(n)) == _lib.INVALID_ARG
    assert L.mals_most_popular_stats(None, out) == _lib.INVALID_ARG
    assert L.mals_group_set_tag_users(None, 0, None) == _lib.INVALID_ARG
    assert L.mals_group_most_popular_items(None, 4, idx, sc, ctypes.byref(n)) == _lib.INVALID_ARG
