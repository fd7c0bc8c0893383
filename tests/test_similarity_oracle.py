"""Pins tests/similarity_oracle.py (the restatement of mostSimilarItems, similarityToItem and recommendedBecause that the
device is compared against) with hand-worked cases."""
import numpy as np

from tests import similarity_oracle as so


def f32(*v):
    return np.array(v, np.float32)


def test_dot_and_norm_are_simple_vector_math():
    Y = np.array([[3, 4], [0, 0], [1, 1]], np.float32)
    assert so.norms(Y).tolist() == [5.0, 0.0, np.sqrt(2.0)]
    assert so.dots(Y, f32(2, -1)).tolist() == [2.0, 0.0, 1.0]
    # every product rounded to fp32 before the fp64 sum: 1.1f * 1.1f is not (double)1.1f * (double)1.1f
    x = f32(1.1)
    assert so.dots(x[None, :], x)[0] == float(np.float32(x[0]) * np.float32(x[0]))
    assert so.dots(x[None, :], x)[0] != float(x[0]) * float(x[0])


def test_division_order_is_the_references():
    # dot / (a * b), the product of the norms first (MostSimilarItemIterator.java:101-102); (dot / a) / b differs here
    a = f32(1 / 7, 3 / 7)
    b = f32(16 / 3, 19 / 3)
    d = so.dots(a[None, :], b)[0]
    na, nb = so.norms(a[None, :])[0], so.norms(b[None, :])[0]
    assert d / (na * nb) != (d / na) / nb
    s = so.cosine64(a[None, :], b)[0]
    assert s == d / (na * nb)
    Y = np.stack([a, b])
    assert so.similarity_to_item(Y, 1, [0])[0] == np.float32(d / (na * nb))


def test_nan_row_and_zero_query_skipped_in_most_similar_but_nan_in_similarity_to():
    Y = np.array([[1, 0], [np.nan, 1], [0, 0], [1, 1], [2, 1]], np.float32)
    idx, sc = so.most_similar(Y, [0], 10)
    assert idx.tolist() == [4, 3]                         # the NaN row 1 and the zero row 2 are skipped, 0 is the query
    assert sc.tolist() == [np.float32(2 / np.sqrt(5.0)), np.float32(1 / np.sqrt(2.0))]
    idx, sc = so.most_similar(Y, [2], 10)                 # a zero query: every similarity is NaN
    assert len(idx) == 0
    out = so.similarity_to_item(Y, 0, [1, 2, 3])
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == np.float32(1 / np.sqrt(2.0))
    assert np.isnan(so.similarity_to_item(Y, 2, [3])[0])


def test_duplicate_query_items_count_twice():
    Y = np.array([[1, 0], [0, 1], [1, 1], [3, 1]], np.float32)
    n = so.norms(Y)
    s_a = so.dots(Y, Y[0]) / (n * n[0])
    s_b = so.dots(Y, Y[1]) / (n * n[1])
    idx, sc = so.most_similar(Y, [0, 0, 1], 4)
    want = ((s_a + s_a + s_b) / 3.0).astype(np.float32)
    assert idx.tolist() == [3, 2]                         # 3: (2*0.949 + 0.316)/3 = 0.738 > 2: (2*0.707 + 0.707)/3
    assert sc.tolist() == [want[3], want[2]]
    _, sc_unique = so.most_similar(Y, [0, 1], 4)
    assert sc_unique.tolist() != sc.tolist()


def test_query_item_excluded_from_most_similar_but_not_from_because():
    Y = np.array([[1, 0], [2, 0], [1, 1], [0, 1]], np.float32)
    idx, sc = so.most_similar(Y, [1], 4)
    assert 1 not in idx.tolist()
    assert idx.tolist() == [0, 2, 3] and sc.tolist() == [1.0, np.float32(1 / np.sqrt(2.0)), 0.0]
    idx, sc = so.recommended_because(Y, [3, 1, 2], 1, 4)
    assert idx.tolist() == [1, 2, 3] and sc[0] == 1.0     # the item itself comes back, first


def test_ties_by_ascending_index_and_tags_struck():
    Y = np.array([[1, 0], [2, 0], [3, 0], [0.5, 0], [0, 1]], np.float32)   # scaled copies: exact ties at 1.0
    idx, sc = so.most_similar(Y, [0], 2)
    assert idx.tolist() == [1, 2] and sc.tolist() == [1.0, 1.0]
    idx, _ = so.most_similar(Y, [0], 3, tags=[2])
    assert idx.tolist() == [1, 3, 4]
    idx, _ = so.recommended_because(Y, [4, 3, 2, 1], 0, 3, tags=[1])
    assert idx.tolist() == [2, 3, 4]
