"""The rescored restatement (tests/rescorer_oracle.py) against a literal transliteration of RecommendIterator.next with an
IDRescorer: filtered items, rescores that are NaN / +-inf (skipped), a finite rescore whose cast overflows (the call
fails), offsets that reorder the catalogue, the mean over several vectors."""
import numpy as np
import pytest

from tests import rescorer_oracle as ro


def data(n=120, k=6, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, k)).astype(np.float32), rng.standard_normal((3, k)).astype(np.float32)


def same(a, b):
    assert np.array_equal(a[0], b[0]), (a[0], b[0])
    assert np.array_equal(np.asarray(a[1], np.float32).view(np.uint32), np.asarray(b[1], np.float32).view(np.uint32))


@pytest.mark.parametrize("nv", [1, 3])
def test_filter_and_weights_match_the_literal_iterator(nv):
    Y, V = data(seed=nv)
    rng = np.random.default_rng(5)
    r = ro.AffineRescorer(filtered=range(1, 120, 2), scale=10.0)     # FilterHalfRescorerProvider: odd ids out, x 10
    same(ro.recommend(Y, V[:nv], 15, r), ro.recommend_literal(Y, V[:nv], 15, r))
    r = ro.AffineRescorer(filtered=[3, 7, 50], scale=rng.uniform(0.1, 8.0, 100), offset=rng.standard_normal(90) * 3)
    got = ro.recommend(Y, V[:nv], 20, r, known=[0, 1, 2], tags=[9])
    same(got, ro.recommend_literal(Y, V[:nv], 20, r, known=[0, 1, 2], tags=[9]))
    assert not set(got[0].tolist()) & {3, 7, 50, 0, 1, 2, 9}


def test_offsets_reorder_the_catalogue():
    Y, V = data(seed=2)
    plain = ro.recommend(Y, V[0], 5, ro.AffineRescorer())
    low = int(np.argmin(Y @ V[0]))
    off = np.zeros(len(Y))
    off[low] = 1e3
    got = ro.recommend(Y, V[0], 5, ro.AffineRescorer(offset=off))
    assert got[0][0] == low and plain[0][0] != low
    same(got, ro.recommend_literal(Y, V[0], 5, ro.AffineRescorer(offset=off)))


def test_non_finite_rescores_are_skipped():
    Y, V = data(seed=3)
    Y[4] = np.inf                                                   # sum +-inf / NaN -> rescore not finite
    Y[5, 0] = np.nan
    sc = np.ones(len(Y))
    sc[6] = 1e308                                                   # scale * sum overflows to +-inf in fp64
    r = ro.AffineRescorer(scale=sc)
    with np.errstate(invalid="ignore", over="ignore"):
        got = ro.recommend(Y, V[:2], 30, r)
        lit = ro.recommend_literal(Y, V[:2], 30, r)
    same(got, lit)
    assert not {4, 5} & set(got[0].tolist())


def test_a_finite_rescore_whose_cast_overflows_fails_the_call():
    Y, V = data(seed=4)
    sc = np.ones(len(Y))
    sc[10] = 1e300                                                  # finite in fp64, not in fp32
    r = ro.AffineRescorer(scale=sc)
    for fn in (ro.recommend, ro.recommend_literal):
        with pytest.raises(ro.BadRecommendationValue):
            fn(Y, V[:1], 5, r)
    # ... unless the item is filtered, known or a tag (skipped before it is scored)
    r2 = ro.AffineRescorer(filtered=[10], scale=sc)
    same(ro.recommend(Y, V[:1], 5, r2), ro.recommend_literal(Y, V[:1], 5, r2))
    same(ro.recommend(Y, V[:1], 5, r, known=[10]), ro.recommend_literal(Y, V[:1], 5, r, known=[10]))


def test_every_item_filtered_is_an_empty_answer():
    Y, V = data(n=40, seed=6)
    r = ro.AffineRescorer(filtered=range(40))
    got = ro.recommend(Y, V[0], 5, r)
    assert len(got[0]) == 0
    same(got, ro.recommend_literal(Y, V[0], 5, r))


def test_the_rescore_applies_to_the_sum_before_the_division():
    Y = np.array([[1.0], [0.0]], np.float32)
    V = np.array([[1.0], [1.0], [1.0], [1.0]], np.float32)           # sum 4 for item 0
    r = ro.AffineRescorer(offset=np.array([0.0, 6.0]))               # item 1: (0 + 6) / 4 = 1.5 > 4 / 4 = 1
    idx, sc = ro.recommend(Y, V, 2, r)
    assert idx.tolist() == [1, 0] and sc.tolist() == [1.5, 1.0]
    same((idx, sc), ro.recommend_literal(Y, V, 2, r))
