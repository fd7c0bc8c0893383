"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the reference's item-to-item similarity (mals_most_similar_items,
mals_similarity_to_item, mals_recommended_because).  Not product code: only tests/ and tools/bench_topn.py may import it.

  SimpleVectorMath.dot     common/src/net/myrrix/common/math/SimpleVectorMath.java:34-41 (fp32 products, fp64 sum from +0.0)
  SimpleVectorMath.norm    common/src/net/myrrix/common/math/SimpleVectorMath.java:46-52 (sqrt of the fp64 sum of fp32 squares)
  mostSimilarItems         online/src/net/myrrix/online/ServerRecommender.java:1171-1266, scored by
                           online/src/net/myrrix/online/MostSimilarItemIterator.java:73-120:
                             skip tag items (:77) and the query's own items (:81-85); s_j = dot / (norm_i * norm_j) -- the
                             product of the norms first (:101-102); skip the item if any s_j is not finite (:104);
                             score = (float) (total / length), total summed in query order, length counting duplicates (:116)
  similarityToItem         online/src/net/myrrix/online/ServerRecommender.java:1268-1304: (float) (dot / (norm_i * norm_to)),
                           NaN returned as NaN
  recommendedBecause       online/src/net/myrrix/online/ServerRecommender.java:1324-1376, scored by
                           online/src/net/myrrix/online/RecommendedBecauseIterator.java:61-75: over the user's known items,
                           tag items and non-finite scores skipped, the item itself NOT excluded
  TopN                     oracle.topn_oracle.select_top_n (TopN.java:49-128)
Among equal scores the reference's order is the hash order of its maps; this restatement, like the device, orders ties by
ascending item index.
"""
import numpy as np

from oracle.topn_oracle import _seq_sum, select_top_n


def dots(Y, x):
    """dot(Y_i, x) for every row, fp64: every product rounded to fp32, summed in fp64 in feature order (SVM:34-41)."""
    p = (np.asarray(Y, np.float32) * np.asarray(x, np.float32)[None, :]).astype(np.float32)
    return _seq_sum(p)


def norms(Y):
    """norm(Y_i) for every row, fp64: sqrt of the fp64 sum of fp32 squares (SVM:46-52; sqrt correctly rounded)."""
    Y = np.asarray(Y, np.float32)
    return np.sqrt(_seq_sum((Y * Y).astype(np.float32)))


def cosine64(Y, x, norm_x=None, norm_y=None):
    """s = dot(Y_i, x) / (norm(Y_i) * norm(x)) in fp64 for every row of Y -- the product first, then the division."""
    x = np.asarray(x, np.float32)
    ny = norms(Y) if norm_y is None else norm_y
    nx = norms(x[None, :])[0] if norm_x is None else norm_x
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return dots(Y, x) / (ny * nx)


def _top(idx, score, how_many):
    """The how_many best (score desc, index asc) of the given items: select_top_n over those that can make it."""
    idx = np.asarray(idx, np.int64)
    score = np.asarray(score, np.float32)
    if len(idx) > how_many:   # only items at or above the how_many-th largest score can be in the result
        kth = np.partition(score, len(score) - how_many)[len(score) - how_many]
        keep = score >= kth
        idx, score = idx[keep], score[keep]
    top = select_top_n(zip(idx.tolist(), score.tolist()), how_many)
    return (np.array([t[0] for t in top], np.int64), np.array([t[1] for t in top], np.float32))


def most_similar_scores(Y, items, Ynorm=None):
    """(score float32 per item, ok per item) for one query of the given items (MostSimilarItemIterator.java:88-116)."""
    Ynorm = norms(Y) if Ynorm is None else Ynorm
    total = np.zeros(len(Y), np.float64)
    ok = np.ones(len(Y), bool)
    for it in items:
        s = cosine64(Y, Y[it], norm_x=Ynorm[it], norm_y=Ynorm)
        ok &= np.isfinite(s)
        with np.errstate(invalid="ignore", over="ignore"):
            total = total + s
    with np.errstate(invalid="ignore", over="ignore"):
        return (total / float(len(items))).astype(np.float32), ok


def most_similar(Y, items, how_many, tags=None, Ynorm=None):
    """mostSimilarItems for one query: items = its item indices (duplicates count).  Returns (indices, scores)."""
    items = [int(i) for i in np.atleast_1d(items)]
    score, ok = most_similar_scores(Y, items, Ynorm)
    if tags is not None and len(tags):
        ok[np.asarray(tags, np.int64)] = False            # MostSimilarItemIterator.java:77
    ok[np.asarray(items, np.int64)] = False               # :81-85
    idx = np.flatnonzero(ok)
    return _top(idx, score[idx], how_many)


def similarity_to_item(Y, to_item, items):
    """similarityToItem: (float)(dot / (norm_i * norm_to)) per item, NaN as NaN."""
    Y = np.asarray(Y, np.float32)
    items = np.asarray(items, np.int64)
    return cosine64(Y[items], Y[to_item]).astype(np.float32)


def recommended_because(Y, known, item, how_many, tags=None):
    """recommendedBecause for one (user, item): known = the user's known item indices."""
    Y = np.asarray(Y, np.float32)
    known = np.asarray(known, np.int64)
    s = cosine64(Y[known], Y[item])
    ok = np.isfinite(s)                                    # RecommendedBecauseIterator.java:72
    if tags is not None and len(tags):
        ok &= ~np.isin(known, np.asarray(tags, np.int64))  # :66
    return _top(known[ok], s[ok].astype(np.float32), how_many)
