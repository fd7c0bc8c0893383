"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the reference's mostSimilarItems with a Rescorer<LongPair> of the shape
the device runs (include/myrrix_als.h, mals_most_similar_items_rescored): a tests.rescorer_oracle.AffineRescorer read as a
pair rescorer.

  mostSimilarItems(long[], int, Rescorer<LongPair>)   online/src/net/myrrix/online/ServerRecommender.java:1180-1265
  MostSimilarItemIterator.next                        online/src/net/myrrix/online/MostSimilarItemIterator.java:73-120
      skip tag items (:77) and the query's own items (:81-85); per query item j, in order: isFiltered(pair) skips the
      candidate (:98); s_j = dot / (norm_c * norm_j), not finite skips it (:104); s_j = rescore(pair, s_j), not finite skips
      it (:109); total += s_j; result = (float)(total / length), not finite: checkState fails the call (:117)

For the pair (candidate c, query item q_j): isFiltered = c in F, with filter_query_items also q_j in F ("either end of the
pair", FilterHalfRescorerProvider.getMostSimilarItemsRescorer); rescore = fl(fl(scale_c * s) + offset_c), PER TERM.
`most_similar` is the vectorised restatement the GPU tests compare with; `most_similar_literal` transliterates next()
candidate by candidate and pins it (tests/test_similar_rescored_oracle.py)."""
import numpy as np

from oracle import topn_oracle as to
from tests import similarity_oracle as so


class BadSimilarityValue(Exception):
    """Preconditions.checkState(isFinite(result), "Bad similarity value") (MostSimilarItemIterator.java:117)"""


def most_similar_literal(Y, items, how_many, rescorer, filter_query_items=False, tags=()):
    """MostSimilarItemIterator.next, line by line, into TopN.selectTopN"""
    Y = np.asarray(Y, np.float32)
    items = [int(i) for i in np.atleast_1d(items)]
    tags = set(int(i) for i in tags)

    def dot(a, b):                                          # SimpleVectorMath.dot
        d = 0.0
        for u, v in zip(a, b):
            d += float(np.float32(u) * np.float32(v))
        return d

    def norm(a):                                            # SimpleVectorMath.norm
        with np.errstate(invalid="ignore"):
            return float(np.sqrt(np.float64(dot(a, a))))

    with np.errstate(over="ignore", invalid="ignore"):
        item_norms = [norm(Y[i]) for i in items]            # the constructor, :61-64
        out = []
        for cand in range(len(Y)):
            if cand in tags:                                # :77
                continue
            if cand in items:                               # :81-85
                continue
            cand_norm = norm(Y[cand])
            total = 0.0
            skipped = False
            for j, to_item in enumerate(items):
                if rescorer is not None:                    # :96-101
                    if rescorer.is_filtered(cand) or (filter_query_items and rescorer.is_filtered(to_item)):
                        skipped = True
                        break
                with np.errstate(divide="ignore"):
                    sim = float(np.float64(dot(Y[cand], Y[to_item])) / (np.float64(cand_norm) * np.float64(item_norms[j])))
                if not np.isfinite(sim):                    # :104
                    skipped = True
                    break
                if rescorer is not None:                    # :107-112
                    sim = rescorer.rescore(cand, sim)
                    if not np.isfinite(sim):
                        skipped = True
                        break
                total += sim
            if skipped:
                continue
            result = np.float32(np.float64(total) / len(items))   # :116
            if not np.isfinite(result):                     # :117
                raise BadSimilarityValue("Bad similarity value")
            out.append((cand, result))
    top = to.select_top_n(out, how_many)
    return np.array([i for i, _ in top], np.int64), np.array([v for _, v in top], np.float32)


def scores(Y, items, rescorer, filter_query_items=False, Ynorm=None):
    """(result float32 per candidate, ok per candidate) for one query: the per-term rule on every row at once"""
    Y = np.asarray(Y, np.float32)
    items = [int(i) for i in np.atleast_1d(items)]
    Ynorm = so.norms(Y) if Ynorm is None else Ynorm
    sc, of, filt = rescorer.arrays(len(Y))
    ok = ~filt
    if filter_query_items and any(rescorer.is_filtered(i) for i in items):
        ok = np.zeros(len(Y), bool)
    total = np.zeros(len(Y), np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for it in items:
            s = so.cosine64(Y, Y[it], norm_x=Ynorm[it], norm_y=Ynorm)
            ok = ok & np.isfinite(s)
            r = sc * s + of                               # numpy: one rounding per operation
            ok = ok & np.isfinite(r)
            total = total + r
        res = (total / float(len(items))).astype(np.float32)
    return res, ok


def most_similar(Y, items, how_many, rescorer, filter_query_items=False, tags=None, Ynorm=None):
    """(item indices, scores) best first, ties by ascending index; raises BadSimilarityValue like the reference."""
    items = [int(i) for i in np.atleast_1d(items)]
    res, ok = scores(Y, items, rescorer, filter_query_items, Ynorm)
    if tags is not None and len(tags):
        ok[np.asarray(tags, np.int64)] = False
    ok[np.asarray(items, np.int64)] = False
    if np.any(ok & ~np.isfinite(res)):
        raise BadSimilarityValue("Bad similarity value")
    idx = np.flatnonzero(ok)
    order = np.lexsort((idx, -res[idx].astype(np.float64)))[:how_many]
    return idx[order], res[idx][order]


def on_the_sum(Y, items, how_many, rescorer, tags=None):
    """the WRONG rule, for contrast: the rescore on the sum of the cosines before the division, as RecommendIterator does
    with its dots (what reusing topn_rs_score for similarity would compute)"""
    items = [int(i) for i in np.atleast_1d(items)]
    Y = np.asarray(Y, np.float32)
    Ynorm = so.norms(Y)
    sc, of, filt = rescorer.arrays(len(Y))
    total = np.zeros(len(Y), np.float64)
    ok = ~filt
    with np.errstate(over="ignore", invalid="ignore"):
        for it in items:
            s = so.cosine64(Y, Y[it], norm_x=Ynorm[it], norm_y=Ynorm)
            ok = ok & np.isfinite(s)
            total = total + s
        r = sc * total + of
        res = (r / float(len(items))).astype(np.float32)
    ok &= np.isfinite(r)
    if tags is not None and len(tags):
        ok[np.asarray(tags, np.int64)] = False
    ok[np.asarray(items, np.int64)] = False
    idx = np.flatnonzero(ok)
    order = np.lexsort((idx, -res[idx].astype(np.float64)))[:how_many]
    return idx[order], res[idx][order]
