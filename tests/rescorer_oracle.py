"""TEST INFRASTRUCTURE ONLY -- CPU restatement of RecommendIterator.next with an IDRescorer of the shape the device runs
(include/myrrix_als.h, "rescorers"): isFiltered(i) = i in a filter set, rescore(i, sum) = fl(fl(scale_i * sum) + offset_i)
in fp64.

  RecommendIterator.next   online/src/net/myrrix/online/RecommendIterator.java:62-109
      skip tags, known items, filtered items; sum = fp64 sum of the dots; sum = rescore(sum), not finite: skip;
      result = (float)(sum / count), not finite: checkState fails the call

`recommend` is the vectorised restatement the GPU tests compare with; `recommend_literal` transliterates next() item by
item and pins it (tests/test_rescorer_oracle.py)."""
import numpy as np

from oracle import topn_oracle as to


class BadRecommendationValue(Exception):
    """Preconditions.checkState(isFinite(result), "Bad recommendation value") (RecommendIterator.java:105)"""


class AffineRescorer:
    """filter: item indices; scale / offset: per-item fp64 arrays (rows past them: 1 / 0) or scalars (uniform)."""

    def __init__(self, filtered=(), scale=None, offset=None):
        self.filtered = set(int(i) for i in filtered)
        self.scale = scale
        self.offset = offset

    def _w(self, a, i, default):
        if a is None:
            return default
        if np.isscalar(a):
            return float(a)
        return float(a[i]) if i < len(a) else default

    def is_filtered(self, i):
        return int(i) in self.filtered

    def rescore(self, i, s):
        p = np.float64(self._w(self.scale, i, 1.0)) * np.float64(s)     # two roundings: Java never contracts a * s + b
        return float(p + np.float64(self._w(self.offset, i, 0.0)))

    def arrays(self, n_items):
        sc = np.ones(n_items, np.float64)
        of = np.zeros(n_items, np.float64)
        for a, out, d in ((self.scale, sc, 1.0), (self.offset, of, 0.0)):
            if a is None:
                continue
            if np.isscalar(a):
                out[:] = float(a)
            else:
                m = min(len(a), n_items)
                out[:m] = np.asarray(a, np.float64)[:m]
        filt = np.zeros(n_items, bool)
        idx = [i for i in self.filtered if i < n_items]
        filt[idx] = True
        return sc, of, filt


def sums(Y, vectors):
    """the fp64 sum over the query's vectors of SimpleVectorMath.dot (fp32 products, fp64 sum in feature order)"""
    vectors = np.atleast_2d(np.asarray(vectors, np.float32))
    total = np.zeros(len(Y), np.float64)
    for x in vectors:
        total = total + to._seq_sum((np.asarray(Y, np.float32) * x[None, :]).astype(np.float32))
    return total, len(vectors)


def recommend(Y, vectors, how_many, rescorer, known=None, tags=None):
    """(item indices, scores) best first, ties by ascending index; raises BadRecommendationValue like the reference."""
    s, n = sums(Y, vectors)
    sc, of, filt = rescorer.arrays(len(Y))
    with np.errstate(over="ignore", invalid="ignore"):
        r = sc * s + of                                   # numpy: one rounding per operation
        res = (r / float(n)).astype(np.float32)
    ok = ~filt & np.isfinite(r)
    for lst in (tags, known):
        if lst is not None and len(lst):
            ok[np.asarray(lst, np.int64)] = False
    if np.any(ok & ~np.isfinite(res)):
        raise BadRecommendationValue("Bad recommendation value")
    idx = np.flatnonzero(ok)
    order = np.lexsort((idx, -res[idx].astype(np.float64)))[:how_many]
    return idx[order], res[idx][order]


def recommend_literal(Y, vectors, how_many, rescorer, known=(), tags=()):
    """RecommendIterator.next, line by line, into TopN.selectTopN"""
    vectors = [np.asarray(v, np.float32) for v in np.atleast_2d(np.asarray(vectors, np.float32))]
    known, tags = set(int(i) for i in known), set(int(i) for i in tags)
    out = []
    for item in range(len(Y)):
        if item in tags:                                   # :72
            continue
        if item in known:                                  # :75-82
            continue
        if rescorer is not None and rescorer.is_filtered(item):   # :84-87
            continue
        total = 0.0
        count = 0
        for f in vectors:                                  # :90-95
            d = 0.0
            for a, b in zip(Y[item], f):
                d += float(np.float32(a) * np.float32(b))
            total += d
            count += 1
        if rescorer is not None:                           # :97-101
            total = rescorer.rescore(item, total)
            if not np.isfinite(total):
                continue
        with np.errstate(over="ignore"):
            result = np.float32(total / count)             # :103
        if not np.isfinite(result):                        # :104
            raise BadRecommendationValue("Bad recommendation value")
        out.append((item, result))
    top = to.select_top_n(out, how_many)
    return np.array([i for i, _ in top], np.int64), np.array([v for _, v in top], np.float32)
