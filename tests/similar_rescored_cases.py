"""TEST INFRASTRUCTURE ONLY -- the catalogues, rescorers and calls of the filter-path test of rescored mostSimilarItems
(tests/test_gpu_similar_rescored.py), shared with tests/test_similar_rescored_margin.py, which emulates exactly these calls
on the CPU to show that the filter can answer them without falling back to the dense path."""
import numpy as np

from tests import rescorer_oracle as ro

FILTER_ITEMS = 150_000          # the smallest size class the filter path takes needs n_items >= 131072
FILTER_KS = (10, 31, 64, 100)   # one per load mode of the streaming kernel (clamped four-float, one per feature, whole rows, ...)
KINDS = ("filter", "weights", "uniform", "combined", "filter_half")


def filter_catalogue(k):
    """benign random rows plus scaled copies of one row (exact cosine ties) and a near-copy (a near-tie)"""
    rng = np.random.default_rng(500 + k)
    Y = rng.standard_normal((FILTER_ITEMS, k)).astype(np.float32)
    base = Y[11].copy()
    for j, s in enumerate((2.0, 0.5, 4.0, 8.0)):
        Y[100 + 37 * j] = base * np.float32(s)
    Y[300] = base
    Y[300, 0] = np.nextafter(base[0], np.float32(np.inf))
    return Y


def rescorer_specs(n_items, seed):
    """{kind: (filtered or None, scale, offset)}: scale / offset arrays, scalars (uniform) or None; all of them weights the
    filter runs for (scale in [2^-20, 2^20], |offset| <= 2^6 scale)"""
    rng = np.random.default_rng(seed)
    filt = np.sort(rng.choice(n_items, n_items // 10, replace=False))
    scale = rng.uniform(0.25, 4.0, n_items)
    offset = rng.standard_normal(n_items) * 0.5
    return {
        "filter": (filt, None, None),
        "weights": (None, scale[: n_items - 100], offset[: n_items - 100]),     # the last rows uncovered
        "uniform": (None, 3.0, -0.75),
        "combined": (filt, scale, offset),
        "filter_half": (np.arange(1, n_items, 2), 10.0, 0.0),                     # FilterHalfRescorerProvider: odd filtered, x 10
    }


def oracle_rescorer(spec):
    filt, scale, offset = spec
    return ro.AffineRescorer(filtered=() if filt is None else filt, scale=scale, offset=offset)


def device_rescorer(core, spec):
    filt, scale, offset = spec
    r = core.rescorer()
    if filt is not None:
        r.set_filter(filt)
    if scale is not None and np.isscalar(scale):
        r.set_uniform(float(scale), float(offset))
    elif scale is not None or offset is not None:
        r.set_weights(scale, offset)
    return r


def filter_calls(k):
    """[(kind, how_many, filter_query_items, queries)] of the filter-path test at k features.  Query items are even (never
    filtered by filter_half) except where a filtered query item is the point."""
    rng = np.random.default_rng(900 + k)
    n = FILTER_ITEMS
    specs = rescorer_specs(n, 700 + k)
    free = np.setdiff1d(np.arange(0, n, 2), specs["filter"][0])          # items no rescorer filters
    calls = []
    for j, kind in enumerate(KINDS):
        singles = [int(i) for i in rng.choice(free, 7, replace=False)] + [11]
        multi = [[11, 11, int(free[500])], [int(free[1000]), int(free[2000])], [int(free[5]), 100, int(free[77])]]
        hms = (10, 64) if k == 64 else ((10,) if (j + k) % 2 else (64,))
        for hm in hms:
            calls.append((kind, hm, False, [[i] for i in singles] + multi))
    # either end of the pair: one query item in F -- that query comes back empty, the others are answered
    f_item = int(specs["filter"][0][3])
    calls.append(("combined", 10, True, [[int(free[9])], [f_item], [int(free[10]), f_item], [int(free[12]), int(free[13])]]))
    if k == 64:   # more than one pass of queries (240 fit one)
        calls.append(("combined", 64, False, [[int(i)] for i in rng.choice(free, 250, replace=False)]))
    return specs, calls
