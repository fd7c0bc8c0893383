"""Long dense rows cut at the bands of the gather table (csrc/band_plan.h, plan_work_lists in csrc/work_plan.h, launch_lists
in csrc/mals_api.hip): the banded lists must compute what the lists cut by count compute.

The table has 2048 rows and a band is 256 of them (MALS_BAND_BYTES, read at every list build), segment_nnz = 64 and a row
is banded from 16 entries per band on (MALS_BAND_MIN_ENTRIES), i.e. from 128 entries.  k = 30 gathers from the padded
table (stride 32), k = 64 runs the register kernels, k = 128 the LDS-staged ones.  The solved rows:

  0  every column: 256 entries per band, cut again by count inside each band
  1  1500 random columns
  2  200 columns, all in band 3
  3  ten columns on each side of every band boundary (... 255 | 256 ..., 511 | 512, ...)
  4  1000 random columns in shuffled order: long enough, not sorted -- keeps the cuts by count
  5  65 columns: longer than segment_nnz, too short for eight bands
  6  empty
  7  600 columns with a single one in band 2 (a piece too small for a slot of its own rides with the next band's)
  8, 9  300 and 700 random columns
  10 .. 23  short rows, the dual path's lengths among them

Tolerances: 1e-4 relative Frobenius against the oracle (tests/test_gpu_parity.py), 1e-5 against the same problem without
banding (the re-segmentation test there: the same fp32 sums in another order); everything else is bitwise."""
import contextlib
import os
import re

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from oracle import oracle

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4
N_TABLE, BAND_ROWS, SEG = 2048, 256, 64
BANDED = [0, 1, 2, 3, 7, 8, 9]
SHORT_LENS = [1, 2, 3, 15, 16, 17, 31, 33, 40, 48, 49, 63, 64, 5]


def rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / max(np.linalg.norm(b.astype(np.float64)), 1e-30))


def stride(k):
    return k if k % 16 == 0 else 16 * ((k + 15) // 16)


@contextlib.contextmanager
def band_env(k, band_rows, min_entries=16, debug=False):
    new = {"MALS_BAND_BYTES": str(4 * stride(k) * band_rows), "MALS_BAND_MIN_ENTRIES": str(min_entries)}
    if debug:
        new["MALS_DEBUG_LISTS"] = "1"
    old = {name: os.environ.get(name) for name in list(new) + ["MALS_DEBUG_LISTS"]}
    os.environ.update(new)
    try:
        yield
    finally:
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v


def problem(k):
    rng = np.random.default_rng(700 + k)
    pick = lambda n, lo=0, hi=N_TABLE: np.sort(rng.choice(np.arange(lo, hi), size=n, replace=False))
    edges = np.concatenate([np.arange(b * BAND_ROWS - 10, b * BAND_ROWS + 10) for b in range(1, N_TABLE // BAND_ROWS)])
    thin = np.concatenate([pick(300, 0, 2 * BAND_ROWS), [2 * BAND_ROWS + 100], pick(299, 3 * BAND_ROWS, N_TABLE)])
    rows = [np.arange(N_TABLE), pick(1500), pick(200, 3 * BAND_ROWS, 4 * BAND_ROWS), edges, rng.permutation(pick(1000)), pick(65),
            np.zeros(0, dtype=np.int64), thin, pick(300), pick(700)]
    rows += [pick(n) for n in SHORT_LENS]
    assert len(rows) == 24 and 255 in edges and 256 in edges and 1791 in edges and 1792 in edges
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    val = rng.integers(1, 6, size=len(col)).astype(np.float32)
    Y0 = (rng.standard_normal((N_TABLE, k)) / np.sqrt(k)).astype(np.float32)
    return row_ptr, col, val, Y0


def solve(k, prob, chunk_rows=0):
    row_ptr, col, val, Y0 = prob
    with pkg.ALSCore(k, segment_nnz=SEG, chunk_rows=chunk_rows) as core:
        core.set_factor_rows(pkg.SIDE_X, len(row_ptr) - 1)
        core.set_factor_rows(pkg.SIDE_Y, N_TABLE)
        core.set_matrix(pkg.SIDE_X, row_ptr, col, val)
        core.set_factors(pkg.SIDE_Y, Y0)
        core.half_iteration(pkg.SIDE_X)
        core.check()
        return core.get_factors(pkg.SIDE_X)


@pytest.fixture(scope="module", params=[30, 64, 128])
def case(request):
    k = request.param
    prob = problem(k)
    return k, prob, oracle.half_iteration(*prob)


def test_banded_lists_match_oracle_and_cuts_by_count(case, capfd):
    k, prob, Xo = case
    with band_env(k, 0):
        plain = solve(k, prob)
    capfd.readouterr()
    with band_env(k, BAND_ROWS, debug=True):
        banded = solve(k, prob)
    lists = capfd.readouterr().err
    with band_env(k, BAND_ROWS):
        again = solve(k, prob)
        chunked = solve(k, prob, chunk_rows=7)
    m = re.search(r"\[lists\] bands (\d+) of (\d+) table rows \(at least (\d+) entries per band\): (\d+) banded rows \((\d+) entries\) in (\d+) segments, "
                  r"(\d+) long enough but unsorted", lists)
    assert m, lists
    n_bands, band_rows, min_avg, n_rows, n_entries, n_segs, n_unsorted = map(int, m.groups())
    lens = np.diff(prob[0])
    assert (n_bands, band_rows, min_avg, n_rows, n_unsorted) == (N_TABLE // BAND_ROWS, BAND_ROWS, 16, len(BANDED), 1), lists
    assert n_entries == int(lens[BANDED].sum())
    by_count = int(sum(-(-int(lens[r]) // SEG) for r in BANDED))
    assert by_count <= n_segs <= by_count + n_bands * len(BANDED)
    e_oracle, e_plain = rel(banded, Xo), rel(banded, plain)
    print("k=%d: banded vs oracle %.3e, vs cuts by count %.3e, plain vs oracle %.3e" % (k, e_oracle, e_plain, rel(plain, Xo)))
    assert e_oracle < REL_TOL
    assert e_plain < 1e-5
    others = [r for r in range(len(lens)) if r not in BANDED]
    assert np.array_equal(banded[others], plain[others])      # nothing changes for a row that is not banded
    assert not np.array_equal(banded[BANDED], plain[BANDED])  # ... and the banded ones did take other cuts
    assert np.array_equal(again, banded)
    assert np.array_equal(chunked, banded)


def test_table_inside_one_band_changes_nothing(case):
    k, prob, _ = case
    with band_env(k, 0):
        plain = solve(k, prob)
    with band_env(k, N_TABLE):
        one_band = solve(k, prob)
    assert np.array_equal(one_band, plain)
