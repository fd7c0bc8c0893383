"""The fixtures of tests/test_gpu_gramian_edges.py checked on the CPU: the integer data really are exact for every
arithmetic the Gramian kernels use (the precondition is asserted, not trusted, and a numpy restatement of one slab of
gramian_split_kernel reproduces the exact product bit for bit), and the edge-dominated data put the weight where they
say.  None of this runs a kernel: it proves that the GPU tests can only fail if a kernel drops, doubles or misplaces
something."""
import numpy as np
import pytest

from tests import gramian_cases as gc

_CACHE = {}


def integer_case(k):
    if k not in _CACHE:
        _CACHE.clear()            # one 136 MB matrix at a time
        _CACHE[k] = gc.integer_matrix(gc.N_ROWS, k, seed=k)
    return _CACHE[k]


@pytest.mark.parametrize("k", gc.ALL_K)
def test_integer_data_meet_the_exactness_precondition(k):
    M, loud = integer_case(k)
    assert M.shape == (gc.N_ROWS, k) and M.dtype == np.float32
    assert np.array_equal(M, np.rint(M))
    quiet = np.ones(len(M), dtype=bool)
    quiet[loud] = False
    assert np.abs(M[quiet]).max() <= 7 and np.abs(M[loud]).max() <= 7 * gc.LOUD
    assert np.array_equal(M[loud] / gc.LOUD, np.rint(M[loud] / gc.LOUD))
    assert M.any(axis=1).all(), "no row is all zero: a dropped row always changes the diagonal"
    assert gc.max_loud_per_window(loud) <= gc.LOUD_PER_WINDOW
    assert set(gc.LOUD_FIXED) <= set(loud.tolist())
    assert len(loud) > len(gc.LOUD_FIXED) + 50, "random loud rows as well"
    # every partial sum of a slab of up to 2048 rows is an integer below 2^24: windows at the slab starts of a range
    # that begins at row 0, and a bound that holds for every start
    assert gc.window_abs_max(M, 2048) < 2 ** 24
    assert gc.sliding_abs_bound(M, 2048) < 2 ** 24


def slabs_to_restate(n_rows, slab, rng):
    """(first row, rows) of the slabs worth restating: every slab with a boundary row, for row ranges that begin at
    row 0, 1 and 7; the ragged last slabs of a few range lengths; a few at random."""
    out = set()
    for r in gc.LOUD_FIXED:
        for begin in (0, 1, 7):
            if r >= begin:
                s0 = begin + (r - begin) // slab * slab
                out.add((s0, min(slab, n_rows - s0)))
    for d in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 513, 1536, 2047):
        tail = d % slab or slab
        out.add((gc.SPLIT_MIN_ROWS + d - tail, tail))
    for s in rng.integers(0, n_rows // slab, size=6):
        out.add((int(s) * slab, slab))
    return sorted(out)


@pytest.mark.parametrize("k", gc.ALL_K)
def test_slab_restatement_is_exact_on_the_integer_data(k):
    M, _ = integer_case(k)
    rng = np.random.default_rng(1000 + k)
    n = 0
    for slab in (512, 2048):
        for r0, rows in slabs_to_restate(len(M), slab, rng):
            blk = M[r0:r0 + rows]
            exact = gc.exact_gramian(blk)
            for step in (16, 32):
                part = gc.split_slab_restatement(blk, step)
                assert np.array_equal(part.astype(np.float64), exact), (k, slab, step, r0, rows)
                n += 1
    assert n >= 100


@pytest.mark.parametrize("s", [-49, -40, -20, 20, 40, 49])
def test_slab_restatement_is_scale_invariant(s):
    """M 2^s gives G 2^(2s) bit for bit: the pw / back bookkeeping and the rescale of the sums are exact up to the
    range the kernel's clamps and the float32 partials can represent (|s| <= 49 for these data)."""
    M, _ = integer_case(80)
    for r0, rows, step in ((0, 512, 16), (1536, 512, 32), (gc.SPLIT_MIN_ROWS, 17, 16), (0, 2048, 32)):
        blk = M[r0:r0 + rows]
        part = gc.split_slab_restatement(blk * np.float32(2.0 ** s), step)
        assert np.array_equal(part.astype(np.float64), gc.exact_gramian(blk) * 2.0 ** (2 * s)), (s, r0, rows, step)


def test_a_dropped_quiet_row_passes_the_norm_and_fails_equality():
    """Why the GPU tests compare element by element.  On the data of test_large_gramian_on_the_f16_pipe_matches_oracle
    (row norms over four decades, one row x 1000) losing any one of most rows moves the relative Frobenius norm of G by
    less than the 5e-7 that test allows (the change is r r^T, of norm |r|^2); on the integer data a lost row -- every
    one has a non-zero element -- changes the diagonal and fails the equality."""
    k, n = 30, 300_001
    rng = np.random.default_rng(k)
    M = rng.standard_normal((n, k)).astype(np.float32)
    M *= np.exp(rng.standard_normal(n) * 2.0).astype(np.float32)[:, None]
    M[12345] *= 1.0e3
    M[200_000:200_016] = 0.0
    r2 = (M.astype(np.float64) ** 2).sum(axis=1)
    unseen = r2 / np.linalg.norm(gc.exact_gramian(M)) < 5e-7
    assert unseen.mean() > 0.9 and unseen[-1], "the last row of the ragged slab is one of them"
    Mi, _ = integer_case(33)
    tail = Mi[gc.SPLIT_MIN_ROWS:gc.SPLIT_MIN_ROWS + 20]
    assert not np.array_equal(gc.exact_gramian(tail[:-1]), gc.exact_gramian(tail))
    assert not np.array_equal(gc.split_slab_restatement(tail[:-1], 32).astype(np.float64), gc.exact_gramian(tail))


def test_range_gramian_equals_the_direct_product():
    M, _ = integer_case(17)
    rg = gc.RangeGramian(M)
    for begin, rows in ((0, 1), (3, 5), (0, 4097), (3, 65537), (7, gc.SPLIT_MIN_ROWS + 33), (0, gc.N_ROWS)):
        assert np.array_equal(rg(begin, rows), gc.exact_gramian(M[begin:begin + rows])), (begin, rows)


@pytest.mark.parametrize("k", gc.EDGE_K)
def test_edge_sets_sit_where_they_say_and_dominate(k):
    n = gc.EDGE_N
    sets = gc.edge_sets(n, k)
    step = gc.step_rows(k)
    b, r = sets["last step of the ragged slab"]
    assert b + r == n and 1 <= r <= step and (b - gc.SPLIT_MIN_ROWS) % step == 0
    b, r = sets["first step of a slab"]
    assert b % 512 == 0 and r == step and b + r < gc.SPLIT_MIN_ROWS
    assert sets["last row of the matrix"] == (n - 1, 1)
    base = gc.edge_base(n, k, seed=k)
    total = float((base.astype(np.float64) ** 2).sum())
    for name, (b, r) in sets.items():
        own = float((base[b:b + r].astype(np.float64) ** 2).sum())
        share = own * gc.EDGE_SCALE ** 2 / (total + own * (gc.EDGE_SCALE ** 2 - 1))
        assert share > 0.75, (name, share)


def test_per_element_error_sees_one_element():
    Ge = np.diag([4.0, 9.0, 1.0])
    G = Ge.copy()
    G[0, 1] += 6.0e-6
    assert abs(gc.per_element_error(G, Ge) - 1.0e-6) < 1e-12
