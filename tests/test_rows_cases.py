"""The CPU statements behind tests/test_gpu_rows_exact.py, from the reference rule alone (tests/rows_cases.py):

  * every row's W and b are exact in fp32, |W| < 2^22, cond_2(W) <= 4, and the operands z = sqrt(w) S y of the split-precision
    gather are exact in ONE f16 term at the scale S gather_scale_kernel chooses -- so a kernel that gathers and sums the
    right entries forms exactly this (W, b), whatever its arithmetic and summation order;
  * MODEL_ULPS: how far an fp32 LAPACK Cholesky with two fp32 substitutions lands from the fp64 solution on these systems,
    and BAR, the bar of the GPU test, derived from it (never from a GPU run);
  * sensitivity: each gather fault, applied to the EXPECTED side, moves at least one row of each table past 8 x BAR at every
    k -- the GPU test at BAR would see it."""
import functools

import numpy as np
import pytest

from tests import rows_cases as rc

# Worst figure of the fp32 model over every k of rc.ALL_K, both tables and every length of rc.boundary_lengths(), in units of
# 2^-23: 1.63 per row in the 2-norm (two-hot, k = 7), 1.77 per element (one-hot, k = 65); rounded up.
MODEL_ULPS = 1.8
# 16 = 4 x 2 x 2: the split rank-16 updates of cholesky_tiles run on 22-bit operands, four times the fp32 rounding by the
# kernel's own comment (csrc/als_kernels.h); the kernels use the hardware's 1-ulp rsq / rcp where LAPACK divides and takes
# square roots exactly (x 2); the sums run in another order (x 2).  28.8 ulps = 3.4e-6.
BAR = 16 * MODEL_ULPS
CAUGHT = 8 * BAR


@functools.lru_cache(maxsize=4)
def case(k, kind):
    M = rc.table(k, kind)
    rows = [rc.row_entries(n, M.shape[0]) for n in rc.boundary_lengths()]
    W, b, xs = rc.systems(M, rows)
    return M, rows, W, b, xs


def test_lengths_and_features_cover_what_they_claim():
    lengths = rc.boundary_lengths()
    assert len(lengths) == len(set(lengths.tolist())) == 137 + 45
    assert set(range(0, 137)) <= set(lengths.tolist()) and {4063, 4096, 4097, 4129} <= set(lengths.tolist())
    assert 75000 < lengths.sum() < 85000
    a, b = rc.shuffled_lengths(rc.ORDER_SEEDS[0]), rc.shuffled_lengths(rc.ORDER_SEEDS[1])
    assert sorted(a.tolist()) == sorted(b.tolist()) == sorted(lengths.tolist()) and not np.array_equal(a, b)
    T = [(k + 15) // 16 for k in rc.ALL_K]
    assert set(T) == set(range(1, 9))
    assert {(k + 15) // 16 for k in rc.ALL_K if k % 16 == 0} == set(range(1, 9))        # FULL, every T
    assert {(k + 15) // 16 for k in rc.ALL_K if k % 16 != 0} == set(range(1, 9))        # ragged, every T
    # rows of more than FINISH_GROUP slots at segment_nnz = 64 exist, on either side of the first group boundary
    assert len(rc.segment_cuts(2049, 64)) == rc.FINISH_GROUP + 1 and len(rc.segment_cuts(2048, 64)) == rc.FINISH_GROUP
    row_ptr, col, val = rc.csr(a, 6000)
    assert row_ptr[-1] == len(col) == len(val) == lengths.sum()
    for r in range(len(a)):
        c = col[row_ptr[r]:row_ptr[r + 1]]
        assert np.all(np.diff(c) > 0) and (len(c) == 0 or (c[0] >= 0 and c[-1] < 6000))
    assert set(np.unique(val).tolist()) == {-4.0, -1.0, 1.0, 4.0} and 0.07 < (val < 0).mean() < 0.13


@pytest.mark.parametrize("kind", rc.TABLES)
@pytest.mark.parametrize("k", rc.ALL_K)
def test_tables_are_what_the_kernels_must_see(k, kind):
    M = rc.table(k, kind)
    n, _ = rc.table_shape(k)
    assert M.shape == (n, k) and M.dtype == np.float32 and n >= rc.boundary_lengths().max()
    nz = M != 0
    hot = 2 if (kind == rc.TWO_HOT and k > 1) else 1
    assert np.all(nz.sum(axis=1) == hot)
    assert set(np.unique(np.abs(M[nz])).tolist()) == {1.0, 2.0}
    assert np.all(nz.sum(axis=0) > 0)                     # no dead feature: G is positive definite on its own
    if hot == 2:
        f, g = np.nonzero(nz)[1].reshape(n, 2).T
        assert np.any(f // 16 != g // 16) or k <= 16       # pairs straddle the 16-feature blocks
        assert np.all(np.abs(M[np.arange(n), f]) == np.abs(M[np.arange(n), g]))
        assert np.any(M[nz].reshape(n, 2).prod(axis=1) < 0) and np.any(M[nz].reshape(n, 2).prod(axis=1) > 0)


@pytest.mark.parametrize("kind", rc.TABLES)
@pytest.mark.parametrize("k", rc.ALL_K)
def test_systems_are_exact_and_well_conditioned(k, kind):
    M, rows, W, b, xs = case(k, kind)
    assert np.all(W == W.astype(np.float32)) and np.all(b == b.astype(np.float32))
    assert np.all(W * 8 == np.round(W * 8)) and np.all(b == np.round(b))
    assert np.abs(W).max() < 2 ** 22 and np.abs(b).max() < 2 ** 22
    ev = np.linalg.eigvalsh(W)
    assert ev.min() > 0 and (ev[:, -1] / ev[:, 0]).max() <= 4.0, (ev[:, -1] / ev[:, 0]).max()
    if kind == rc.ONE_HOT:
        assert all(np.count_nonzero(Wi - np.diag(np.diag(Wi))) == 0 for Wi in W)
    else:
        assert k == 1 or any(np.count_nonzero(Wi[:16, 16:]) for Wi in W) or k <= 16     # off-diagonal tiles carry data
    # the split-precision operands: one f16 term each, at the kernel's scale
    G = rc.exact_gramian(M)
    S = rc.gather_scale(G, 4.0)
    y = np.unique(np.abs(M))
    z = np.array([np.sqrt(w) * S * yy for w in (1.0, 4.0) for yy in y if yy != 0])
    assert np.all(z == z.astype(np.float16).astype(np.float64)) and np.all(z <= 2.0 ** 14) and np.all(z >= 2.0 ** -14)
    assert np.all(z == np.exp2(np.round(np.log2(z))))     # powers of two: the lower terms of the split are zero


def test_other_weights_stay_exact():
    """alpha = 4, lambda = 2^-5 (the further case of the GPU test): w in {4, 16}, the ridge again n_u / 8."""
    k = 64
    for kind in rc.TABLES:
        M = rc.table(k, kind)
        rows = [rc.row_entries(n, M.shape[0]) for n in rc.boundary_lengths()]
        W, b, xs = rc.systems(M, rows, alpha=4.0, lam=2.0 ** -5)
        assert np.all(W == W.astype(np.float32)) and np.all(b == b.astype(np.float32)) and np.abs(W).max() < 2 ** 22
        ev = np.linalg.eigvalsh(W)
        assert (ev[:, -1] / ev[:, 0]).max() <= 4.0
        S = rc.gather_scale(rc.exact_gramian(M), 4.0, alpha=4.0)
        z = np.array([np.sqrt(w) * S * yy for w in (4.0, 16.0) for yy in (1.0, 2.0)])
        assert np.all(z == z.astype(np.float16).astype(np.float64)) and np.all(z <= 2.0 ** 14)
        assert rc.row_ulps(rc.fp32_model(W, b), xs).max() <= MODEL_ULPS


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_mode_flags_keep_the_one_hot_systems_exact(flags):
    """reconstructR / lossIgnoresUnspecified on the one-hot table: still exact and diagonal; without the Gramian under it a
    short row's W is badly conditioned (ridge n_u / 8 against the hit features), which a diagonal system's element error
    does not feel.  An empty row has W = 0 under lossIgnoresUnspecified -- singular for the reference as well -- and is
    left out of those cases."""
    for k in (30, 64, 100, 128):
        M = rc.table(k, rc.ONE_HOT)
        lengths = rc.boundary_lengths()
        if flags & 2:
            lengths = lengths[lengths > 0]
        rows = [rc.row_entries(n, M.shape[0]) for n in lengths]
        W, b, xs = rc.systems(M, rows, flags=flags)
        assert np.all(W == W.astype(np.float32)) and np.all(b == b.astype(np.float32)) and np.abs(W).max() < 2 ** 22
        assert all(np.count_nonzero(Wi - np.diag(np.diag(Wi))) == 0 for Wi in W) and np.all(np.diagonal(W, axis1=1, axis2=2) > 0)
        assert rc.element_ulps(rc.fp32_model(W, b), xs).max() <= MODEL_ULPS


@pytest.mark.parametrize("k", rc.ALL_K)
def test_model_figure_and_bar(k):
    worst = 0.0
    for kind in rc.TABLES:
        M, rows, W, b, xs = case(k, kind)
        xm = rc.fp32_model(W, b)
        per_row = rc.row_ulps(xm, xs).max()
        per_el = rc.element_ulps(xm, xs).max() if kind == rc.ONE_HOT else 0.0
        print("k=%d table %d: fp32 model %.2f ulp per row, %.2f per element" % (k, kind, per_row, per_el))
        worst = max(worst, per_row, per_el)
    assert worst <= MODEL_ULPS
    assert BAR == 16 * MODEL_ULPS and 2.0 ** -20 < BAR * rc.ULP < 2.0 ** -18


@pytest.mark.parametrize("k", rc.ALL_K)
def test_every_fault_moves_a_row_past_eight_bars(k):
    for kind in rc.TABLES:
        M, rows, W, b, xs = case(k, kind)
        M64, G = M.astype(np.float64), rc.exact_gramian(M)
        for name in rc.MUTATIONS:
            if name == "one entry's feature moved by 16" and k <= 16:
                continue                                   # one feature block: nowhere to move to
            moved = applicable = 0
            for (cols, vals), x in zip(rows, xs):
                m = rc.mutate(name, M64, G, cols, vals, k)
                if m is None:
                    continue
                applicable += 1
                xm = rc.solve64(*m)[None]
                err = rc.element_ulps(xm, x[None]).max() if kind == rc.ONE_HOT else rc.row_ulps(xm, x[None]).max()
                moved += bool(err > CAUGHT)
            print("k=%d table %d, %s: %d of %d rows past 8 x BAR" % (k, kind, name, moved, applicable))
            assert applicable > 0 and moved > 0, (k, kind, name, moved, applicable)
