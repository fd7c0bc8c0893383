"""The per-row solve kernels -- als_persistent_kernel, als_persistent_kernel_h, als_lds_kernel_h, als_prereduce_kernel and
als_finish_kernel (csrc/als_kernels.h, csrc/lds_kernels.h) -- entry by entry, on systems of exact small integers
(tests/rows_cases.py; the CPU statements it rests on are tests/test_rows_cases.py), through the C-ABI.

Every row's W and b are exact in fp32 and in the f16 splits and cond(W) < 4, so all a correct kernel may lose is the k x k
factorisation and the two substitutions: every ROW must land within BAR (28.8 ulps of 2^-23, sixteen times what an fp32
LAPACK Cholesky loses on the same systems) of the fp64 solution -- per element on the one-hot table, where zeros must also be
exact zeros, in the 2-norm on the two-hot one.  A dropped, doubled or misplaced entry, weight, lane, feature block or ridge
count is off by 8 x BAR and more (test_rows_cases.py).  The fp64 safety net is off (refine limit 0) and asserted to have
stayed off, the dual path likewise: the bare fp32 kernels are what is measured.

One case per (k, arithmetic, list kind); both tables and both row orders run inside it.  A failure names k, arithmetic, list
kind, table, row length and the worst feature."""
import contextlib
import functools
import os
import re

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from tests import rows_cases as rc
from tests.test_rows_cases import BAR

pytestmark = pytest.mark.gpu

BAND_ROWS, BAND_MIN_ENTRIES = 750, 16      # eight bands of the 6000-row table; a sorted row is banded from 128 entries on


def stride(k):
    return k if k % 16 == 0 else 16 * ((k + 15) // 16)


@contextlib.contextmanager
def environment(new):
    old = {name: os.environ.get(name) for name in new}
    for name, v in new.items():
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = v
    try:
        yield
    finally:
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v


# arithmetic -> (gramian_mode, environment, the split-precision kernels must have run)
ARITHMETIC = {
    "fp32": (_lib.GRAMIAN_FP32, {}, False),                                   # als_persistent_kernel
    "split": (_lib.GRAMIAN_SPLIT_F16, {"MALS_LDS_GATHER": None}, True),       # als_persistent_kernel_h; k = 128: als_lds_kernel_h
    "split-registers": (_lib.GRAMIAN_SPLIT_F16, {"MALS_LDS_GATHER": "0"}, True),   # k = 128 through als_persistent_kernel_h
    "split3": (_lib.GRAMIAN_SPLIT3_F16, {}, True),                            # als_persistent_kernel_h<4, ., ., 3>
}
# list kind -> (ALSCore arguments, banded)
LIST_KINDS = {
    "fused": (dict(), False),                       # everything in the rows kernel up to 4096 entries, 4097 .. 4129 cut
    "seg64": (dict(segment_nnz=64), False),         # from 2049 entries on more than 32 slots: als_prereduce_kernel
    "seg192": (dict(segment_nnz=192), False),
    "banded": (dict(segment_nnz=64), True),         # the long ascending rows cut at the table's bands
    "seg64-chunked": (dict(segment_nnz=64, chunk_rows=7), False),
}


def arithmetics(k):
    a = ["fp32", "split"]
    if k == 128:
        a.append("split-registers")
    if k in (50, 64):
        a.append("split3")
    return a


@functools.lru_cache(maxsize=None)
def table(k, kind):
    return rc.table(k, kind)


@functools.lru_cache(maxsize=None)
def expected_rows(k, kind, flags, alpha, lam):
    """length -> x* (float64 [k]); computed once per table and weight rule, shared by every case and never changed."""
    M = table(k, kind)
    lengths = rc.boundary_lengths()
    rows = [rc.row_entries(n, M.shape[0]) for n in lengths]
    _, _, xs = rc.systems(M, rows, flags=flags, alpha=alpha, lam=lam)
    xs.setflags(write=False)
    return {int(n): x for n, x in zip(lengths, xs)}


@functools.lru_cache(maxsize=None)
def problem(n_table, order_seed, min_len):
    lengths = rc.shuffled_lengths(order_seed, min_len)
    return lengths, rc.csr(lengths, n_table)


def solve(core, M, csr_arrays):
    n_rows = len(csr_arrays[0]) - 1
    core.set_factor_rows(pkg.SIDE_X, n_rows)
    core.set_factor_rows(pkg.SIDE_Y, M.shape[0])
    core.set_matrix(pkg.SIDE_X, *csr_arrays)
    core.set_factors(pkg.SIDE_Y, M)
    core.reset_stats()
    core.half_iteration(pkg.SIDE_X)
    return core.get_factors(pkg.SIDE_X), core.stats(), core.gather_scale()


def row_errors(X, xs, kind):
    """(per-element figure that locates the worst feature, per-row error in ulps): per element on the one-hot table, in the
    2-norm on the two-hot one."""
    if kind == rc.ONE_HOT:
        e = rc.element_ulps(X, xs)
        return e, e.max(axis=1)
    return np.abs(X.astype(np.float64) - xs), rc.row_ulps(X, xs)


def judge(X, lengths, xs_by_len, kind, what):
    """Every row against its x*; returns the worst row's error in ulps."""
    xs = np.stack([xs_by_len[int(n)] for n in lengths])
    assert np.all(np.isfinite(X)), what
    e, per_row = row_errors(X, xs, kind)
    r = int(per_row.argmax())
    f = int(e[r].argmax())
    report = "%s: worst row %d of %d entries at %.2f ulp (bar %.1f), worst feature %d: got %r, expected %r" % (
        what, r, int(lengths[r]), per_row[r], BAR, f, float(X[r, f]), float(xs[r, f]))
    print(report)
    assert per_row[r] <= BAR, report
    assert np.all(X[lengths == 0] == 0.0), what
    return float(per_row[r])


def run_case(k, arithmetic, list_kind, capfd, flags=0, alpha=rc.ALPHA, lam=rc.LAMBDA, tables=rc.TABLES):
    mode, env, split = ARITHMETIC[arithmetic]
    kw, banded = LIST_KINDS[list_kind]
    env = dict(env)
    env["MALS_BAND_BYTES"] = str(4 * stride(k) * BAND_ROWS) if banded else None
    env["MALS_BAND_MIN_ENTRIES"] = str(BAND_MIN_ENTRIES) if banded else None
    env["MALS_DEBUG_LISTS"] = "1" if banded else None
    env["MALS_REFINE_LIMIT"] = None
    env["MALS_FORCE_RANGE_FLAG"] = None
    min_len = 1 if flags & rc.FLAG_LOSS_IGNORES_UNSPECIFIED else 0    # W = 0: singular for the reference as well
    common = dict(alpha=alpha, lam=lam, flags=flags, gramian_mode=mode, solve_mode=_lib.SOLVE_DIRECT)
    worst = 0.0
    with environment(env):
        for kind in tables:
            M = table(k, kind)
            xs_by_len = expected_rows(k, kind, flags, alpha, lam)
            S = rc.gather_scale(rc.exact_gramian(M), 4.0, flags, alpha)
            for order_seed in rc.ORDER_SEEDS:
                lengths, csr_arrays = problem(M.shape[0], order_seed, min_len)
                what = "k=%d %s %s flags=%d table=%d order=%d" % (k, arithmetic, list_kind, flags, kind, order_seed)
                if banded:
                    print(capfd.readouterr().out, end="")     # (keep what the earlier solves reported)
                with pkg.ALSCore(k, **common, **kw) as core:
                    core.set_refine_limit(0)
                    X, st, gs = solve(core, M, csr_arrays)
                if banded:
                    captured = capfd.readouterr()
                    print(captured.out, end="")
                    m = re.search(r"\[lists\] bands (\d+) of (\d+) table rows .*: (\d+) banded rows", captured.err)
                    n_bands = int(csr_arrays[1].max()) // BAND_ROWS + 1
                    assert m and int(m.group(1)) == n_bands >= 6 and int(m.group(2)) == BAND_ROWS, what
                    # band_row_eligible (csrc/band_plan.h); every row's columns ascend
                    n_banded = int(((lengths > kw["segment_nnz"]) & (lengths // n_bands >= BAND_MIN_ENTRIES)).sum())
                    assert int(m.group(3)) == n_banded >= 45, (what, m.group(0))
                assert st["rows_refined"] == 0 and st["rows_dual"] == 0 and st["rows_solved"] == len(lengths), (what, st)
                if split:    # the range flag: the split-precision kernels did the work, at the scale the CPU statements assume
                    assert gs[2] == 1.0 and gs[0] == S, (what, gs, S)
                else:        # no split-precision gather was ever prepared on this handle
                    assert gs[0] == 0.0 and gs[2] == 0.0, (what, gs)
                worst = max(worst, judge(X, lengths, xs_by_len, kind, what))
                if kw.get("chunk_rows"):
                    whole = dict(kw)
                    del whole["chunk_rows"]
                    with pkg.ALSCore(k, **common, **whole) as core:
                        core.set_refine_limit(0)
                        Xw, stw, _ = solve(core, M, csr_arrays)
                    assert stw["rows_refined"] == 0 and stw["rows_solved"] == len(lengths), (what, stw)
                    assert np.array_equal(X, Xw), what
    print("WORST k=%d %s %s flags=%d alpha=%g: %.2f ulp" % (k, arithmetic, list_kind, flags, alpha, worst))


MATRIX = [(k, a, kind) for k in rc.ALL_K for a in arithmetics(k) for kind in LIST_KINDS]


@pytest.mark.parametrize("k,arithmetic,list_kind", MATRIX, ids=["k%d-%s-%s" % c for c in MATRIX])
def test_every_row_on_exact_systems(k, arithmetic, list_kind, capfd):
    run_case(k, arithmetic, list_kind, capfd)


@pytest.mark.parametrize("k,arithmetic", [(30, "split"), (64, "fp32"), (128, "split")])
def test_one_entry_less_on_the_device_is_seen(k, arithmetic):
    """The check itself, end to end: the same rows uploaded WITHOUT their last entry, judged against the full rows' x* -- what a
    kernel that drops a row's last entry would deliver.  Nearly every row must be out by more than 8 x BAR, the longest
    (4129 entries, one entry in 4129) included, and judge() must refuse the result."""
    mode, env, _ = ARITHMETIC[arithmetic]
    for kind in rc.TABLES:
        M = table(k, kind)
        xs_by_len = expected_rows(k, kind, 0, rc.ALPHA, rc.LAMBDA)
        lengths = rc.shuffled_lengths(rc.ORDER_SEEDS[0], 1)
        rows = [rc.row_entries(n, M.shape[0]) for n in lengths]
        row_ptr = np.concatenate([[0], np.cumsum(lengths - 1)]).astype(np.int64)
        col = np.concatenate([c[:-1] for c, _ in rows]).astype(np.int32)
        val = np.concatenate([v[:-1] for _, v in rows]).astype(np.float32)
        with environment(dict(env, MALS_BAND_BYTES=None, MALS_REFINE_LIMIT=None)):
            with pkg.ALSCore(k, alpha=rc.ALPHA, lam=rc.LAMBDA, gramian_mode=mode, solve_mode=_lib.SOLVE_DIRECT) as core:
                core.set_refine_limit(0)
                X, st, _ = solve(core, M, (row_ptr, col, val))
        assert st["rows_refined"] == 0 and st["rows_solved"] == len(lengths)
        xs = np.stack([xs_by_len[int(n)] for n in lengths])
        _, per_row = row_errors(X, xs, kind)
        assert (per_row > 8 * BAR).sum() >= 0.9 * len(lengths), (k, kind, int((per_row > 8 * BAR).sum()))
        assert per_row[int(lengths.argmax())] > 8 * BAR and lengths.max() == 4129
        with pytest.raises(AssertionError):
            judge(X, lengths, xs_by_len, kind, "one entry dropped")


@pytest.mark.parametrize("list_kind", ["fused", "seg64"])
@pytest.mark.parametrize("arithmetic", ["fp32", "split"])
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("k", [30, 64, 100, 128])
def test_mode_flags_on_the_one_hot_table(k, flags, arithmetic, list_kind, capfd):
    """reconstructR and lossIgnoresUnspecified: another weight rule, an image of zeros under W.  One-hot only: a diagonal
    system's element error does not depend on the conditioning, which is poor for short rows without the Gramian.  Rows
    with no entry are left out under lossIgnoresUnspecified (W = 0: singular for the reference as well).

    One combination is not an exact system: flags = 2 in split precision has w = 1 + |r| in {2, 5}, whose square roots are
    not f16 numbers, so W_ff is an fp32 sum of up to n_u / k rounded terms (each within 6 ulp: a 1-ulp square root, a 22-bit
    operand, squared) and carries that sum's rounding, which grows with the number of 32-entry super-steps one accumulator
    takes: measured 14.5 ulp on the 4064-entry row at k = 30 in the fused kernel (7.5 at k = 64, 3.5 at k = 100, 2.9 at
    k = 128), 1.8 .. 2.9 ulp once the row is cut at 64 entries.  It stays under BAR and is deterministic (fixed summation
    order), but there the bar rests on that measurement's margin, not on exactness; flags 1 and 3 (w in {0, 1}) and the fp32
    kernels are exact under every flag."""
    run_case(k, arithmetic, list_kind, capfd, flags=flags, tables=(rc.ONE_HOT,))


@pytest.mark.parametrize("list_kind", ["fused", "seg64"])
@pytest.mark.parametrize("arithmetic", ["fp32", "split", "split3"])
def test_other_alpha_and_lambda(arithmetic, list_kind, capfd):
    """alpha = 4, lambda = 2^-5: w in {4, 16}, the ridge n_u / 8 as before -- the weights stay exact."""
    run_case(64, arithmetic, list_kind, capfd, alpha=4.0, lam=2.0 ** -5)
