"""The dual ("short row") path -- the forward rotation (rotate_rows_kernel<T,false,F64>, rotate_rows_split_kernel<T,false>),
als_dual_kernel<T,TN> and the un-rotation (rotate_rows_kernel<T,true,false>, rotate_rows_split_kernel<T,true>) of
csrc/dual_kernels.h -- row by row, on systems of exact small integers (tests/dual_cases.py; the CPU statements it rests on
are tests/test_dual_cases.py), through the C-ABI.

Every row's W and b are exact and cond(W) < 10, so all a correct path may lose is its own arithmetic: every ROW must land within
DUAL_BAR of the fp64 solution of the exact system -- 52.8 ulps of 2^-23 per element on the one-hot table (G diagonal, Q = I,
both rotations exact: als_dual_kernel alone, and zeros must be exact zeros), 62.4 ulps in the 2-norm on the two-hot table (a
full Q) -- sixteen times what the CPU emulation of the path loses on the same rows (E_emu 3.3 / 3.9 ulp, test_dual_cases.py),
never a figure from a GPU run.  A dropped or misplaced entry, weight, lane block, feature block or ridge count is off by
8 x DUAL_BAR and more on nearly every row it applies to.  The fp64 safety net is off (refine limit 0) and asserted to have
stayed off; rows_dual is asserted to count exactly the rows of 1 .. nmax entries.

  A  every length 0 .. nmax + 8 (above nmax: the direct kernels, judged too), three distinct rows of each, two orders (one
     under the non-default rotation settings), both tables, at every T = 2 .. 8 full and ragged and at the k % 8 == 0, k % 16 != 0 counts (the split rotation's ragged
     last chunk), under every pairing of rotation kernels the library has; the pairing that ran is read from the
     MALS_DEBUG_LISTS report.
  B  the wave loop: MALS_BLOCKS_PER_CU=1 shrinks the grid to 4 n_cu waves and every class list holds 14 n_cu + 5 distinct
     rows, so every wave runs the software-pipelined row loop of als_dual_kernel (cur / nxt / nx2, the next row's entries
     loaded during this row's arithmetic, xmax carried across rows) over a first, middle and last row, some waves one
     row more than others; the listed un-rotation's last tile ends ragged; once in three and more chunks (the
     un-rotation's operand scale slots alternate with the chunk).
  C  the check itself: rows uploaded without their last entry are refused.

Measured on the MI355X, worst row of all cases, next to E_emu (every case prints its own WORST line):
  one-hot  4.26 ulp (wave loop, k = 96 and 128, default rotation; part A: 3.35 at k = 120)    E_emu 3.3    bar 52.8
  two-hot  5.33 ulp (wave loop, k = 128, fp32 rotations; part A: 3.49 at k = 113 and 120)     E_emu 3.9    bar 62.4

Follow-up, not part of this module: the persistent row loop of the rows kernels (tests/test_gpu_rows_exact.py) is in the same
position -- every case there has fewer rows than the grid has waves, so each wave takes one row; a MALS_BLOCKS_PER_CU=1
case with thousands of distinct rows per list would close that as B does here."""
import functools
import re

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from tests import dual_cases as dc
from tests import rows_cases as rc
from tests.test_dual_cases import CAUGHT, DUAL_BAR, SHARE
from tests.test_gpu_dual import dual_max_len
from tests.test_gpu_rows_exact import environment

pytestmark = pytest.mark.gpu

# setting -> (environment, (forward, back) at k % 8 == 0, (forward, back) otherwise): prepare_dual_host (csrc/mals_api.hip)
ROTATION = {
    "default": ({"MALS_ROTATE_F64": None, "MALS_ROTATE_NO_SPLIT": None}, ("split", "split"), ("fp32", "fp32")),
    "no-split": ({"MALS_ROTATE_F64": None, "MALS_ROTATE_NO_SPLIT": "1"}, ("fp32", "fp32"), ("fp32", "fp32")),
    "f64": ({"MALS_ROTATE_F64": "1", "MALS_ROTATE_NO_SPLIT": None}, ("fp64", "split"), ("fp64", "fp32")),
    "f64-no-split": ({"MALS_ROTATE_F64": "1", "MALS_ROTATE_NO_SPLIT": "1"}, ("fp64", "fp32"), ("fp64", "fp32")),
}


def settings(k):
    """Without the split kernels (k % 8 != 0) NO_SPLIT changes nothing: each forward arithmetic once."""
    return list(ROTATION) if k % 8 == 0 else ["default", "f64"]


def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def table(k, kind):
    return dc.table(k, kind)


@functools.lru_cache(maxsize=4)
def rows_of(k, n_waves):
    """(ids, rows) of every_length(k) (n_waves = 0) or wave_loop(k, n_waves): the same rows on both tables."""
    ids = dc.wave_loop(k, n_waves) if n_waves else dc.every_length(k)
    return ids, [dc.row(n, r, dc.table_rows(k)) for n, r in ids]


@functools.lru_cache(maxsize=8)
def expectation(k, kind, n_waves):
    """(ids, rows, x* float64 [R, k], id -> index): computed once per (k, table), shared by the rotation settings and never
    changed."""
    ids, rows = rows_of(k, n_waves)
    xs = dc.expected(table(k, kind), rows)
    xs.setflags(write=False)
    return ids, rows, xs, {i: j for j, i in enumerate(ids)}


def solve(core, M, csr_arrays):
    n_rows = len(csr_arrays[0]) - 1
    core.set_refine_limit(0)
    core.set_factor_rows(pkg.SIDE_X, n_rows)
    core.set_factor_rows(pkg.SIDE_Y, M.shape[0])
    core.set_matrix(pkg.SIDE_X, *csr_arrays)
    core.set_factors(pkg.SIDE_Y, M)
    core.reset_stats()
    core.half_iteration(pkg.SIDE_X)
    return core.get_factors(pkg.SIDE_X), core.stats(), core.num_chunks(pkg.SIDE_X)


def row_errors(X, xs, kind):
    """(per-element figure that locates the worst feature, per-row error in ulps)."""
    if kind == dc.ONE_HOT:
        e = rc.element_ulps(X, xs)
        return e, e.max(axis=1)
    return np.abs(X.astype(np.float64) - xs), rc.row_ulps(X, xs)


def judge(X, ids, xs, kind, what):
    """Every row against its x*; returns the worst row's error in ulps."""
    assert np.all(np.isfinite(X)), what
    e, per_row = row_errors(X, xs, kind)
    i = int(per_row.argmax())
    f = int(e[i].argmax())
    report = "%s: worst row %d (%d entries, replica %d) at %.2f ulp (bar %.1f), worst feature %d: got %r, expected %r" % (
        what, i, ids[i][0], ids[i][1], per_row[i], DUAL_BAR[kind], f, float(X[i, f]), float(xs[i, f]))
    print(report)
    assert per_row[i] <= DUAL_BAR[kind], report
    assert np.all(X[np.array([n == 0 for n, _ in ids])] == 0.0), what
    return float(per_row[i])


def run(k, setting, kind, order, capfd, n_waves=0, env=None, upload=None, **core_kw):
    """One half-iteration over the rows `order` (ids) of table `kind` under a rotation setting.  Asserts what every case asserts
    but the bar; returns (X, x* in the order of the rows, number of chunks).  upload: what to upload of a row (cols, vals)."""
    M = table(k, kind)
    ids, rows, xs, index = expectation(k, kind, n_waves)
    at = [index[i] for i in order]
    uploaded = [rows[j] if upload is None else upload(rows[j]) for j in at]
    rot_env, even, ragged = ROTATION[setting]
    what = "k=%d %s table=%d" % (k, setting, kind)
    e = dict(rot_env, MALS_DEBUG_LISTS="1", MALS_REFINE_LIMIT=None, MALS_BLOCKS_PER_CU=None, MALS_OVERLAP=None)
    e.update(env or {})
    print(capfd.readouterr().out, end="")          # (keep what the earlier solves reported)
    with environment(e):
        with pkg.ALSCore(k, alpha=dc.ALPHA, lam=dc.LAMBDA, solve_mode=_lib.SOLVE_DUAL, **core_kw) as core:
            X, st, n_chunks = solve(core, M, dc.csr(uploaded))
    captured = capfd.readouterr()
    print(captured.out, end="")
    m = re.search(r"\[lists\] rotation forward (\w+), back (\w+)", captured.err)
    assert m and (m.group(1), m.group(2)) == (even if k % 8 == 0 else ragged), (what, captured.err)
    lengths = np.array([len(c) for c, _ in uploaded])
    n_dual = int(((lengths >= 1) & (lengths <= dual_max_len(k))).sum())
    assert st["rows_refined"] == 0 and st["rows_dual"] == n_dual > 0 and st["rows_solved"] == len(order), (what, st, n_dual)
    assert np.all(X[lengths == 0] == 0.0), what
    return X, xs[at], n_chunks


A_CASES = [(k, s) for k in dc.ALL_K for s in settings(k)]


@pytest.mark.parametrize("k,setting", A_CASES, ids=["k%d-%s" % c for c in A_CASES])
def test_every_length_class_and_rotation(k, setting, capfd):
    """A.  Every length, every class, every rotation.  Both row orders under the default setting, the first under the others:
    the module's running time is held under that of tests/test_gpu_rows_exact.py."""
    worst = {}
    for kind in dc.TABLES:
        for order_seed in (dc.ORDER_SEEDS if setting == "default" else dc.ORDER_SEEDS[:1]):
            order = dc.shuffled(dc.every_length(k), order_seed)
            X, xs, _ = run(k, setting, kind, order, capfd)
            w = judge(X, order, xs, kind, "k=%d %s table=%d order=%d" % (k, setting, kind, order_seed))
            worst[kind] = max(worst.get(kind, 0.0), w)
    print("WORST k=%d %s: one-hot %.2f ulp, two-hot %.2f ulp" % (k, setting, worst[dc.ONE_HOT], worst[dc.TWO_HOT]))


B_CASES = [(k, s) for k in dc.WAVE_LOOP_K for s in ("default", "no-split")]      # (k-major: the expectations are cached per k)


@pytest.mark.parametrize("k,setting", B_CASES, ids=["k%d-%s" % c for c in B_CASES])
def test_wave_loop(k, setting, capfd):
    """B.  A grid of n_cu workgroups, 14 n_cu + 5 distinct rows in every class: more than three rows per wave."""
    n_waves = 4 * n_cu()
    worst = {}
    for kind in dc.TABLES:
        ids = expectation(k, kind, n_waves)[0]
        counts = dc.class_counts(ids, k)
        assert len(counts) == dual_max_len(k) // 16 and all(c > 12 * n_cu() and c % n_waves != 0 for c in counts), counts
        assert sum(counts) % 64 != 0 and sum(counts) % 32 != 0 and len(set(ids)) == len(ids)
        order = dc.shuffled(ids, dc.ORDER_SEEDS[0])
        X, xs, _ = run(k, setting, kind, order, capfd, n_waves=n_waves, env={"MALS_BLOCKS_PER_CU": "1"})
        worst[kind] = judge(X, order, xs, kind, "wave loop k=%d %s table=%d, rows per class %s" % (k, setting, kind, counts))
    print("WORST wave loop k=%d %s: one-hot %.2f ulp, two-hot %.2f ulp" % (k, setting, worst[dc.ONE_HOT], worst[dc.TWO_HOT]))


def test_wave_loop_in_chunks(capfd):
    """B, once more in four chunks: the un-rotation takes its operand scale from the slot of its own chunk (chunk & 1), so
    the result need not be the unchunked one bit for bit -- the bar is the same."""
    k, setting = 64, "default"
    n_waves = 4 * n_cu()
    worst = {}
    for kind in dc.TABLES:
        ids = expectation(k, kind, n_waves)[0]
        order = dc.shuffled(ids, dc.ORDER_SEEDS[1])
        X, xs, n_chunks = run(k, setting, kind, order, capfd, n_waves=n_waves, env={"MALS_BLOCKS_PER_CU": "1"}, chunk_rows=len(ids) // 3)
        assert n_chunks >= 3, n_chunks
        worst[kind] = judge(X, order, xs, kind, "wave loop k=%d %s table=%d in %d chunks" % (k, setting, kind, n_chunks))
    print("WORST wave loop in chunks k=%d %s: one-hot %.2f ulp, two-hot %.2f ulp" % (k, setting, worst[dc.ONE_HOT], worst[dc.TWO_HOT]))


@pytest.mark.parametrize("k", [40, 64, 128])
def test_one_entry_less_on_the_device_is_seen(k, capfd):
    """C.  The check itself, end to end: the same rows uploaded WITHOUT their last entry, judged against the full rows' x* --
    what a kernel that drops a row's last entry would deliver.  The share of rows out by more than 8 x DUAL_BAR is that of
    the CPU statement (test_dual_cases.py), and judge() must refuse the result."""
    for kind in dc.TABLES:
        order = [i for i in dc.shuffled(dc.every_length(k), dc.ORDER_SEEDS[0]) if i[0] >= 1]
        X, xs, _ = run(k, "default", kind, order, capfd, upload=lambda row: (row[0][:-1], row[1][:-1]))
        _, per_row = row_errors(X, xs, kind)
        seen = int((per_row > CAUGHT[kind]).sum())
        print("k=%d table %d: %d of %d rows without their last entry past 8 x DUAL_BAR" % (k, kind, seen, len(order)))
        assert seen >= SHARE[kind] * len(order), (k, kind, seen, len(order))
        with pytest.raises(AssertionError):
            judge(X, order, xs, kind, "one entry dropped")
