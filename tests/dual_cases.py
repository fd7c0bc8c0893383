"""Inputs for the row-by-row tests of the dual ("short row") path (tests/test_gpu_dual_exact.py: the forward rotation,
als_dual_kernel<T,TN>, the un-rotation; csrc/dual_kernels.h) and the CPU statements that make them trustworthy
(tests/test_dual_cases.py).  No GPU, no torch.

The tables, values, alpha = 1 and lambda = 1/8 are those of tests/rows_cases.py, so every row's k x k system W x = b is made
of exact small integers (eighths for the ridge) and the expectation is an fp64 solve of it.  What differs:

  * the table has 8 k rows, not 6000: G's diagonal is then ~20 (one-hot) or ~40 (two-hot) instead of ~234, one entry of a
    short row moves x visibly and cond(W) stays under 8 -- every mutation below shows (test_dual_cases.py);
  * row (length n, replica r) is row_entries(n, n_table, seed=r): DISTINCT rows of one length, thousands per class in the
    wave-loop case, so that a wave computing on the prefetched entries of the wrong row is seen.

  one-hot  G is diagonal: mals::symmetric_eigen (csrc/host_eigen.h) skips every Householder step and deflates at once, Q = I and
           L = diag(G) exactly.  Both rotations are then exact in all three arithmetics (the split one as well: 8192 x 1 and the
           table's 1 and 2 are f16 numbers), x' has exact zeros off the row's hot features -- this isolates als_dual_kernel, a
           row is judged per element and zeros must be exact zeros.
  two-hot  Q is a full orthogonal matrix: the rotation kernels, their tile tails and the listed un-rotation carry data; a
           row is judged in the 2-norm."""
import contextlib

import numpy as np

from tests import rows_cases as rc

# every T = ceil(k / 16) = 2 .. 8, each full and ragged, and the k % 8 == 0, k % 16 != 0 family (the split rotation's ragged
# last 32-feature chunk: 24, 40, 56, 72, 88, 104, 120)
ALL_K = [17, 24, 32, 40, 48, 50, 56, 64, 65, 72, 80, 88, 96, 100, 104, 112, 113, 120, 128]
WAVE_LOOP_K = [32, 64, 96, 128]      # T = 2 (reduce_groups store), 4 (halving, P = 4), 6 (P = 8), 8 (TN = 4 stores the other way)
REPLICAS = 3
ORDER_SEEDS = rc.ORDER_SEEDS
ONE_HOT, TWO_HOT, TABLES = rc.ONE_HOT, rc.TWO_HOT, rc.TABLES
ALPHA, LAMBDA = rc.ALPHA, rc.LAMBDA
COND_BOUND = 10.0     # cond_2(W) of every row stays below (worst: 8.9, the two-hot table at k = 128; under 7.3 elsewhere)
BOUNDARY_LENGTHS = (16, 17, 32, 33, 48, 49, 64)     # the lane <-> entry blocks of als_dual_kernel


def dual_max_blocks(T):
    """csrc/dual_kernels.h"""
    return 4 if T >= 6 else (3 if T >= 4 else T // 2)


def dual_max_len(k):
    """Largest row the dual path takes at k features."""
    return 16 * dual_max_blocks((k + 15) // 16)


def table_rows(k):
    return 8 * k


def table(k, kind):
    return rc.table(k, kind, shape=(table_rows(k), 0.5))


def row(n, r, n_table):
    return rc.row_entries(n, n_table, seed=r)


def every_length(k, replicas=REPLICAS):
    """[(length, replica)]: every length 0 .. nmax + 8 (above nmax: the direct kernel), `replicas` distinct rows of each."""
    return [(n, r) for n in range(0, dual_max_len(k) + 9) for r in range(replicas)]


def shuffled(ids, order_seed):
    ids = list(ids)
    return [ids[i] for i in np.random.default_rng(order_seed).permutation(len(ids))]


def wave_loop(k, n_waves):
    """[(length, replica)] with 3.5 n_waves + 5 rows in every class of the dual path (each wave of a grid of n_waves waves
    then walks a first, at least one middle and a last row, and some waves one row more than others), all distinct,
    plus a few empty rows and rows for the direct kernel.  Should the dual rows come to a multiple of 64 the first class
    gets one more: the listed un-rotation's last tile must end ragged."""
    per_class = (7 * n_waves) // 2 + 5
    ids = []
    for cls in range(dual_max_blocks((k + 15) // 16)):
        count = per_class + (1 if cls == 0 and (per_class * dual_max_blocks((k + 15) // 16)) % 64 == 0 else 0)
        ids += [(16 * cls + 1 + i % 16, i // 16) for i in range(count)]
    nmax = dual_max_len(k)
    return ids + [(0, r) for r in range(5)] + [(nmax + 1 + r, r) for r in range(5)]


def class_counts(ids, k):
    """Rows per dual class (1-16, 17-32, ...) among these rows."""
    n = np.array([n for n, _ in ids])
    return [int(((n > 16 * c) & (n <= 16 * c + 16)).sum()) for c in range(dual_max_blocks((k + 15) // 16))]


def csr(rows):
    """(row_ptr int64, col int32, val float32) of rows = [(cols, vals)]."""
    row_ptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    col = np.concatenate([c for c, _ in rows] or [np.zeros(0, np.int32)]).astype(np.int32)
    val = np.concatenate([v for _, v in rows] or [np.zeros(0, np.float32)]).astype(np.float32)
    return row_ptr, col, val


def expected(M, rows, batch=256, threads=8):
    """x* (float64 [R, k]) of rows = [(cols, vals)]: the fp64 solution of every row's exact (W, b) (rc.row_system, default
    mode), `batch` rows at a time (14 000 systems of 128 x 128 doubles at once are 1.8 GB), the batches on a few threads
    (LAPACK solves one small system after the other on one core)."""
    from concurrent.futures import ThreadPoolExecutor
    M64, G = M.astype(np.float64), rc.exact_gramian(M)
    k = M.shape[1]
    out = np.zeros((len(rows), k))

    def solve_batch(lo):
        part = rows[lo:lo + batch]
        nmax = max(1, max(len(c) for c, _ in part))
        cols = np.zeros((len(part), nmax), dtype=np.int64)
        w, cb = np.zeros((len(part), nmax)), np.zeros((len(part), nmax))
        for i, (c, v) in enumerate(part):
            cols[i, :len(c)] = c
            w[i, :len(c)], cb[i, :len(c)] = rc.weights(v, 0, ALPHA)
        Y = M64[cols]                                                        # [R, nmax, k]; padding: weight 0
        n_u = np.array([len(c) for c, _ in part], dtype=np.float64)
        W = np.matmul((Y * w[:, :, None]).transpose(0, 2, 1), Y)
        W += G[None]
        d = np.einsum("rii->ri", W)                          # (a view of the diagonals)
        d += (LAMBDA * ALPHA * n_u)[:, None]
        b = np.einsum("rn,rnk->rk", cb, Y)
        if np.count_nonzero(W) == np.count_nonzero(d):       # every W diagonal (the one-hot table): nothing to eliminate
            out[lo:lo + len(part)] = b / d
        else:
            out[lo:lo + len(part)] = np.linalg.solve(W, b[:, :, None])[:, :, 0]

    try:        # one BLAS thread per batch thread, where that can be said: the small products gain nothing from more
        from threadpoolctl import threadpool_limits
        blas = threadpool_limits(limits=1)
    except ImportError:
        blas = contextlib.nullcontext()
    with blas, ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(solve_batch, range(0, len(rows), batch)))
    return out


# ---- mutations of the expected side: what a dual kernel with the named fault would compute ---------------------------------
def _duplicate_column(e):
    return "entry %d's column for entry %d" % (e - 1, e)


MUTATIONS = ["drop the last entry", "ridge count n + 1", _duplicate_column(16), _duplicate_column(32), _duplicate_column(48),
             "weights swapped across entries 15/16", "one entry's feature moved by 16"]
# and one of the arithmetic, applied in tests/dual_emulation.py (drop_low_half): the f16 low half left out of Z
SINGLE_F16 = "single-f16 operand"


def mutate(name, M64, G, cols, vals, k):
    """The (W, b) a kernel with the named fault would form for the row, or None where the fault cannot show on this row."""
    n = len(cols)
    c, v = cols.copy(), vals.copy()
    if name == "drop the last entry":            # the ridge count kept
        return rc.row_system(M64, G, c[:-1], v[:-1], ridge_count=n) if n >= 1 else None
    if name == "ridge count n + 1":              # sD[(n-1)*KP] read one row off
        return rc.row_system(M64, G, c, v, ridge_count=n + 1) if n >= 1 else None
    for e in (16, 32, 48):                       # the lane <-> entry blocks
        if name == _duplicate_column(e):
            if n <= e:
                return None
            c[e] = c[e - 1]
            return rc.row_system(M64, G, c, v)
    if name == "weights swapped across entries 15/16":
        if n <= 16 or vals[15] == vals[16]:
            return None
        v[15], v[16] = vals[16], vals[15]
        return rc.row_system(M64, G, c, v)
    if name == "one entry's feature moved by 16":
        return rc.mutate(name, M64, G, cols, vals, k)
    raise KeyError(name)
