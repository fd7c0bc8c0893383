"""Inputs for the entry-by-entry tests of the per-row solve kernels (tests/test_gpu_rows_exact.py) and the CPU statements
that make them trustworthy (tests/test_rows_cases.py).  No GPU, no torch.

The factor table and the values are chosen so that every row's system W x = b (ALS:447-494) is made of small exact integers
(in eighths, for the ridge) and W is very well conditioned.  Gathering and summing then cannot round -- neither the fp32
MFMAs of als_persistent_kernel nor the two- and three-term f16 splits of als_persistent_kernel_h / als_lds_kernel_h, whose
operands sqrt(w) S y are powers of two -- and only the k x k factorisation and the two triangular solves are left, a few
ulps.  One dropped, doubled or misplaced entry, weight, lane, feature block or ridge count then sticks out by orders of
magnitude (tests/test_rows_cases.py shows it for each by mutating the expected side).

Row j of a table has a hot feature f(j) and a scale s_j in {1, 2}:

  one-hot  M[j] = s_j e_f(j).  W is diagonal, x_f = b_f / W_ff: every entry of a row shows in exactly one output element and
           any cross-talk between two entries' contraction slots creates an off-diagonal that must not exist.
  two-hot  M[j] = s_j (e_f(j) +- e_g(j)), g != f drawn over all features, so that pairs straddle the 16-feature blocks and
           the off-diagonal tiles, the rank-16 updates of cholesky_tiles and solve_tiles carry data.  (k = 1 has no second
           feature: that table is the one-hot one again.)

Values are r in {+-1, +-4}, about 10 % negative; alpha = 1 so that w = alpha |r| in {1, 4} has an exact square root;
lambda = 1/8 so that the ridge lambda alpha n_u = n_u / 8 is exact.  The rules for W and b below restate chunk_weights and
add_ridge (csrc/als_kernels.h) read against ALS:466-488; the expected x* is an fp64 solve of the exact (W, b).

A row's columns and values depend on its length only (seeded by it), so the two order seeds shuffle the same rows."""
import numpy as np

ALL_K = [1, 7, 16, 17, 30, 32, 33, 48, 50, 64, 65, 80, 90, 96, 100, 112, 113, 128]   # every T = ceil(k/16), full and ragged
ONE_HOT, TWO_HOT = 1, 2
TABLES = (ONE_HOT, TWO_HOT)
FLAG_RECONSTRUCT_R, FLAG_LOSS_IGNORES_UNSPECIFIED = 1, 2
ALPHA, LAMBDA = 1.0, 0.125
ORDER_SEEDS = (1, 2)
ULP = 2.0 ** -23
FINISH_GROUP = 32        # csrc/work_plan.h: a row of more segments than this goes through als_prereduce_kernel first


def table_shape(k):
    """(rows, share of rows with scale 2).  k = 1 piles the whole table on one diagonal element: with 6000 rows at the
    usual scales that element is ~15000 and a ridge counted with n_u rounded up to 4 (3/8 at most) moves x by 2.5e-5,
    under 8 x BAR; the smaller and quieter table (it still holds the longest row's 4129 distinct columns) keeps every
    mutation of tests/test_rows_cases.py visible."""
    return (4200, 0.1) if k == 1 else (6000, 0.5)


def table(k, kind, seed=0, shape=None):
    """float32 [n, k].  Every feature is the hot one of n / k rows (+-1), so the Gramian's diagonal is level.
    shape: another (rows, share of rows with scale 2) than table_shape(k) (tests/dual_cases.py)."""
    n, p2 = shape or table_shape(k)
    rng = np.random.default_rng([seed, k, kind])
    f = rng.permutation(n) % k
    s = np.where(rng.random(n) < p2, 2.0, 1.0).astype(np.float32)
    M = np.zeros((n, k), dtype=np.float32)
    M[np.arange(n), f] = s
    if kind == TWO_HOT and k > 1:
        g = (f + rng.integers(1, k, size=n)) % k
        M[np.arange(n), g] = s * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=n)
    return M


def boundary_lengths():
    """Every length 0 .. 136 and the neighbourhoods of the larger powers of two: 4-entry steps, 32-entry super-steps, 64-entry
    chunks, the cuts at 64 / 192 / 4096 entries and the 32-slot groups of als_prereduce_kernel (from 2049 entries at 64)."""
    around = [n + d for n in (256, 512, 1024, 2048, 4096) for d in (-33, -32, -31, -1, 0, 1, 31, 32, 33)]
    return np.concatenate([np.arange(0, 137), np.array(around)]).astype(np.int64)


def shuffled_lengths(order_seed, min_len=0):
    lengths = boundary_lengths()
    lengths = lengths[lengths >= min_len]
    np.random.default_rng(order_seed).shuffle(lengths)
    return lengths


def row_entries(length, n_table, seed=0):
    """(ascending distinct columns int32, values float32 in {+-1, +-4}) of THE row of this length."""
    rng = np.random.default_rng([seed, 77, int(length)])
    cols = np.sort(rng.choice(n_table, size=int(length), replace=False)).astype(np.int32)
    vals = rng.choice(np.array([1.0, 4.0], dtype=np.float32), size=int(length))
    vals = np.where(rng.random(int(length)) < 0.1, -vals, vals).astype(np.float32)
    return cols, vals


def csr(lengths, n_table, seed=0):
    """(row_ptr int64, col int32, val float32) of the rows of these lengths, in this order."""
    rows = [row_entries(n, n_table, seed) for n in lengths]
    row_ptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    col = np.concatenate([c for c, _ in rows] or [np.zeros(0, np.int32)]).astype(np.int32)
    val = np.concatenate([v for _, v in rows] or [np.zeros(0, np.float32)]).astype(np.float32)
    return row_ptr, col, val


def exact_gramian(M):
    M64 = M.astype(np.float64)
    return M64.T @ M64


def weights(vals, flags, alpha):
    """(Gramian weight, right-hand-side weight) per entry: chunk_weights (csrc/als_kernels.h), ALS:466-482."""
    r = vals.astype(np.float64)
    base = 1.0 if flags & FLAG_LOSS_IGNORES_UNSPECIFIED else 0.0
    if flags & FLAG_RECONSTRUCT_R:
        return np.full(len(r), base), r
    ar = alpha * np.abs(r)
    return base + ar, np.where(r > 0, 1.0 + ar, 0.0)


def row_system(M64, G, cols, vals, flags=0, alpha=ALPHA, lam=LAMBDA, ridge_count=None):
    """The exact (W, b) of one row in float64: the Gramian (zeros under lossIgnoresUnspecified, ALS:524-539), the weighted
    outer products, the ridge lambda alpha n_u on the diagonal (add_ridge, ALS:488-492)."""
    k = M64.shape[1]
    w, cb = weights(vals, flags, alpha)
    Y = M64[cols]
    W = (Y * w[:, None]).T @ Y
    if not flags & FLAG_LOSS_IGNORES_UNSPECIFIED:
        W = W + G
    n_u = len(cols) if ridge_count is None else ridge_count
    W = W + (lam * alpha * n_u) * np.eye(k)
    b = (Y * cb[:, None]).sum(axis=0)
    return W, b


def solve64(W, b):
    return np.linalg.solve(W, b) if np.any(b) else np.zeros(len(b))


def systems(M, rows, flags=0, alpha=ALPHA, lam=LAMBDA):
    """rows: list of (cols, vals).  Returns (W [R, k, k], b [R, k], x* [R, k]) in float64."""
    M64, G = M.astype(np.float64), exact_gramian(M)
    Ws, bs = zip(*[row_system(M64, G, c, v, flags, alpha, lam) for c, v in rows])
    W, b = np.stack(Ws), np.stack(bs)
    return W, b, np.stack([solve64(Wi, bi) for Wi, bi in zip(W, b)])


def fp32_model(W, b):
    """The arithmetic the kernels are measured against: an fp32 LAPACK Cholesky of every W and two fp32 substitutions."""
    W32, b32 = W.astype(np.float32), b.astype(np.float32)
    L = np.linalg.cholesky(W32)
    assert L.dtype == np.float32
    R, k = b32.shape
    y = np.zeros((R, k), dtype=np.float32)
    for i in range(k):
        y[:, i] = (b32[:, i] - np.einsum("rj,rj->r", L[:, i, :i], y[:, :i]).astype(np.float32)) / L[:, i, i]
    x = np.zeros((R, k), dtype=np.float32)
    for i in range(k - 1, -1, -1):
        x[:, i] = (y[:, i] - np.einsum("rj,rj->r", L[:, i + 1:, i], x[:, i + 1:]).astype(np.float32)) / L[:, i, i]
    return x


def element_ulps(x, xs):
    """[R, k] |x - x*| / |x*| in units of 2^-23; where x* == 0: 0 if x == 0 exactly, inf otherwise."""
    x, xs = np.asarray(x, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(x - xs) / np.abs(xs) / ULP
    return np.where(xs == 0, np.where(x == 0, 0.0, np.inf), e)


def row_ulps(x, xs):
    """[R] ||x - x*||_2 / ||x*||_2 in units of 2^-23; for x* == 0: 0 if x == 0 exactly, inf otherwise."""
    x, xs = np.asarray(x, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    d, n = np.linalg.norm(x - xs, axis=1), np.linalg.norm(xs, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = d / n / ULP
    return np.where(n == 0, np.where(d == 0, 0.0, np.inf), e)


def gather_scale(G, max_abs_val, flags=0, alpha=ALPHA):
    """S of the split-precision gather as gather_scale_kernel chooses it for a table below 262144 rows: the power of two
    with sqrt(max_f G_ff) sqrt(w_max) S < 2^14."""
    base = 1.0 if flags & FLAG_LOSS_IGNORES_UNSPECIFIED else 0.0
    w_max = base + (0.0 if flags & FLAG_RECONSTRUCT_R else abs(alpha) * float(max_abs_val))
    bound = float(np.sqrt(np.diag(G).max())) * float(np.float32(np.sqrt(w_max)))
    if not bound > 0:
        return 1.0
    _, eb = np.frexp(bound)
    return float(np.ldexp(1.0, int(min(max(14 - eb, -60), 60))))


def segment_cuts(length, segment_nnz):
    """First entries of the segments plan_work_lists (csrc/work_plan.h) cuts a row of more than segment_nnz entries into by
    count, for segment_nnz <= 512 (above, the cut also depends on the device's size): equal parts, whole 4-entry steps.
    tests/test_work_plan.py holds this against the planner itself."""
    assert segment_nnz <= 512 and segment_nnz % 32 == 0 and length > segment_nnz
    nseg = -(-length // segment_nnz)
    per = (-(-length // nseg) + 3) & ~3
    return list(range(0, length, per))


# ---- mutations of the expected side: what a gather bug of each kind would compute ----------------------------------------
def mutate(name, M64, G, cols, vals, k):
    """The (W, b) a kernel with the named fault would form for the row, or None where the fault cannot show on this row."""
    n = len(cols)
    c, v = cols.copy(), vals.copy()
    if name == "drop the last entry":
        if n < 1:
            return None
        return row_system(M64, G, c[:-1], v[:-1], ridge_count=n)
    if name == "entry 63's column for entry 64":
        if n < 65:
            return None
        c[64] = c[63]
        return row_system(M64, G, c, v)
    if name in ("weights swapped across entry 32", "weights swapped across entry 64"):
        e = 32 if name.endswith("32") else 64
        if n <= e:
            return None
        v[e - 1], v[e] = vals[e], vals[e - 1]
        return row_system(M64, G, c, v)
    if name == "ridge count rounded up to 4":
        if n % 4 == 0:
            return None
        return row_system(M64, G, c, v, ridge_count=(n + 3) & ~3)
    if name == "one entry's feature moved by 16":
        if n < 1 or k <= 16:
            return None           # a single feature block: there is no other block to land in
        Mm = M64.copy()
        e = n // 2
        Mm[c[e]] = np.roll(M64[c[e]], 16)
        if np.array_equal(Mm[c[e]], M64[c[e]]):
            return None
        w, cb = weights(v, 0, ALPHA)
        Y = Mm[c]
        W = G + (Y * w[:, None]).T @ Y + (LAMBDA * ALPHA * n) * np.eye(k)
        return W, (Y * cb[:, None]).sum(axis=0)
    if name in ("last segment left out, cut at 64", "last segment left out, cut at 192"):
        seg = 64 if name.endswith("64") else 192
        if n <= seg:
            return None
        last = segment_cuts(n, seg)[-1]
        return row_system(M64, G, c[:last], v[:last], ridge_count=n)
    raise KeyError(name)


MUTATIONS = ["drop the last entry", "entry 63's column for entry 64", "weights swapped across entry 32",
             "weights swapped across entry 64", "ridge count rounded up to 4", "one entry's feature moved by 16",
             "last segment left out, cut at 64", "last segment left out, cut at 192"]
