"""Inputs for the element-by-element Gramian tests (tests/test_gpu_gramian_edges.py) and the CPU statements that make
them trustworthy (tests/test_gramian_cases.py).

Two seeded generators:

  * integer_matrix: entries are integers in [-7, 7], no row is all zero, a few "loud" rows are multiplied by 64 and sit
    on slab and step boundaries as well as at random places.  Every partial sum any of the Gramian kernels forms of
    such rows is an integer below 2^24 (in units of the running power-of-two scale), so the fp64 MFMA, the two-f16
    split (lo = 0: a value of at most 9 significant bits is an f16 at any power-of-two scale), the fp32 slab sums, their
    exact rescale and the fp64 sums across slabs are all exact: the GPU result must EQUAL the integer Gramian.
  * edge_base / EDGE_SETS: standard normal rows of which a short index range -- the last step of the ragged slab, the
    first step of a slab, the last row -- is scaled by 2^10 and so carries nearly all of G.

split_slab_restatement restates one slab of gramian_split_kernel (csrc/als_kernels.h) in numpy: the per-step maximum,
the scale 2^pw lowered with an exact rescale of the sums, the one cut of the slab where a much quieter step follows,
the f16 hi / lo split by round-to-nearest, three product passes accumulated in float32 and the multiply back.  On the
integer data it reproduces the exact product bit for bit (asserted on the CPU), so a GPU mismatch can only be a row or
a feature dropped, doubled or misplaced."""
import numpy as np

SPLIT_MIN_ROWS = 262144            # GRAMIAN_SPLIT_MIN_ROWS (csrc/mals_api.hip): the split-f16 kernel runs from here on
N_ROWS = SPLIT_MIN_ROWS + 2200     # rows of the integer replica: 136 MB at k = 128
LOUD = 64                          # factor of a loud row
LOUD_WINDOW, LOUD_PER_WINDOW = 512, 4
ALL_K = [1, 7, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128]   # every T = ceil(k/16), ragged and full

# loud rows placed on purpose (all kernels' step is 16 or 32 rows, slabs are 512 .. 2048 rows, or 64 forced):
LOUD_FIXED = [
    0, 511,                        # first row; last row of the first 512-row slab
    512, 512 + 15,                 # first row of a slab; last row of its first 16-row step
    1024 + 16, 1024 + 31,          # first row of a second 16-row step; last row of a first 32-row step
    1536 + 32, 1536 + 63,          # first row of the second buffer at 32-row steps; last row of that buffer pair
    2047, 2048,                    # either side of a 1024- and a 2048-row slab boundary
    2048 + 64,                     # first row of the second buffer pair
    SPLIT_MIN_ROWS - 1,            # last row of the last full slab
    SPLIT_MIN_ROWS,                # the one-row slab (d = 1)
    SPLIT_MIN_ROWS + 16,           # one row past a full 16-row step (d = 17)
    SPLIT_MIN_ROWS + 32,           # one row past a full 32-row step / a 16-row buffer pair (d = 33)
    SPLIT_MIN_ROWS + 512,          # one-row slab behind a full one (d = 513)
    SPLIT_MIN_ROWS + 1535,         # last row of d = 1536
    SPLIT_MIN_ROWS + 2046,         # last row of d = 2047
]


def tiles(k):
    return (k + 15) // 16


def step_rows(k):
    """Rows per step of gramian_split_kernel<T>: 32 for T <= 4 (E = 8), 16 above (E = 4)."""
    return 32 if tiles(k) <= 4 else 16


def max_loud_per_window(loud_rows, window=LOUD_WINDOW):
    """Largest number of loud rows in any `window` consecutive rows."""
    r = np.sort(np.asarray(loud_rows, dtype=np.int64))
    if len(r) == 0:
        return 0
    first_outside = np.searchsorted(r, r + window, side="left")   # window [r_i, r_i + window)
    return int((first_outside - np.arange(len(r))).max())


def loud_rows(n_rows, seed):
    """The fixed boundary rows plus one random row in every 2048-row block that has no fixed row within 1024 rows."""
    rng = np.random.default_rng(seed)
    fixed = np.array([r for r in LOUD_FIXED if r < n_rows], dtype=np.int64)
    n_blocks = n_rows // 2048
    cand = np.arange(n_blocks, dtype=np.int64) * 2048 + rng.integers(0, 2048, size=n_blocks)
    if len(fixed) and len(cand):
        cand = cand[np.abs(cand[:, None] - fixed[None, :]).min(axis=1) > 1024]
    rows = np.unique(np.concatenate([fixed, cand]))
    assert max_loud_per_window(rows) <= LOUD_PER_WINDOW
    return rows


def integer_matrix(n_rows, k, seed):
    """(M float32 [n_rows, k], loud row indices).  Integers in [-7, 7], loud rows x 64, no all-zero row."""
    rng = np.random.default_rng(seed)
    M = rng.integers(-7, 8, size=(n_rows, k)).astype(np.float32)
    zero = np.flatnonzero(~M.any(axis=1))
    M[zero, zero % k] = 1.0
    loud = loud_rows(n_rows, seed + 1)
    M[loud] *= np.float32(LOUD)
    return M, loud


def exact_gramian(M):
    """M^T M in float64: exact for integer data (every sum far below 2^53)."""
    M64 = M.astype(np.float64)
    return M64.T @ M64


class RangeGramian:
    """Exact Gramians of row ranges of one integer matrix from prefix sums at every `block` rows plus the few rows
    between a range's ends and the nearest checkpoints -- all integers in float64, so every step is exact."""

    def __init__(self, M, block=4096):
        self.M, self.block = M, block
        n, k = M.shape
        nb = n // block
        cum = np.zeros((nb + 1, k, k))
        for b in range(nb):
            cum[b + 1] = cum[b] + exact_gramian(M[b * block:(b + 1) * block])
        self.cum = cum

    def prefix(self, x):
        b = x // self.block
        return self.cum[b] + exact_gramian(self.M[b * self.block:x])

    def __call__(self, row_begin, n_rows):
        return self.prefix(row_begin + n_rows) - self.prefix(row_begin)


def window_abs_max(M, window=2048, offset=0):
    """max element of |M|^T |M| over the rows [offset + i window, offset + (i + 1) window), the largest over i: the
    bound on every partial sum a slab of at most `window` rows starting at such a row can form."""
    A = np.abs(M[offset:]).astype(np.float64)
    worst = 0.0
    for r0 in range(0, len(A), window):
        blk = A[r0:r0 + window]
        worst = max(worst, float((blk.T @ blk).max()))
    return worst


def sliding_abs_bound(M, window=2048):
    """An upper bound of max(|M|^T |M|) over EVERY `window` consecutive rows (any slab start): the sum of the rows'
    squared largest |element|."""
    m2 = np.abs(M).max(axis=1).astype(np.float64) ** 2
    c = np.concatenate([[0.0], np.cumsum(m2)])
    w = min(window, len(m2))
    return float((c[w:] - c[:-w]).max())


FLUSH_BINADES = 5                  # GRAMIAN_FLUSH_BINADES (csrc/als_kernels.h)


# The integer fixtures fire the cut in every slab that has a loud row ahead of quiet steps (a loud step at want = 5, a
# quiet one at want = 11), so the exact GPU cases test it against the integer product, not against this restatement.
def split_slab_partials(rows, step):
    """One slab of gramian_split_kernel on `rows` (float32 [n, k]) with `step` rows per step: the two float32 partials the
    kernel stores for the slab, as full k x k matrices.  The first holds the sums up to the first step that is 2^5 quieter
    than a step before it, where the kernel cuts the slab, the second the rest (zeros when there is no cut: the kernel then
    neither writes nor reads it)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, k = rows.shape
    acc = np.zeros((k, k), dtype=np.float32)
    first = np.zeros((k, k), dtype=np.float32)
    flushed = False
    pw = 100

    def back(p):
        return np.float32(2.0 ** (0 if p == 100 else min(max(-2 * p, -126), 126)))

    for r0 in range(0, n, step):
        raw = rows[r0:r0 + step]
        m = np.float32(np.abs(raw).max())
        if m != 0:
            eb = ((int(m.view(np.int32)) >> 23) & 255) - 126       # step max < 2^eb
            want = 14 - eb
            if not flushed and pw != 100 and want >= pw + FLUSH_BINADES:
                first, acc, pw, flushed = acc * back(pw), np.zeros((k, k), dtype=np.float32), 100, True
            if want < pw:
                if pw != 100:
                    acc = acc * np.float32(2.0 ** max(2 * (want - pw), -120))
                pw = want
        pwc = 0 if pw == 100 else min(max(pw, -100), 100)
        z = raw * np.float32(2.0 ** pwc)
        hi = z.astype(np.float16).astype(np.float32)
        lo = (z - hi).astype(np.float16).astype(np.float32)          # z - hi is exact in float32
        acc = acc + hi.T @ hi
        acc = acc + hi.T @ lo
        acc = acc + lo.T @ hi
    return first, acc * back(pw)


def split_slab_restatement(rows, step):
    """The slab's contribution to G: its two float32 partials summed in float64, as the stages behind the kernel do."""
    first, second = split_slab_partials(rows, step)
    assert first.dtype == np.float32 and second.dtype == np.float32
    return first.astype(np.float64) + second.astype(np.float64)


# ---- edge-dominated real data ------------------------------------------------------------------------------------
EDGE_N = SPLIT_MIN_ROWS + 17       # 512 full slabs and a ragged one of 17 rows
EDGE_SCALE = 2.0 ** 10
EDGE_K = [30, 48, 65, 96, 100, 128]


def edge_base(n_rows, k, seed):
    return np.random.default_rng(seed).standard_normal((n_rows, k)).astype(np.float32)


def edge_sets(n_rows, k, slab=512):
    """name -> (first row, number of rows) of the rows that are scaled by 2^10."""
    step = step_rows(k)
    ragged0 = (n_rows // slab) * slab
    tail = n_rows - ragged0
    last_step0 = ragged0 + ((tail - 1) // step) * step
    return {
        "last step of the ragged slab": (last_step0, n_rows - last_step0),
        "first step of a slab": (300 * slab, step),
        "last row of the matrix": (n_rows - 1, 1),
    }


def per_element_error(G, Ge):
    """max |G_ij - Ge_ij| / sqrt(Ge_ii Ge_jj)."""
    d = np.sqrt(np.diag(Ge))
    return float((np.abs(G - Ge) / (d[:, None] * d[None, :])).max())
