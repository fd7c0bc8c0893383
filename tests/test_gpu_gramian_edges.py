"""The Gramian kernels (csrc/als_kernels.h: gramian_partial_kernel, gramian_split_kernel + gramian_reduce_slabs_kernel,
gramian_finalize_kernel, gramian_pack_kernel) element by element, at every tile count T = ceil(k/16) and every tail.

  * integer data (tests/gramian_cases.py; their exactness is proved on the CPU by tests/test_gramian_cases.py): every
    row range, slab size and power-of-two scale must give the exact integer Gramian -- np.array_equal, no tolerance;
  * edge-dominated real data: max |G_ij - Ge_ij| / sqrt(Ge_ii Ge_jj) against the float64 product at the kernel's own
    5e-7, with the weight in the last step of the ragged slab, the first step of a slab, the last row;
  * the recorded maximum |element| (operand bound of the split-precision gather) with the maximum on the edges, after
    the factors changed, and through the group's max-reduction;
  * the two writers of the fp32 image Gf (finalize and pack) through the rows they produce."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from oracle import oracle
from tests import gramian_cases as gc

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4          # the project's bar on factors (relative Frobenius vs the oracle)
GRAMIAN_TOL = 5e-7      # the project's bar on the Gramian kernels
SIDE = pkg.SIDE_Y

D_SPLIT = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 513, 1536, 2047]     # rows past 262144 at row_begin = 0
D_SHIFTED = [0, 1, 17, 33, 65, 513]                                            # ... and at row_begin = 1 and 7
N_F64 = [1, 2, 3, 4, 5, 63, 64, 65, 255, 257, 4097, 65535, 65537, 262143]      # fp64 kernel, at row_begin = 0 and 3


def rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / max(np.linalg.norm(b.astype(np.float64)), 1e-30))


def replica(k, M, **kw):
    core = pkg.ALSCore(k, **kw)
    core.set_factor_rows(SIDE, len(M))
    core.set_factors(SIDE, M)
    return core


def mismatch(G, Ge):
    """None when G equals Ge and its own transpose exactly, else what differs."""
    if np.array_equal(G, Ge) and np.array_equal(G, G.T):
        return None
    wrong = G != Ge
    i, j = np.unravel_index(int(np.argmax(np.where(wrong, np.abs(np.nan_to_num(G - Ge, nan=np.inf)), 0.0))), G.shape)
    return {"wrong": int(wrong.sum()), "asymmetric": int((G != G.T).sum()), "at": [int(i), int(j)], "got": float(G[i, j]), "want": float(Ge[i, j])}


def check_ranges(core, k, expect, cases, scale=1.0):
    """gramian_partial on every (row_begin, n_rows) of `cases`; returns the list of the ranges that are not exact."""
    import torch
    out = torch.empty(k, k, dtype=torch.float64, device="cuda")
    bad = []
    for begin, n in cases:
        out.fill_(float("nan"))          # an element the kernels do not write stays NaN
        torch.cuda.synchronize()
        core.gramian_partial(SIDE, begin, n, out)
        torch.cuda.synchronize()
        m = mismatch(out.cpu().numpy(), expect(begin, n) * scale)
        if m is not None:
            bad.append(dict(m, row_begin=begin, n_rows=n))
    return bad


# ---- 2. every instantiation, every tail: exact integer Gramians -----------------------------------------------------
@pytest.mark.parametrize("k", gc.ALL_K)
def test_integer_gramian_is_exact_on_every_path_and_tail(k):
    M, _ = gc.integer_matrix(gc.N_ROWS, k, seed=k)
    rg = gc.RangeGramian(M)
    cases = [(0, gc.SPLIT_MIN_ROWS + d) for d in D_SPLIT]
    cases += [(b, gc.SPLIT_MIN_ROWS + d) for b in (1, 7) for d in D_SHIFTED]
    cases += [(b, n) for b in (0, 3) for n in N_F64]
    with replica(k, M) as core:
        bad = check_ranges(core, k, rg, cases)
        G = core.gramian(SIDE, fetch=True)           # the whole replica through mals_gramian (split path)
        G2 = core.gramian(SIDE, fetch=True)
    assert not bad, (k, bad)
    assert mismatch(G, rg(0, gc.N_ROWS)) is None, (k, mismatch(G, rg(0, gc.N_ROWS)))
    assert np.array_equal(G, G2)


@pytest.mark.parametrize("k", [48, 80, 112])
def test_integer_gramian_is_scale_invariant(k):
    """M 2^s -> G 2^(2s), bit for bit: the running scale 2^pw, the exact rescale of the sums and the multiply back.
    |s| <= 40 is tested; the kernel's contract is about |s| <= 49 for values of this size (its comment)."""
    M, _ = gc.integer_matrix(gc.N_ROWS, k, seed=k)
    rg = gc.RangeGramian(M)
    cases = [(0, gc.SPLIT_MIN_ROWS + 17), (1, gc.SPLIT_MIN_ROWS + 33), (7, gc.SPLIT_MIN_ROWS + 513)]
    Ge = rg(0, gc.N_ROWS)
    for s in (-40, -20, 20, 40):
        with replica(k, M * np.float32(2.0 ** s)) as core:
            bad = check_ranges(core, k, rg, cases, scale=2.0 ** (2 * s))
            G = core.gramian(SIDE, fetch=True)
        assert not bad, (k, s, bad)
        assert mismatch(G, Ge * 2.0 ** (2 * s)) is None, (k, s, mismatch(G, Ge * 2.0 ** (2 * s)))


SLAB_K = [33, 81, 113]


def slab_cases(slab):
    tails = sorted({slab - 32, slab - 16, slab - 1, slab, slab + 1, slab + 16, slab + 32})
    return [(0, gc.SPLIT_MIN_ROWS + d) for d in tails] + [(1, gc.SPLIT_MIN_ROWS + slab + 1), (7, gc.SPLIT_MIN_ROWS + slab - 1)]


def slab_child():
    """Runs in a fresh process (the slab size is read once per process): one JSON line with what was not exact."""
    slab = int(os.environ["MALS_GRAMIAN_SLAB_ROWS"])
    report = {"slab": slab, "checked": 0, "bad": []}
    for k in SLAB_K:
        M, _ = gc.integer_matrix(gc.N_ROWS, k, seed=k)
        rg = gc.RangeGramian(M)
        cases = slab_cases(slab)
        with replica(k, M) as core:
            bad = check_ranges(core, k, rg, cases)
            G = core.gramian(SIDE, fetch=True)
        m = mismatch(G, rg(0, gc.N_ROWS))
        if m is not None:
            bad.append(dict(m, row_begin=0, n_rows=gc.N_ROWS))
        report["checked"] += len(cases) + 1
        report["bad"] += [dict(b, k=k) for b in bad]
    print(json.dumps(report))


@pytest.mark.parametrize("slab", [64, 1024, 2048])
def test_integer_gramian_is_exact_at_every_slab_size(slab):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MALS_GRAMIAN_SLAB_ROWS=str(slab))
    code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_gramian_edges import slab_child; slab_child()" % root
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    report = json.loads(p.stdout.strip().splitlines()[-1])
    assert report["slab"] == slab and report["checked"] == len(SLAB_K) * (len(slab_cases(slab)) + 1)
    assert report["bad"] == [], report["bad"]


# ---- 3. the lo terms and the scale logic at the edges: real data, per element ------------------------------------------
_EDGE = {}


def edge_case(k):
    """(base matrix, its float64 Gramian) -- computed once per k and shared by the three index sets."""
    if k not in _EDGE:
        _EDGE.clear()
        base = gc.edge_base(gc.EDGE_N, k, seed=k)
        _EDGE[k] = (base, gc.exact_gramian(base))
    return _EDGE[k]


@pytest.mark.parametrize("where", ["last step of the ragged slab", "first step of a slab", "last row of the matrix"])
@pytest.mark.parametrize("k", gc.EDGE_K)
def test_edge_dominated_gramian_element_by_element(k, where):
    """Rows scaled by 2^10 in the last step of the ragged slab, the first step of a slab, the last row.  A lost hi.lo
    pass in such a step costs ~2^-11; the bar is the kernel's 5e-7.

    Measured max |G_ij - Ge_ij| / sqrt(Ge_ii Ge_jj) on an MI355X:
        k     last step of the ragged slab   first step of a slab   last row of the matrix
        30    2.75e-7                        2.91e-7                2.65e-7
        48    2.75e-7                        3.21e-7                3.30e-7
        65    2.98e-7                        2.75e-7                2.98e-7
        96    3.16e-7                        2.46e-7                3.16e-7
        100   3.11e-7                        2.66e-7                3.11e-7
        128   3.98e-7                        2.85e-7                3.98e-7
    What is left is the split product itself: lo.lo dropped (<= 2^-22) and two 22-bit operands (2 x 2^-23), 4.8e-7 in
    the worst case.  The first-step column measured 4.6 .. 8.9e-7 (over the bar at five of the six k) while the slab
    kept ONE set of float32 sums: every later step of the slab (15 of 32 rows, 31 of 16 rows) added its quiet products
    to sums the loud step dominates and rounded at up to 2^-24 of them.  The kernel now ends the slab in front of a
    step that is 2^5 quieter than one before it (once per slab); a second launch sums the rest from zero."""
    base, G0 = edge_case(k)
    b, r = gc.edge_sets(gc.EDGE_N, k)[where]
    with replica(k, base) as core:
        core.set_factors(SIDE, base[b:b + r] * np.float32(gc.EDGE_SCALE), b)
        G = core.gramian(SIDE, fetch=True)
    R = base[b:b + r].astype(np.float64)
    Ge = G0 + (gc.EDGE_SCALE ** 2 - 1.0) * (R.T @ R)      # the float64 product of the scaled matrix, to 1e-15
    err = gc.per_element_error(G, Ge)
    print("k=%d %s: per-element error %.3e" % (k, where, err))
    assert np.array_equal(G, G.T)
    assert err < GRAMIAN_TOL, (k, where, err)


@pytest.mark.parametrize("k", [16, 40, 80, 96])
def test_large_gramian_at_the_remaining_tile_counts(k):
    """The data of test_gpu_parity.test_large_gramian_on_the_f16_pipe_matches_oracle at T = 1, 3, 5, 6 (5 and 6: the
    16-row-step body with two buffers), with its assertions and the per-element metric on top.
    Measured per-element error on an MI355X: k = 16 2.30e-7, k = 40 2.19e-7, k = 80 2.16e-7, k = 96 3.23e-7.  (k = 96
    draws one row, 153884, that alone is 61 % of the trace of G and sits in the middle of its 512-row slab: 5.99e-7
    before the kernel gave the quiet steps behind such a row a partial of their own.)"""
    rng = np.random.default_rng(k)
    n = 300_001
    M = rng.standard_normal((n, k)).astype(np.float32)
    M *= np.exp(rng.standard_normal(n) * 2.0).astype(np.float32)[:, None]     # row norms over ~4 decades
    M[12345] *= 1.0e3
    M[200_000:200_016] = 0.0
    with replica(k, M) as core:
        G = core.gramian(SIDE, fetch=True)
        G2 = core.gramian(SIDE, fetch=True)
    Go = oracle.gramian(M)
    Ge = gc.exact_gramian(M)
    err = gc.per_element_error(G, Ge)
    print("k=%d: per-element error %.3e, relative Frobenius %.3e" % (k, err, rel(G, Ge)))
    assert np.array_equal(G, G2)
    assert np.array_equal(G, G.T)
    assert rel(G, Go) < GRAMIAN_TOL, (k, rel(G, Go))
    assert rel(G, Ge) < GRAMIAN_TOL, (k, rel(G, Ge))
    assert err < GRAMIAN_TOL, (k, err)


# ---- 4. the recorded maximum ------------------------------------------------------------------------------------------
PEAK = 37.5


def direct_rows_problem(n_items, k, seed, n_rows=100):
    """~100 rows of 100-200 entries (direct kernels at every k) over standard normal item rows."""
    rng = np.random.default_rng(seed)
    cols = [np.unique(rng.integers(0, n_items, size=int(m))) for m in rng.integers(100, 201, size=n_rows)]
    row_ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    col = np.concatenate(cols).astype(np.int32)
    val = rng.integers(1, 6, size=len(col)).astype(np.float32)
    M = rng.standard_normal((n_items, k)).astype(np.float32)
    return (row_ptr, col, val), M


@pytest.mark.parametrize("k", [81, 64])
def test_recorded_maximum_on_the_edges_and_never_stale(k):
    """k = 81: T = 6 with the lone feature 80 in the last 16-block; k = 64: the kfull body.  The maximum sits in the
    first element, the last element (ragged last step, last block), the first row of the ragged slab and the first
    feature of the last row; after the row is overwritten the bound must follow."""
    n_items = gc.SPLIT_MIN_ROWS + 17
    csr, M = direct_rows_problem(n_items, k, seed=400 + k)
    n_rows = len(csr[0]) - 1
    quiet_max = np.float32(np.abs(M).max())
    assert quiet_max < 8.0
    G0 = gc.exact_gramian(M)
    X0 = oracle.solve_rows(*csr, M, G0, threads=8)
    with pkg.ALSCore(k, solve_mode=_lib.SOLVE_DIRECT) as core:
        core.set_factor_rows(pkg.SIDE_X, n_rows)
        core.set_factor_rows(pkg.SIDE_Y, n_items)
        core.set_matrix(pkg.SIDE_X, *csr)
        core.set_factors(pkg.SIDE_Y, M)
        for i, j in ((0, 0), (n_items - 1, k - 1), (gc.SPLIT_MIN_ROWS, k - 1), (n_items - 1, 0)):
            old = M[i].copy()
            M[i, j] = PEAK
            core.set_factors(pkg.SIDE_Y, M[i:i + 1], i)
            core.half_iteration(pkg.SIDE_X)
            _, _, flag, bound = core.gather_scale()
            X = core.get_factors(pkg.SIDE_X)
            new, o64 = M[i].astype(np.float64), old.astype(np.float64)
            Xo = oracle.solve_rows(*csr, M, G0 - np.outer(o64, o64) + np.outer(new, new), threads=8)
            assert flag == 1.0, (i, j, flag)
            assert np.float32(bound) == np.float32(PEAK), (i, j, bound)
            assert rel(X, Xo) < REL_TOL, (i, j, rel(X, Xo))
            # the row back to normal values: a stale maximum must not survive
            M[i] = old
            core.set_factors(pkg.SIDE_Y, M[i:i + 1], i)
            core.half_iteration(pkg.SIDE_X)
            _, _, flag, bound = core.gather_scale()
            assert flag == 1.0 and np.float32(bound) == quiet_max, (i, j, flag, bound, quiet_max)
            assert rel(core.get_factors(pkg.SIDE_X), X0) < REL_TOL


@pytest.mark.parametrize("n_items,peak_row,exact", [
    (2 * gc.SPLIT_MIN_ROWS + 37, "first", True),     # both slices on the split kernel; the maximum in member 0's first row
    (2 * gc.SPLIT_MIN_ROWS + 37, "last", True),      # ... in member 1's last row
    (gc.SPLIT_MIN_ROWS + 300_000, "last", True),     # two ragged slices of 281072 rows: equal ranges, both on the split kernel
    (2 * gc.SPLIT_MIN_ROWS - 1, "first", False),     # 262144 + 262143 rows: member 1 runs the fp64 kernel, its maximum is unknown
])
def test_group_maximum_reaches_every_member(n_items, peak_row, exact):
    """group_gramian cuts the replica into equal row ranges (ceil(n / world) rows each), every member records the
    maximum of its range and the slot-wise maximum over the members is installed with the summed Gramian.  A range
    below 262144 rows runs the fp64 kernel, which marks its maximum unknown: the bound is then the diagonal's."""
    k = 80
    csr, M = direct_rows_problem(n_items, k, seed=500 + n_items % 1000)
    n_rows = len(csr[0]) - 1
    M[0 if peak_row == "first" else n_items - 1, 3] = PEAK
    per = (n_items + 1) // 2
    assert per >= gc.SPLIT_MIN_ROWS and (n_items - per >= gc.SPLIT_MIN_ROWS) == exact
    Xo = oracle.solve_rows(*csr, M, gc.exact_gramian(M), threads=8)
    with pkg.GroupALS.single_process(k, [0, 0], backend=_lib.GROUP_PEER_COPY) as g:
        g.set_factor_rows(pkg.SIDE_X, n_rows)
        g.set_factor_rows(pkg.SIDE_Y, n_items)
        g.set_matrix(pkg.SIDE_X, *csr)
        g.set_factors(pkg.SIDE_Y, M)
        g.half_iteration(pkg.SIDE_X)
        g.synchronize()
        scales = [g.local(i)[0].gather_scale() for i in range(2)]
        X = g.get_factors(pkg.SIDE_X, 0, n_rows)
    for _, _, flag, bound in scales:
        if exact:
            assert flag == 1.0 and np.float32(bound) == np.float32(PEAK), scales
        else:
            assert bound > PEAK, scales
    assert scales[0] == scales[1]
    assert rel(X, Xo) < REL_TOL, rel(X, Xo)


# ---- 5. the two writers of Gf -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [3000, gc.SPLIT_MIN_ROWS + 17])
@pytest.mark.parametrize("k", [7, 33, 50, 81, 100, 128])
def test_both_writers_of_the_fp32_image_give_the_same_rows(k, n_items):
    """half_iteration solves from the image gramian_finalize_kernel wrote (<T,true,16> below 262144 rows, <T,false>
    above); set_gramian of the very same doubles goes through gramian_pack_kernel.  Both images are (float) of the same
    values in the same layout, so with the fp32 gather (no operand scale in play) the rows must be identical."""
    rng = np.random.default_rng(600 + k)
    cols = [np.unique(rng.integers(0, n_items, size=int(m))) for m in rng.integers(150, 301, size=60)]
    row_ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    col = np.concatenate(cols).astype(np.int32)
    val = rng.integers(1, 6, size=len(col)).astype(np.float32)
    M = (rng.standard_normal((n_items, k)) * 0.1).astype(np.float32)
    with pkg.ALSCore(k, gramian_mode=_lib.GRAMIAN_FP32, solve_mode=_lib.SOLVE_DIRECT) as core:
        core.set_factor_rows(pkg.SIDE_X, 60)
        core.set_factor_rows(pkg.SIDE_Y, n_items)
        core.set_matrix(pkg.SIDE_X, row_ptr, col, val)
        core.set_factors(pkg.SIDE_Y, M)
        core.half_iteration(pkg.SIDE_X)
        Xa = core.get_factors(pkg.SIDE_X)
        G = core.gramian(pkg.SIDE_Y, fetch=True)
        core.set_gramian(pkg.SIDE_Y, G)
        core.solve_side(pkg.SIDE_X)
        core.check()
        Xb = core.get_factors(pkg.SIDE_X)
    assert np.all(np.isfinite(Xa)) and np.abs(Xa).max() > 0
    assert np.array_equal(Xa, Xb), (k, n_items, rel(Xa, Xb))
    assert rel(Xa, oracle.solve_rows(row_ptr, col, val, M, gc.exact_gramian(M), threads=4)) < REL_TOL
