"""numpy restatement of the top-N filter of csrc/topn_kernels.h (sample -> threshold -> filter -> exact rescore -> final),
arithmetic step by step: the prepare kernel's query operand x (bf16, round to nearest as v_cvt_pk_bf16_f32 does), |x| and
the margin entry {bf16_up(M |x|), bf16_up(floor), -tau hi, -tau lo}; the stream kernel's approximate score (exact bf16
products, fp32 accumulation per 32-feature MFMA step), its |y_i|' and margin step (MODE 0: the lower bound, MODE 1: the
hit test; cosine mode: the hi / lo tau |y| slots); the threshold's bucket rule and topn_plan's tile stride.  The margin
constants are read from the header, so the tests follow whatever it says.  Test infrastructure (CPU): what this returns
is compared with oracle/topn_oracle.py and tests/similarity_oracle.py so that the FILTER is validated without a GPU."""
import os
import re

import numpy as np
import torch

from oracle import topn_oracle as to
from tests import similarity_oracle as so

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "myrrix-recommender_amd", "csrc", "topn_kernels.h")


def _constant(text, name):
    m = re.search(r"constexpr\s+(?:float|int)\s+%s\s*=\s*([-+0-9.eE]+)f?\s*;" % name, text)
    assert m, name
    return float(m.group(1))


with open(HEADER) as _f:
    _TEXT = _f.read()
TOPN_MARGIN = np.float32(_constant(_TEXT, "TOPN_MARGIN"))
TOPN_COS_MARGIN = np.float32(_constant(_TEXT, "TOPN_COS_MARGIN"))
TOPN_MARGIN_FLOOR = np.float32(_constant(_TEXT, "TOPN_MARGIN_FLOOR"))
TOPN_SAMPLE_GROUPS = int(_constant(_TEXT, "TOPN_SAMPLE_GROUPS"))
TOPN_FILTER_MAX_N = int(_constant(_TEXT, "TOPN_FILTER_MAX_N"))
THRESHOLD_THREADS = 1024          # topn_threshold_kernel's block: thread t owns buckets t, t + 1024, ...


def bf16(v):
    """fp32 -> bf16 -> fp32, round to nearest even (torch's cast; v_cvt_pk_bf16_f32 on gfx950)."""
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def bf16_up(v):
    """the kernels' bf16_up: positive values rounded away from zero, negative ones truncated (both: toward +inf)."""
    u = np.atleast_1d(np.asarray(v, np.float32)).view(np.uint32).astype(np.uint64)
    u = np.where(u & 0x80000000, u, u + 0xFFFF) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(v))


def f32(v):
    return np.float32(v) if np.ndim(v) == 0 else np.asarray(v, np.float32)


# ---- topn_plan / topn_launch_stream_QT ---------------------------------------------------------------------------------
def plan(n_items, how_many, k):
    """(S, cap, tile_stride, n_groups) as topn_plan and the sample's launch compute them."""
    S = (k + 31) // 32
    cap = 48 * how_many + 2048
    target = max(512 * how_many, max(16384, n_items // 8))
    tile_stride = max(1, n_items // target)
    tiles = (n_items + 16 * tile_stride - 1) // (16 * tile_stride)
    stages = (tiles + 3) // 4
    n_groups = max(1, min(stages, TOPN_SAMPLE_GROUPS))
    return S, cap, tile_stride, n_groups


def filter_path(n_items, how_many):
    """topn_dense_only, negated (MALS_TOPN_FULL unset)."""
    return not (n_items < 131072 or n_items >= 0xFFFFFFFF or how_many > TOPN_FILTER_MAX_N or n_items // 16 < 64 * how_many)


def sampled(items, tile_stride):
    return (np.asarray(items, np.int64) >> 4) % tile_stride == 0


def bucket(items, tile_stride, n_groups):
    """the sample bucket of sampled items (topn_threshold_kernel's `drop`; the stream kernel's MODE 0 comment)"""
    items = np.asarray(items, np.int64)
    return 16 * (((items >> 4) // tile_stride >> 2) % n_groups) + (items & 15)


# ---- topn_prepare_kernel -----------------------------------------------------------------------------------------------
def prepare(vectors, cos=False):
    """One query of n vectors (n x k fp32) -> (x as the filter sees it before the bf16 cast (fp32), |x| (fp32), the margin
    entry's slots 0 and 1 (bf16 values))."""
    v = np.atleast_2d(np.asarray(vectors, np.float32))
    n = len(v)
    if cos:
        qn = so.norms(v)
        assert np.all(qn > 0) and np.all(np.isfinite(qn)), "zero / non-finite query items are answered without the filter"
        x = f32((v.astype(np.float64) / qn[:, None]).sum(axis=0) / n)
        nrm = np.float32(1.000001)
        m0 = bf16_up(f32(TOPN_COS_MARGIN * nrm))
    else:
        x = f32(v.astype(np.float64).sum(axis=0) / n)
        norms = np.sqrt((v.astype(np.float64) ** 2).sum(axis=1)).sum()
        nrm = np.float32(norms / n * 1.000001)
        m0 = bf16_up(f32(TOPN_MARGIN * nrm))
    return x, nrm, m0, bf16_up(TOPN_MARGIN_FLOOR)


# ---- topn_stream_kernel ------------------------------------------------------------------------------------------------
def approx_scores(Y, x):
    """sum_f bf16(y_f) bf16(x_f) for every row: exact products, summed per MFMA step s (features 8 S g + 8 s + j of the
    four lane groups g) and added to the fp32 accumulator once per step."""
    Y = np.asarray(Y, np.float32)
    k = Y.shape[1]
    S = (k + 31) // 32
    CH = 8 * S
    Yb = bf16(Y).astype(np.float64)
    xb = bf16(x).astype(np.float64)
    acc = np.zeros(len(Y), np.float32)
    for s in range(S):
        f = np.array([CH * g + 8 * s + j for g in range(4) for j in range(8)])
        f = f[f < k]
        acc = f32(acc.astype(np.float64) + Yb[:, f] @ xb[f])
    return acc


def item_norms(Y):
    """(n0, ny): the stream kernel's fp32 |y_i| (lane-sequential FMA sums of squares, then the two xor-shuffle adds, sqrt)
    and |y_i|' = n0 * 1.0000005 (the margin's factor)."""
    Y = np.asarray(Y, np.float32)
    k = Y.shape[1]
    CH = 8 * ((k + 31) // 32)
    part = []
    for g in range(4):
        a = np.zeros(len(Y), np.float32)
        for s in range(CH):
            if g * CH + s < k:
                y = Y[:, g * CH + s].astype(np.float64)
                a = f32(y * y + a.astype(np.float64))              # one rounding: the FMA
        part.append(a)
    nsq = f32(f32(part[0] + part[1]) + f32(part[2] + part[3]))   # xor 16, then xor 32
    n0 = f32(np.sqrt(nsq))
    return n0, f32(n0 * np.float32(1.0000005))


def margin_i(ny, m0, floor):
    """the margin the margin step adds (MODE 1) or subtracts (MODE 0): bf16_up(|y_i|') * bf16_up(M |x|) + floor, exact"""
    return bf16_up(ny).astype(np.float64) * np.float64(m0) + np.float64(floor)


def lower_bound(approx, ny, n0, m0, floor, cos=False):
    """MODE 0: the value a sampled item offers its bucket (-inf: never wins)"""
    lb = f32(approx.astype(np.float64) - margin_i(ny, m0, floor))
    if cos:
        ok = (n0 > 0) & np.isfinite(n0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            lb = f32(lb * f32(np.float32(1) / n0))
        lb = np.where(ok, lb, np.float32(-np.inf)).astype(np.float32)
    return lb


def tau_slots(tau, cos=False):
    """MODE 1: the -tau entries of the query's margin operand (recommend: {hi, lo}; cosine: {hi, hi, lo, lo})"""
    v = np.float32(-tau) if tau > -np.inf else np.float32(1e30)
    hi = np.float32(bf16(np.float32(v)).ravel()[0])
    lo = np.float32(bf16_up(np.float32(v - hi)).ravel()[0])
    return np.float64(hi), np.float64(lo)


def hits(approx, ny, n0, m0, floor, tau, cos=False):
    """MODE 1: (item, query) is a hit iff the accumulator after the margin step is not below zero (+0 counts, -0 not)"""
    hi, lo = tau_slots(tau, cos)
    if cos:   # A = {|y|' up, +-1, |y| hi, lo, hi, lo} against B = {M_c, floor, -tau hi, hi, lo, lo}; a zero row: -floor
        ok = (n0 > 0) & np.isfinite(n0)
        nh = bf16(n0).astype(np.float64)
        nl = bf16(f32(n0 - nh)).astype(np.float64)
        add = bf16_up(ny).astype(np.float64) * np.float64(m0) + np.where(ok, 1.0, -1.0) * np.float64(floor)
        add = add + nh * hi + nl * hi + nh * lo + nl * lo
    else:     # A = {|y|' up, 1, 1, 1} against B = {M, floor, -tau hi, -tau lo}
        add = margin_i(ny, m0, floor) + hi + lo
    acc = f32(approx.astype(np.float64) + add)
    h = (acc > 0) | ((acc == 0) & ~np.signbit(acc)) | np.isnan(acc)
    if cos:
        h &= ok
    return h


# ---- topn_threshold_kernel ---------------------------------------------------------------------------------------------
def threshold(lb, n_items, how_many, tile_stride, n_groups, drop=()):
    """tau: the how_many-th largest of the per-thread maxima of the bucket row (buckets whose best item is dropped --
    known / excluded / tag items -- left out whole); -inf if fewer than how_many threads hold a finite entry."""
    items = np.flatnonzero(sampled(np.arange(n_items), tile_stride))
    b = bucket(items, tile_stride, n_groups)
    v = lb[items]
    n_row = 16 * n_groups
    bmax = np.full(n_row, -np.inf, np.float32)
    bidx = np.full(n_row, -1, np.int64)
    order = np.lexsort((items, -v.astype(np.float64), b))         # per bucket: best first, ties to the lower index
    first = np.ones(len(order), bool)
    first[1:] = b[order][1:] != b[order][:-1]
    win = order[first]
    keep = v[win] > -np.inf                                       # an item that never beats -inf does not win its bucket
    bmax[b[win][keep]] = v[win][keep]
    bidx[b[win][keep]] = items[win][keep]
    if len(drop):
        bmax[np.isin(bidx, np.asarray(drop, np.int64))] = -np.inf
    per_thread = np.full(THRESHOLD_THREADS, -np.inf, np.float32)
    np.maximum.at(per_thread, np.arange(n_row) % THRESHOLD_THREADS, bmax)
    fin = np.sort(per_thread[per_thread > -np.inf])[::-1]
    return np.float32(fin[how_many - 1]) if len(fin) >= how_many else np.float32(-np.inf)


# ---- the whole pass ----------------------------------------------------------------------------------------------------
def topn(Y, vectors, how_many, cos=False, exclude=(), known=(), tags=(), norms=None):
    """One query through the filter as the device runs it.  vectors: the query's vectors (recommend: the user's vector or
    the recommendToMany set; cosine: the query items' rows, and exclude = those items -- mostSimilarItems strikes them).
    exclude / known: items struck from the answer and from the sample's buckets.  Returns (indices, scores, info) where info holds tau,
    the candidate count and whether the dense path would have answered (then the result is the exact one).  norms:
    item_norms(Y), when the caller runs several queries on one Y."""
    Y = np.asarray(Y, np.float32)
    n_items, k = Y.shape
    assert filter_path(n_items, how_many)
    S, cap, tile_stride, n_groups = plan(n_items, how_many, k)
    x, nrm, m0, floor = prepare(vectors, cos)
    approx = approx_scores(Y, x)
    n0, ny = item_norms(Y) if norms is None else norms
    struck = np.unique(np.concatenate([np.asarray(a, np.int64).ravel() for a in (exclude, known, tags)] + [np.zeros(0, np.int64)]))
    lb = lower_bound(approx, ny, n0, m0, floor, cos)
    tau = threshold(lb, n_items, how_many, tile_stride, n_groups, drop=struck)
    h = hits(approx, ny, n0, m0, floor, tau, cos)
    cand = np.flatnonzero(h)
    info = {"tau": tau, "candidates": len(cand), "tile_stride": tile_stride, "n_groups": n_groups}
    v = np.atleast_2d(np.asarray(vectors, np.float32))
    info["dense"] = bool(not tau > -np.inf or len(cand) > cap)
    if cos:
        items = [int(i) for i in np.atleast_1d(exclude)]
        if info["dense"]:
            oidx, osc = so.most_similar(Y, items, how_many, tags=np.asarray(tags, np.int64) if len(tags) else None)
            return oidx, osc, info
        Yn = so.norms(Y)
        total = np.zeros(len(cand), np.float64)
        ok = np.ones(len(cand), bool)
        for it in items:
            s = so.cosine64(Y[cand], Y[it], norm_x=Yn[it], norm_y=Yn[cand])
            ok &= np.isfinite(s)
            total = total + s
        sc = f32(total / float(len(items)))
    else:
        if info["dense"]:
            oidx, osc = to.recommend(Y, v if len(v) > 1 else v[0], how_many, struck if len(struck) else None)
            return oidx, osc, info
        sc = to.scores(Y[cand], v[0]) if len(v) == 1 else to.scores_to_many(Y[cand], v)
        ok = np.ones(len(cand), bool)
    ok &= ~np.isin(cand, struck)
    c, s = cand[ok], sc[ok]
    order = np.lexsort((c, -s.astype(np.float64)))[:how_many]
    return c[order], s[order], info


# ---- adversarial catalogues: coherent bf16 rounding -------------------------------------------------------------------
# Values just below / above a bf16 rounding midpoint: D rounds DOWN by almost 2^-8 of itself, U rounds UP by as much, BUMP
# (just below the midpoint above 1 + 2^-7) rounds down too.  Products of two such values miss by almost 2 * 2^-8 in the
# same direction, so a row whose every term is D x D (or U x U) reaches the worst case of the approximation.
D = np.float32(1 + 2.0 ** -8 - 2.0 ** -20)
U = np.float32(1 + 2.0 ** -8 + 2.0 ** -20)
BUMP = np.float32(1 + 3 * 2.0 ** -8 - 2.0 ** -20)
D_HIGH = np.float32(1 + 2.0 ** -8 - 2.0 ** -21)   # still rounds down; a hair above D exactly


def _background(rng, n_items, k, x):
    """small random rows, each pointing away from x: they never compete with the planted items"""
    Y = (rng.standard_normal((n_items, k)) * 0.01).astype(np.float32)
    s = Y.astype(np.float64) @ np.asarray(x, np.float64)
    Y[s > 0] *= np.float32(-1)
    return Y


def _layout(n_items, how_many, k, n_high):
    """(high-error items: sampled tiles, one per bucket and per threshold thread; winners: unsampled tiles, the last one in
    the partial last tile)"""
    _, _, stride, n_groups = plan(n_items, how_many, k)
    assert n_high <= min(n_groups, THRESHOLD_THREADS // 16)
    high = 16 * (4 * stride * np.arange(n_high, dtype=np.int64))     # stage j, bucket 16 j: thread 16 j
    win = 16 * (4 * stride * np.arange(how_many, dtype=np.int64) + 1) + np.arange(how_many) % 16
    win = np.append(win, n_items - 1)
    assert sampled(high, stride).all() and not sampled(win, stride).any() and n_items % 16
    assert len(np.unique(bucket(high, stride, n_groups) % THRESHOLD_THREADS)) == n_high
    return high, win


def recommend_catalogue(k, how_many, n_items=140_003, seed=0):
    """(Y, x, high, win) for recommend: x = D on the first half, U on the second; each high-error item B is U on x's U half
    (approximate score too HIGH by ~1.41 * 2^-8 |x||y|), each winner T is D on x's D half with one BUMP (too LOW by as much,
    exact score 2^-7 above B's).  The last winner also has D_HIGH for D: the best exact score of all.  The oracle answers the
    winners; a filter whose margin is under sqrt(2) * 2^-8 answers the B's."""
    h = k // 2
    x = np.ones(k, np.float32)
    x[:h], x[h:2 * h] = D, U
    rng = np.random.default_rng(seed)
    Y = _background(rng, n_items, k, x)
    high, win = _layout(n_items, how_many, k, how_many)
    Y[high] = 0
    Y[high, h:2 * h] = U
    Y[win] = 0
    Y[win, :h] = D
    Y[win[-1], :h] = D_HIGH
    Y[win, 0] = BUMP
    return Y, x, high, win


def cosine_query(k):
    """(unit vector with the D / U pattern on 2 h components of magnitude 2^-e, the rest in two adjuster components (the
    last two), h, 2^-e): the pattern as large as it fits, so that the cosines of B and T are as large as they can be"""
    best = None
    for e in range(1, 8):
        c = 2.0 ** -e
        h = min((k - 2) // 2, int(0.97 / (2 * c * c * float(U) ** 2)))
        if h >= 1 and (best is None or h * c * c > best[0] * best[1] ** 2):
            best = (h, c)
    h, c = best
    x = np.zeros(k, np.float64)
    x[:h] = c * np.float64(D)
    x[h:2 * h] = c * np.float64(U)
    a = np.sqrt((1.0 - (x * x).sum()) / 2)
    x[k - 2:] = a
    return x.astype(np.float32), h, np.float32(c)


def cosine_catalogue(k, how_many, adjust=2.0 ** -10, n_items=140_003, seed=0):
    """(Y, query item, high, win) for mostSimilarItems: the query item's row is cosine_query(k); each B is U on the U half;
    each winner T is D on the D half with `adjust` on the last adjuster component (the last winner: 2 adjust, the best
    cosine of all) -- the exact cosine a little above B's, the approximation well below."""
    xq, h, c = cosine_query(k)
    rng = np.random.default_rng(seed)
    Y = _background(rng, n_items, k, xq)
    high, win = _layout(n_items, how_many, k, how_many)
    q = 16 * 3 + 5                                                  # tile 3: never sampled (stride >= 4 here)
    assert not sampled(q, plan(n_items, how_many, k)[2]) and q not in win
    Y[q] = xq
    Y[high] = 0
    Y[high, h:2 * h] = U
    Y[win] = 0
    Y[win, :h] = D
    Y[win, k - 1] = np.float32(adjust)
    Y[win[-1], k - 1] = np.float32(2 * adjust)
    return Y, q, high, win


def _off_midpoint(rng, n, up, far=False):
    """n positive values (mantissas a little above 1) just off bf16 rounding midpoints: up -> they round UP by nearly half an ulp, else DOWN; far: the
    offset from the midpoint anywhere in (0, half of the half ulp) -- the same rounding, a different exact value"""
    g = bf16(rng.uniform(1, 1.0625, n).astype(np.float32)).astype(np.float64)   # mantissas near 1: relative error near 2^-8
    half = 2.0 ** -8
    off = rng.uniform(2.0 ** -20, half / 2, n) if far else np.full(n, 2.0 ** -20)
    return (g + half + (off if up else -off)).astype(np.float32)


FAMILY_GAP = 0.25   # the winners' exact scores lie (0, FAMILY_GAP) * 2^-8 |x||y| above the high-error rows'


def _tune(y, x, target, t1, t2):
    """set the bf16-exact features t1, t2 of row y (zero so far) so that its exact score against x is target: t1 carries
    the bulk, t2 the residual (a residual of ~2^-16 of it is left)"""
    y[t1] = bf16(np.float32((target - float(to.scores(y[None, :], x)[0])) / float(x[t1]))).ravel()[0]
    y[t2] = bf16(np.float32((target - float(to.scores(y[None, :], x)[0])) / float(x[t2]))).ravel()[0]


def random_family(seed, n_items=140_003, n_patterns=4):
    """A randomized family of the catalogues: (Y, patterns [P x k], how_many, k).  Each pattern x is signed values just off
    bf16 midpoints (mantissas near 1), half of its features rounding down (D set), half up (U set).  Per pattern
    how_many + 4 high-error rows B (U set, rounding up: approximate score too high by ~sqrt(2) * 2^-8 |x||y|; sampled tiles,
    one per bucket and threshold thread), all with one exact score L, and max(1, how_many / 2) winners T (D set, rounding
    down: too low by as much; unsampled tiles, three of the family's in the partial last tile), each a random amount in
    (0, FAMILY_GAP * 2^-8 |x||y|) above L.  Two bf16-exact features of each row set its exact score.  Every winner belongs
    in the answer; a margin M hides a winner whose gap is under about (2 sqrt(2) - 2 M / 2^-8) 2^-8 |x||y| -- a margin
    below ~1.3 * 2^-8 misses most of them.  The other rows are small and point away from every pattern."""
    rng = np.random.default_rng(880_000 + seed)
    k = int(rng.choice([30, 64, 100, 128]))
    how_many = int(rng.choice([1, 10, 64]))
    _, _, stride, n_groups = plan(n_items, how_many, k)
    n_high, n_win = how_many + 4, max(1, how_many // 2)
    assert n_patterns * n_high <= n_groups
    sign = np.where(rng.random((n_patterns, k)) < 0.5, -1, 1).astype(np.float32)
    X = np.zeros((n_patterns, k), np.float32)
    sets = []
    for p in range(n_patterns):
        perm = rng.permutation(k)
        dset, uset = perm[:k // 2], perm[k // 2:]
        X[p, dset] = _off_midpoint(rng, len(dset), up=False)
        X[p, uset] = _off_midpoint(rng, len(uset), up=True)
        sets.append((dset, uset))
    X *= sign
    Y = (rng.standard_normal((n_items, k)) * 0.001).astype(np.float32)
    away = np.sign(Y.astype(np.float64) @ X.sum(axis=0).astype(np.float64))
    Y *= -away[:, None].astype(np.float32)
    Y = np.where(np.abs(Y) < 1e-6, 0, Y).astype(np.float32)
    j = np.arange(n_patterns * n_high)
    high = 16 * (4 * stride * j) + (j // 64) % 16                   # distinct stages, buckets and threshold threads
    j = np.arange(n_patterns * n_win)
    low = 16 * (4 * stride * j + 1 + j % 3) + j % 16
    low[:min(3, len(low))] = n_items - 1 - np.arange(min(3, len(low)))   # the partial last tile
    assert sampled(high, stride).all() and not sampled(low, stride).any()
    for p in range(n_patterns):
        dset, uset = sets[p]
        xn = float(np.linalg.norm(X[p].astype(np.float64)))
        rows = {}
        for r in high[p * n_high:(p + 1) * n_high]:
            y = np.zeros(k, np.float32)
            y[uset[2:]] = _off_midpoint(rng, len(uset) - 2, up=True) * sign[p, uset[2:]]
            rows[r] = (y, uset)
        for r in low[p * n_win:(p + 1) * n_win]:
            y = np.zeros(k, np.float32)
            y[dset[2:]] = _off_midpoint(rng, len(dset) - 2, up=False) * sign[p, dset[2:]]
            rows[r] = (y, dset)
        level = max(float(to.scores(y[None, :], X[p])[0]) for y, _ in rows.values()) + 0.5 * float(np.abs(X[p]).min())
        for r, (y, fset) in rows.items():
            gap = 0.0 if fset is uset else rng.uniform(0.02, 1) * FAMILY_GAP * 2.0 ** -8 * xn * float(np.linalg.norm(y.astype(np.float64)))
            _tune(y, X[p], level + gap, fset[0], fset[1])
            Y[r] = y
    return Y, X, how_many, k
