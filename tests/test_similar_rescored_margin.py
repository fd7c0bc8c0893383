"""The rescored cosine filter's bound (csrc/topn_kernels.h, RESCORED COSINE MODE) against its worst case, on a CPU
restatement of the margin step the kernels run (the A / B slots of topn_stream_kernel<..., COS, RS> and
topn_prepare_kernel<true, true>, the item data of mals_rescorer_set_*), on top of tests/topn_filter_emulation.py:
  (a) rows whose bf16 roundings all point one way, scale at both ends of the supported range, offsets at its edge, one query
      item and three: the sample's bound never exceeds the exact rescored score, and the hit test passes every item at tau
      equal to its own exact score;
  (b) a margin that ignores scale_i, and one that puts 1 / n on the offset, each drop a winner;
  (c) the calls of the GPU filter-path test (tests/similar_rescored_cases.py), emulated: no query has more candidates than
      half of its candidate buffer, so the filter can answer every one of them without the dense path."""
import re

import numpy as np
import pytest

from tests import rescorer_oracle as ro
from tests import similar_rescored_cases as cases
from tests import similar_rescored_oracle as sro
from tests import similarity_oracle as so
from tests import topn_filter_emulation as fe

COVER = np.float32(fe._constant(fe._TEXT, "TOPN_RS_COVER"))
MAX_SCALE = float(re.search(r"constexpr\s+double\s+TOPN_RS_MAX_SCALE\s*=\s*([0-9.eE+-]+)\s*;", fe._TEXT).group(1))
MAX_OS = float(re.search(r"constexpr\s+double\s+TOPN_COS_RS_MAX_OS\s*=\s*([0-9.eE+-]+)\s*;", fe._TEXT).group(1))
C101 = np.float32(COVER * np.float32(1.01))
COVER_O = np.float64(fe.bf16_up(C101))              # topn_prepare_kernel<true, true>: lanes (2, c) slot 1


def bf(v):
    return np.asarray(fe.bf16(np.asarray(v, np.float32)), np.float64)


def in_range(scale, offset):
    """topn_cos_rs_in_range"""
    return 1.0 / MAX_SCALE <= scale <= MAX_SCALE and abs(offset) <= MAX_OS * scale


def item_terms(n0, scale, offset, filtered=None, wild=None):
    """the stream kernel's per-item products: rs32 / os32 from the item's bf16 pairs (mals_rescorer_set_*), P = fl32(n0 rs32),
    Q = fl32(n0 os32), each split into a bf16 pair (lo to nearest); a filtered item: P = 0, Q = -1e30.  Returns (Ph, Pl, Qh,
    Ql, fp32 scale (NaN: filtered))"""
    scale = np.broadcast_to(np.asarray(scale, np.float64), n0.shape)
    offset = np.broadcast_to(np.asarray(offset, np.float64), n0.shape)
    rs, os_ = 1.0 / scale, offset / scale
    rh = bf(fe.f32(rs))
    rl = bf(fe.f32(rs - rh))
    oh = bf(fe.f32(os_))
    ol = bf(fe.f32(os_ - oh))
    rs32, os32 = fe.f32(rh + rl), fe.f32(oh + ol)
    with np.errstate(over="ignore", invalid="ignore"):
        P = fe.f32(n0.astype(np.float64) * rs32)
        Q = fe.f32(n0.astype(np.float64) * os32)
    sf = scale.astype(np.float32)
    if filtered is not None:
        P = np.where(filtered, np.float32(0), P).astype(np.float32)
        Q = np.where(filtered, np.float32(-1e30), Q).astype(np.float32)
        sf = np.where(filtered, np.float32(np.nan), sf).astype(np.float32)
    if wild is not None:     # weights outside the range: P = 0, Q = +1e30 (a hit of every query), never a bucket's winner
        P = np.where(wild, np.float32(0), P).astype(np.float32)
        Q = np.where(wild, np.float32(1e30), Q).astype(np.float32)
        sf = np.where(wild, np.float32(np.nan), sf).astype(np.float32)
    with np.errstate(invalid="ignore"):
        Ph, Qh = bf(P), bf(Q)
        Pl, Ql = bf(fe.f32(P - Ph)), bf(fe.f32(Q - Qh))
    return Ph, Pl, Qh, Ql, sf


def lower_bound(approx, ny, n0, m0, floor, it, offset_div=1.0):
    """MODE 0: ((approx - M_c |y|' - floor + Q - cover |Q hi|) / n0) * scale_f32; -inf: never wins a bucket"""
    Ph, Pl, Qh, Ql, sf = it
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        acc = fe.f32(approx.astype(np.float64) - fe.margin_i(ny, m0, floor) + (Qh + Ql) / offset_div - np.abs(Qh) * COVER_O)
        lb = fe.f32(fe.f32(acc * fe.f32(np.float32(1) / n0)) * sf)
    ok = (n0 > 0) & np.isfinite(n0) & ~np.isnan(lb)
    return np.where(ok, lb, np.float32(-np.inf)).astype(np.float32)


def hits(approx, ny, n0, m0, floor, it, tau, offset_div=1.0):
    """MODE 1: approx + M_c |y|' +- floor + (P hi + P lo)(-tau hi + -tau lo) + Q + covers is not below zero.  approx: [items]
    or [items, queries] with tau [queries]"""
    Ph, Pl, Qh, Ql, sf = it
    tau = np.atleast_1d(np.asarray(tau, np.float32))
    v = np.where(tau > -np.inf, -tau, np.float32(1e30)).astype(np.float32)
    th = bf(v)
    tl = np.asarray(fe.bf16_up(fe.f32(v - th)), np.float64)
    ct = np.asarray(fe.bf16_up(fe.f32(C101 * np.abs(v))), np.float64)
    ok = (n0 > 0) & np.isfinite(n0)
    own = fe.bf16_up(ny).astype(np.float64) * np.float64(m0) + np.where(ok, 1.0, -1.0) * np.float64(floor) + (Qh + Ql) / offset_div + np.abs(Qh) * COVER_O
    one = approx.ndim == 1
    a = approx[:, None] if one else approx
    with np.errstate(over="ignore", invalid="ignore"):
        acc = fe.f32(a.astype(np.float64) + own[:, None] + (Ph + Pl)[:, None] * (th + tl)[None, :] + Ph[:, None] * ct[None, :])
    h = ((acc > 0) | ((acc == 0) & ~np.signbit(acc)) | np.isnan(acc)) & ok[:, None]
    return h[:, 0] if one else h


# ---- (a) the bound at the worst roundings --------------------------------------------------------------------------------
def worst_catalogue(k, n):
    """(Y, query items): the query items are cosine_query(k) -- a unit vector whose D half rounds down and whose U half rounds
    up -- and exact power-of-two multiples of it (the same unit vector); the rows carry D on the D half (approximation too
    low) or U on the U half (too high), at several magnitudes and both signs"""
    xq, h, c = fe.cosine_query(k)
    rows = [xq * np.float32(s) for s in (1.0, 2.0, 0.5)[:n]]
    for mag in (1.0, 2.0 ** 10, 2.0 ** -10, 3.0):
        for sign in (1.0, -1.0):
            d = np.zeros(k, np.float32)
            d[:h] = fe.D
            u = np.zeros(k, np.float32)
            u[h:2 * h] = fe.U
            both = d + u
            for r in (d, u, both):
                rows.append((r * np.float32(mag * sign)).astype(np.float32))
    return np.stack(rows).astype(np.float32), list(range(n))


EDGE_SCALES = [1.0 / MAX_SCALE, MAX_SCALE, 1.0, 1.0 / MAX_SCALE * 1.37, MAX_SCALE / 1.0000001, 0.7, 3.7, 12345.678]


@pytest.mark.parametrize("k", [10, 31, 64, 100, 128])
@pytest.mark.parametrize("n", [1, 3])
def test_bound_holds_at_the_worst_roundings(k, n):
    Y, items = worst_catalogue(k, n)
    x, nrm, m0, floor = fe.prepare(Y[items], cos=True)
    approx = fe.approx_scores(Y, x)
    n0, ny = fe.item_norms(Y)
    Yn = so.norms(Y)
    cand = np.arange(n, len(Y))
    for scale in EDGE_SCALES:
        for os_ in (0.0, MAX_OS, -MAX_OS, 0.37, -1.0, 17.3):
            offset = os_ * scale
            assert in_range(scale, offset)
            exact, ok = sro.scores(Y, items, ro.AffineRescorer(scale=scale, offset=offset), Ynorm=Yn)
            assert ok[cand].all() and np.isfinite(exact[cand]).all()
            it = item_terms(n0, scale, offset)
            lb = lower_bound(approx, ny, n0, m0, floor, it)
            assert np.all(lb[cand].astype(np.float64) <= exact[cand].astype(np.float64)), (scale, offset, lb[cand], exact[cand])
            for i in cand:
                one = tuple(a[i:i + 1] for a in it)
                assert hits(approx[i:i + 1], ny[i:i + 1], n0[i:i + 1], m0, floor, one, exact[i])[0], (scale, offset, i, exact[i])


def test_random_weights_in_range():
    rng = np.random.default_rng(5)
    for k in (10, 64, 128):
        for n in (1, 3):
            Y, items = worst_catalogue(k, n)
            x, nrm, m0, floor = fe.prepare(Y[items], cos=True)
            approx = fe.approx_scores(Y, x)
            n0, ny = fe.item_norms(Y)
            Yn = so.norms(Y)
            cand = np.arange(n, len(Y))
            for _ in range(25):
                scale = np.exp2(rng.uniform(-20, 20, len(Y)))
                offset = rng.uniform(-MAX_OS, MAX_OS, len(Y)) * scale * np.exp2(-rng.uniform(0, 12, len(Y)))
                exact, ok = sro.scores(Y, items, ro.AffineRescorer(scale=scale, offset=offset), Ynorm=Yn)
                it = item_terms(n0, scale, offset)
                lb = lower_bound(approx, ny, n0, m0, floor, it)
                assert np.all(lb[cand].astype(np.float64) <= exact[cand].astype(np.float64))
                for i in cand:
                    one = tuple(a[i:i + 1] for a in it)
                    assert hits(approx[i:i + 1], ny[i:i + 1], n0[i:i + 1], m0, floor, one, exact[i])[0], (scale[i], offset[i], i)


def test_the_range_predicate():
    assert in_range(1.0, 64.0) and in_range(1.0, -64.0) and not in_range(1.0, 64.1)
    assert in_range(2.0 ** -20, 2.0 ** -14) and not in_range(2.0 ** -20, 2.0 ** -13)
    assert in_range(2.0 ** 20, 2.0 ** 26) and not in_range(2.0 ** 21, 0.0) and not in_range(2.0 ** -21, 0.0)


def test_an_item_outside_the_range_is_a_candidate_of_every_query_and_never_sets_the_threshold():
    """a rescorer may keep a few items with weights outside the range on the filter path: in the sample they never win a
    bucket, in the hit test they pass at any tau -- the exact rescore decides what they score"""
    Y, items = worst_catalogue(64, 1)
    x, nrm, m0, floor = fe.prepare(Y[items], cos=True)
    approx = fe.approx_scores(Y, x)
    n0, ny = fe.item_norms(Y)
    scale = np.ones(len(Y))
    offset = np.zeros(len(Y))
    wild = np.zeros(len(Y), bool)
    for i, (s, f) in zip((3, 4, 5), ((1.0, 1e39), (2.0 ** 30, 0.0), (1e-30, -1e300))):
        scale[i], offset[i], wild[i] = s, f, True
        assert not in_range(s, f)
    it = item_terms(n0, scale, offset, wild=wild)
    lb = lower_bound(approx, ny, n0, m0, floor, it)
    assert np.all(lb[wild] == -np.inf) and np.all(lb[~wild] > -np.inf)
    for tau in (-1e6, 0.0, 0.99, 1e6, 2.0 ** 27, 1e30):
        assert hits(approx, ny, n0, m0, floor, it, np.float32(tau))[wild].all(), tau


# ---- (b) wrong margins drop a winner -------------------------------------------------------------------------------------
def filter_topn(Y, items, how_many, scale, offset, wrong=None):
    """sample / threshold / filter / exact rescore of one query, every item its own bucket: tau = the N-th largest lower bound;
    the candidates' exact rescored scores, the N best (ties by index).  wrong = "scale": the hit test adds the cosine margin
    in the rescored domain, scale_i ignored; wrong = "offset_over_n": the offset enters divided by the number of query items,
    as RESCORED MODE's does"""
    x, nrm, m0, floor = fe.prepare(Y[items], cos=True)
    approx = fe.approx_scores(Y, x)
    n0, ny = fe.item_norms(Y)
    it = item_terms(n0, scale, offset)
    lb = lower_bound(approx, ny, n0, m0, floor, it)
    lb[items] = -np.inf                                      # the query's own items are struck from the buckets
    tau = np.sort(lb)[-how_many]
    if wrong == "scale":
        h = fe.f32(scale * approx.astype(np.float64) / n0 + offset + fe.margin_i(ny, m0, floor) / n0 - np.float64(tau)) >= 0
    elif wrong == "offset_over_n":
        h = hits(approx, ny, n0, m0, floor, it, tau, offset_div=float(len(items)))
    else:
        h = hits(approx, ny, n0, m0, floor, it, tau)
    exact, ok = sro.scores(Y, items, ro.AffineRescorer(scale=scale, offset=offset))
    h = h & ok
    h[items] = False
    c = np.flatnonzero(h)
    order = np.lexsort((c, -exact[c].astype(np.float64)))[:how_many]
    return c[order], exact[c][order]


def test_a_margin_that_ignores_the_scale_drops_a_winner():
    """Item W rounds down on every feature of the query's D half (its approximate cosine is ~2^-7 below its exact one) and
    carries scale 1000; the fillers are unscaled with offsets that put their exact scores just below W's.  Their lower bounds
    set tau; the right hit test passes W, one that adds M_c in the rescored domain without scale_i loses it."""
    k = 64
    xq, h, c = fe.cosine_query(k)
    n_fill = 20
    w = np.zeros(k, np.float32)
    w[:h] = fe.D
    fill = np.zeros(k, np.float32)
    fill[:2 * h] = 1.0                                       # bf16-exact rows
    Y = np.stack([xq, w] + [fill * np.float32(1 + j) for j in range(n_fill)]).astype(np.float32)
    cos = so.cosine64(Y, Y[0])
    scale = np.ones(len(Y))
    scale[1] = 1000.0
    offset = np.zeros(len(Y))
    offset[2:] = scale[1] * cos[1] - cos[2:] - 0.02 * (1 + np.arange(n_fill))   # exact scores just below W's
    r = ro.AffineRescorer(scale=scale, offset=offset)
    for hm in (1, 3):
        oidx, osc = sro.most_similar(Y, [0], hm, r)
        assert oidx[0] == 1
        got = filter_topn(Y, [0], hm, scale, offset)
        assert np.array_equal(got[0], oidx) and np.array_equal(got[1].view(np.uint32), osc.view(np.uint32))
        naive = filter_topn(Y, [0], hm, scale, offset, wrong="scale")
        assert 1 not in naive[0].tolist() and not np.array_equal(naive[0], oidx)


def test_a_margin_with_the_offset_over_n_drops_a_winner():
    """Two query items; W has a low cosine and offset 8, the fillers a high cosine and offset 5.  Per term W scores m + 8 and
    wins; a hit test that divides the offset by n sees m + 4 < tau and loses it."""
    k = 32
    rng = np.random.default_rng(9)
    xq, h, c = fe.cosine_query(k)
    q2 = xq * np.float32(2)
    w = (rng.standard_normal(k) * 0.3).astype(np.float32)
    fills = [(xq + (rng.standard_normal(k) * 0.02).astype(np.float32)).astype(np.float32) for _ in range(12)]
    Y = np.stack([xq, q2, w] + fills).astype(np.float32)
    offset = np.full(len(Y), 5.0)
    offset[2] = 8.0
    scale = np.ones(len(Y))
    r = ro.AffineRescorer(scale=scale, offset=offset)
    for hm in (1, 4):
        oidx, osc = sro.most_similar(Y, [0, 1], hm, r)
        assert oidx[0] == 2
        got = filter_topn(Y, [0, 1], hm, scale, offset)
        assert np.array_equal(got[0], oidx) and np.array_equal(got[1].view(np.uint32), osc.view(np.uint32))
        wrong = filter_topn(Y, [0, 1], hm, scale, offset, wrong="offset_over_n")
        assert 2 not in wrong[0].tolist()


# ---- (c) the GPU filter-path test's calls, emulated ----------------------------------------------------------------------
def approx_batch(Yb, X):
    """fe.approx_scores for several queries on one catalogue: Yb = bf16(Y) as float64 (converted once), X [queries][k]"""
    k = Yb.shape[1]
    S = (k + 31) // 32
    xb = fe.bf16(X).astype(np.float64)
    acc = np.zeros((len(Yb), len(X)), np.float32)
    for s in range(S):
        f = np.array([8 * S * g + 8 * s + j for g in range(4) for j in range(8)])
        f = f[f < k]
        acc = fe.f32(acc.astype(np.float64) + Yb[:, f] @ xb[:, f].T)
    return acc


@pytest.mark.parametrize("k", cases.FILTER_KS)
def test_the_filter_path_test_stays_within_half_of_its_candidate_buffers(k):
    """every query of every call of tests/test_gpu_similar_rescored.py's filter-path test: the emulated candidate count is at
    most half of the capacity 48 how_many + 2048 (sample stride: topn_plan's), and the sample yields a threshold -- so the
    test's "answered by the filter path, no fallback" is a condition the design meets with room"""
    Y = cases.filter_catalogue(k)
    n_items = len(Y)
    n0, ny = fe.item_norms(Y)
    specs, calls = cases.filter_calls(k)
    Yb = fe.bf16(Y).astype(np.float64)
    x11 = fe.prepare(Y[11:12], cos=True)[0]
    assert np.array_equal(approx_batch(Yb[:4096], x11[None, :])[:, 0], fe.approx_scores(Y[:4096], x11))
    worst = 0.0
    for kind, how_many, flag, queries in calls:
        assert fe.filter_path(n_items, how_many)
        S, cap, stride, n_groups = fe.plan(n_items, how_many, k)
        filt, scale, offset = specs[kind]
        o = cases.oracle_rescorer(specs[kind])
        sc, of, fm = o.arrays(n_items)
        assert all(in_range(s, f) for s, f in zip(sc[::997], of[::997]))
        it = item_terms(n0, sc, of, fm)
        live = [q for q in queries if not (flag and any(o.is_filtered(i) for i in q))]
        for b in range(0, len(live), 32):
            chunk = live[b:b + 32]
            prep = [fe.prepare(Y[q], cos=True) for q in chunk]
            _, _, m0, floor = prep[0]                                   # (cosine: |x| and with it the margin entry is the same for every query)
            approx = approx_batch(Yb, np.stack([p[0] for p in prep]))
            taus = []
            for j, q in enumerate(chunk):
                lb = lower_bound(approx[:, j], ny, n0, m0, floor, it)
                taus.append(fe.threshold(lb, n_items, how_many, stride, n_groups, drop=np.asarray(q, np.int64)))
            assert all(t > -np.inf for t in taus), (kind, how_many, taus)
            h = hits(approx, ny, n0, m0, floor, it, np.asarray(taus, np.float32))
            counts = h.sum(axis=0)
            worst = max(worst, float(counts.max()) / cap)
            assert np.all(2 * counts <= cap), (kind, how_many, counts, cap)
    print("k = %d: the fullest candidate buffer is at %.3f of its capacity" % (k, worst))
