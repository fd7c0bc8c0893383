"""Rescored recommendations on the device (mals_*_rescored, include/myrrix_als.h "rescorers"; the filter's bound in
csrc/topn_kernels.h, RESCORED MODE) against the CPU restatement tests/rescorer_oracle.py: indices and score bits identical
in every case, on the dense path and on the filter path."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd.core import MalsError
from tests import rescorer_oracle as ro

pytestmark = pytest.mark.gpu

FILTER_ITEMS = 140000      # >= 131072: the filter path (how_many <= 64)
DENSE_ITEMS = 3000


def catalogue(n_items, k, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_items, k)) * 0.3).astype(np.float32)


def core_with(Y, X=None):
    core = pkg.ALSCore(Y.shape[1])
    core.set_factor_rows(pkg.SIDE_Y, len(Y))
    core.set_factors(pkg.SIDE_Y, Y)
    if X is not None:
        core.set_factor_rows(pkg.SIDE_X, len(X))
        core.set_factors(pkg.SIDE_X, X)
    return core


def check(idx, sc, cnt, oidx, osc):
    n = len(oidx)
    assert cnt == n, (cnt, n)
    assert np.all(idx[n:] == -1)
    assert np.array_equal(idx[:n], oidx), (idx[:n], oidx)
    assert np.array_equal(sc[:n].view(np.uint32), np.asarray(osc, np.float32).view(np.uint32)), (sc[:n], osc)


def rescorers(core, n_items, rng):
    """(device Rescorer, oracle rescorer) of every kind the issue names"""
    filt = rng.choice(n_items, n_items // 10, replace=False)
    scale = rng.uniform(0.25, 4.0, n_items)
    offset = rng.standard_normal(n_items) * 0.5
    out = []
    for kind in ("filter", "weights", "uniform", "combined", "filter_half"):
        r = core.rescorer()
        if kind == "filter":
            r.set_filter(filt)
            o = ro.AffineRescorer(filtered=filt)
        elif kind == "weights":
            r.set_weights(scale[: n_items - 100], offset[: n_items - 100])      # the last rows uncovered
            o = ro.AffineRescorer(scale=scale[: n_items - 100], offset=offset[: n_items - 100])
        elif kind == "uniform":
            r.set_uniform(3.0, -0.75)
            o = ro.AffineRescorer(scale=3.0, offset=-0.75)
        elif kind == "combined":
            r.set_filter(filt)
            r.set_weights(scale, offset)
            o = ro.AffineRescorer(filtered=filt, scale=scale, offset=offset)
        else:   # FilterHalfRescorerProvider: odd ids filtered, x 10
            odd = np.arange(1, n_items, 2)
            r.set_filter(odd)
            r.set_uniform(10.0, 0.0)
            o = ro.AffineRescorer(filtered=odd, scale=10.0)
        out.append((kind, r, o))
    return out


@pytest.mark.parametrize("k", [2, 30, 64, 100, 128])
@pytest.mark.parametrize("n_items", [DENSE_ITEMS, FILTER_ITEMS])
def test_rescored_vectors_match_the_oracle(k, n_items):
    Y = catalogue(n_items, k, 10 + k)
    rng = np.random.default_rng(k)
    V = (rng.standard_normal((4, k)) * 0.3).astype(np.float32)
    with core_with(Y) as core:
        for kind, r, o in rescorers(core, n_items, rng):
            for hm in (10, 64, 100):
                idx, sc, cnt = core.recommend_vectors(V, hm, rescorer=r)
                for q in range(len(V)):
                    oidx, osc = ro.recommend(Y, V[q], hm, o)
                    check(idx[q], sc[q], cnt[q], oidx, osc)
            r.close()


def test_full_dense_path_gives_the_same_answers():
    k = 30
    Y = catalogue(FILTER_ITEMS, k, 3)
    rng = np.random.default_rng(3)
    V = (rng.standard_normal((3, k)) * 0.3).astype(np.float32)
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import myrrix_recommender_amd as pkg
Y = np.load(%r); V = np.load(%r)
core = pkg.ALSCore(Y.shape[1]); core.set_factor_rows(pkg.SIDE_Y, len(Y)); core.set_factors(pkg.SIDE_Y, Y)
r = core.rescorer(); r.set_filter(np.arange(0, len(Y), 7)); r.set_weights(np.linspace(0.5, 2.0, len(Y)), np.linspace(-1, 1, len(Y)))
idx, sc, cnt = core.recommend_vectors(V, 40, rescorer=r)
np.save(%r, idx); np.save(%r, sc)
r.close(); core.close()
"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        paths = [os.path.join(d, n) for n in ("Y.npy", "V.npy", "i_full.npy", "s_full.npy", "i_f.npy", "s_f.npy")]
        np.save(paths[0], Y)
        np.save(paths[1], V)
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        for full, (pi, ps) in ((True, paths[2:4]), (False, paths[4:6])):
            env = dict(os.environ)
            env.pop("MALS_TOPN_FULL", None)
            if full:
                env["MALS_TOPN_FULL"] = "1"
            subprocess.run([sys.executable, "-c", code % (root, paths[0], paths[1], pi, ps)], check=True, env=env, timeout=600)
        assert np.array_equal(np.load(paths[2]), np.load(paths[4]))
        assert np.array_equal(np.load(paths[3]).view(np.uint32), np.load(paths[5]).view(np.uint32))
        o = ro.AffineRescorer(filtered=np.arange(0, len(Y), 7), scale=np.linspace(0.5, 2.0, len(Y)), offset=np.linspace(-1, 1, len(Y)))
        idx, sc = np.load(paths[2]), np.load(paths[3])
        for q in range(len(V)):
            oidx, osc = ro.recommend(Y, V[q], 40, o)
            check(idx[q], sc[q], len(oidx), oidx, osc)


@pytest.mark.parametrize("n_items", [DENSE_ITEMS, FILTER_ITEMS])
def test_edge_cases(n_items):
    k = 32
    Y = catalogue(n_items, k, 8)
    rng = np.random.default_rng(8)
    V = (rng.standard_normal((2, k)) * 0.3).astype(np.float32)
    with core_with(Y) as core:
        r = core.rescorer()
        # every item filtered: an empty answer
        r.set_filter(np.arange(n_items))
        idx, sc, cnt = core.recommend_vectors(V, 20, rescorer=r)
        assert np.all(cnt == 0) and np.all(idx == -1)
        # an offset that makes a low-dot item win: tau is taken in the rescored domain
        r.set_filter(None)
        low = int(np.argmin(Y @ V[0]))
        off = np.zeros(n_items)
        off[low] = 10.0                                  # above every dot of the catalogue
        r.set_weights(None, off)
        idx, sc, cnt = core.recommend_vectors(V[:1], 20, rescorer=r)
        assert idx[0, 0] == low
        oidx, osc = ro.recommend(Y, V[0], 20, ro.AffineRescorer(offset=off))
        check(idx[0], sc[0], cnt[0], oidx, osc)
        # heavy rescored ties: offsets that dominate the dots (hundreds of items tie) -- the per-query dense fallback
        off = np.where(np.arange(n_items) % 3 == 0, 1e6, 0.0)
        r.set_weights(None, off)
        o = ro.AffineRescorer(offset=off)
        for hm in (10, 64):
            idx, sc, cnt = core.recommend_vectors(V, hm, rescorer=r)
            for q in range(len(V)):
                check(idx[q], sc[q], cnt[q], *ro.recommend(Y, V[q], hm, o))
        # scales across the filter's range, and beyond it (the dense path)
        for lo, hi in ((2.0 ** -20, 2.0 ** -18), (2.0 ** 18, 2.0 ** 20), (1e-30, 1e30)):
            sc_w = np.exp(rng.uniform(np.log(lo), np.log(hi), n_items))
            off = rng.standard_normal(n_items) * (lo + hi) / 4
            r.set_weights(sc_w, off)
            o = ro.AffineRescorer(scale=sc_w, offset=off)
            idx, sc, cnt = core.recommend_vectors(V, 30, rescorer=r)
            for q in range(len(V)):
                check(idx[q], sc[q], cnt[q], *ro.recommend(Y, V[q], 30, o))
        r.close()


def test_argument_rules():
    Y = catalogue(100, 8, 1)
    with core_with(Y) as core:
        r = core.rescorer()
        for bad in ([0.0], [-1.0], [np.inf], [np.nan]):
            with pytest.raises(MalsError):
                r.set_weights(np.array(bad * 100), None)
        with pytest.raises(MalsError):
            r.set_weights(None, np.full(100, np.nan))
        with pytest.raises(MalsError):
            r.set_uniform(0.0, 0.0)
        with pytest.raises(MalsError):
            r.set_uniform(1.0, np.inf)
        with pytest.raises(MalsError):
            r.set_filter([100])
        r.close()


def test_to_many_anonymous_and_by_user_with_a_rescorer():
    k, n_items = 24, FILTER_ITEMS
    Y = catalogue(n_items, k, 21)
    rng = np.random.default_rng(21)
    X = (rng.standard_normal((50, k)) * 0.3).astype(np.float32)
    with core_with(Y, X) as core:
        r = core.rescorer()
        filt = rng.choice(n_items, n_items // 10, replace=False)
        sc_w, off = rng.uniform(0.5, 2.0, n_items), rng.standard_normal(n_items) * 0.2
        r.set_filter(filt)
        r.set_weights(sc_w, off)
        o = ro.AffineRescorer(filtered=filt, scale=sc_w, offset=off)
        users = np.array([0, 7, 49], np.int64)
        idx, sc, cnt = core.recommend(users, 25, consider_known_items=True, rescorer=r)
        for q, u in enumerate(users):
            check(idx[q], sc[q], cnt[q], *ro.recommend(Y, X[u], 25, o))
        queries = [X[0:3], X[10:11], X[20:25]]
        excl = [[1, 2, 3], [], [int(filt[0]), 5]]
        idx, sc, cnt = core.recommend_to_many(queries, 30, exclude=excl, rescorer=r)
        for q in range(3):
            check(idx[q], sc[q], cnt[q], *ro.recommend(Y, queries[q], 30, o, known=excl[q]))
        r.close()


@pytest.mark.parametrize("n_items", [DENSE_ITEMS, FILTER_ITEMS])
def test_recommend_to_anonymous_with_a_rescorer(n_items):
    """recommendToAnonymous (SR:511-559) with a rescorer: the fold-in vector of the query's items (tests/foldin_oracle.py),
    the items themselves excluded, then the rescored top-N -- a filtered item that would have won, an offset that wins"""
    from tests import foldin_oracle as fo
    from tests.test_gpu_foldin import core_for, model
    k = 24
    X, Y, ptr, col = model(30, n_items, k, 17)
    c, (sx, sy) = core_for(X, Y, ptr, col)
    rng = np.random.default_rng(n_items)
    queries = [[1, 2, 3], [-1, 4], [-1], [7, 7, 99], [5]]
    values = [[1.0, 2.0, -1.0], [0.5, 3.0], [1.0], [1.0, 0.0, -2.0], [2.0]]
    acc = [fo.anonymous_features(Y, items, values[q], sy) for q, items in enumerate(queries)]
    excl = [sorted(j for j in items if j >= 0) for items in queries]
    plain0 = ro.recommend(Y, acc[0][0], 3, ro.AffineRescorer(), known=excl[0])[0]
    filt = np.union1d(rng.choice(n_items, n_items // 10, replace=False), [plain0[0]])   # query 0's plain winner filtered
    scale = rng.uniform(0.5, 2.0, n_items)
    offset = rng.standard_normal(n_items) * 0.1
    s3, _ = ro.sums(Y, acc[3][0])
    low = int(np.argmin(np.where(np.isin(np.arange(n_items), np.union1d(filt, excl[3])), np.inf, s3)))
    offset[low] = 4.0 * float(np.max(np.abs(s3)) + 1.0)      # query 3's worst item wins through its offset
    o = ro.AffineRescorer(filtered=filt, scale=scale, offset=offset)
    with c:
        r = c.rescorer()
        r.set_filter(filt)
        r.set_weights(scale, offset)
        idx, sc, cnt, st = c.recommend_to_anonymous(queries, 8, values, rescorer=r)
        assert st.tolist() == [0, 0, 2, 0, 0] and cnt[2] == 0
        for q in range(len(queries)):
            if st[q]:
                continue
            assert acc[q][1]
            check(idx[q], sc[q], cnt[q], *ro.recommend(Y, acc[q][0], 8, o, known=excl[q]))
        assert plain0[0] not in idx[0].tolist() and idx[3, 0] == low
        r.close()


FILTER_RUN = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import myrrix_recommender_amd as pkg
rng = np.random.default_rng(5)
Y = (rng.standard_normal((%d, 32)) * 0.3).astype(np.float32)
V = (rng.standard_normal((8, 32)) * 0.3).astype(np.float32)
core = pkg.ALSCore(32); core.set_factor_rows(pkg.SIDE_Y, len(Y)); core.set_factors(pkg.SIDE_Y, Y)
r = core.rescorer(); r.set_filter(rng.choice(len(Y), len(Y) // 10, replace=False))
if %r:   # offsets that dominate the dots: thousands of rescored ties, the per-query dense fallback
    r.set_weights(None, np.where(np.arange(len(Y)) %% 3 == 0, 1e6, 0.0))
else:
    r.set_weights(rng.uniform(0.5, 2.0, len(Y)), rng.standard_normal(len(Y)) * 0.1)
before = core.recommend_front_stats()
for q in range(8):
    core.recommend_vectors(V[q:q + 1], 20, rescorer=r)
print("passes", core.recommend_front_stats()["passes"] - before["passes"])
r.close(); core.close()
"""


def test_the_rescored_filter_path_answers_without_falling_back():
    """the parity tests pass on the dense path too: here the filter is seen to answer (coalesced passes, no query sent to
    the dense path under MALS_TOPN_DEBUG), and the same check sees the fallback when rescored ties force it"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("MALS_TOPN_FULL", None)
    env["MALS_TOPN_DEBUG"] = "1"
    out = {}
    for ties in (False, True):
        p = subprocess.run([sys.executable, "-c", FILTER_RUN % (root, FILTER_ITEMS, ties)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        out[ties] = p
    assert "passes 8" in out[False].stdout
    assert "to the dense path" not in out[False].stderr, out[False].stderr
    assert "passes 8" in out[True].stdout and "to the dense path" in out[True].stderr


def test_a_rescorer_changed_between_calls_and_rows_grown_after_it_was_set():
    k, n_items = 16, FILTER_ITEMS
    Y = catalogue(n_items, k, 31)
    rng = np.random.default_rng(31)
    V = (rng.standard_normal((2, k)) * 0.3).astype(np.float32)
    with core_with(Y) as core:
        r = core.rescorer()
        r.set_uniform(2.0, 0.5)
        check(*[a[0] for a in core.recommend_vectors(V[:1], 20, rescorer=r)], *ro.recommend(Y, V[0], 20, ro.AffineRescorer(scale=2.0, offset=0.5)))
        sc_w = rng.uniform(0.5, 2.0, n_items)
        r.set_weights(sc_w, None)
        check(*[a[0] for a in core.recommend_vectors(V[:1], 20, rescorer=r)], *ro.recommend(Y, V[0], 20, ro.AffineRescorer(scale=sc_w)))
        # rows grown after the rescorer was set: unscaled, unfiltered
        core.grow_factor_rows(pkg.SIDE_Y, n_items + 500)
        Y2 = core.get_factors(pkg.SIDE_Y)
        assert len(Y2) == n_items + 500
        check(*[a[0] for a in core.recommend_vectors(V[:1], 20, rescorer=r)], *ro.recommend(Y2, V[0], 20, ro.AffineRescorer(scale=sc_w)))
        r.close()


def test_32_threads_three_rescorers_and_none_and_one_overflowing_call():
    k, n_items = 32, FILTER_ITEMS
    Y = catalogue(n_items, k, 41)
    rng = np.random.default_rng(41)
    V = (rng.standard_normal((32, 4, k)) * 0.3).astype(np.float32)
    with core_with(Y) as core:
        rs = []
        for kind, r, o in rescorers(core, n_items, rng)[:2]:
            rs.append((r, o))
        r = core.rescorer()
        r.set_uniform(2.0 ** 20, 1.0)                    # the top of the filter's range
        rs.append((r, ro.AffineRescorer(scale=2.0 ** 20, offset=1.0)))
        rs.append((None, ro.AffineRescorer()))
        big = (V[31, 0] * 1e33).astype(np.float32)       # thread 31 (rescorer 3 * 2^20): results overflow fp32, only its calls fail
        expect = {}
        for t in range(32):
            r, o = rs[2 if t == 31 else t % 4]
            if t == 31:
                with pytest.raises(ro.BadRecommendationValue):
                    ro.recommend(Y, big, 10, o)
                continue
            expect[t] = [ro.recommend(Y, V[t, j], 10, o) for j in range(4)]
        before = core.recommend_front_stats()
        errors, results = {}, {}
        barrier = threading.Barrier(32)

        def worker(t):
            r, _ = rs[2 if t == 31 else t % 4]
            try:
                barrier.wait()
                for rep in range(3):
                    for j in range(4):
                        q = big[None] if t == 31 else V[t, j][None]
                        results[(t, rep, j)] = core.recommend_vectors(q, 10, rescorer=r)
            except Exception as e:   # noqa: BLE001
                errors[t] = e

        th = [threading.Thread(target=worker, args=(t,)) for t in range(32)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert set(errors) == {31}, errors
        assert isinstance(errors[31], MalsError) and "Bad recommendation value" in str(errors[31])
        for (t, rep, j), (idx, sc, cnt) in results.items():
            check(idx[0], sc[0], cnt[0], *expect[t][j])
        st = core.recommend_front_stats()
        assert st["passes"] - before["passes"] < st["calls"] - before["calls"]   # calls were folded into passes
        for r, _ in rs:
            if r is not None:
                r.close()
