"""The candidate filter on the device (mals_lsh_*, include/myrrix_als.h; csrc/lsh_kernels.h and the LSH instantiations of
csrc/topn_kernels.h) against the restatement of LocationSensitiveHash.java in tests/lsh_oracle.py: signatures bit for bit,
and every recommend call equal to the unfiltered oracle with the query's non-candidates added to its exclusions."""
import threading

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from oracle import topn_oracle as to
from tests import lsh_oracle as lo
from tests import rescorer_oracle as ro
from tests.test_gpu_topn import big_core, same_ranking

pytestmark = pytest.mark.gpu


def random_vectors(H, k, seed):
    return np.random.default_rng(seed).integers(0, 2, (H, k)).astype(bool)


def core_with(Y, X=None):
    core = pkg.ALSCore(Y.shape[1])
    core.set_factor_rows(pkg.SIDE_Y, len(Y))
    core.set_factors(pkg.SIDE_Y, Y)
    if X is not None:
        core.set_factor_rows(pkg.SIDE_X, len(X))
        core.set_factors(pkg.SIDE_X, X)
    return core


def excluded(isig, qsig, mb, known=None, n_items=None):
    """the exclusions of the unfiltered oracle: the query's non-candidates (and its known items)"""
    non = lo.non_candidates(isig, qsig, mb, n_items)
    return non if known is None or not len(known) else np.union1d(non, np.asarray(known, np.int64))


def check(idx, sc, cnt, oidx, osc):
    assert cnt == len(oidx), (cnt, len(oidx))
    same_ranking(idx, sc, oidx, osc)
    assert np.all(np.isneginf(sc[len(oidx):]))


# ---- 1. signatures, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,H,rows", [(1, 1, 70), (30, 20, 1000), (64, 64, 4099), (128, 33, 257), (100, 20, 3000)])
def test_signatures_and_mean(k, H, rows):
    rng = np.random.default_rng(1000 * k + H)
    Y = (rng.standard_normal((rows, k)) / np.sqrt(k)).astype(np.float32)
    rv = random_vectors(H, k, rows)
    with core_with(Y) as core:
        assert core.lsh_info()["num_hashes"] == 0
        core.lsh_build(num_hashes=H, max_bits_differing=H // 2, random_vectors=rv)
        info = core.lsh_info()
        assert (info["num_hashes"], info["max_bits_differing"], info["rows_signed"], info["rows_now"]) == (H, H // 2, rows, rows)
        mean, sig = core.lsh_get()
        want = lo.signatures(Y, rv, mean)                   # with the mean the device returned
        assert np.array_equal(sig, want), np.flatnonzero(sig != want)[:10]
        if H == 64:
            assert np.any(sig >> np.uint64(63))             # the top bit is in use
        assert np.all(sig < np.uint64(2) ** np.uint64(H)) if H < 64 else True
        m2, part = core.lsh_get(5, 11)
        assert np.array_equal(part, sig[5:16]) and np.array_equal(m2.view(np.uint64), mean.view(np.uint64))
        # the mean: n fp64 additions in some order and one division
        Y64 = Y.astype(np.float64)
        ref = Y64.sum(axis=0) / rows
        bound = (rows + 1) * 2.0 ** -53 * np.abs(Y64).sum(axis=0) / rows
        err = np.abs(mean - ref)
        print("mean: max err %.3e, bound there %.3e" % (err.max(), bound[np.argmax(err)]))
        assert np.all(err <= bound)
        Q = (rng.standard_normal((37, k)) / np.sqrt(k)).astype(np.float32)
        assert np.array_equal(core.lsh_signatures(Q), lo.signatures(Q, rv, mean))
        # the same build again: the same bits (a fixed order of the sum)
        core.lsh_build(num_hashes=H, max_bits_differing=H // 2, random_vectors=rv)
        mean_b, sig_b = core.lsh_get()
        assert np.array_equal(mean_b.view(np.uint64), mean.view(np.uint64)) and np.array_equal(sig_b, sig)


# ---- 2. exact zeros ---------------------------------------------------------------------------------------------------------
def test_totals_that_are_exactly_zero_give_bit_zero():
    k, H, rows = 8, 20, 500
    rng = np.random.default_rng(2)
    Y = rng.integers(-3, 4, (rows, k)).astype(np.float32)
    mean = rng.integers(-1, 2, k).astype(np.float64)
    rv = random_vectors(H, k, 22)
    tot = lo.totals(Y, rv, mean)
    zeros = tot == 0.0
    assert zeros.sum() > 20                                  # integer totals: many are exactly 0
    with core_with(Y) as core:
        core.lsh_build(num_hashes=H, max_bits_differing=3, random_vectors=rv, mean=mean)
        got_mean, sig = core.lsh_get()
        assert np.array_equal(got_mean.view(np.uint64), mean.view(np.uint64))
        assert np.array_equal(sig, lo.signatures(Y, rv, mean))
        for i, h in zip(*np.nonzero(zeros)):
            assert (int(sig[i]) >> (H - 1 - h)) & 1 == 0
        assert np.array_equal(core.lsh_signatures(Y[:50]), sig[:50])


# ---- 3. the dense path ------------------------------------------------------------------------------------------------------
def test_dense_path_every_kind_of_call():
    from tests import foldin_oracle as fo
    from tests.test_gpu_foldin import core_for, model
    k, n_items, H, N = 30, 3000, 20, 10
    X, Y, ptr, col = model(40, n_items, k, 33, nnz_per_user=20)
    rv = random_vectors(H, k, 3)
    mb = lo.max_bits_differing(0.3, H)
    core, (sx, sy) = core_for(X, Y, ptr, col)
    with core:
        core.lsh_build(num_hashes=H, sample_ratio=0.3, random_vectors=rv)
        assert core.lsh_info()["max_bits_differing"] == mb == 8
        mean, isig = core.lsh_get()
        assert np.array_equal(isig, lo.signatures(Y, rv, mean))
        qsig = lambda v: lo.signatures(np.atleast_2d(v), rv, mean)   # noqa: E731
        frac = [lo.candidates(isig, qsig(X[u]), mb).mean() for u in range(8)]
        assert 0.1 < np.mean(frac) < 0.5, frac
        # recommend, with and without the known items
        users = np.array([0, 7, 21, 39], np.int64)
        for consider in (False, True):
            idx, sc, cnt = core.recommend(users, N, consider_known_items=consider)
            for q, u in enumerate(users):
                known = None if consider else col[ptr[u]:ptr[u + 1]]
                check(idx[q], sc[q], cnt[q], *to.recommend(Y, X[u], N, excluded(isig, qsig(X[u]), mb, known)))
        # recommend_vectors with exclusions
        V = X[10:13] * np.float32(1.5)
        excl = [[1, 2, 3], [], list(range(100, 160))]
        idx, sc, cnt = core.recommend_vectors(V, N, exclude=excl)
        for q in range(3):
            check(idx[q], sc[q], cnt[q], *to.recommend(Y, V[q], N, excluded(isig, qsig(V[q]), mb, excl[q])))
        # recommend_to_many, 1-3 vectors per query; one query returns an item that only its SECOND vector makes a candidate
        found = None
        for a in range(0, 38):
            pair = X[a:a + 2]
            s = qsig(pair)
            oidx, _ = to.recommend(Y, pair, N, excluded(isig, s, mb))
            first, second = lo.candidates(isig, s[:1], mb), lo.candidates(isig, s[1:], mb)
            through_second = [i for i in oidx if not first[i] and second[i]]
            if through_second:
                found = (a, through_second)
                break
        assert found is not None
        queries = [X[found[0]:found[0] + 2], X[5:6], X[20:23]]
        idx, sc, cnt = core.recommend_to_many(queries, N)
        for q in range(3):
            check(idx[q], sc[q], cnt[q], *to.recommend(Y, queries[q], N, excluded(isig, qsig(queries[q]), mb)))
        assert set(found[1]) <= set(idx[0].tolist())
        # recommend_to_anonymous: the folded-in vector is signed on the device
        anon = [[1, 2, 3], [7], [50, 60]]
        values = [[1.0, 2.0, -1.0], [2.0], [1.0, 1.0]]
        acc = [fo.anonymous_features(Y, items, values[q], sy) for q, items in enumerate(anon)]
        idx, sc, cnt, st = core.recommend_to_anonymous(anon, N, values)
        assert st.tolist() == [0, 0, 0]
        for q in range(3):
            check(idx[q], sc[q], cnt[q], *to.recommend(Y, acc[q][0], N, excluded(isig, qsig(acc[q][0]), mb, anon[q])))
        # one rescored twin: a filter set and weights
        rng = np.random.default_rng(9)
        filt = rng.choice(n_items, n_items // 10, replace=False)
        scale, offset = rng.uniform(0.5, 2.0, n_items), rng.standard_normal(n_items) * 0.05
        with core.rescorer() as r:
            r.set_filter(filt)
            r.set_weights(scale, offset)
            o = ro.AffineRescorer(filtered=filt, scale=scale, offset=offset)
            idx, sc, cnt = core.recommend(users, N, consider_known_items=True, rescorer=r)
            for q, u in enumerate(users):
                check(idx[q], sc[q], cnt[q], *ro.recommend(Y, X[u], N, o, known=excluded(isig, qsig(X[u]), mb)))
        info = core.lsh_info()
        assert info["filter_queries"] == 0 and info["dense_queries"] > 0


# ---- 4. the filter path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n_items,N,ratio,H", [(64, 140_000, 10, 0.1, 20), (16, 140_000, 10, 0.1, 20), (128, 131_072, 5, 0.3, 33),
                                                 (30, 140_000, 50, 0.3, 20)])
def test_filter_path(k, n_items, N, ratio, H, monkeypatch):
    monkeypatch.delenv("MALS_TOPN_FULL", raising=False)
    n_users = 250
    core, X, Y, rp, col = big_core(k, n_items, n_users, 60, 40 + k)
    rv = random_vectors(H, k, 4 + k)
    mb = lo.max_bits_differing(ratio, H)
    with core:
        core.lsh_build(num_hashes=H, sample_ratio=ratio, random_vectors=rv)
        mean, isig = core.lsh_get()
        rows = np.random.default_rng(k).choice(n_items, 1500, replace=False)
        assert np.array_equal(isig[rows], lo.signatures(Y[rows], rv, mean))
        rng = np.random.default_rng(7)
        checked = [0, 15, 16, n_users - 1] + rng.choice(np.arange(17, n_users - 1), 4, replace=False).tolist()
        expect, changed = {}, 0
        for q in checked:
            known = col[rp[q]:rp[q + 1]]
            qs = lo.signatures(X[q:q + 1], rv, mean)
            cand = lo.candidates(isig, qs, mb)
            assert cand.sum() - len(known) >= N
            expect[q] = to.recommend(Y, X[q], N, excluded(isig, qs, mb, known))
            plain = to.recommend(Y, X[q], N, known)
            changed += not np.array_equal(plain[0], expect[q][0])
            print("query %d: candidate fraction %.3f, filtered top-N differs: %s" % (q, cand.mean(), not np.array_equal(plain[0], expect[q][0])))
        assert 2 * changed >= len(checked)           # from the oracles alone: a filter that did nothing would fail below
        users = np.arange(n_users, dtype=np.int64)
        before = core.lsh_info()
        idx, sc, cnt = core.recommend(users, N)
        one = {q: core.recommend(np.array([q], np.int64), N) for q in (0, 16, n_users - 1)}
        after = core.lsh_info()
        print("filter / dense queries: %d / %d" % (after["filter_queries"] - before["filter_queries"], after["dense_queries"] - before["dense_queries"]))
        for q in checked:
            check(idx[q], sc[q], cnt[q], *expect[q])
        for q, (i1, s1, c1) in one.items():
            assert np.array_equal(i1[0], idx[q]) and np.array_equal(s1[0].view(np.uint32), sc[q].view(np.uint32)) and c1[0] == cnt[q]
        # the sample counts candidates only: no query of these calls needed the dense path
        assert after["dense_queries"] - before["dense_queries"] == 0
        assert after["filter_queries"] - before["filter_queries"] == n_users + len(one)
        monkeypatch.setenv("MALS_TOPN_FULL", "1")
        full = core.recommend(users, N)
        assert np.array_equal(full[0], idx) and np.array_equal(full[1].view(np.uint32), sc.view(np.uint32)) and np.array_equal(full[2], cnt)
        assert core.lsh_info()["dense_queries"] - after["dense_queries"] == n_users


def test_filter_path_rescored_to_many_and_anonymous():
    """The filter path's other instantiations at 140 000 items: a rescorer with the candidate filter (the RS + LSH streaming
    kernels), queries of several vectors (not tested in the stream: their buckets are dropped before the threshold, their
    candidates struck after the exact scores) and an anonymous user's folded-in vector -- none of them by the dense path."""
    from tests import foldin_oracle as fo
    from tests.test_gpu_foldin import core_for, model
    k, n_items, H, N = 24, 140_000, 20, 10
    X, Y, ptr, col = model(40, n_items, k, 44)
    rv = random_vectors(H, k, 44)
    core, (sx, sy) = core_for(X, Y, ptr, col)
    with core:
        core.lsh_build(num_hashes=H, sample_ratio=0.3, random_vectors=rv)
        mb = core.lsh_info()["max_bits_differing"]
        mean, isig = core.lsh_get()
        qsig = lambda v: lo.signatures(np.atleast_2d(v), rv, mean)   # noqa: E731
        before = core.lsh_info()
        # rescored, by user
        rng = np.random.default_rng(45)
        filt = rng.choice(n_items, n_items // 10, replace=False)
        scale, offset = rng.uniform(0.5, 2.0, n_items), rng.standard_normal(n_items) * 0.05
        users = np.array([0, 15, 16, 39], np.int64)
        with core.rescorer() as r:
            r.set_filter(filt)
            r.set_weights(scale, offset)
            o = ro.AffineRescorer(filtered=filt, scale=scale, offset=offset)
            idx, sc, cnt = core.recommend(users, N, consider_known_items=True, rescorer=r)
            changed = 0
            for q, u in enumerate(users):
                want = ro.recommend(Y, X[u], N, o, known=excluded(isig, qsig(X[u]), mb))
                check(idx[q], sc[q], cnt[q], *want)
                changed += not np.array_equal(want[0], ro.recommend(Y, X[u], N, o)[0])
            assert changed >= 2
            # ... and a rescored query of two vectors
            pair = [X[3:5]]
            idx, sc, cnt = core.recommend_to_many(pair, N, rescorer=r)
            check(idx[0], sc[0], cnt[0], *ro.recommend(Y, pair[0], N, o, known=excluded(isig, qsig(pair[0]), mb)))
        # queries of 2, 1 and 3 vectors with exclusions
        queries = [X[0:2], X[15:16], X[16:19]]
        excl = [[5, 6], [], [int(i) for i in range(1000, 1040)]]
        idx, sc, cnt = core.recommend_to_many(queries, N, exclude=excl)
        through_other = 0
        for q in range(3):
            s = qsig(queries[q])
            want = to.recommend(Y, queries[q], N, excluded(isig, s, mb, excl[q]))
            check(idx[q], sc[q], cnt[q], *want)
            first = lo.candidates(isig, s[:1], mb)
            through_other += sum(1 for i in want[0] if not first[i])
        assert through_other >= 1              # an item returned that only a later vector makes a candidate
        # an anonymous user
        anon = [[1, 2, 3], [70_000]]
        values = [[1.0, 2.0, -1.0], [2.0]]
        acc = [fo.anonymous_features(Y, items, values[q], sy) for q, items in enumerate(anon)]
        idx, sc, cnt, st = core.recommend_to_anonymous(anon, N, values)
        assert st.tolist() == [0, 0]
        for q in range(2):
            check(idx[q], sc[q], cnt[q], *to.recommend(Y, acc[q][0], N, excluded(isig, qsig(acc[q][0]), mb, anon[q])))
        after = core.lsh_info()
        print("filter / dense queries: %d / %d" % (after["filter_queries"] - before["filter_queries"], after["dense_queries"] - before["dense_queries"]))
        assert after["dense_queries"] - before["dense_queries"] == 0
        assert after["filter_queries"] - before["filter_queries"] == 4 + 1 + 3 + 2


def test_random_vectors_drawn_like_the_reference():
    """random_vectors=None: drawn hash-major from MersenneTwister(seed).nextBoolean(), as LSH:113-119 draws them."""
    from myrrix_recommender_amd import random_mt
    k, H, rows = 12, 20, 300
    rng = np.random.default_rng(12)
    Y = (rng.standard_normal((rows, k)) / np.sqrt(k)).astype(np.float32)
    gen = random_mt.MersenneTwister(42)
    want = np.array([[gen.nextBoolean() for _ in range(k)] for _ in range(H)], bool)
    with core_with(Y) as core:
        rv = core.lsh_build(num_hashes=H, sample_ratio=0.3, seed=42)
        assert rv.shape == (H, k) and np.array_equal(rv, want)
        assert 0.3 < rv.mean() < 0.7
        mean, sig = core.lsh_get()
        assert np.array_equal(sig, lo.signatures(Y, want, mean))
        assert core.lsh_info()["max_bits_differing"] == lo.max_bits_differing(0.3, H)


# ---- 5. the edges of maxBitsDiffering -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [3000, 140_000])
def test_edges_of_max_bits_differing(n_items):
    k, H, N = 16, 20, 8
    rng = np.random.default_rng(n_items)
    Y = (rng.standard_normal((n_items, k)) / np.sqrt(k)).astype(np.float32)
    V = (rng.standard_normal((5, k)) / np.sqrt(k)).astype(np.float32)
    rv = random_vectors(H, k, 5)
    with core_with(Y) as core:
        plain = core.recommend_vectors(V, N)
        # -1: no bucket matches, nothing is a candidate
        core.lsh_build(num_hashes=H, max_bits_differing=-1, random_vectors=rv)
        assert core.lsh_info()["max_bits_differing"] == -1
        idx, sc, cnt = core.recommend_vectors(V, N)
        assert np.all(cnt == 0) and np.all(idx == -1) and np.all(np.isneginf(sc))
        # ... but new items are: the five rows grown after the build, minus the excluded one, in score order
        core.grow_factor_rows(pkg.SIDE_Y, n_items + 5)
        new = (rng.standard_normal((5, k)) / np.sqrt(k)).astype(np.float32)
        core.set_factors(pkg.SIDE_Y, new, row_begin=n_items)
        Y2 = np.concatenate([Y, new])
        info = core.lsh_info()
        assert info["rows_signed"] == n_items and info["rows_now"] == n_items + 5
        excl = [[n_items + 1], [], [0, 1], [n_items, n_items + 4], []]
        idx, sc, cnt = core.recommend_vectors(V, N, exclude=excl)
        for q in range(5):
            old = np.arange(n_items)
            oidx, osc = to.recommend(Y2, V[q], N, np.union1d(old, np.asarray(excl[q], np.int64)))
            assert len(oidx) == 5 - sum(e >= n_items for e in excl[q])
            check(idx[q], sc[q], cnt[q], oidx, osc)
    with core_with(Y) as core:
        # H: every bucket matches -- the handle without a filter, bit for bit; and after a clear
        core.lsh_build(num_hashes=H, max_bits_differing=H, random_vectors=rv)
        got = core.recommend_vectors(V, N)
        assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                   for a, b in zip(got, plain))
        core.lsh_build(num_hashes=H, sample_ratio=0.1, random_vectors=rv)
        narrowed = core.recommend_vectors(V, N)
        assert not np.array_equal(narrowed[0], plain[0])
        core.lsh_clear()
        assert core.lsh_info()["num_hashes"] == 0
        got = core.recommend_vectors(V, N)
        assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                   for a, b in zip(got, plain))
        # declaring Y's rows anew drops the filter with the rows it signed
        core.lsh_build(num_hashes=H, sample_ratio=0.1, random_vectors=rv)
        core.set_factor_rows(pkg.SIDE_Y, n_items)
        assert core.lsh_info()["num_hashes"] == 0


# ---- 6. signatures are a snapshot -------------------------------------------------------------------------------------------
def test_signatures_are_a_snapshot_of_the_build():
    from tests.test_gpu_foldin import core_for, model
    k, n_items, H, N = 24, 3000, 20, 10
    X, Y, ptr, col = model(30, n_items, k, 61)
    rv = random_vectors(H, k, 6)
    core, _ = core_for(X, Y, ptr, col)
    with core:
        core.lsh_build(num_hashes=H, sample_ratio=0.3, random_vectors=rv)
        mb = core.lsh_info()["max_bits_differing"]
        mean, isig = core.lsh_get()
        user, item = 3, 1234
        core.set_preferences([user], [item], [5.0])
        X2, Y2 = core.get_factors(pkg.SIDE_X), core.get_factors(pkg.SIDE_Y)
        assert not np.array_equal(Y2[item], Y[item])                        # the item's vector moved ...
        mean2, isig2 = core.lsh_get()
        assert np.array_equal(isig2, isig) and np.array_equal(mean2, mean)  # ... its signature did not
        moved_sig = lo.signatures(Y2[item:item + 1], rv, mean)[0]
        print("signature of the moved vector %x, kept %x" % (int(moved_sig), int(isig[item])))
        idx, sc, cnt = core.recommend(np.array([user, 9], np.int64), N, consider_known_items=True)
        for q, u in enumerate((user, 9)):
            qs = lo.signatures(X2[u:u + 1], rv, mean)                       # the query is signed as it is NOW
            check(idx[q], sc[q], cnt[q], *to.recommend(Y2, X2[u], N, excluded(isig, qs, mb)))


# ---- 7. calls the filter does not touch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [3000, 140_000])
def test_similarity_calls_never_consult_the_filter(n_items):
    k, H = 16, 20
    core, X, Y, rp, col = big_core(k, n_items, 20, 40, 77)
    rv = random_vectors(H, k, 7)
    with core:
        items = [[3], [10, 11], [n_items - 1]]
        users, because = np.array([0, 5, 19], np.int64), np.array([17, 200, 2999], np.int64)
        a = core.most_similar_items(items, 12)
        b = core.recommended_because(users, because, 6)
        c = core.similarity_to_item(5, np.arange(50, dtype=np.int64))
        core.lsh_build(num_hashes=H, sample_ratio=0.05, random_vectors=rv)
        a2 = core.most_similar_items(items, 12)
        b2 = core.recommended_because(users, because, 6)
        c2 = core.similarity_to_item(5, np.arange(50, dtype=np.int64))
        for x, y in list(zip(a, a2)) + list(zip(b, b2)) + [(c, c2)]:
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
        info = core.lsh_info()
        assert info["filter_queries"] == 0 and info["dense_queries"] == 0


# ---- 8. the serving front -----------------------------------------------------------------------------------------------------
def test_front_with_the_filter_built():
    k, n_items, H, N, n_users = 16, 140_000, 20, 10, 250
    core, X, Y, rp, col = big_core(k, n_items, n_users, 40, 88)
    rv = random_vectors(H, k, 8)
    with core:
        users = np.arange(n_users, dtype=np.int64)
        plain = core.recommend(users, N)
        core.lsh_build(num_hashes=H, sample_ratio=0.3, random_vectors=rv)
        alone = {u: core.recommend(np.array([u], np.int64), N) for u in range(n_users)}
        errors, results = [], {}
        barrier = threading.Barrier(8)

        def worker(t):
            try:
                barrier.wait()
                for i in range(50):
                    u = (t * 50 + 7 * i) % n_users
                    results[(t, i)] = (u, core.recommend(np.array([u], np.int64), N))
            except Exception as e:   # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errors, errors
        assert len(results) == 400
        for u, (idx, sc, cnt) in results.values():
            assert np.array_equal(idx, alone[u][0]) and np.array_equal(sc.view(np.uint32), alone[u][1].view(np.uint32)) and np.array_equal(cnt, alone[u][2])
        # a build between two batches: the first batch saw the old filter (every bucket matches), the second the new one
        core.lsh_build(num_hashes=H, max_bits_differing=H, random_vectors=rv)
        first = core.recommend(users, N)
        core.lsh_build(num_hashes=H, sample_ratio=0.1, random_vectors=rv)
        second = core.recommend(users, N)
        assert np.array_equal(first[0], plain[0]) and np.array_equal(first[1].view(np.uint32), plain[1].view(np.uint32))
        mean, isig = core.lsh_get()
        mb = core.lsh_info()["max_bits_differing"]
        differ = 0
        for q in (0, 100, n_users - 1):
            qs = lo.signatures(X[q:q + 1], rv, mean)
            check(second[0][q], second[1][q], second[2][q], *to.recommend(Y, X[q], N, excluded(isig, qs, mb, col[rp[q]:rp[q + 1]])))
            differ += not np.array_equal(second[0][q], first[0][q])
        assert differ >= 1



def test_a_build_is_ordered_against_the_calls_of_other_threads():
    """mals_lsh_build is an exclusive ticket of the front: while request threads keep calling, every answer is the old
    filter's or the new one's, never a mixture; a thread that has seen the new filter never sees the old one again; and a
    call that starts after the build has returned sees the new one."""
    k, n_items, H, N, n_users = 16, 140_000, 20, 10, 40
    core, X, Y, rp, col = big_core(k, n_items, n_users, 40, 99)
    rv = random_vectors(H, k, 9)
    with core:
        def alone():
            return {u: core.recommend(np.array([u], np.int64), N) for u in range(n_users)}

        def same(a, b):
            return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])

        core.lsh_build(num_hashes=H, sample_ratio=0.1, random_vectors=rv)
        new = alone()
        core.lsh_build(num_hashes=H, sample_ratio=0.3, random_vectors=rv)
        old = alone()
        assert sum(not same(old[u], new[u]) for u in range(n_users)) > n_users // 2
        built = threading.Event()
        barrier = threading.Barrier(9)
        errors, logs = [], {}

        def worker(t):
            try:
                log = logs.setdefault(t, [])
                barrier.wait()
                i = after = 0
                while after < 10 and i < 5000:
                    u = (7 * t + i) % n_users
                    started_after = built.is_set()
                    log.append((u, started_after, core.recommend(np.array([u], np.int64), N)))
                    after += started_after
                    i += 1
            except Exception as e:   # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
        for x in th:
            x.start()
        barrier.wait()
        for u in range(5):
            core.recommend(np.array([u], np.int64), N)       # the threads are calling by now
        core.lsh_build(num_hashes=H, sample_ratio=0.1, random_vectors=rv)
        built.set()
        for x in th:
            x.join()
        assert not errors, errors
        for t, log in logs.items():
            seen_new = False
            assert sum(1 for _, started_after, _ in log if started_after) >= 10
            for u, started_after, got in log:
                is_old, is_new = same(got, old[u]), same(got, new[u])
                assert is_old or is_new, (t, u)
                if started_after or seen_new:
                    assert is_new, (t, u)
                if is_new and not is_old:
                    seen_new = True
