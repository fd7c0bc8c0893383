"""Item-to-item similarity on the device (mals_most_similar_items, mals_similarity_to_item, mals_recommended_because)
against tests/similarity_oracle.py: indices and score bits identical, nothing tolerated."""
import os
import threading

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib, synth
from oracle import topn_oracle as to
from tests import similarity_oracle as so

pytestmark = pytest.mark.gpu


def same_ranking(idx, sc, cnt, oidx, osc):
    n = len(oidx)
    assert cnt == n, (cnt, n)
    assert np.all(idx[n:] == -1) and np.all(sc[n:] == -np.inf)
    assert np.array_equal(idx[:n], oidx), (idx[:n], oidx)
    assert np.array_equal(sc[:n].view(np.uint32), np.asarray(osc, np.float32).view(np.uint32)), (sc[:n], osc)


def y_core(Y):
    k = Y.shape[1]
    core = pkg.ALSCore(k)
    core.set_factor_rows(pkg.SIDE_Y, len(Y))
    core.set_factors(pkg.SIDE_Y, Y)
    return core


def hard_Y(n_items, k, seed):
    """random rows, 5 % zero rows, one NaN row, scaled copies of one row (exact ties) and near-copies (near-ties)"""
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((n_items, k)).astype(np.float32)
    Y[rng.choice(n_items, n_items // 20, replace=False)] = 0.0
    Y[7] = np.nan
    base = Y[11].copy() if np.any(Y[11]) else np.ones(k, np.float32)
    Y[11] = base
    for j, s in enumerate((2.0, 0.5, 4.0, 8.0)):
        Y[100 + 37 * j] = base * np.float32(s)                     # cosine exactly the same as 11's
    Y[300] = base
    Y[300, 0] = np.nextafter(base[0], np.float32(np.inf))         # a near-tie
    return Y


def check_queries(core, Y, queries, how_many, tags=None):
    idx, sc, cnt = core.most_similar_items(queries, how_many)
    Yn = so.norms(Y)
    for q, items in enumerate(queries):
        oidx, osc = so.most_similar(Y, items, how_many, tags=tags, Ynorm=Yn)
        same_ranking(idx[q], sc[q], cnt[q], oidx, osc)
        got = set(idx[q, :cnt[q]].tolist())
        assert not got & set(np.atleast_1d(items).tolist())
        if tags is not None:
            assert not got & set(tags)
    return idx, sc, cnt


@pytest.mark.parametrize("k", [2, 10, 30, 64, 100, 128])
def test_most_similar_dense_path(k):
    Y = hard_Y(1000, k, 10 + k)
    Y[3] = 0.0                                                      # a zero query item: its query is answered empty
    tags = [5, 6, 12, 400]
    with y_core(Y) as core:
        core.set_tag_items(tags)
        for how_many in (1, 10, 100):
            check_queries(core, Y, [11, 0, 3, 7, 999], how_many, tags)
        check_queries(core, Y, [[11, 20], [20, 20, 31], [3, 11], [1, 2, 3, 4, 9]], 64, tags)
        _, _, cnt = core.most_similar_items([3, 7], 10)
        assert cnt.tolist() == [0, 0]


@pytest.mark.parametrize("k", [10, 64, 100])
def test_most_similar_filter_path_matches_dense(k):
    n_items = 150_000
    Y = hard_Y(n_items, k, 20 + k)
    Y[3] = 0.0
    tags = [12, 13, 137, 5000]
    rng = np.random.default_rng(k)
    batch = [int(i) for i in rng.choice(n_items, 300 if k == 64 else 40, replace=False)] + [11, 3, 7]   # > one pass at k = 64
    multi = [[11, 11, 500], [1000, 2000], [11, 100, 3]]
    with y_core(Y) as core:
        core.set_tag_items(tags)
        res = {}
        for how_many in ((1, 10, 64, 100) if k == 64 else (10,)):
            res[how_many] = core.most_similar_items(batch, how_many)
        res["multi"] = core.most_similar_items(multi, 10)
        Yn = so.norms(Y)
        for how_many in res:
            queries = multi if how_many == "multi" else batch
            hm = 10 if how_many == "multi" else how_many
            idx, sc, cnt = res[how_many]
            for q in list(range(0, len(queries), 23)) + [len(queries) - 3, len(queries) - 2, len(queries) - 1]:
                oidx, osc = so.most_similar(Y, queries[q], hm, tags=tags, Ynorm=Yn)
                same_ranking(idx[q], sc[q], cnt[q], oidx, osc)
        assert res[10][2][-2] == 0 and res[10][2][-1] == 0          # the zero and the NaN query items
        os.environ["MALS_TOPN_FULL"] = "1"
        try:
            for how_many in ((10, 64) if k == 64 else (10,)):
                idx, sc, cnt = core.most_similar_items(batch, how_many)
                assert np.array_equal(idx, res[how_many][0]) and np.array_equal(cnt, res[how_many][2])
                assert np.array_equal(sc.view(np.uint32), res[how_many][1].view(np.uint32))
        finally:
            del os.environ["MALS_TOPN_FULL"]


@pytest.fixture(scope="module")
def model():
    """150 000 items, 3000 users, two half-iterations: factors, R and a handle"""
    k, n_users, n_items = 32, 3000, 150_000
    r_csr, c_csr, Y0 = synth.numpy_problem(n_users, n_items, 200_000, k, seed=77)
    core = pkg.ALSCore(k)
    core.set_factor_rows(pkg.SIDE_X, n_users)
    core.set_factor_rows(pkg.SIDE_Y, n_items)
    core.set_matrix(pkg.SIDE_X, *r_csr)
    core.set_matrix(pkg.SIDE_Y, *c_csr)
    core.set_factors(pkg.SIDE_Y, Y0)
    core.half_iteration(pkg.SIDE_X)
    core.half_iteration(pkg.SIDE_Y)
    yield core, r_csr
    core.close()


def test_half_iteration_enqueued_before_the_call_is_seen(model):
    core, _ = model
    Y_before = core.get_factors(pkg.SIDE_Y)
    core.half_iteration(pkg.SIDE_X)
    core.half_iteration(pkg.SIDE_Y)                                  # enqueued; the call below must see its Y
    queries = [0, 17, 4242, 149_999]
    idx, sc, cnt = core.most_similar_items(queries, 10)
    Y = core.get_factors(pkg.SIDE_Y)
    assert not np.array_equal(Y, Y_before)
    Yn = so.norms(Y)
    for q, it in enumerate(queries):
        oidx, osc = so.most_similar(Y, it, 10, Ynorm=Yn)
        same_ranking(idx[q], sc[q], cnt[q], oidx, osc)


def test_recommended_because_rows_of_r_and_known_items(model):
    core, r_csr = model
    Y = core.get_factors(pkg.SIDE_Y)
    rp, col = r_csr[0], r_csr[1]
    users = [u for u in range(3000) if rp[u + 1] - rp[u] >= 3][:20]
    items = [int(col[rp[u]]) for u in users]                         # the item is one of the user's own: it comes back
    tags = [int(col[rp[users[0]] + 1])]
    core.set_tag_items(tags)
    try:
        idx, sc, cnt = core.recommended_because(users, items, 5)
        for q, u in enumerate(users):
            oidx, osc = so.recommended_because(Y, col[rp[u]:rp[u + 1]], items[q], 5, tags=tags)
            same_ranking(idx[q], sc[q], cnt[q], oidx, osc)
            if items[q] not in tags:
                assert items[q] in idx[q, :cnt[q]].tolist()
        assert tags[0] not in idx[0].tolist()
    finally:
        core.set_tag_items(None)
    # knownItemIDs instead of the rows of R: user 0 knows 6000 items (more than one chunk of candidates)
    rng = np.random.default_rng(5)
    lists = [rng.choice(150_000, 6000 if u == 0 else 4, replace=False).astype(np.int32) for u in range(3000)]
    kp = np.zeros(3001, np.int64)
    kp[1:] = np.cumsum([len(x) for x in lists])
    core.set_known_items(kp, np.concatenate(lists))
    try:
        qu, qi = [0, 1, 0], [int(lists[0][10]), 9, 77]
        idx, sc, cnt = core.recommended_because(qu, qi, 100)
        for q in range(3):
            oidx, osc = so.recommended_because(Y, lists[qu[q]], qi[q], 100)
            same_ranking(idx[q], sc[q], cnt[q], oidx, osc)
        assert cnt[0] == 100 and idx[0, 0] == qi[0]
    finally:
        core.set_known_items(None, None)


def test_similarity_to_item_nan_and_bad_indices():
    Y = hard_Y(1000, 16, 3)
    with y_core(Y) as core:
        items = [0, 7, 11, 100, 3, 999]
        out = core.similarity_to_item(11, items)
        want = so.similarity_to_item(Y, 11, items)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) or (
            np.array_equal(np.isnan(out), np.isnan(want)) and np.array_equal(out[~np.isnan(out)], want[~np.isnan(want)]))
        assert np.isnan(out[1])
        for bad in ([0, 1000], [-1]):
            with pytest.raises(pkg.MalsError) as e:
                core.similarity_to_item(11, bad)
            assert e.value.status == _lib.INVALID_ARG
        with pytest.raises(pkg.MalsError) as e:
            core.similarity_to_item(1000, [0])
        assert e.value.status == _lib.INVALID_ARG
        with pytest.raises(pkg.MalsError) as e:
            core.most_similar_items([0, 1000], 5)
        assert e.value.status == _lib.INVALID_ARG


def test_concurrent_similarity_and_recommend_calls(model):
    core, r_csr = model
    X, Y = core.get_factors(pkg.SIDE_X), core.get_factors(pkg.SIDE_Y)
    Yn = so.norms(Y)
    before = core.recommend_front_stats()
    results, errors = [], []

    def worker(t):
        try:
            rng = np.random.default_rng(t)
            for c in range(4):
                if (t + c) % 2:
                    it = int(rng.integers(150_000))
                    hm = (5, 10, 64)[(t + c) % 3]
                    results.append(("sim", it, hm, core.most_similar_items([it], hm)))
                else:
                    u = int(rng.integers(3000))
                    results.append(("rec", u, 10, core.recommend([u], 10)))
        except Exception as e:   # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(32)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert len(results) == 128
    for kind, a, hm, (idx, sc, cnt) in results:
        if kind == "sim":
            oidx, osc = so.most_similar(Y, a, hm, Ynorm=Yn)
        else:
            oidx, osc = to.recommend(Y, X[a], hm, r_csr[1][r_csr[0][a]:r_csr[0][a + 1]])
        same_ranking(idx[0], sc[0], cnt[0], oidx, osc)
    after = core.recommend_front_stats()
    calls, passes = after["calls"] - before["calls"], after["passes"] - before["passes"]
    assert calls == 128 and 0 < passes < calls                     # calls were folded into shared passes


def test_group_matches_one_handle():
    k, n_users, n_items = 16, 400, 1500
    r_csr, c_csr, Y0 = synth.numpy_problem(n_users, n_items, 12000, k, seed=9)
    with pkg.GroupALS.single_process(k, [0, 0], backend=_lib.GROUP_PEER_COPY) as g:
        g.set_factor_rows(pkg.SIDE_X, n_users)
        g.set_factor_rows(pkg.SIDE_Y, n_items)
        g.set_matrix(pkg.SIDE_X, *r_csr)
        g.set_matrix(pkg.SIDE_Y, *c_csr)
        g.set_factors(pkg.SIDE_Y, Y0)
        g.iterate(1)
        X = g.get_factors(pkg.SIDE_X, 0, n_users)
        Y = g.get_factors(pkg.SIDE_Y, 0, n_items)
        bx = g.bounds(pkg.SIDE_X)
        users = np.array([0, int(bx[1]) - 1, int(bx[1]), n_users - 1], np.int64)   # both members' users
        items = np.array([int(r_csr[1][r_csr[0][u]]) if r_csr[0][u + 1] > r_csr[0][u] else 0 for u in users], np.int64)
        g_ms = g.most_similar_items([[1, 2], [3]], 10)
        g_st = g.similarity_to_item(5, [1, 2, 3])
        g_rb = g.recommended_because(users, items, 8)
    with pkg.ALSCore(k) as core:
        core.set_factor_rows(pkg.SIDE_X, n_users)
        core.set_factor_rows(pkg.SIDE_Y, n_items)
        core.set_matrix(pkg.SIDE_X, *r_csr)
        core.set_factors(pkg.SIDE_X, X)
        core.set_factors(pkg.SIDE_Y, Y)
        one = (core.most_similar_items([[1, 2], [3]], 10), core.similarity_to_item(5, [1, 2, 3]),
               core.recommended_because(users, items, 8))
    for a, b in zip(g_ms + g_rb, one[0] + one[2]):
        assert np.array_equal(np.asarray(a).view(np.uint32) if a.dtype == np.float32 else a,
                              np.asarray(b).view(np.uint32) if b.dtype == np.float32 else b)
    assert np.array_equal(g_st.view(np.uint32), one[1].view(np.uint32))
