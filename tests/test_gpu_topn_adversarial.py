"""The top-N filter at its bf16 error bound, on the device: the catalogues of tests/topn_filter_emulation.py (high-error
items in sampled tiles, one per bucket; the true winners, rounding the other way, in unsampled tiles and the partial
last tile) through every entry point that runs the filter, against the oracles and against the dense path
(MALS_TOPN_FULL=1): indices and score bits identical."""
import threading

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from oracle import topn_oracle as to
from tests import similarity_oracle as so
from tests import topn_filter_emulation as fe
from tests.test_gpu_topn import same_ranking

pytestmark = pytest.mark.gpu

KNOWN = np.array([5, 77, 1234], np.int32)


def catalogue_core(Y, X):
    """a handle with Y, users X, user 0 knowing KNOWN (none of them planted), the others nothing"""
    k = Y.shape[1]
    core = pkg.ALSCore(k)
    core.set_factor_rows(pkg.SIDE_X, len(X))
    core.set_factor_rows(pkg.SIDE_Y, len(Y))
    core.set_factors(pkg.SIDE_X, X)
    core.set_factors(pkg.SIDE_Y, Y)
    rp = np.full(len(X) + 1, len(KNOWN), np.int64)
    rp[0] = 0
    core.set_matrix(pkg.SIDE_X, rp, KNOWN, np.ones(len(KNOWN), np.float32))
    return core


def answers(core, x, how_many):
    """(name, (idx, sc, cnt)) of every by-vector entry point for the query x (user 0 of the handle is x)"""
    return [("recommend_vectors", core.recommend_vectors(x[None, :], how_many)),
            ("recommend", core.recommend(np.array([0], np.int64), how_many)),
            ("recommend_considering_known", core.recommend(np.array([0], np.int64), how_many, consider_known_items=True)),
            ("recommend_to_many", core.recommend_to_many([np.stack([x, x])], how_many))]


@pytest.mark.parametrize("k", [30, 64, 100, 128])
def test_recommend_catalogue(k, monkeypatch):
    for how_many in (1, 10, 64):
        Y, x, high, win = fe.recommend_catalogue(k, how_many, seed=k)
        X = np.stack([x, -x])
        plain = to.recommend(Y, x, how_many)
        known = to.recommend(Y, x, how_many, KNOWN)
        assert plain[0][0] == win[-1]
        with catalogue_core(Y, X) as core:
            got = answers(core, x, how_many)
            monkeypatch.setenv("MALS_TOPN_FULL", "1")
            full = answers(core, x, how_many)
            monkeypatch.delenv("MALS_TOPN_FULL")
        for (name, (idx, sc, cnt)), (_, f) in zip(got, full):
            oidx, osc = known if name == "recommend" else plain
            assert cnt[0] == how_many, name
            same_ranking(idx[0], sc[0], oidx, osc)
            assert all(np.array_equal(a, b) for a, b in zip((idx, sc, cnt), f)), name


@pytest.mark.parametrize("k", [30, 64, 100, 128])
def test_most_similar_catalogue(k, monkeypatch):
    for how_many in (1, 10, 64):
        Y, q, high, win = fe.cosine_catalogue(k, how_many, seed=k)
        oidx, osc = so.most_similar(Y, [q], how_many)
        assert oidx[0] == win[-1]
        with catalogue_core(Y, Y[:1]) as core:
            idx, sc, cnt = core.most_similar_items([[q]], how_many)
            monkeypatch.setenv("MALS_TOPN_FULL", "1")
            full = core.most_similar_items([[q]], how_many)
            monkeypatch.delenv("MALS_TOPN_FULL")
        assert cnt[0] == how_many
        same_ranking(idx[0], sc[0], oidx, osc)
        assert all(np.array_equal(a, b) for a, b in zip((idx, sc, cnt), full))


@pytest.mark.parametrize("seed", range(20))
def test_randomized_family(seed):
    """fe.random_family: 256 queries (4 patterns at power-of-two scales) per call -- full passes on every slot -- each
    compared with the oracle (a power-of-two scale scales every score exactly: one oracle answer per pattern)"""
    Y, P, how_many, k = fe.random_family(seed)
    rng = np.random.default_rng(seed)
    which = np.arange(256) % len(P)
    scale = np.exp2(rng.integers(-4, 5, 256)).astype(np.float32)
    Q = (P[which] * scale[:, None]).astype(np.float32)
    ref = [to.recommend(Y, p, how_many) for p in P]
    with catalogue_core(Y, P[:1]) as core:
        idx, sc, cnt = core.recommend_vectors(Q, how_many)
    for i in range(256):
        oidx, osc = ref[which[i]]
        assert cnt[i] == how_many, (seed, i)
        same_ranking(idx[i], sc[i], oidx, (osc * scale[i]).astype(np.float32))


def test_serving_front_from_16_threads():
    """the adversarial query from 16 request threads at once, mixed with ordinary calls (a random user's recommend): the
    serving front folds them into shared passes; every answer equals the oracle"""
    k, how_many = 64, 10
    Y, x, high, win = fe.recommend_catalogue(k, how_many, seed=16)
    rng = np.random.default_rng(16)
    X = np.concatenate([x[None, :], (rng.standard_normal((63, k)) * 0.5).astype(np.float32)])
    adv = to.recommend(Y, x, how_many)
    results, errors = [], []
    with catalogue_core(Y, X) as core:
        def worker(t):
            try:
                r = np.random.default_rng(t)
                for c in range(6):
                    if (t + c) % 2:
                        results.append(("adv", 0, core.recommend_vectors(x[None, :], how_many)))
                    else:
                        u = int(r.integers(1, 64))
                        results.append(("user", u, core.recommend(np.array([u], np.int64), how_many)))
            except Exception as e:   # noqa: BLE001 -- reported below
                errors.append(e)
        threads = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    assert not errors, errors
    assert len(results) == 96
    for kind, u, (idx, sc, cnt) in results:
        oidx, osc = adv if kind == "adv" else to.recommend(Y, X[u], how_many)   # (only user 0 knows items)
        same_ranking(idx[0], sc[0], oidx, osc)


def test_two_member_group_equals_one_handle():
    """the cosine catalogue on a two-member group: mostSimilarItems of its query item, and recommend for users whose vector
    is that item's row -- adversarial for both (a margin of 1.25 * 2^-8 answers the high-error rows in both modes)"""
    k, how_many = 64, 10
    Y, q, high, win = fe.cosine_catalogue(k, how_many, seed=2)
    rng = np.random.default_rng(2)
    n_users = 64
    X = (rng.standard_normal((n_users, k)) * 0.5).astype(np.float32)
    X[0] = X[n_users - 1] = Y[q]                                    # one adversarial user on each member
    rp = np.arange(n_users + 1, dtype=np.int64) * len(KNOWN)
    col = np.tile(KNOWN, n_users)
    val = np.ones(len(col), np.float32)
    order = np.argsort(col, kind="stable")
    crp = np.zeros(len(Y) + 1, np.int64)
    np.add.at(crp, col.astype(np.int64) + 1, 1)
    crp = np.cumsum(crp)
    ccol = (np.arange(len(col)) // len(KNOWN))[order].astype(np.int32)
    users = np.array([0, 1, n_users - 2, n_users - 1], np.int64)
    with pkg.GroupALS.single_process(k, [0, 0], backend=_lib.GROUP_PEER_COPY) as g:
        g.set_factor_rows(pkg.SIDE_X, n_users)
        g.set_factor_rows(pkg.SIDE_Y, len(Y))
        g.set_matrix(pkg.SIDE_X, rp, col, val)
        g.set_matrix(pkg.SIDE_Y, crp, ccol, val)
        g.set_factors(pkg.SIDE_X, X)
        g.set_factors(pkg.SIDE_Y, Y)
        bx = g.bounds(pkg.SIDE_X)
        assert bx[1] < n_users - 1                                   # the two adversarial users live on different members
        g_rec = g.recommend(users, how_many)
        g_sim = g.most_similar_items([[q]], how_many)
    with catalogue_core(Y, X) as core:
        core.set_matrix(pkg.SIDE_X, rp, col, val)
        one = (core.recommend(users, how_many), core.most_similar_items([[q]], how_many))
    for a, b in zip(g_rec + g_sim, one[0] + one[1]):
        assert np.array_equal(np.asarray(a).view(np.uint32) if a.dtype == np.float32 else a,
                              np.asarray(b).view(np.uint32) if b.dtype == np.float32 else b)
    for i, u in enumerate(users):
        oidx, osc = to.recommend(Y, X[u], how_many, KNOWN)
        same_ranking(g_rec[0][i], g_rec[1][i], oidx, osc)
    assert to.recommend(Y, Y[q], how_many, KNOWN)[0][0] == win[-1]
    oidx, osc = so.most_similar(Y, [q], how_many)
    assert oidx[0] == win[-1]
    same_ranking(g_sim[0][0], g_sim[1][0], oidx, osc)
