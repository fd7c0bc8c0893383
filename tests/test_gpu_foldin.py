"""The online write path on the device (mals_set_preferences, mals_remove_preferences, mals_grow_factor_rows and the
fold-in reads) against tests/foldin_oracle.py: factor bits, statuses, known items and top-N answers identical."""
import threading

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd.core import HostSolver, MalsError
from oracle import topn_oracle as to
from tests import foldin_oracle as fo
from tests import similarity_oracle as so

pytestmark = pytest.mark.gpu
X_, Y_ = pkg.SIDE_X, pkg.SIDE_Y


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gram_solver(M):
    M = np.asarray(M, np.float64)
    return HostSolver.create(M.T @ M)


def model(n_users, n_items, k, seed, nnz_per_user=5):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n_users, k)) * 0.3).astype(np.float32)
    Y = (rng.standard_normal((n_items, k)) * 0.3).astype(np.float32)
    rows = [np.sort(rng.choice(n_items, nnz_per_user, replace=False)) for _ in range(n_users)]
    ptr = np.zeros(n_users + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows).astype(np.int32)
    return X, Y, ptr, col


def core_for(X, Y, ptr, col, sx=True, sy=True):
    k = X.shape[1]
    c = pkg.ALSCore(k)
    c.set_factor_rows(X_, len(X))
    c.set_factor_rows(Y_, len(Y))
    c.set_factors(X_, X)
    c.set_factors(Y_, Y)
    c.set_matrix(X_, ptr, col, np.ones(len(col), np.float32))
    solvers = (gram_solver(X) if sx else None, gram_solver(Y) if sy else None)
    c.set_foldin_solver(X_, solvers[0])
    c.set_foldin_solver(Y_, solvers[1])
    return c, solvers


def known_of(ptr, col):
    return {u: set(col[ptr[u]:ptr[u + 1]].tolist()) for u in range(len(ptr) - 1) if ptr[u + 1] > ptr[u]}


def check_model(c, X, Y):
    assert np.array_equal(bits(c.get_factors(X_)), bits(X))
    assert np.array_equal(bits(c.get_factors(Y_)), bits(Y))


@pytest.mark.parametrize("k", [2, 8, 30, 50, 64, 100, 128])
def test_device_solve_is_solve_ftod(k):
    rng = np.random.default_rng(k)
    A = rng.standard_normal((3 * k, k))
    A[:, k // 2] = 0.0                     # a zero column: tau == 0 there
    A[:, 1 % k] *= 1e3                      # a dominant column: pivoted first
    G = A.T @ A + np.eye(k) * 1e-3
    s = HostSolver.create(G)
    with pkg.ALSCore(k) as c:
        c.set_factor_rows(Y_, 4)
        c.set_foldin_solver(Y_, s)
        b = rng.standard_normal((200, k)).astype(np.float32)
        b[3] = 0.0
        x = c.foldin_solve(Y_, b)
    for q in range(len(b)):
        assert np.array_equal(x[q].view(np.uint64), s.solve_ftod(b[q]).view(np.uint64)), q


def test_distinct_pairs_batch_k64():
    k, n = 64, 10000
    X, Y, ptr, col = model(3000, 4000, k, 1)
    c, (sx, sy) = core_for(X, Y, ptr, col)
    rng = np.random.default_rng(2)
    u = rng.permutation(3000)[:n % 3000].tolist() + rng.integers(0, 3000, n - n % 3000).tolist()
    i = rng.integers(0, 4000, n)
    v = rng.choice([1.0, 2.0, -1.0, 0.5], n).astype(np.float32)
    st = c.set_preferences(u, i, v)
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    sto = fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy)
    assert np.array_equal(st, sto)
    check_model(c, Xo, Yo)
    assert c.foldin_stats()["applied"] == n and c.foldin_stats()["levels"] > 1
    c.close()


def test_repeated_rows_hot_item_values_and_growth():
    k = 16
    X, Y, ptr, col = model(50, 40, k, 3)
    c, (sx, sy) = core_for(X, Y, ptr, col)
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    rng = np.random.default_rng(4)
    u = rng.integers(0, 50, 300)
    i = np.full(300, 7)                                    # a hot item: 300 levels
    v = rng.choice([1.0, -1.0, 0.0, 5.0, -5.0, 1e30, -1e30, 0.25], 300).astype(np.float32)
    assert np.array_equal(c.set_preferences(u, i, v), fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy))
    check_model(c, Xo, Yo)
    # new users and items: zero rows, then a mix of new and old rows
    c.grow_factor_rows(X_, 70)
    c.grow_factor_rows(Y_, 45)
    Xo = np.vstack([Xo, np.zeros((20, k), np.float32)])
    Yo = np.vstack([Yo, np.zeros((5, k), np.float32)])
    check_model(c, Xo, Yo)
    u = rng.integers(0, 70, 500)
    i = rng.integers(0, 45, 500)
    v = rng.choice([1.0, 2.0, -1.0], 500).astype(np.float32)
    assert np.array_equal(c.set_preferences(u, i, v), fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy))
    check_model(c, Xo, Yo)
    # grown users are users of recommend; their known items are what the writes gave them
    users = np.arange(50, 70)
    idx, sc, cnt = c.recommend(users, 10)
    for q, uu in enumerate(users):
        oi, os_ = to.recommend(Yo, Xo[uu], 10, known=sorted(known.get(int(uu), ())))
        assert np.array_equal(idx[q, :cnt[q]], oi) and np.array_equal(bits(sc[q, :cnt[q]]), bits(os_))
    c.close()


def test_null_solvers():
    k = 8
    X, Y, ptr, col = model(20, 30, k, 5)
    u, i = np.arange(20), np.arange(20)
    v = np.ones(20, np.float32)
    c, (_, sy) = core_for(X, Y, ptr, col, sx=False)
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    assert np.array_equal(c.set_preferences(u, i, v), fo.set_preferences(Xo, Yo, known, u, i, v, None, sy))
    assert np.array_equal(Yo, Y)
    check_model(c, Xo, Yo)
    c.close()
    c, (sx, _) = core_for(X, Y, ptr, col, sy=False)
    st = c.set_preferences(u, i, v, raise_on_error=False)
    assert np.all(st == pkg._lib.INVALID_ARG)
    check_model(c, X, Y)
    with pytest.raises(MalsError):
        c.set_preferences(u, i, v)
    c.close()


def test_nan_rows_and_per_update_status():
    k = 8
    X, Y, ptr, col = model(20, 30, k, 6)
    c, (sx, sy) = core_for(X, Y, ptr, col)     # the generation's solvers, from the rows before one went bad
    X[3] = np.nan
    c.set_factors(X_, X)
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    u = np.array([1, 3, 2, 3, 4])
    i = np.array([1, 2, 3, 4, 5])
    v = np.ones(5, np.float32)
    st = c.set_preferences(u, i, v, raise_on_error=False)
    assert st.tolist() == [0, 2, 0, 2, 0]
    assert np.array_equal(st, fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy))
    check_model(c, Xo, Yo)
    assert c.foldin_stats()["failed"] == 2
    c.close()


def top_same(c, Xo, Yo, known, users, how_many=10):
    idx, sc, cnt = c.recommend(users, how_many)
    for q, u in enumerate(users):
        oi, os_ = to.recommend(Yo, Xo[u], how_many, known=sorted(known.get(int(u), ())))
        assert cnt[q] == len(oi)
        assert np.array_equal(idx[q, :cnt[q]], oi), (u, idx[q, :cnt[q]], oi)
        assert np.array_equal(bits(sc[q, :cnt[q]]), bits(os_))


@pytest.mark.parametrize("dense", [False, True])
def test_remove_and_recommend_after_writes(dense, monkeypatch):
    if dense:
        monkeypatch.setenv("MALS_TOPN_FULL", "1")
    k = 32
    X, Y, ptr, col = model(60, 3000, k, 7, nnz_per_user=3)
    c, (sx, sy) = core_for(X, Y, ptr, col)
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    users = np.arange(60)
    top_same(c, Xo, Yo, known, users)
    # set: the recommended items become known and leave the answers
    idx, _, _ = c.recommend(users, 2)
    u, i = users, idx[:, 0]
    v = np.ones(60, np.float32)
    assert np.array_equal(c.set_preferences(u, i, v), fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy))
    top_same(c, Xo, Yo, known, users)
    # remove: ignored pairs, emptied users zeroed and reported, removed items come back
    ru = [0, 0, 1, 59] + [2] * len(known[2])
    ri = [2999, int(idx[0, 0]), int(col[ptr[1]]), int(idx[59, 0])] + sorted(known[2])
    got = c.remove_preferences(ru, ri)
    exp = fo.remove_preferences(Xo, known, ru, ri)
    assert got.tolist() == exp and 2 in exp
    check_model(c, Xo, Yo)
    top_same(c, Xo, Yo, known, users)
    # recommendedBecause sees the same known sets
    q_items = np.arange(60) % 3000
    bi, bs, bc = c.recommended_because(users, q_items, 5)
    for q, uu in enumerate(users):
        oi, os_ = so.recommended_because(Yo, sorted(known.get(int(uu), ())), int(q_items[q]), 5)
        assert np.array_equal(bi[q, :bc[q]], oi) and np.array_equal(bits(bs[q, :bc[q]]), bits(os_))
    # re-added
    c.set_preferences([2], [5], [1.0])
    fo.set_preferences(Xo, Yo, known, [2], [5], [1.0], sx, sy)
    check_model(c, Xo, Yo)
    top_same(c, Xo, Yo, known, users)
    c.close()


def test_estimates_and_anonymous_reads():
    k = 24
    X, Y, ptr, col = model(30, 500, k, 8)
    c, (sx, sy) = core_for(X, Y, ptr, col)
    u = np.array([0, -1, 5, 7])
    i = np.array([3, 4, -1, 9])
    assert np.array_equal(bits(c.estimate_preferences(u, i)), bits(fo.estimate_preferences(X, Y, u, i)))
    queries = [[1, 2, 3], [-1, 4], [-1], [7, 7, 499]]
    values = [[1.0, 2.0, -1.0], [0.5, 3.0], [1.0], [1.0, 0.0, -2.0]]
    f, st = c.anonymous_features(queries, values, raise_on_error=False)
    assert st.tolist() == [0, 0, 2, 0]
    for q, items in enumerate(queries):
        acc, ok = fo.anonymous_features(Y, items, values[q], sy)
        if ok:
            assert np.array_equal(bits(f[q]), bits(acc))
    est, st2 = c.estimate_for_anonymous([10, 11, 12, 13], queries, values)
    for q, items in enumerate(queries):
        e, ok = fo.estimate_for_anonymous(Y, [10, 11, 12, 13][q], items, values[q], sy)
        if ok:
            assert bits(est[q]) == bits(e)
    idx, sc, cnt, st3 = c.recommend_to_anonymous(queries, 8, values)
    assert st3.tolist() == [0, 0, 2, 0] and cnt[2] == 0
    for q, items in enumerate(queries):
        if st3[q]:
            continue
        acc, _ = fo.anonymous_features(Y, items, values[q], sy)
        oi, os_ = to.recommend(Y, acc, 8, known=sorted(j for j in items if j >= 0))
        assert np.array_equal(idx[q, :cnt[q]], oi) and np.array_equal(bits(sc[q, :cnt[q]]), bits(os_))
    c.close()


def test_half_iteration_after_write_sees_new_factors():
    k = 16
    X, Y, ptr, col = model(80, 60, k, 9)
    rng = np.random.default_rng(10)
    c, (sx, sy) = core_for(X, Y, ptr, col)
    c.set_matrix(Y_, *transpose(ptr, col, 60))
    c.half_iteration(X_)                                  # Gramian of Y now cached
    c.set_preferences(rng.integers(0, 80, 50), rng.integers(0, 60, 50), np.ones(50, np.float32))
    Xw, Yw = c.get_factors(X_), c.get_factors(Y_)
    c.half_iteration(X_)
    fresh, _ = core_for(Xw, Yw, ptr, col)
    fresh.set_matrix(Y_, *transpose(ptr, col, 60))
    fresh.half_iteration(X_)
    assert np.array_equal(bits(c.get_factors(X_)), bits(fresh.get_factors(X_)))
    c.close()
    fresh.close()


def transpose(ptr, col, n_items):
    users = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    order = np.lexsort((users, col))
    tptr = np.zeros(n_items + 1, np.int64)
    np.add.at(tptr, col[order] + 1, 1)
    return np.cumsum(tptr), users[order].astype(np.int32), np.ones(len(col), np.float32)


def test_readers_and_a_writer():
    k = 32
    X, Y, ptr, col = model(64, 2000, k, 11, nnz_per_user=2)
    c, (sx, sy) = core_for(X, Y, ptr, col)
    rng = np.random.default_rng(12)
    batches = [(rng.integers(0, 64, 40), rng.integers(0, 2000, 40), np.ones(40, np.float32)) for _ in range(20)]
    models = []
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    models.append((Xo.copy(), Yo.copy(), {a: set(b) for a, b in known.items()}))
    for (u, i, v) in batches:
        fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy)
        models.append((Xo.copy(), Yo.copy(), {a: set(b) for a, b in known.items()}))
    answers = {m: {} for m in range(len(models))}
    for m, (Xm, Ym, km) in enumerate(models):
        for uu in range(64):
            answers[m][uu] = to.recommend(Ym, Xm[uu], 5, known=sorted(km.get(uu, ())))
    written = [0]
    lock = threading.Lock()
    errors, statuses = [], []
    stop = threading.Event()

    def writer():
        for b, (u, i, v) in enumerate(batches):
            statuses.append(c.set_preferences(u, i, v))
            with lock:
                written[0] = b + 1
        stop.set()

    def reader(seed):
        r = np.random.default_rng(seed)
        try:
            while not stop.is_set():
                uu = int(r.integers(0, 64))
                with lock:
                    before = written[0]
                idx, sc, cnt = c.recommend([uu], 5)
                with lock:
                    after = written[0]
                ok = [m for m in range(before, min(after + 2, len(models))) if
                      np.array_equal(idx[0, :cnt[0]], answers[m][uu][0]) and np.array_equal(bits(sc[0, :cnt[0]]), bits(answers[m][uu][1]))]
                if not ok:
                    errors.append((uu, before, after))
        except Exception as e:   # pragma: no cover
            errors.append(repr(e))

    th = [threading.Thread(target=reader, args=(s,)) for s in range(16)] + [threading.Thread(target=writer)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errors, errors[:5]
    assert len(statuses) == 20 and all(not s.any() for s in statuses)
    check_model(c, Xo, Yo)
    c.close()


def test_new_generation_drops_the_overlay():
    k = 8
    X, Y, ptr, col = model(10, 200, k, 13)
    c, (sx, sy) = core_for(X, Y, ptr, col)
    idx, _, _ = c.recommend([0], 3)
    c.set_preferences([0], [int(idx[0, 0])], [1.0])
    Xw, Yw = c.get_factors(X_), c.get_factors(Y_)
    assert int(idx[0, 0]) not in c.recommend([0], 3)[0][0].tolist()
    c.set_known_items(ptr, col)                        # a new generation's known items: the write's item is back
    oi, _ = to.recommend(Yw, Xw[0], 3, known=sorted(col[ptr[0]:ptr[1]].tolist()))
    assert np.array_equal(c.recommend([0], 3)[0][0], oi)
    c.set_preferences([0], [int(oi[0])], [1.0])
    c.set_matrix(X_, ptr, col, np.ones(len(col), np.float32))
    Xw, Yw = c.get_factors(X_), c.get_factors(Y_)
    oi2, _ = to.recommend(Yw, Xw[0], 3, known=sorted(col[ptr[0]:ptr[1]].tolist()))
    assert np.array_equal(c.recommend([0], 3)[0][0], oi2)
    c.close()


def small_core(X, Y, sx, sy):
    k = X.shape[1]
    c = pkg.ALSCore(k)
    c.set_factor_rows(X_, len(X))
    c.set_factor_rows(Y_, len(Y))
    c.set_factors(X_, X)
    c.set_factors(Y_, Y)
    ptr = np.arange(len(X) + 1, dtype=np.int64)
    c.set_matrix(X_, ptr, (np.arange(len(X)) % len(Y)).astype(np.int32), np.ones(len(X), np.float32))
    c.set_foldin_solver(X_, sx)
    c.set_foldin_solver(Y_, sy)
    return c


def diag_solver(d):
    return HostSolver.create(np.diag(np.asarray(d, np.float64)), singularity_threshold=1e-310)


def test_non_finite_deltas_stop_the_loops_on_the_device():
    # item loop: X^T X = diag(1, 1e-300) turns x_u = (1, 3e38) into (NaN, inf): stops at once, nothing moves
    X = np.array([[1.0, 3e38]], np.float32)
    Y = np.array([[0.25, 0.0]], np.float32)
    sx, sy = diag_solver([1.0, 1e-300]), diag_solver([1.0, 1.0])
    c = small_core(X, Y, sx, sy)
    Xo, Yo, known = X.copy(), Y.copy(), {}
    st = c.set_preferences([0], [0], [1.0], raise_on_error=False)
    code, why, _ = fo.update_features(Xo, Yo, 0, 0, 1.0, sx, sy)
    assert st.tolist() == [code] == [fo.INVALID_ARG] and why == fo.WHY_ITEM_DELTA
    check_model(c, Xo, Yo)
    assert "item fold-in delta" in pkg._lib.load().mals_last_error(c._h).decode()
    c.close()
    # user loop: Y^T Y = diag(1, 1e-300) on y_i = (1, 3e38): the item row is complete, the user row stops at element 0
    X = np.array([[0.5, 0.0]], np.float32)
    Y = np.array([[1.0, 3e38]], np.float32)
    sx, sy = diag_solver([1.0, 1.0]), diag_solver([1.0, 1e-300])
    c = small_core(X, Y, sx, sy)
    Xo, Yo = X.copy(), Y.copy()
    st = c.set_preferences([0], [0], [1.0], raise_on_error=False)
    code, why, _ = fo.update_features(Xo, Yo, 0, 0, 1.0, sx, sy)
    assert st.tolist() == [code] == [fo.INVALID_ARG] and why == fo.WHY_USER_DELTA
    assert not np.array_equal(Yo, Y)
    check_model(c, Xo, Yo)
    c.close()


def test_learning_rate_and_big_fold_in_counter():
    k = 8
    X, Y, ptr, col = model(20, 30, k, 14)
    c, (sx, _) = core_for(X, Y, ptr, col)
    sy = HostSolver.create(np.eye(k) * 1e-6, singularity_threshold=1e-12)   # userFoldIn = 1e6 y_i: norm > 1e4
    c.set_foldin_solver(Y_, sy)
    c.set_foldin_learn_rate(0.5)
    Xo, Yo = X.copy(), Y.copy()
    u, i = np.arange(20), np.arange(20)
    v = np.full(20, 2.0, np.float32)
    st = c.set_preferences(u, i, v, raise_on_error=False)
    big = 0
    exp = []
    for t in range(20):
        code, _, b = fo.update_features(Xo, Yo, int(u[t]), int(i[t]), v[t], sx, sy, rate=0.5)
        exp.append(code)
        big += b
    assert st.tolist() == exp and big > 0
    check_model(c, Xo, Yo)
    s = c.foldin_stats()
    assert s["big_foldin"] == big and s["device_ms_last"] > 0
    c.close()


def test_tags_survive_item_growth_and_refusals():
    k = 8
    X, Y, ptr, col = model(10, 300, k, 15)
    c, (sx, sy) = core_for(X, Y, ptr, col)
    Xo = X.copy()
    top = c.recommend([0], 3)[0][0]
    tags = [int(top[0]), 7]
    c.set_tag_items(tags)
    c.grow_factor_rows(Y_, 320)
    assert c.tag_item_count() == 2
    Yo = np.vstack([Y, np.zeros((20, k), np.float32)])
    idx, sc, cnt = c.recommend([0], 5)
    oi, os_ = to.recommend(Yo, Xo[0], 5, known=sorted(col[ptr[0]:ptr[1]].tolist()), tags=tags)
    assert np.array_equal(idx[0, :cnt[0]], oi) and np.array_equal(bits(sc[0, :cnt[0]]), bits(os_))
    with pytest.raises(MalsError):
        c.grow_factor_rows(Y_, 100)        # a replica only grows
    c.close()
    import torch
    c = pkg.ALSCore(k)
    t = torch.zeros((10, k), dtype=torch.float32, device="cuda")
    c.bind_factors(X_, t)
    with pytest.raises(MalsError, match="mals_bind_factors"):
        c.grow_factor_rows(X_, 20)
    c.close()


def test_group_members_are_refused():
    k = 8
    with pkg.GroupALS.single_process(k, [0], backend=pkg._lib.GROUP_PEER_COPY) as g:
        m, _ = g.local(0)
        with pytest.raises(MalsError, match="group"):
            m.set_preferences([0], [0], [1.0])
        with pytest.raises(MalsError, match="group"):
            m.grow_factor_rows(X_, 10)
