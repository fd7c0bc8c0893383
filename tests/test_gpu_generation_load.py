"""mals_load_generation (include/myrrix_als.h, "loading a new generation") against a TWIN handle: after the load a second
handle is made the old way (set_factor_rows, set_factors, set_matrix / set_known_items, set_tag_items, set_tag_users) from
what tests/generation_load_oracle.py says the merged model is, and the two must answer bit for bit alike.  The load copies
and re-indexes, it computes nothing in floating point: every comparison is for equality."""
import ctypes
import threading

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from myrrix_recommender_amd.core import HostSolver, MalsError, factor_digest_host, generation_join_host
from tests import generation_load_oracle as glo
from tests.test_generation_join_host import EXTREME, colliding_ids

pytestmark = pytest.mark.gpu
X_, Y_ = pkg.SIDE_X, pkg.SIDE_Y


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate([np.asarray(sorted(r), np.int32) for r in rows]) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, idx.astype(np.int32)


def solver_of(M):
    M = M.astype(np.float64)
    return HostSolver.create(M.T @ M + 1e-3 * np.eye(M.shape[1]))


def factors(rng, n, k):
    return (rng.standard_normal((n, k)) * 0.3).astype(np.float32)


class Live:
    """A serving handle and its mirror in Python: ids per row, the users' known items (sets of item rows), the tag rows, the
    rows written since the last load."""

    def __init__(self, k, user_ids, item_ids, seed, solvers=False, max_known=12, known=None):
        rng = np.random.default_rng(seed)
        self.k = k
        self.user_ids, self.item_ids = [int(u) for u in user_ids], [int(i) for i in item_ids]
        nu, ni = len(self.user_ids), len(self.item_ids)
        X, Y = factors(rng, nu, k), factors(rng, ni, k)
        self.known = known if known is not None else \
            [set(rng.choice(ni, int(rng.integers(0, min(max_known, ni) + 1)), replace=False).tolist()) for _ in range(nu)]
        self.core = pkg.ALSCore(k)
        self.core.set_factor_rows(X_, nu)
        self.core.set_factor_rows(Y_, ni)
        ptr, idx = csr(self.known)
        self.core.set_matrix(X_, ptr, idx, np.ones(len(idx), np.float32))
        self.core.set_factors(X_, X)
        self.core.set_factors(Y_, Y)
        self.solvers = (solver_of(X), solver_of(Y)) if solvers else None
        if solvers:
            self.core.set_foldin_solver(X_, self.solvers[0])
            self.core.set_foldin_solver(Y_, self.solvers[1])
        self.tag_users, self.tag_items = [], []
        self.recent = (set(), set())

    def set_tags(self, tag_users, tag_items):
        self.tag_users, self.tag_items = list(tag_users), list(tag_items)
        self.core.set_tag_users(self.tag_users)
        self.core.set_tag_items(self.tag_items)

    def grow(self, new_user_ids, new_item_ids):
        self.user_ids += [int(u) for u in new_user_ids]
        self.item_ids += [int(i) for i in new_item_ids]
        self.known += [set() for _ in new_user_ids]
        self.core.grow_factor_rows(X_, len(self.user_ids))
        self.core.grow_factor_rows(Y_, len(self.item_ids))

    def write(self, users, items, values=None):
        values = np.ones(len(users), np.float32) if values is None else values
        st = self.core.set_preferences(users, items, values)
        assert not st.any()
        for u, i in zip(users, items):
            self.known[u].add(int(i))
            self.recent[0].add(int(u))
            self.recent[1].add(int(i))

    def mark(self, side, rows):
        self.core.mark_recent(side, rows)
        self.recent[side].update(int(r) for r in rows)

    def generation(self):
        """the live generation as the oracle's dicts, in row order, with the vectors as the device holds them"""
        X, Y = self.core.get_factors(X_), self.core.get_factors(Y_)
        return {"X": {u: X[r] for r, u in enumerate(self.user_ids)}, "Y": {i: Y[r] for r, i in enumerate(self.item_ids)},
                "known": {u: {self.item_ids[i] for i in self.known[r]} for r, u in enumerate(self.user_ids)},
                "item_tags": {self.user_ids[r] for r in self.tag_users}, "user_tags": {self.item_ids[r] for r in self.tag_items}}

    def close(self):
        self.core.close()


def new_model(k, user_ids, item_ids, seed, item_tags=(), user_tags=(), max_known=10, known=None):
    rng = np.random.default_rng(seed)
    user_ids, item_ids = [int(u) for u in user_ids], [int(i) for i in item_ids]
    if known is None:
        known = [set(rng.choice(len(item_ids), int(rng.integers(0, min(max_known, len(item_ids)) + 1)), replace=False).tolist()) for _ in user_ids]
    return {"user_ids": user_ids, "item_ids": item_ids, "X": factors(rng, len(user_ids), k), "Y": factors(rng, len(item_ids), k),
            "known_rows": known, "item_tags": set(item_tags), "user_tags": set(user_tags)}


def expected(live, new, keep=False):
    gen = live.generation()
    glo.load_model(gen, {u: new["X"][r] for r, u in enumerate(new["user_ids"])}, {i: new["Y"][r] for r, i in enumerate(new["item_ids"])},
                   {u: {new["item_ids"][i] for i in new["known_rows"][r]} for r, u in enumerate(new["user_ids"])},
                   new["item_tags"], new["user_tags"], {live.user_ids[r] for r in live.recent[0]}, {live.item_ids[r] for r in live.recent[1]},
                   remove_not_updated_data=not keep)
    return glo.dense(gen, live.user_ids, live.item_ids, new["user_ids"], new["item_ids"])


def load(live, new, keep=False, device=False, recompute_solvers=False):
    """the load on the live handle, checked against the oracle's maps, ids and counts; the mirror follows.  Returns (the
    oracle's dense merged model, the result dict)."""
    d = expected(live, new, keep)
    recent = [sorted(live.recent[0]), sorted(live.recent[1])]
    cur = [np.array(live.user_ids, np.int64), np.array(live.item_ids, np.int64)]
    args = [np.array(new["user_ids"], np.int64), np.array(new["item_ids"], np.int64), new["X"], new["Y"]]
    known = csr(new["known_rows"])
    tags = [np.array(sorted(new["item_tags"]), np.int64), np.array(sorted(new["user_tags"]), np.int64)]
    if device:
        import torch
        args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
        known = tuple(torch.from_numpy(a).cuda() for a in known)
        tags = [torch.from_numpy(a).cuda() for a in tags]
    res, ids, maps = live.core.load_generation(cur[0], cur[1], *args, new_known=known, item_tag_ids=tags[0], user_tag_ids=tags[1],
                                               keep_not_updated=keep, recompute_solvers=recompute_solvers)
    flags = _lib.GENERATION_KEEP_NOT_UPDATED if keep else 0
    for s, (want_ids, want_map) in enumerate(((d["user_ids"], d["user_map"]), (d["item_ids"], d["item_map"]))):
        host_map, counts = generation_join_host(cur[s], args[s].cpu().numpy() if device else args[s], recent[s], flags)
        assert np.array_equal(maps[s], host_map) and np.array_equal(maps[s], want_map)
        assert np.array_equal(ids[s], want_ids)
        assert [res["n_merged"][s], res["n_updated"][s], res["n_kept"][s], res["n_pruned"][s]] == \
            [counts["n_merged"], counts["n_updated"], counts["n_kept"], counts["n_pruned"]]
    assert res["n_known_dropped"] == d["n_known_dropped"] and res["n_tag_ids_without_row"] == d["n_tag_ids_without_row"]
    live.user_ids, live.item_ids = d["user_ids"].tolist(), d["item_ids"].tolist()
    ptr, idx = d["known"]
    live.known = [set(idx[ptr[r]:ptr[r + 1]].tolist()) for r in range(len(live.user_ids))]
    live.tag_users, live.tag_items = d["tag_users"].tolist(), d["tag_items"].tolist()
    live.recent = (set(), set())
    return d, res


def twin_of(d, k, solvers=None):
    t = pkg.ALSCore(k)
    t.set_factor_rows(X_, len(d["user_ids"]))
    t.set_factor_rows(Y_, len(d["item_ids"]))
    ptr, idx = d["known"]
    t.set_matrix(X_, ptr, idx, np.ones(len(idx), np.float32))
    t.set_factors(X_, d["X"])
    t.set_factors(Y_, d["Y"])
    t.set_known_items(ptr, idx)
    t.set_tag_items(d["tag_items"])
    t.set_tag_users(d["tag_users"])
    if solvers:
        t.set_foldin_solver(X_, solvers[0])
        t.set_foldin_solver(Y_, solvers[1])
    return t


def same_answers(a, b):
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


def compare(core, twin, d, users=None, seed=3):
    nu, ni = len(d["user_ids"]), len(d["item_ids"])
    rng = np.random.default_rng(seed)
    for side, want in ((X_, d["X"]), (Y_, d["Y"])):
        got = core.get_factors(side)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(twin.get_factors(side)), bits(want))
        assert core.factor_digest(side) == twin.factor_digest(side) == factor_digest_host(want)
    users = np.arange(nu) if users is None else np.asarray(users)
    how_many = min(10, ni)
    for consider in (False, True):
        same_answers(core.recommend(users, how_many, consider_known_items=consider), twin.recommend(users, how_many, consider_known_items=consider))
    items = rng.permutation(ni)[:32]
    same_answers(core.most_similar_items(items, how_many), twin.most_similar_items(items, how_many))
    bu, bi = rng.choice(users, 32), rng.integers(0, ni, 32)
    same_answers(core.recommended_because(bu, bi, 5), twin.recommended_because(bu, bi, 5))
    a, b = core.most_popular_items(min(20, ni)), twin.most_popular_items(min(20, ni))
    same_answers(a[:2], b[:2])
    assert a[2] == b[2]
    assert core.tag_item_count() == twin.tag_item_count() == len(d["tag_items"])
    assert core.tag_user_count() == twin.tag_user_count() == len(d["tag_users"])


def base_ids(seed=1):
    """300 live / 260 new users, 200 live / 180 new items, partial overlap, shuffled in the new model"""
    rng = np.random.default_rng(seed)
    pool = rng.permutation(np.unique(rng.integers(-10**15, 10**15, 2000, dtype=np.int64)))
    lu, li = pool[:300], pool[300:500]
    nu = rng.permutation(np.concatenate([lu[40:220], pool[500:580]]))
    ni = rng.permutation(np.concatenate([li[30:150], pool[600:660]]))
    return lu, li, nu, ni


@pytest.mark.parametrize("k", [1, 30, 64, 128])
@pytest.mark.parametrize("device", [False, True])
def test_base_shape_against_the_twin(k, device):
    lu, li, nu, ni = base_ids()
    live = Live(k, lu, li, seed=k, solvers=True)
    live.set_tags([5, 10, 41, 60, 250, 299], [3, 10, 31, 50, 160, 199])             # 10, 60 / 10, 50: live tags that are not recent
    live.write([0, 5, 41, 100, 250, 299, 299], [3, 31, 40, 160, 199, 0, 7])          # kept and updated rows, tags among them
    live.mark(X_, [1, 2, 39, 220, 221])
    live.mark(Y_, [29, 150, 151])
    assert np.array_equal(live.core.get_recent(X_), sorted(live.recent[0])) and np.array_equal(live.core.get_recent(Y_), sorted(live.recent[1]))
    new = new_model(k, nu, ni, seed=100 + k, item_tags=[int(nu[0]), int(lu[250]), 12345], user_tags=[int(ni[1]), int(li[199]), 777])
    before_updated = live.core.get_factors(X_)[41].copy()
    d, res = load(live, new, device=device)
    assert res["n_kept"][0] > 0 and res["n_pruned"][0] > 0 and res["n_updated"][0] == 180 and res["n_known_dropped"] > 0
    assert res["n_tag_ids_without_row"] == 2
    # a row written recently that the new model also has ends with the new model's vector
    r41 = int(d["user_map"][41])
    assert 0 <= r41 < 260 and np.array_equal(bits(live.core.get_factors(X_)[r41]), bits(new["X"][r41]))
    assert not np.array_equal(bits(before_updated), bits(new["X"][r41]))
    twin = twin_of(d, k, live.solvers)
    compare(live.core, twin, d)
    assert len(live.core.get_recent(X_)) == 0 and len(live.core.get_recent(Y_)) == 0
    # the same writes on a kept row, a new row and a grown row of both
    kept_user, new_user = int(d["user_map"][0]), 0
    assert kept_user >= 260
    for c in (live.core, twin):
        c.grow_factor_rows(X_, len(d["user_ids"]) + 1)
        c.set_preferences([kept_user, new_user, len(d["user_ids"]), kept_user], [0, 1, 2, int(d["item_map"][29])], np.array([1.0, 2.0, 0.5, 3.0], np.float32))
    for side in (X_, Y_):
        assert np.array_equal(bits(live.core.get_factors(side)), bits(twin.get_factors(side)))
    users = [kept_user, new_user, len(d["user_ids"])]
    same_answers(live.core.recommend(users, 10), twin.recommend(users, 10))
    same_answers(live.core.most_popular_items(20)[:2], twin.most_popular_items(20)[:2])
    twin.close()
    live.close()


def test_grown_rows_survive_a_model_built_without_them():
    """The motivating scenario: three users and three items appear on the live handle while the rebuild runs."""
    k = 30
    lu, li, _, _ = base_ids(seed=2)
    live = Live(k, lu[:120], li[:90], seed=7, solvers=True)
    new = new_model(k, lu[:120], li[:90], seed=8)                       # built from the ids the handle had when the rebuild began
    live.grow([900001, 900002, 900003], [800001, 800002, 800003])
    live.write([120, 121, 122, 5, 6, 7, 120, 121], [3, 4, 5, 90, 91, 92, 90, 91], np.array([1.0, 2.0, 1.5, 1.0, 0.5, 1.0, 2.0, 1.0], np.float32))
    grown_x, grown_y = live.core.get_factors(X_)[120:123].copy(), live.core.get_factors(Y_)[90:93].copy()
    assert (np.abs(grown_x).sum(axis=1) > 0).all() and (np.abs(grown_y).sum(axis=1) > 0).all()
    d, res = load(live, new)
    assert res["n_kept"] == [3, 3] and res["n_pruned"] == [0, 0] and res["n_updated"] == [120, 90] and res["n_known_dropped"] == 0
    assert d["user_ids"][120:].tolist() == [900001, 900002, 900003] and d["item_ids"][90:].tolist() == [800001, 800002, 800003]
    assert np.array_equal(bits(live.core.get_factors(X_)[120:123]), bits(grown_x))
    assert np.array_equal(bits(live.core.get_factors(Y_)[90:93]), bits(grown_y))
    ptr, idx = d["known"]
    assert idx[ptr[120]:ptr[121]].tolist() == [3, 90] and idx[ptr[121]:ptr[122]].tolist() == [4, 91] and idx[ptr[122]:ptr[123]].tolist() == [5]
    twin = twin_of(d, k, live.solvers)
    compare(live.core, twin, d)
    idx10, _, cnt = live.core.recommend([120, 121, 122], 10)                # the three users are recommended to,
    assert (cnt == 10).all() and not np.isin(idx10[0], [3, 90]).any()       # without their known items,
    cons, _, _ = live.core.recommend(np.arange(123), 93, consider_known_items=True)
    assert all(np.isin([90, 91, 92], row).all() for row in cons)            # and the three items are candidates
    twin.close()
    live.close()


def test_two_hundred_thousand_rows_cross_every_scan_tile():
    k, n = 2, 200003
    rng = np.random.default_rng(5)
    lu = rng.permutation(np.arange(10**6, 10**6 + n, dtype=np.int64))
    li = np.arange(50, dtype=np.int64)
    live = Live(k, lu, li, seed=9, known=[{int(i)} for i in rng.integers(0, 50, n)])
    nu = rng.permutation(np.concatenate([lu[::7], np.arange(5 * 10**6, 5 * 10**6 + 1000, dtype=np.int64)]))
    kept = np.unique(np.concatenate([np.arange(0, n, 997), [1, 2047, 2048, 2049, 4095, 4096, n - 2, n - 1], rng.integers(0, n, 3000)]))
    live.mark(X_, kept)
    live.mark(Y_, [49])
    new = new_model(k, nu, li[:40], seed=10, known=[{int(i)} for i in rng.integers(0, 40, len(nu))])
    d, res = load(live, new, device=True)
    assert res["n_kept"][0] == len(set(kept.tolist()) - set(range(0, n, 7))) and res["n_kept"][1] == 1 and res["n_pruned"][1] == 9
    twin = twin_of(d, k)
    compare(live.core, twin, d, users=np.concatenate([np.arange(0, len(d["user_ids"]), 431), np.arange(len(d["user_ids"]) - 40, len(d["user_ids"]))]))
    twin.close()
    live.close()


def test_colliding_and_extreme_ids_on_the_device():
    k = 4
    col = colliding_ids(300, 300)
    others = colliding_ids(420, 300, seed=9)
    others = others[~np.isin(others, col)][:100]
    rng = np.random.default_rng(12)
    lu = rng.permutation(np.concatenate([col[:150], others, np.array(EXTREME, np.int64)]))
    li = np.array(EXTREME + [5, 6, 7], np.int64)
    live = Live(k, lu, li, seed=13)
    live.mark(X_, rng.permutation(len(lu))[:120])
    live.mark(Y_, [0, 3, 6])
    new = new_model(k, col, np.array([0, 9, EXTREME[0], 5], np.int64), seed=14)
    d, res = load(live, new)
    assert res["n_updated"] == [150, 3]
    twin = twin_of(d, k)
    compare(live.core, twin, d)
    twin.close()
    live.close()


@pytest.mark.parametrize("case", ["nothing_kept", "everything_kept", "keep_not_updated"])
def test_nothing_kept_everything_kept_and_the_keep_flag(case):
    k = 30
    lu, li, nu, ni = base_ids(seed=3)
    live = Live(k, lu[:150], li[:100], seed=21)
    live.set_tags([3, 7], [2, 9])
    if case == "nothing_kept":
        new = new_model(k, nu, ni, seed=22)
    elif case == "everything_kept":
        live.mark(X_, np.arange(150))
        live.mark(Y_, np.arange(100))
        new = new_model(k, np.arange(1, 60, dtype=np.int64), np.arange(1, 50, dtype=np.int64), seed=23)      # disjoint ids
    else:
        live.mark(X_, [0, 1])
        new = new_model(k, nu, ni, seed=24, item_tags=[int(nu[3])])
    d, res = load(live, new, keep=case == "keep_not_updated")
    if case == "nothing_kept":
        assert res["n_kept"] == [0, 0] and len(d["tag_users"]) == 0
    elif case == "everything_kept":
        assert res["n_kept"] == [150, 100] and res["n_updated"] == [0, 0] and res["n_known_dropped"] == 0 and len(d["tag_users"]) == 2
    else:
        assert res["n_pruned"] == [0, 0] and res["n_kept"][0] == 150 - res["n_updated"][0] and len(d["tag_users"]) == 3
    twin = twin_of(d, k)
    compare(live.core, twin, d)
    twin.close()
    live.close()


def answers(core, users, n_items):
    return (core.recommend(users, 10), core.recommend(users, 10, consider_known_items=True), core.most_similar_items([0, 1, 2], 5),
            core.most_popular_items(10)[:2], core.get_factors(X_), core.get_factors(Y_), core.factor_digest(X_), core.get_recent(X_))


def test_a_duplicate_id_fails_and_changes_nothing():
    k = 30
    lu, li, nu, ni = base_ids(seed=4)
    live = Live(k, lu[:100], li[:80], seed=31, solvers=True)
    live.set_tags([4], [6])
    live.write([1, 2], [3, 4])
    users = np.arange(100)
    before = answers(live.core, users, 80)
    new = new_model(k, nu[:50], ni[:40], seed=32)
    cur = [np.array(live.user_ids, np.int64), np.array(live.item_ids, np.int64)]
    known = csr(new["known_rows"])
    bad_new = np.array(new["user_ids"], np.int64)
    bad_new[17] = bad_new[3]
    bad_cur = cur[1].copy()
    bad_cur[79] = bad_cur[0]
    def unchanged():
        after = answers(live.core, users, 80)
        for a, b in zip(before, after):
            if isinstance(a, tuple):
                same_answers(a, b)
            else:
                assert np.array_equal(np.asarray(a), np.asarray(b))

    for cu, ci, n_u in ((cur[0], cur[1], bad_new), (cur[0], bad_cur, np.array(new["user_ids"], np.int64)),
                        (cur[0][:99], cur[1], np.array(new["user_ids"], np.int64))):          # the last: not one id per live row
        with pytest.raises(MalsError) as ei:
            live.core.load_generation(cu, ci, n_u, np.array(new["item_ids"], np.int64), new["X"], new["Y"], new_known=known)
        assert ei.value.status == _lib.INVALID_ARG
        unchanged()
    # a model of another feature count (the binding always passes the handle's: this one goes through the C struct)
    wide = [np.zeros((50, k + 1), np.float32), np.zeros((40, k + 1), np.float32)]
    new_ids = [np.array(new["user_ids"], np.int64), np.array(new["item_ids"], np.int64)]
    L = _lib.GenerationLoad()
    L.struct_size, L.features, L.cur_mem_kind, L.new_mem_kind = ctypes.sizeof(_lib.GenerationLoad), k + 1, _lib.MEM_HOST, _lib.MEM_HOST
    for s in range(2):
        L.cur_ids[s], L.n_cur[s] = cur[s].ctypes.data_as(ctypes.c_void_p), len(cur[s])
        L.new_ids[s], L.n_new[s] = new_ids[s].ctypes.data_as(ctypes.c_void_p), len(new_ids[s])
        L.new_rows[s] = wide[s].ctypes.data_as(ctypes.c_void_p)
    L.new_known_ptr, L.new_known_idx = known[0].ctypes.data_as(ctypes.c_void_p), known[1].ctypes.data_as(ctypes.c_void_p)
    R = _lib.GenerationResult()
    R.struct_size = ctypes.sizeof(_lib.GenerationResult)
    assert live.core._L.mals_load_generation(live.core._h, ctypes.byref(L), ctypes.byref(R)) == _lib.INVALID_ARG
    assert b"features" in live.core._L.mals_last_error(live.core._h)
    unchanged()
    L.struct_size -= 8                                                       # and a struct of another size
    assert live.core._L.mals_load_generation(live.core._h, ctypes.byref(L), ctypes.byref(R)) == _lib.INVALID_ARG
    unchanged()
    with pytest.raises(MalsError) as ei:                                     # the new model's known items are needed
        live.core.load_generation(cur[0], cur[1], np.array(new["user_ids"], np.int64), np.array(new["item_ids"], np.int64), new["X"], new["Y"])
    assert ei.value.status == _lib.INVALID_ARG
    d, _ = load(live, new)                                                   # and the handle still loads
    twin = twin_of(d, k)
    compare(live.core, twin, d)
    twin.close()
    live.close()


def test_a_second_load_prunes_what_the_first_kept():
    k = 30
    lu, li, nu, ni = base_ids(seed=6)
    live = Live(k, lu[:150], li[:100], seed=41, solvers=True)
    live.write([0, 1, 2], [0, 1, 2])                                         # rows the new model does not have
    new = new_model(k, nu, ni, seed=42)
    d1, res1 = load(live, new)
    assert res1["n_kept"] == [3, 3] and d1["user_ids"][260:].tolist() == [int(u) for u in lu[:3]]
    assert len(live.core.get_recent(X_)) == 0 and len(live.core.get_recent(Y_)) == 0     # :97-98
    d2, res2 = load(live, new)                                               # nothing written in between
    assert res2["n_kept"] == [0, 0] and res2["n_pruned"] == [3, 3] and res2["n_updated"] == [260, 180]
    assert d2["user_map"][260:].tolist() == [-1, -1, -1]
    twin = twin_of(d2, k)
    compare(live.core, twin, d2)
    twin.close()
    live.close()


def test_recomputed_solvers_are_those_of_the_merged_replicas():
    k = 30
    lu, li, nu, ni = base_ids(seed=6)
    live = Live(k, lu[:150], li[:100], seed=43, solvers=True)
    live.write([0, 1], [0, 1])
    new = new_model(k, nu, ni, seed=44)
    d, res = load(live, new, recompute_solvers=True)
    assert res["solver_status"] == _lib.OK and res["n_kept"] == [2, 2]
    twin = twin_of(d, k)
    for side in (X_, Y_):
        s, _ = twin.recompute_solver(side)
        twin.set_foldin_solver(side, s)
    for c in (live.core, twin):                                              # a kept row, a new row
        c.set_preferences([261, 0], [0, 181], np.array([1.0, 2.0], np.float32))
    for side in (X_, Y_):
        assert np.array_equal(bits(live.core.get_factors(side)), bits(twin.get_factors(side)))
    assert np.array_equal(live.core.get_recent(X_), [0, 261]) and np.array_equal(live.core.get_recent(Y_), [0, 181])
    twin.close()
    live.close()


def test_readers_see_the_old_generation_or_the_new_one():
    k = 30
    lu, li, nu, ni = base_ids(seed=8)
    live = Live(k, lu, li, seed=51)
    live.write([0, 1, 2, 3], [0, 1, 2, 3])
    new = new_model(k, nu, ni, seed=52)
    users = [np.array([0, 1, 2, 3]), np.array([10, 50]), np.array([100, 200, 259]), np.array([7])]
    before = [live.core.recommend(u, 10) for u in users]
    got = [[] for _ in users]
    errors = []
    started = threading.Barrier(len(users) + 1)
    loaded = threading.Event()

    def reader(t):
        # at least 300 calls, and 20 more once the load has returned; 5000 at the most: the thread ends on its own
        try:
            started.wait()
            after_load = 0
            while len(got[t]) < 5000 and (len(got[t]) < 300 or after_load < 20):
                after_load += loaded.is_set()
                got[t].append(live.core.recommend(users[t], 10))
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=reader, args=(t,), daemon=True) for t in range(len(users))]   # a hung call must not hold the run
    for th in threads:
        th.start()
    started.wait()
    try:
        d, _ = load(live, new)
    finally:
        loaded.set()
    for th in threads:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in threads) and not errors, errors
    after = [live.core.recommend(u, 10) for u in users]
    n_old = n_new = 0
    for t in range(len(users)):
        for ans in got[t]:
            is_old = all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(ans, before[t]))
            is_new = all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(ans, after[t]))
            assert is_old or is_new
            n_old += is_old
            n_new += is_new
    assert n_new >= 20 * len(users)
    twin = twin_of(d, k)
    compare(live.core, twin, d)
    twin.close()
    live.close()


def test_recent_rows_go_with_a_replaced_replica():
    """mals_set_factor_rows gives a side other rows: what was written to the old ones is forgotten, and mals_get_recent never
    reports a row the replica does not have."""
    lu, li, _, _ = base_ids(seed=9)
    live = Live(4, lu[:60], li[:40], seed=61)
    live.write([3, 59], [2, 39])
    assert live.core.get_recent(X_).tolist() == [3, 59] and live.core.get_recent(Y_).tolist() == [2, 39]
    live.core.set_factor_rows(X_, 20)
    assert live.core.get_recent(X_).tolist() == [] and live.core.get_recent(Y_).tolist() == [2, 39]
    live.core.mark_recent(X_, [19])
    with pytest.raises(MalsError):
        live.core.mark_recent(X_, [20])
    assert live.core.get_recent(X_).tolist() == [19]
    live.close()
