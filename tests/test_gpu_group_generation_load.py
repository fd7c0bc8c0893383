"""mals_group_load_generation (include/myrrix_als.h, "loading a new generation into a group") against ONE handle holding the
whole live model and given the same history: the same writes, removals, grown rows and mark_recent calls go to a W-member
group (W members on device 0 with the peer-copy backend, or the one-rank RCCL group) and to an ALSCore, the same new model is
loaded into both, and the group must then hold and answer bit for bit what the handle does.  The handle's own load is held to
tests/generation_load_oracle.py by tests/test_gpu_generation_load.py, whose helpers are used here.  The load copies and
re-indexes, it computes nothing in floating point: every comparison is for equality.

The item maps of every case are not monotone (the new model's ids are shuffled), so a kept user's base row, which the group
leaves in base-row order (csrc/generation_group_kernels.h), is not ascending after the load: a reader that assumed ascending
rows would answer otherwise than the handle, whose kept sets are sorted."""
import threading

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from myrrix_recommender_amd.core import MalsError, factor_digest_host
from myrrix_recommender_amd.group import generation_plan_host, plan_shards
from tests import generation_load_oracle as glo
from tests.test_gpu_generation_load import Live, base_ids, bits, csr, factors, load, new_model, same_answers

pytestmark = pytest.mark.gpu
X_, Y_ = pkg.SIDE_X, pkg.SIDE_Y


class Both:
    """The single handle (Live: the handle and its mirror in Python) and a group with the same model and the same history."""

    def __init__(self, W, k, user_ids, item_ids, seed, rccl=False, known=None, max_known=12):
        self.W, self.k = W, k
        self.live = Live(k, user_ids, item_ids, seed, solvers=True, max_known=max_known, known=known)
        c = self.live.core
        if rccl:
            assert W == 1
            self.g = pkg.GroupALS.from_torch_distributed(k, 0, world=1, rank=0, one_rank_communicator=True)
        else:
            self.g = pkg.GroupALS.single_process(k, [0] * W, backend=_lib.GROUP_PEER_COPY)
        g = self.g
        g.set_factor_rows(X_, len(self.live.user_ids))
        g.set_factor_rows(Y_, len(self.live.item_ids))
        g.set_factors(X_, c.get_factors(X_))
        g.set_factors(Y_, c.get_factors(Y_))
        ptr, idx = csr(self.live.known)
        g.set_matrix(X_, ptr, idx, np.ones(len(idx), np.float32))
        g.set_foldin_solver(X_, self.live.solvers[0])
        g.set_foldin_solver(Y_, self.live.solvers[1])

    def set_tags(self, tag_users, tag_items):
        self.live.set_tags(tag_users, tag_items)
        self.g.set_tag_users(tag_users)
        for m in range(self.W):
            self.g.local(m)[0].set_tag_items(tag_items)

    def grow(self, new_user_ids, new_item_ids):
        self.live.grow(new_user_ids, new_item_ids)
        self.g.grow_factor_rows(X_, len(self.live.user_ids))
        self.g.grow_factor_rows(Y_, len(self.live.item_ids))

    def write(self, users, items, values=None):
        values = np.ones(len(users), np.float32) if values is None else np.asarray(values, np.float32)
        self.live.write(users, items, values)
        assert not self.g.set_preferences(users, items, values).any()

    def remove(self, users, items):
        a = self.live.core.remove_preferences(users, items)
        b = self.g.remove_preferences(users, items)
        assert np.array_equal(a, b)
        for u, i in zip(users, items):
            self.live.known[u].discard(int(i))
            self.live.recent[0].add(int(u))
            self.live.recent[1].add(int(i))
        return a

    def mark(self, side, rows):
        self.live.mark(side, rows)
        self.g.mark_recent(side, rows)

    def check_recent(self):
        for side in (X_, Y_):
            want = sorted(self.live.recent[side])
            assert np.array_equal(self.g.get_recent(side), want) and np.array_equal(self.live.core.get_recent(side), want)

    def load(self, new, keep=False, device=False, recompute_solvers=False):
        """The same load on the group and on the handle (which tests.test_gpu_generation_load.load holds to the oracle);
        ids, maps and every count of the group's result against the handle's.  Returns (the oracle's merged model, the
        handle's result, the old bounds of the group)."""
        cur = [np.array(self.live.user_ids, np.int64), np.array(self.live.item_ids, np.int64)]
        args = [np.array(new["user_ids"], np.int64), np.array(new["item_ids"], np.int64), new["X"], new["Y"]]
        known = csr(new["known_rows"])
        tags = [np.array(sorted(new["item_tags"]), np.int64), np.array(sorted(new["user_tags"]), np.int64)]
        if device:
            import torch
            args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
            known = tuple(torch.from_numpy(a).cuda() for a in known)
            tags = [torch.from_numpy(a).cuda() for a in tags]
        self.check_recent()
        old_bounds = self.g.bounds(X_).copy()
        gres, gids, gmaps = self.g.load_generation(cur[0], cur[1], *args, new_known=known, item_tag_ids=tags[0], user_tag_ids=tags[1],
                                                   keep_not_updated=keep, recompute_solvers=recompute_solvers)
        d, res = load(self.live, new, keep=keep, device=device, recompute_solvers=recompute_solvers)
        for s, (want_ids, want_map) in enumerate(((d["user_ids"], d["user_map"]), (d["item_ids"], d["item_map"]))):
            assert np.array_equal(gids[s], want_ids) and np.array_equal(gmaps[s], want_map)
        for name in ("n_merged", "n_updated", "n_kept", "n_pruned", "n_known_dropped", "n_tag_ids_without_row", "solver_status"):
            assert gres[name] == res[name], (name, gres[name], res[name])
        assert gres["n_known_dropped"] == d["n_known_dropped"]
        return d, res, old_bounds

    def compare(self, d, seed=5, users=None):
        """Everything the issue lists after a load: replicas, bounds, the recent bits, and the readers' answers for every
        merged user against the handle's."""
        g, c, k = self.g, self.live.core, self.k
        nu, ni = len(d["user_ids"]), len(d["item_ids"])
        for side, want in ((X_, d["X"]), (Y_, d["Y"])):
            out, equal = g.replica_digest(side)
            assert equal and len(out) == self.W and int(out[0]) == factor_digest_host(want) == c.factor_digest(side)
        bx = g.bounds(X_)
        assert np.array_equal(bx, plan_shards(d["known"][0], self.W, k)) and bx[-1] == nu
        assert np.array_equal(g.bounds(Y_), plan_shards(np.zeros(ni + 1, np.int64), self.W, k))
        assert len(g.get_recent(X_)) == 0 and len(g.get_recent(Y_)) == 0
        rng = np.random.default_rng(seed)
        users = np.arange(nu) if users is None else np.asarray(users)
        how_many = min(10, ni)
        for consider in (False, True):
            same_answers(g.recommend(users, how_many, consider_known_items=consider), c.recommend(users, how_many, consider_known_items=consider))
        bu, bi = rng.choice(users, 32), rng.integers(0, ni, 32)
        same_answers(g.recommended_because(bu, bi, 5), c.recommended_because(bu, bi, 5))
        a, b = g.most_popular_items(min(20, ni)), c.most_popular_items(min(20, ni))
        same_answers(a[:2], b[:2])
        assert a[2] == b[2]
        eu, ei = rng.integers(0, nu, 64), rng.integers(0, ni, 64)
        same_answers([g.estimate_preferences(eu, ei)], [c.estimate_preferences(eu, ei)])
        items = rng.permutation(ni)[:16]
        same_answers(g.most_similar_items(items, how_many), c.most_similar_items(items, how_many))

    def close(self):
        self.g.close()
        self.live.close()


def history(b, rng, n_writes, hot_item, empty_users):
    """n_writes writes in four batches with a hot item among them, then removals that empty `empty_users`"""
    nu, ni = len(b.live.user_ids), len(b.live.item_ids)
    active_users, active_items = rng.choice(nu, nu // 2, replace=False), rng.choice(ni, ni // 2, replace=False)   # the rest is not recent
    for _ in range(4):
        n = n_writes // 4
        users = rng.choice(active_users, n)
        items = np.where(rng.random(n) < 0.2, hot_item, rng.choice(active_items, n))
        b.write(users.tolist(), items.tolist(), (rng.random(n) * 2 + 0.25).astype(np.float32))
    removed = []
    for u in empty_users:
        items = sorted(b.live.known[u])
        if items:
            removed += b.remove([u] * len(items), items).tolist()
    assert sorted(removed) == sorted(u for u in empty_users)
    b.remove([1, 2], [0, 1])   # (a removal that empties nobody, of items the users may not know)


# ---- 4. the base shape ---------------------------------------------------------------------------------------------------
def base_shape(W, k, device, rccl=False):
    rng = np.random.default_rng(1000 * W + k)
    lu, li, nu, ni = base_ids()
    b = Both(W, k, lu, li, seed=k, rccl=rccl)
    b.set_tags([5, 10, 41, 60, 250, 299], [3, 10, 31, 50, 160, 199])
    b.grow([900001, 900002, 900003], [800001, 800002])
    # the emptied users have known items to lose (the grown ones get theirs first)
    b.write([300, 301, 302, 7], [200, 201, 5, 200], [1.0, 2.0, 0.5, 1.0])
    empty = [u for u in (7, 230, 301) if b.live.known[u]]
    history(b, rng, 2000, hot_item=17, empty_users=empty)
    b.mark(X_, [1, 2, 39, 220, 221, 302])
    b.mark(Y_, [29, 150, 151, 201])
    new = new_model(k, nu, ni, seed=100 + k, item_tags=[int(nu[0]), int(lu[250]), 12345], user_tags=[int(ni[1]), int(li[199]), 777])
    d, res, _ = b.load(new, device=device)
    assert res["n_kept"][0] > 0 and res["n_pruned"][0] > 0 and res["n_updated"][0] == 180 and res["n_known_dropped"] > 0
    b.compare(d)
    # a second batch of group writes and a second load: the recent bits were cleared and are recorded again, and what the first
    # load kept is pruned now unless it was written again
    n_users, n_items = len(d["user_ids"]), len(d["item_ids"])
    kept_users = [r for r in range(260, n_users)]
    assert len(kept_users) > 4
    rewritten = kept_users[:2]
    b.write(rewritten + [0, 1], [3, int(d["item_map"][29]) if d["item_map"][29] >= 0 else 4, 5, 6], [1.0, 0.5, 2.0, 1.0])
    b.remove([rewritten[0]], [3])
    b.check_recent()
    ids_u, ids_i = d["user_ids"], d["item_ids"]
    nu2 = rng.permutation(ids_u[:200])
    ni2 = rng.permutation(np.concatenate([ids_i[:150], [700001, 700002]]))
    new2 = new_model(k, nu2, ni2, seed=200 + k, item_tags=[int(nu2[3])], user_tags=[int(ni2[2])])
    d2, res2, _ = b.load(new2, device=device)
    assert n_items > 150 and res2["n_kept"][0] == len(rewritten) and res2["n_pruned"][0] == n_users - 200 - len(rewritten)
    b.compare(d2)
    b.close()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("k", [1, 30, 64, 128])
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_base_shape(W, k, device):
    base_shape(W, k, device)


def test_base_shape_on_the_one_rank_rccl_group():
    base_shape(1, 30, False, rccl=True)


# ---- 5. edges of the known-item kernels ------------------------------------------------------------------------------------
def edge_ids(n_users, n_items, seed=3):
    rng = np.random.default_rng(seed)
    pool = rng.permutation(np.unique(rng.integers(-10**15, 10**15, 2 * (n_users + n_items) + 100, dtype=np.int64)))
    return pool[:n_users], pool[n_users:n_users + n_items], pool[n_users + n_items:]


def edge_known(rng, n_users, n_items, sizes):
    known = []
    for u in range(n_users):
        n = sizes[u] if u < len(sizes) else int(rng.integers(0, 6))
        known.append(set(rng.choice(n_items, n, replace=False).tolist()))
    return known


@pytest.mark.parametrize("case", ["row_lengths", "all_pruned", "member_without_kept", "two_new_users", "no_new_users", "scan_tiles"])
def test_known_item_kernel_edges(case):
    W, k = 3, 4
    rng = np.random.default_rng(11)
    n_users, n_items = (5200, 300) if case == "scan_tiles" else (60, 300)
    lu, li, spare = edge_ids(n_users, n_items)
    # scan_tiles: 150 heavy users in front, so that the plan gives the last old owner the 5050 light ones behind them
    sizes = [0, 1, 63, 64, 65, 200] * 3 if case != "scan_tiles" else [200] * 150
    known = edge_known(rng, n_users, n_items, sizes)
    keep = case != "all_pruned"
    if case == "all_pruned":
        # user 20 knows items 280..299 only; the new model has none of them and none is recent: every entry of its row is dropped
        known[20] = set(range(280, 300))
    b = Both(W, k, lu, li, seed=9, known=known)
    old_bounds = b.g.bounds(X_)
    new_items = rng.permutation(np.concatenate([li[:280:2], spare[:40]]))   # half the live items, shuffled: the item map is not monotone
    if case == "two_new_users":
        new_users = np.array([lu[7], spare[50]])
    elif case == "no_new_users":
        new_users = np.zeros(0, np.int64)
    elif case == "member_without_kept":
        new_users = rng.permutation(np.concatenate([lu[old_bounds[1]:old_bounds[2]], spare[60:70]]))   # every user of old member 1 is updated
    elif case == "scan_tiles":
        new_users = rng.permutation(np.concatenate([lu[:150], spare[60:70]]))      # the 5050 light users are kept, plain
    else:
        new_users = rng.permutation(np.concatenate([lu[30:], spare[60:80]]))       # users 0 .. 29 (every row length, three times) are kept
    if case == "all_pruned":
        b.mark(X_, list(range(0, 30)))      # kept because recent; nothing else is
        b.mark(Y_, [0, 1, 2])
    if case == "scan_tiles":
        assert n_users - max(150, int(old_bounds[2])) >= 5000      # 5000 kept plain users on ONE old owner: five tiles of its scan
    new = new_model(k, new_users, new_items, seed=21, max_known=8)
    d, res, _ = b.load(new, keep=keep)
    if case == "all_pruned":
        assert d["user_map"][20] >= len(new_users) and d["known"][0][d["user_map"][20] + 1] == d["known"][0][d["user_map"][20]]
        assert res["n_known_dropped"] >= 20
    if case == "member_without_kept":
        kept_rows = np.flatnonzero(d["user_map"] >= len(new_users))
        assert not ((kept_rows >= old_bounds[1]) & (kept_rows < old_bounds[2])).any() and len(kept_rows) > 0
    if case == "two_new_users":
        assert (np.diff(b.g.bounds(X_)) > 0).all() and b.g.bounds(X_)[1] >= 2     # members 1 and 2 own kept users only
    if case == "no_new_users":
        assert res["n_kept"][0] == n_users and res["n_merged"][0] == n_users
    if case == "scan_tiles":
        assert res["n_kept"][0] == 5050
    b.compare(d)
    b.close()


# ---- 6. mixed paths ------------------------------------------------------------------------------------------------------------
def test_mixed_paths_move_to_another_owner():
    W, k = 3, 8
    rng = np.random.default_rng(31)
    n_users, n_items = 90, 120
    lu, li, spare = edge_ids(n_users, n_items, seed=5)
    known = [set(rng.choice(n_items, int(rng.integers(4, 12)), replace=False).tolist()) for _ in range(n_users)]
    b = Both(W, k, lu, li, seed=4, known=known)
    old_bounds = b.g.bounds(X_)
    last = list(range(int(old_bounds[2]), n_users))        # the users of the last old owner
    assert len(last) >= 12
    added, replaced, plain = last[0:3], last[3:6], last[6:]
    b.grow([int(s) for s in spare[:3]], [int(spare[10])])
    grown = [n_users, n_users + 1, n_users + 2]
    b.write(added + grown + [grown[0]], [1, 2, 3, 4, 5, 120, 7], [1.0, 0.5, 2.0, 1.0, 1.5, 1.0, 0.5])
    for u in replaced:
        b.remove([u], [sorted(b.live.known[u])[0]])
    # the new model: every user of old members 0 and 1, with hardly any known items -- the kept tail is heavy, so the new owners'
    # cuts fall inside it
    new_users = rng.permutation(lu[:int(old_bounds[2])])
    new_items = rng.permutation(np.concatenate([li[::2], spare[20:30], [spare[10]]]))
    new = new_model(k, new_users, new_items, seed=41, max_known=1)
    d, res, old = b.load(new, keep=True)
    n_new = len(new_users)
    kept_rows = np.flatnonzero(d["user_map"] >= n_new)
    assert np.array_equal(d["user_map"][kept_rows], n_new + np.arange(len(kept_rows)))
    kptr = d["known"][0]
    sizes = np.diff(kptr)[n_new:]
    bounds, moves = generation_plan_host(W, k, csr(new["known_rows"])[0], sizes, kept_rows, old)
    assert np.array_equal(bounds, b.g.bounds(X_))
    assert moves[2, 0, 1] - moves[2, 0, 0] + moves[2, 1, 1] - moves[2, 1, 0] > 0      # users of old member 2 moved to member 0 or 1

    def owner(u):
        return min(W - 1, int(np.searchsorted(bounds, u, side="right")) - 1)

    moved = {kind: [u for u in rows if owner(int(d["user_map"][u])) != 2] for kind, rows in (("added", added), ("replaced", replaced), ("plain", plain))}
    assert moved["plain"] and (moved["added"] or moved["replaced"]), moved
    b.compare(d)
    mixed = [int(d["user_map"][u]) for u in added + replaced + grown + plain]
    b.compare(d, users=mixed, seed=6)
    # the moved users are written again on their new owners, as on the handle
    b.write([mixed[0], mixed[3], mixed[-1]], [0, 1, 2], [1.0, 2.0, 0.5])
    b.remove([mixed[1]], [sorted(b.live.known[mixed[1]])[0]])
    same_answers(b.g.recommend(mixed, 10), b.live.core.recommend(mixed, 10))
    same_answers(b.g.most_popular_items(20)[:2], b.live.core.most_popular_items(20)[:2])
    b.close()


# ---- 7. no known items anywhere ------------------------------------------------------------------------------------------------
def test_no_known_items_cuts_by_rows():
    W, k = 3, 6
    rng = np.random.default_rng(51)
    lu, li, spare = edge_ids(50, 40, seed=8)
    X, Y = factors(rng, 50, k), factors(rng, 40, k)
    g = pkg.GroupALS.single_process(k, [0] * W, backend=_lib.GROUP_PEER_COPY)
    g.set_factor_rows(X_, 50)
    g.set_factor_rows(Y_, 40)
    g.set_factors(X_, X)
    g.set_factors(Y_, Y)
    g.mark_recent(X_, [3, 4, 49])
    g.mark_recent(Y_, [39])
    assert g.get_recent(X_).tolist() == [3, 4, 49]
    new_users = rng.permutation(np.concatenate([lu[10:40], spare[:7]]))
    new_items = rng.permutation(np.concatenate([li[:30], spare[10:15]]))
    new = new_model(k, new_users, new_items, seed=61)
    gen = {"X": {int(u): X[r] for r, u in enumerate(lu)}, "Y": {int(i): Y[r] for r, i in enumerate(li)}, "known": None, "item_tags": set(), "user_tags": set()}
    glo.load_model(gen, {int(u): new["X"][r] for r, u in enumerate(new_users)}, {int(i): new["Y"][r] for r, i in enumerate(new_items)}, None, set(), set(),
                   {int(lu[3]), int(lu[4]), int(lu[49])}, {int(li[39])})
    d = glo.dense(gen, [int(u) for u in lu], [int(i) for i in li], [int(u) for u in new_users], [int(i) for i in new_items])
    res, ids, maps = g.load_generation(lu, li, new_users, new_items, new["X"], new["Y"])
    assert np.array_equal(ids[0], d["user_ids"]) and np.array_equal(ids[1], d["item_ids"])
    assert np.array_equal(maps[0], d["user_map"]) and np.array_equal(maps[1], d["item_map"])
    assert res["n_kept"] == [3, 1] and res["n_known_dropped"] == 0
    n_users, n_items = len(d["user_ids"]), len(d["item_ids"])
    assert np.array_equal(g.bounds(X_), plan_shards(np.zeros(n_users + 1, np.int64), W, k)) and g.bounds(X_)[-1] == n_users
    assert np.array_equal(g.bounds(Y_), plan_shards(np.zeros(n_items + 1, np.int64), W, k))
    for side, want in ((X_, d["X"]), (Y_, d["Y"])):
        out, equal = g.replica_digest(side)
        assert equal and int(out[0]) == factor_digest_host(want)
        assert np.array_equal(bits(g.get_factors(side, 0, len(want))), bits(want))
    assert len(g.get_recent(X_)) == 0 and len(g.get_recent(Y_)) == 0
    g.close()


# ---- 8. all or nothing ---------------------------------------------------------------------------------------------------------
def test_failing_loads_change_nothing():
    W, k = 3, 8
    rng = np.random.default_rng(71)
    lu, li, nu, ni = base_ids(seed=4)
    b = Both(W, k, lu, li, seed=2)
    b.set_tags([5, 10], [3, 10])
    b.write([0, 5, 41, 100, 250, 299], [3, 31, 40, 160, 199, 0])
    b.mark(X_, [1, 2])
    g = b.g
    users = np.arange(len(lu))

    def state():
        return (g.bounds(X_).tolist(), g.get_recent(X_).tolist(), g.get_recent(Y_).tolist(), g.replica_digest(X_)[0].tolist(),
                g.replica_digest(Y_)[0].tolist(), [a.tobytes() for a in g.recommend(users, 10)], [a.tobytes() for a in g.most_popular_items(20)[:2]])

    before = state()
    new = new_model(k, nu, ni, seed=5)
    known = csr(new["known_rows"])
    cur = [np.array(b.live.user_ids, np.int64), np.array(b.live.item_ids, np.int64)]
    good = [np.array(new["user_ids"], np.int64), np.array(new["item_ids"], np.int64), new["X"], new["Y"]]
    dup = good[0].copy()
    dup[17] = dup[3]
    with pytest.raises(MalsError) as e:      # a duplicate id in new_ids
        g.load_generation(cur[0], cur[1], dup, good[1], good[2], good[3], new_known=known)
    assert e.value.status == _lib.INVALID_ARG and "twice" in str(e.value)
    assert state() == before
    g.features = k + 1                       # a features mismatch (the rows are n_new x (k + 1), the struct says k + 1)
    try:
        with pytest.raises(MalsError) as e:
            g.load_generation(cur[0], cur[1], good[0], good[1], factors(rng, len(good[0]), k + 1), factors(rng, len(good[1]), k + 1), new_known=known)
    finally:
        g.features = k
    assert e.value.status == _lib.INVALID_ARG and "features" in str(e.value)
    assert state() == before
    with pytest.raises(MalsError) as e:      # no known items for a group that holds some
        g.load_generation(cur[0], cur[1], *good)
    assert e.value.status == _lib.INVALID_ARG and "known items" in str(e.value)
    assert state() == before
    # and the good load still goes through afterwards
    d, res, _ = b.load(new)
    b.compare(d)
    b.close()


# ---- 9. readers during a load --------------------------------------------------------------------------------------------------
def test_readers_see_the_old_or_the_new_generation():
    W, k = 2, 16
    lu, li, nu, ni = base_ids(seed=6)
    b = Both(W, k, lu, li, seed=3)
    b.write([0, 5, 41, 100, 250, 299], [3, 31, 40, 160, 199, 0])
    b.mark(X_, list(range(0, 300, 7)))
    users = [0, 41, 100, 150, 200, 259]
    old = {u: [a.tobytes() for a in b.g.recommend([u], 10)] for u in users}
    new = new_model(k, nu, ni, seed=7)
    cur = [np.array(b.live.user_ids, np.int64), np.array(b.live.item_ids, np.int64)]
    d, res = load(b.live, new)                           # the handle first: its answers are the new generation's
    fresh = {u: [a.tobytes() for a in b.live.core.recommend([u], 10)] for u in users}
    stop, bad, errors, seen = threading.Event(), [], [], [0, 0]

    def reader(t):
        try:
            while not stop.is_set():
                u = users[(t + seen[0]) % len(users)]
                got = [a.tobytes() for a in b.g.recommend([u], 10)]
                if got == old[u]:
                    seen[0] += 1
                elif got == fresh[u]:
                    seen[1] += 1
                else:
                    bad.append(u)
        except Exception as ex:     # noqa: BLE001 -- reported below
            errors.append(repr(ex))

    threads = [threading.Thread(target=reader, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    try:
        b.g.load_generation(cur[0], cur[1], np.array(new["user_ids"], np.int64), np.array(new["item_ids"], np.int64), new["X"], new["Y"],
                            new_known=csr(new["known_rows"]))
        for u in users:             # (still racing the readers)
            assert [a.tobytes() for a in b.g.recommend([u], 10)] == fresh[u]
    finally:
        stop.set()
        for t in threads:
            t.join()
    assert not errors and not bad, (errors[:3], bad[:10])
    for u in users:
        assert [a.tobytes() for a in b.g.recommend([u], 10)] == fresh[u]
    b.compare(d)
    b.close()


# ---- 10. member handles --------------------------------------------------------------------------------------------------------
def test_a_member_handle_still_refuses_the_single_handle_load():
    k = 8
    lu, li, nu, ni = base_ids(seed=9)
    b = Both(2, k, lu, li, seed=1)
    new = new_model(k, nu, ni, seed=2)
    member, _ = b.g.local(0)
    with pytest.raises(MalsError) as e:
        member.load_generation(np.array(b.live.user_ids, np.int64), np.array(b.live.item_ids, np.int64), np.array(new["user_ids"], np.int64),
                               np.array(new["item_ids"], np.int64), new["X"], new["Y"], new_known=csr(new["known_rows"]))
    assert e.value.status == _lib.INVALID_ARG and "group" in str(e.value)
    # nothing changed: the group load still works and agrees with the handle
    d, res, _ = b.load(new)
    b.compare(d)
    b.close()


# ---- MALS_GENERATION_RECOMPUTE_SOLVERS: computed once, installed on every member ---------------------------------------------------
def test_recomputed_solvers_reach_every_member():
    W, k = 3, 16
    lu, li, nu, ni = base_ids(seed=12)
    b = Both(W, k, lu, li, seed=6)
    b.write([0, 5, 41, 100, 250, 299], [3, 31, 40, 160, 199, 0])
    new = new_model(k, nu, ni, seed=13)
    d, res, _ = b.load(new, recompute_solvers=True)
    assert res["solver_status"] == _lib.OK
    b.compare(d)
    # the writes after the load use the recomputed solvers: every member's replicas follow the handle's bit for bit
    n_users = len(d["user_ids"])
    b.write([0, 5, n_users - 1, 130], [1, 2, 3, 4], [1.0, 0.5, 2.0, 1.5])
    for side in (X_, Y_):
        out, equal = b.g.replica_digest(side)
        assert equal and int(out[0]) == b.live.core.factor_digest(side)
    users = [0, 5, n_users - 1, 130]
    same_answers(b.g.recommend(users, 10), b.live.core.recommend(users, 10))
    b.close()
