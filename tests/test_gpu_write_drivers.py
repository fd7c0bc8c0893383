"""The one driver per online write (csrc/foldin_host.h, popular_host.h) gives the same answer through each of its callers: a
handle (mals_set_preferences ...: the driver over one member inside the handle's ticket), a single-process group of one
member and a group of two members on the one device (the mals_group_* twins: the same driver over the members).

The smallest shapes at which the shared driver can still go wrong: 12 users x 9 items, k = 16, the known items from a small
user-side matrix (2 per user, so the two members of the second group own users 0-5 and 6-11).  Gramians of 12 and of 9 rows
have rank < 16, which HostSolver refuses as singular, so the two fold-in solvers are those of X^T X + I/10 and Y^T Y + I/10:
a write asks no more of its solvers than that every set-up holds the same ones.  What the model must be after a write is
tests/test_gpu_foldin.py's and tests/test_gpu_group_foldin.py's subject (against the oracle); here the three set-ups are
held against each other, and against what the definitions say of the counters."""
import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from myrrix_recommender_amd.core import HostSolver

pytestmark = pytest.mark.gpu
X_, Y_ = pkg.SIDE_X, pkg.SIDE_Y
N_USERS, N_ITEMS, K = 12, 9, 16
SETUPS = ("handle", "group of 1", "group of 2")


def model():
    rng = np.random.default_rng(2024)
    X = (rng.standard_normal((N_USERS, K)) * 0.3).astype(np.float32)
    Y = (rng.standard_normal((N_ITEMS, K)) * 0.3).astype(np.float32)
    rows = [np.sort(rng.choice(N_ITEMS, 2, replace=False)) for _ in range(N_USERS)]
    ptr = np.arange(N_USERS + 1, dtype=np.int64) * 2
    col = np.concatenate(rows).astype(np.int32)
    return X, Y, ptr, col


X0, Y0, PTR, COL = model()
KNOWN = {u: [int(c) for c in COL[PTR[u]:PTR[u + 1]]] for u in range(N_USERS)}


def ridge_solver(M):
    M = np.asarray(M, np.float64)
    return HostSolver.create(M.T @ M + 0.1 * np.eye(K))


class Setup:
    """One of the three callers behind one face: `w` takes the writes and reads (an ALSCore or a GroupALS: the methods have
    the same names), `members` are the handles that hold a replica."""

    def __init__(self, name):
        self.name = name
        self.solvers = (ridge_solver(X0), ridge_solver(Y0))
        ones = np.ones(len(COL), np.float32)
        if name == "handle":
            self.w = pkg.ALSCore(K)
            self.members = [self.w]
        else:
            world = 1 if name == "group of 1" else 2
            self.w = pkg.GroupALS.single_process(K, [0] * world, backend=_lib.GROUP_PEER_COPY)
            self.members = [self.w.local(m)[0] for m in range(world)]
        self.w.set_factor_rows(X_, N_USERS)
        self.w.set_factor_rows(Y_, N_ITEMS)
        self.w.set_factors(X_, X0)
        self.w.set_factors(Y_, Y0)
        self.w.set_matrix(X_, PTR, COL, ones)
        self.w.set_foldin_solver(X_, self.solvers[0])
        self.w.set_foldin_solver(Y_, self.solvers[1])
        if name == "group of 2":
            assert [int(b) for b in self.w.bounds(X_)] == [0, 6, 12]

    def digests(self):
        """(digest of X, digest of Y), every member's the same"""
        if self.name == "handle":
            return self.w.factor_digest(X_), self.w.factor_digest(Y_)
        out = []
        for side in (X_, Y_):
            d, eq = self.w.replica_digest(side)
            assert eq and len(d) == len(self.members), (self.name, d)
            out.append(int(d[0]))
        return tuple(out)

    def counters(self):
        s = self.w.foldin_stats()
        return {key: s[key] for key in ("applied", "failed", "big_foldin", "levels")}

    def recounts(self):
        return [m.most_popular_stats()["recounts"] for m in self.members]

    def close(self):
        self.w.close()


@pytest.fixture
def setups():
    made = [Setup(name) for name in SETUPS]
    assert len({s.digests() for s in made}) == 1
    yield made
    for s in made:
        s.close()


def levels_of(users, items):
    """The level plan by its definition: 1 + the larger level of the last earlier update of the same user and of the same
    item (0: none); the batch's levels are the largest."""
    level = []
    for t in range(len(users)):
        lu = next((level[s] for s in range(t - 1, -1, -1) if users[s] == users[t]), 0)
        li = next((level[s] for s in range(t - 1, -1, -1) if items[s] == items[t]), 0)
        level.append(1 + max(lu, li))
    return max(level)


def all_equal(values):
    return all(np.array_equal(v, values[0]) for v in values[1:])


# ---- the cases (tools and job scripts run them too: each returns what it observed) ---------------------------------------
def set_case(s):
    rng = np.random.default_rng(7)
    users = rng.choice([4, 5, 6, 7, 8], 64)            # 5 users, of both members of the group of 2
    items = rng.choice([0, 3, 5, 8], 64)               # 4 items
    values = rng.choice([1.0, 2.0, -1.0, 0.5], 64).astype(np.float32)
    before = s.counters()
    status = s.w.set_preferences(users, items, values, raise_on_error=False)
    after = s.counters()
    delta = {key: after[key] - before[key] for key in after}
    idx, _, cnt = s.w.recommend(np.arange(N_USERS), N_ITEMS, consider_known_items=False)
    return {"users": users, "items": items, "status": status, "delta": delta, "digests": s.digests(),
            "recommended": [set(idx[u, :cnt[u]].tolist()) for u in range(N_USERS)]}


def remove_case(s):
    # user 7 (the second member's) loses both items first, then user 2 (the first member's); around them pairs that are
    # ignored (an item the user does not know) and one that shrinks a set without emptying it
    unknown_of_0 = next(i for i in range(N_ITEMS) if i not in KNOWN[0])
    users = [0, 7, 3, 7, 2, 2, 7]
    items = [unknown_of_0, KNOWN[7][1], KNOWN[3][0], KNOWN[7][0], KNOWN[2][0], KNOWN[2][1], KNOWN[7][0]]
    removed = s.w.remove_preferences(users, items)
    return {"removed": removed.tolist(), "digests": s.digests(), "x_rows": [m.get_factors(X_) for m in s.members]}


def grow_case(s):
    s.w.grow_factor_rows(X_, N_USERS + 3)
    s.w.grow_factor_rows(Y_, N_ITEMS + 2)
    grown_user, item = N_USERS + 1, N_ITEMS + 1
    before = s.counters()
    status = s.w.set_preferences([grown_user], [item], [1.0], raise_on_error=False)
    after = s.counters()
    calls = [m.recommend_front_stats()["calls"] for m in s.members]
    idx, _, cnt = s.w.recommend([grown_user], N_ITEMS + 2, consider_known_items=False)
    answered = [m.recommend_front_stats()["calls"] - c for m, c in zip(s.members, calls)]
    every, _, cnt_every = s.w.recommend([grown_user], N_ITEMS + 2, consider_known_items=True)
    return {"status": status, "delta": {key: after[key] - before[key] for key in after}, "digests": s.digests(), "item": item,
            "recommended": set(idx[0, :cnt[0]].tolist()), "scored": set(every[0, :cnt_every[0]].tolist()),
            "answered": answered,
            "rows": [(m.factor_device_ptr(X_)[1], m.factor_device_ptr(Y_)[1]) for m in s.members]}


# ---- the tests ------------------------------------------------------------------------------------------------------------
def test_set_is_one_write_through_every_caller(setups):
    got = [set_case(s) for s in setups]
    levels = levels_of(got[0]["users"].tolist(), got[0]["items"].tolist())
    assert levels > 16                                   # 64 updates of 5 x 4 rows: the chains are deep
    for s, g in zip(setups, got):
        print(s.name, g["delta"], g["digests"])
        assert g["delta"]["levels"] == levels, s.name
        assert g["delta"]["applied"] == 64 and g["delta"]["failed"] == 0, s.name      # each update once, not once per member
        assert not g["status"].any(), s.name
        for u, i in zip(g["users"].tolist(), g["items"].tolist()):                    # the owner recorded the known item
            assert i not in g["recommended"][u], (s.name, u, i)
    assert all_equal([g["status"] for g in got])
    assert got[0]["digests"] == got[1]["digests"] == got[2]["digests"]
    assert got[0]["digests"] != (pkg.factor_digest_host(X0), pkg.factor_digest_host(Y0))


def test_remove_empties_the_same_users_in_batch_order(setups):
    got = [remove_case(s) for s in setups]
    for s, g in zip(setups, got):
        print(s.name, g["removed"], g["digests"])
        assert g["removed"] == [7, 2], s.name            # batch order, not member order: user 7 is the SECOND member's
        for rows in g["x_rows"]:                         # zero on every member
            assert not rows[[2, 7]].any() and rows[[0, 3]].any(axis=1).all(), s.name
    assert got[0]["digests"] == got[1]["digests"] == got[2]["digests"]


def test_grow_then_a_write_for_a_grown_user(setups):
    got = [grow_case(s) for s in setups]
    for s, g in zip(setups, got):
        print(s.name, g["delta"], g["digests"])
        assert g["rows"] == [(N_USERS + 3, N_ITEMS + 2)] * len(s.members), s.name
        assert g["status"].tolist() == [0], s.name
        assert (g["delta"]["applied"], g["delta"]["failed"], g["delta"]["levels"]) == (1, 0, 1), s.name
        # the grown user's known item is its owner's -- the handle itself, the last member of a group, which answers
        assert g["item"] in g["scored"] and g["item"] not in g["recommended"], s.name
        assert g["recommended"] == g["scored"] - {g["item"]}, s.name
        assert g["answered"][-1] >= 1 and not any(g["answered"][:-1]), s.name
    assert got[0]["delta"] == got[1]["delta"] == got[2]["delta"]
    assert got[0]["digests"] == got[1]["digests"] == got[2]["digests"]


def test_popular_counts_once_and_selects_alike(setups):
    for s in setups:                                     # writes first: users of both members with a set of their own
        set_case(s)
        s.w.remove_preferences([1, 9], [KNOWN[1][0], KNOWN[9][1]])
    tops = []
    for s in setups:
        before = s.recounts()
        idx, sc, n = s.w.most_popular_items(5)
        counted = s.recounts()
        assert [c - b for c, b in zip(counted, before)] == [1] * len(s.members), s.name
        again = s.w.most_popular_items(5)
        assert s.recounts() == counted, s.name           # the second call does not recount
        assert np.array_equal(again[0], idx) and np.array_equal(again[1], sc) and again[2] == n, s.name
        print(s.name, idx.tolist(), sc.tolist(), n)
        tops.append((idx, sc, n))
    assert tops[0][2] == 5
    assert all_equal([t[0] for t in tops]) and all_equal([t[1] for t in tops]) and tops[0][2] == tops[1][2] == tops[2][2]
    # on the handle: a rescorer that filters the top item removes exactly it
    core = setups[0].w
    six, six_scores, n6 = core.most_popular_items(6)
    assert n6 == 6
    with core.rescorer() as r:
        r.set_filter([int(six[0])])
        idx, sc, n = core.most_popular_items(5, rescorer=r)
    assert n == 5 and np.array_equal(idx, six[1:]) and np.array_equal(sc, six_scores[1:])
    assert setups[0].recounts() == [1]
