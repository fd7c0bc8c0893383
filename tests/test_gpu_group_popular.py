"""mals_group_most_popular_items: the known items are sharded by owner, every member counts its own users, one member adds
the partial counts and selects -- the answer is bit for bit what ONE handle holding the whole model returns, and both are
the oracle's (tests/popular_oracle.py).  N members on device 0 with the peer-copy backend, as test_gpu_group_foldin.py."""
import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from myrrix_recommender_amd.core import MalsError
from tests import popular_oracle as po
from tests.test_gpu_group_foldin import group_for, known_of, model

pytestmark = pytest.mark.gpu
X_, Y_ = pkg.SIDE_X, pkg.SIDE_Y


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def single_for(X, Y, ptr, col, solvers):
    core = pkg.ALSCore(X.shape[1])
    core.set_factor_rows(X_, len(X))
    core.set_factor_rows(Y_, len(Y))
    core.set_factors(X_, X)
    core.set_factors(Y_, Y)
    core.set_matrix(X_, ptr, col, np.ones(len(col), np.float32))
    core.set_foldin_solver(X_, solvers[0])
    core.set_foldin_solver(Y_, solvers[1])
    return core


def agree(g, core, sets, n_items, tag_users, tag_items, how_many):
    a, b = g.most_popular_items(how_many), core.most_popular_items(how_many)
    oi, ov = po.most_popular(po.counts_from_sets(sets, n_items, tag_users), how_many, tag_items)
    for idx, sc, n in (a, b):
        assert n == len(oi) and np.array_equal(idx[:n], oi), (idx[:n], oi)
        assert np.array_equal(bits(sc[:n]), bits(ov))
        assert np.all(idx[n:] == -1) and np.all(np.isneginf(sc[n:]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]


@pytest.mark.parametrize("world", [3, 1])
def test_a_group_answers_like_one_handle(world):
    n_users, n_items, k = 90, 70, 8
    X, Y, ptr, col = model(n_users, n_items, k, 40 + world, nnz_per_user=6)
    g, solvers = group_for(world, X, Y, ptr, col)
    core = single_for(X, Y, ptr, col, solvers)
    try:
        b = g.bounds(X_)
        sets = {u: set(s) for u, s in known_of(ptr, col).items()}
        tag_users = sorted({int(b[0]) + 1, int(b[-1]) - 2, n_users + 5})      # two different slices (world 3); one names nobody
        tag_items = [3, 69]
        for m in range(1 if world == 1 else world):
            g.local(m)[0].set_tag_items(tag_items)
        core.set_tag_items(tag_items)
        g.set_tag_users(tag_users)
        core.set_tag_users(tag_users)
        if world == 3:
            assert [g.local(m)[0].tag_user_count() for m in range(3)] == [1, 0, 1]   # each member keeps those it owns
        for how_many in (1, 10, 200):
            agree(g, core, sets, n_items, tag_users, tag_items, how_many)
        # a write batch that touches users of every owner and a grown user
        g.grow_factor_rows(X_, n_users + 3)
        core.grow_factor_rows(X_, n_users + 3)
        users = [int(b[r]) for r in range(len(b) - 1)] + [int(b[r + 1]) - 1 for r in range(len(b) - 1)] + [n_users + 1, tag_users[0]]
        items = [int((7 * u + 1) % n_items) for u in users]
        vals = np.ones(len(users), np.float32)
        assert np.array_equal(g.set_preferences(users, items, vals), core.set_preferences(users, items, vals))
        for u, i in zip(users, items):
            sets.setdefault(u, set()).add(i)
        agree(g, core, sets, n_items, tag_users, tag_items, 25)
        # a removal on the first and the last owner
        ru = [users[0], int(b[-1]) - 1]
        ri = [sorted(sets[u])[0] for u in ru]
        assert np.array_equal(g.remove_preferences(ru, ri), core.remove_preferences(ru, ri))
        for u, i in zip(ru, ri):
            sets[u].discard(i)
        agree(g, core, sets, n_items, tag_users, tag_items, 70)
        with pytest.raises(MalsError) as e:                       # a member answers through its group only
            g.local(0)[0].most_popular_items(5)
        assert e.value.status == _lib.INVALID_ARG
        # a new generation drops the set on every member, with the overlays
        g.set_matrix(X_, ptr, col, np.ones(len(col), np.float32))
        assert [g.local(m)[0].tag_user_count() for m in range(1 if world == 1 else world)] == [0] * (1 if world == 1 else world)
    finally:
        core.close()
        g.close()
