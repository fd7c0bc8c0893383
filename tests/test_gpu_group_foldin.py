"""The online write path and the fold-in reads on a group (the mals_group_* twins) against tests/foldin_oracle.py: a group
write is the same write on ONE model -- every member's X and Y, the statuses, the known items (through recommend) and the
fold-in reads are bit for bit the oracle's -- and the replica digest proves on the device that the members agree.

One device here: N members on device 0 with the peer-copy backend, and the one-rank RCCL group (see test_gpu_group.py)."""
import ctypes
import multiprocessing as mp
import os
import threading

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from myrrix_recommender_amd.core import HostSolver, MalsError
from oracle import oracle
from oracle import topn_oracle as to
from tests import foldin_oracle as fo
from tests import similarity_oracle as so
from tests.test_gpu_group import REL_TOL, rel

pytestmark = pytest.mark.gpu
X_, Y_ = pkg.SIDE_X, pkg.SIDE_Y
MOCK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "cpp", "libmock_rccl.so")


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


def transpose(ptr, col, n_items):
    users = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    order = np.lexsort((users, col))
    tptr = np.zeros(n_items + 1, np.int64)
    np.add.at(tptr, col[order] + 1, 1)
    return np.cumsum(tptr), users[order].astype(np.int32), np.ones(len(col), np.float32)


def known_of(ptr, col):
    return {u: set(col[ptr[u]:ptr[u + 1]].tolist()) for u in range(len(ptr) - 1) if ptr[u + 1] > ptr[u]}


def group_for(world, X, Y, ptr, col, sx=True, sy=True, rccl=False):
    k = X.shape[1]
    if rccl:
        g = pkg.GroupALS.from_torch_distributed(k, 0, world=1, rank=0, one_rank_communicator=True)
    else:
        g = pkg.GroupALS.single_process(k, [0] * world, backend=_lib.GROUP_PEER_COPY)
    g.set_factor_rows(X_, len(X))
    g.set_factor_rows(Y_, len(Y))
    g.set_factors(X_, X)
    g.set_factors(Y_, Y)
    g.set_matrix(X_, ptr, col, np.ones(len(col), np.float32))
    solvers = (gram_solver(X) if sx else None, gram_solver(Y) if sy else None)
    g.set_foldin_solver(X_, solvers[0])
    g.set_foldin_solver(Y_, solvers[1])
    return g, solvers


def n_members(g):
    return 1 if g.world == 1 else g.world


def check_group(g, Xo, Yo):
    """Every member's replicas are the oracle's bits, and the device digests say the same without a copy."""
    for m in range(n_members(g)):
        core, _ = g.local(m)
        assert np.array_equal(bits(core.get_factors(X_)), bits(Xo)), m
        assert np.array_equal(bits(core.get_factors(Y_)), bits(Yo)), m
    for side, M in ((X_, Xo), (Y_, Yo)):
        d, eq = g.replica_digest(side)
        assert eq and len(d) == n_members(g)
        assert int(d[0]) == pkg.factor_digest_host(M)


def top_same(g, Xo, Yo, known, users, how_many=10):
    idx, sc, cnt = g.recommend(users, how_many)
    for q, u in enumerate(users):
        oi, os_ = to.recommend(Yo, Xo[u], how_many, known=sorted(known.get(int(u), ())))
        assert cnt[q] == len(oi)
        assert np.array_equal(idx[q, :cnt[q]], oi), (u, idx[q, :cnt[q]], oi)
        assert np.array_equal(bits(sc[q, :cnt[q]]), bits(os_))


# ---- 1. a batch on a group is the batch on one model ----------------------------------------------------------------
@pytest.mark.parametrize("world,k,rccl", [(1, 8, False), (2, 30, False), (3, 64, False), (4, 128, False), (1, 30, True)])
def test_a_batch_on_a_group_is_the_batch_on_one_model(world, k, rccl):
    X, Y, ptr, col = model(300, 200, k, 100 + world)
    g, (sx, sy) = group_for(world, X, Y, ptr, col, rccl=rccl)
    rng = np.random.default_rng(world)
    n = 2000
    u = rng.integers(0, 300, n)                      # 2 000 updates of 300 users: every user several times
    i = rng.integers(0, 200, n)
    i[rng.choice(n, 300, replace=False)] = 7         # a hot item: 300 levels
    v = rng.choice([1.0, 2.0, -1.0, 0.5, 0.0, 1e30], n).astype(np.float32)
    st = g.set_preferences(u, i, v, raise_on_error=False)
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    sto = fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy)
    assert np.array_equal(st, sto)
    check_group(g, Xo, Yo)
    s = g.foldin_stats()
    assert s["applied"] == int((sto == 0).sum()) and s["failed"] == int((sto != 0).sum())   # each update once, not once per member
    assert s["applied"] + s["failed"] == n and s["levels"] >= 300 and s["device_ms_last"] > 0
    g.close()


# ---- 2. ownership at the edges -----------------------------------------------------------------------------------------
def test_known_items_live_with_the_owner_at_every_slice_edge():
    world, k = 3, 16
    X, Y, ptr, col = model(61, 400, k, 21, nnz_per_user=3)
    g, (sx, sy) = group_for(world, X, Y, ptr, col)
    b = g.bounds(X_)
    assert b[0] == 0 and b[-1] == 61 and np.all(np.diff(b) > 0)
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    everyone = np.arange(61)
    edge = np.array(sorted({int(e) for r in range(world) for e in (b[r], b[r + 1] - 1)}))
    top, _, _ = g.recommend(edge, 1)                 # the item each edge user would be recommended: the write makes it known
    u, i, v = edge, top[:, 0], np.ones(len(edge), np.float32)
    assert np.array_equal(g.set_preferences(u, i, v), fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy))
    check_group(g, Xo, Yo)
    top_same(g, Xo, Yo, known, everyone)             # an owner that did not record it, or a non-owner that did, fails here
    # one batch whose users all belong to the middle member
    u = np.arange(b[1], b[2])
    i = (u * 7) % 400
    v = np.full(len(u), 2.0, np.float32)
    assert np.array_equal(g.set_preferences(u, i, v), fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy))
    check_group(g, Xo, Yo)
    top_same(g, Xo, Yo, known, everyone)
    g.close()


def test_fewer_users_than_members():
    world, k = 3, 2                                  # (two users: X^T X has rank 2)
    X, Y, ptr, col = model(2, 50, k, 22, nnz_per_user=2)
    g, (sx, sy) = group_for(world, X, Y, ptr, col)
    b = g.bounds(X_)
    assert b[-1] == 2 and (np.diff(b) == 0).any()    # some slices are empty
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    top, _, _ = g.recommend([0, 1], 2)
    u, i, v = [0, 1, 0], [int(top[0, 0]), int(top[1, 0]), int(top[0, 1])], np.ones(3, np.float32)
    assert np.array_equal(g.set_preferences(u, i, v), fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy))
    check_group(g, Xo, Yo)
    top_same(g, Xo, Yo, known, [0, 1], how_many=5)
    g.close()


# ---- 3. null solvers and failed updates ---------------------------------------------------------------------------------
def test_null_solvers_through_a_group():
    k = 8
    X, Y, ptr, col = model(20, 30, k, 5)
    u, i = np.arange(20), np.arange(20)
    v = np.ones(20, np.float32)
    g, (_, sy) = group_for(2, X, Y, ptr, col, sx=False)
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    assert np.array_equal(g.set_preferences(u, i, v), fo.set_preferences(Xo, Yo, known, u, i, v, None, sy))
    assert np.array_equal(Yo, Y)
    check_group(g, Xo, Yo)
    g.close()
    g, (sx, _) = group_for(2, X, Y, ptr, col, sy=False)
    st = g.set_preferences(u, i, v, raise_on_error=False)
    assert np.all(st == _lib.INVALID_ARG)
    check_group(g, X, Y)
    with pytest.raises(MalsError, match="without a Y\\^T Y solver") as e:
        g.set_preferences(u, i, v)
    assert e.value.status == _lib.INVALID_ARG
    top_same(g, X, Y, known_of(ptr, col), np.arange(20), how_many=5)      # a failed update adds no known item, on any member
    g.close()


def test_nan_rows_and_per_update_status_through_a_group():
    k = 8
    X, Y, ptr, col = model(20, 30, k, 6)
    g, (sx, sy) = group_for(2, X, Y, ptr, col)      # the generation's solvers, from the rows before one went bad
    X[3] = np.nan
    g.set_factors(X_, X)
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    u = np.array([1, 3, 2, 3, 4, 19])
    i = np.array([1, 2, 3, 4, 5, 6])
    v = np.ones(6, np.float32)
    st = g.set_preferences(u, i, v, raise_on_error=False)
    assert st.tolist() == [0, 2, 0, 2, 0, 0]
    assert np.array_equal(st, fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy))
    check_group(g, Xo, Yo)
    assert g.foldin_stats()["failed"] == 2 and g.foldin_stats()["applied"] == 4
    with pytest.raises(MalsError, match="update 1: estimate is not finite") as e:      # the first failure's code and text
        g.set_preferences(u, i, v)
    assert e.value.status == _lib.INVALID_ARG
    fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy)
    check_group(g, Xo, Yo)
    g.close()


# ---- 4. remove -------------------------------------------------------------------------------------------------------
def test_remove_on_a_group():
    world, k = 3, 16
    X, Y, ptr, col = model(60, 300, k, 7, nnz_per_user=3)
    g, (sx, sy) = group_for(world, X, Y, ptr, col)
    b = g.bounds(X_)
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    users = np.arange(60)
    mid = int(b[1])                                   # a user of the middle member
    assert b[1] < b[2] and mid + 1 < b[2]
    idx, _, _ = g.recommend(users, 2)
    u, i, v = users, idx[:, 0], np.ones(60, np.float32)
    assert np.array_equal(g.set_preferences(u, i, v), fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy))
    # ignored pairs (an item nobody knows, an item of another user), pairs that shrink a set, and every item of `mid`
    ru = [0, 0, 1, 59, mid + 1] + [mid] * len(known[mid]) + [mid]
    ri = [299, int(idx[0, 0]), int(col[ptr[1]]), int(idx[59, 0]), int(idx[0, 0])] + sorted(known[mid]) + [5]
    got = g.remove_preferences(ru, ri)
    exp = fo.remove_preferences(Xo, known, ru, ri)
    assert got.tolist() == exp == [mid]
    for m in range(world):                            # the emptied user's row is zero on EVERY member
        assert not g.local(m)[0].get_factors(X_, mid, 1).any()
    check_group(g, Xo, Yo)
    top_same(g, Xo, Yo, known, users)
    bi, bs, bc = g.recommended_because(users, users % 300, 5)
    for q, uu in enumerate(users):
        oi, os_ = so.recommended_because(Yo, sorted(known.get(int(uu), ())), int(uu % 300), 5)
        assert np.array_equal(bi[q, :bc[q]], oi) and np.array_equal(bits(bs[q, :bc[q]]), bits(os_))
    # a later write recreates the removed user from zeros
    g.set_preferences([mid], [5], [1.0])
    fo.set_preferences(Xo, Yo, known, [mid], [5], [1.0], sx, sy)
    check_group(g, Xo, Yo)
    top_same(g, Xo, Yo, known, users)
    g.close()


# ---- 5. grow ---------------------------------------------------------------------------------------------------------
def test_grow_on_a_group_and_a_half_iteration_afterwards():
    world, k = 3, 16
    X, Y, ptr, col = model(50, 40, k, 3)
    g, (sx, sy) = group_for(world, X, Y, ptr, col)
    g.set_matrix(Y_, *transpose(ptr, col, 40))
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    g.grow_factor_rows(X_, 70)
    g.grow_factor_rows(Y_, 45)
    Xo = np.vstack([Xo, np.zeros((20, k), np.float32)])
    Yo = np.vstack([Yo, np.zeros((5, k), np.float32)])
    check_group(g, Xo, Yo)
    rng = np.random.default_rng(4)
    u = rng.integers(0, 70, 500)                      # old and new rows mixed
    i = rng.integers(0, 45, 500)
    v = rng.choice([1.0, 2.0, -1.0], 500).astype(np.float32)
    assert np.array_equal(g.set_preferences(u, i, v), fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy))
    check_group(g, Xo, Yo)
    new_users = np.arange(50, 70)                     # the last rank's
    top_same(g, Xo, Yo, known, new_users)
    top_same(g, Xo, Yo, known, np.arange(50))
    uu = int(next(x for x in new_users if len(known.get(int(x), ())) >= 2))
    bi, bs, bc = g.recommended_because([uu], [3], 5)
    oi, os_ = so.recommended_because(Yo, sorted(known[uu]), 3, 5)
    assert np.array_equal(bi[0, :bc[0]], oi) and np.array_equal(bits(bs[0, :bc[0]]), bits(os_))
    with pytest.raises(MalsError):
        g.recommend([70], 3)
    # the header: a half-iteration solves the rows of the installed matrix; the grown rows keep what the writes gave them and
    # count in the opposite Gramian; the replicas stay bitwise equal
    g.half_iteration(X_)
    g.synchronize()
    Xh = g.get_factors(X_, 0, 70)
    assert np.array_equal(bits(Xh[50:]), bits(Xo[50:]))
    r_ptr, r_col = ptr, col
    Xref = oracle.half_iteration(r_ptr, r_col, np.ones(len(col), np.float32), Yo, threads=4)      # Y^T Y over all 45 rows of Y
    assert rel(Xh[:50], Xref) < REL_TOL
    assert not np.array_equal(bits(Xh[:50]), bits(Xo[:50]))
    for side, rows in ((X_, 70), (Y_, 45)):
        d, eq = g.replica_digest(side)
        assert eq
        assert int(d[0]) == pkg.factor_digest_host(g.get_factors(side, 0, rows))
    for m in range(world):
        assert np.array_equal(bits(g.local(m)[0].get_factors(X_)), bits(Xh))
    g.close()


# ---- 6. reads rotate and agree -----------------------------------------------------------------------------------------
def test_reads_rotate_over_the_members_and_agree():
    k = 24
    X, Y, ptr, col = model(30, 500, k, 8)
    g, (sx, sy) = group_for(3, X, Y, ptr, col)
    before = [g.local(m)[0].recommend_front_stats()["calls"] for m in range(3)]
    u = np.array([0, -1, 5, 7])
    i = np.array([3, 4, -1, 9])
    queries = [[1, 2, 3], [-1, 4], [-1], [7, 7, 499]]
    values = [[1.0, 2.0, -1.0], [0.5, 3.0], [1.0], [1.0, 0.0, -2.0]]
    to_items = [10, 11, 12, 13]
    est_o = fo.estimate_preferences(X, Y, u, i)
    feat_o = [fo.anonymous_features(Y, items, values[q], sy) for q, items in enumerate(queries)]
    efa_o = [fo.estimate_for_anonymous(Y, to_items[q], items, values[q], sy) for q, items in enumerate(queries)]
    top_o = [to.recommend(Y, feat_o[q][0], 8, known=sorted(j for j in items if j >= 0)) if feat_o[q][1] else None for q, items in enumerate(queries)]
    for _ in range(6):
        assert np.array_equal(bits(g.estimate_preferences(u, i)), bits(est_o))
        f, st = g.anonymous_features(queries, values, raise_on_error=False)
        assert st.tolist() == [0, 0, 2, 0]
        est, st2 = g.estimate_for_anonymous(to_items, queries, values)
        idx, sc, cnt, st3 = g.recommend_to_anonymous(queries, 8, values)
        assert st2.tolist() == st3.tolist() == [0, 0, 2, 0] and cnt[2] == 0
        for q in range(len(queries)):
            if not feat_o[q][1]:
                continue
            assert np.array_equal(bits(f[q]), bits(feat_o[q][0]))
            assert efa_o[q][1] and bits(est[q]) == bits(efa_o[q][0])
            assert np.array_equal(idx[q, :cnt[q]], top_o[q][0]) and np.array_equal(bits(sc[q, :cnt[q]]), bits(top_o[q][1]))
    with pytest.raises(MalsError):
        g.anonymous_features(queries, values)
    served = [g.local(m)[0].recommend_front_stats()["calls"] - before[m] for m in range(3)]
    assert sum(1 for s in served if s > 0) > 1, served      # 24 calls over 3 members: more than one of them answered
    assert min(served) > 0, served
    g.close()


# ---- 7. half-iteration after a write -----------------------------------------------------------------------------------
def test_half_iteration_after_a_group_write_sees_the_new_factors():
    k = 16
    X, Y, ptr, col = model(80, 60, k, 9)
    rng = np.random.default_rng(10)
    g, _ = group_for(2, X, Y, ptr, col)
    c_csr = transpose(ptr, col, 60)
    g.set_matrix(Y_, *c_csr)
    g.half_iteration(X_)                                  # the Gramian of Y is cached on every member now
    g.set_preferences(rng.integers(0, 80, 50), rng.integers(0, 60, 50), np.ones(50, np.float32))
    Xw, Yw = g.get_factors(X_, 0, 80), g.get_factors(Y_, 0, 60)
    ones = np.ones(len(col), np.float32)
    g.half_iteration(X_)
    g.synchronize()
    Xh = g.get_factors(X_, 0, 80)
    assert rel(Xh, oracle.half_iteration(ptr, col, ones, Yw, threads=4)) < REL_TOL
    g.half_iteration(Y_)
    g.synchronize()
    Yh = g.get_factors(Y_, 0, 60)
    assert rel(Yh, oracle.half_iteration(*c_csr, Xh, threads=4)) < REL_TOL
    assert not np.array_equal(Xh, Xw) and not np.array_equal(Yh, Yw)
    for m in range(2):
        core, _ = g.local(m)
        assert np.array_equal(bits(core.get_factors(X_)), bits(Xh)) and np.array_equal(bits(core.get_factors(Y_)), bits(Yh))
    assert g.replica_digest(X_)[1] and g.replica_digest(Y_)[1]
    g.close()


# ---- 8. a new generation drops the overlays ------------------------------------------------------------------------------
def test_a_new_generation_drops_the_overlays_on_every_member():
    k = 8
    X, Y, ptr, col = model(12, 200, k, 13)
    g, (sx, sy) = group_for(3, X, Y, ptr, col)
    users = np.arange(12)
    idx, _, _ = g.recommend(users, 3)
    g.set_preferences(users, idx[:, 0], np.ones(12, np.float32))
    after, _, _ = g.recommend(users, 3)
    assert all(int(idx[q, 0]) not in after[q].tolist() for q in range(12))
    g.set_matrix(X_, ptr, col, np.ones(len(col), np.float32))      # the next generation's R: the writes' items are back
    Xw, Yw = g.get_factors(X_, 0, 12), g.get_factors(Y_, 0, 200)
    top_same(g, Xw, Yw, known_of(ptr, col), users, how_many=3)
    g.close()


# ---- 9. two writers, readers alongside -----------------------------------------------------------------------------------
def run_threads(fns):
    errors = []

    def guarded(fn):
        try:
            fn()
        except Exception as e:   # pragma: no cover
            errors.append(repr(e))

    th = [threading.Thread(target=guarded, args=(fn,)) for fn in fns]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errors, errors[:3]


def test_two_writers_of_disjoint_rows_commute():
    k = 16
    X, Y, ptr, col = model(80, 60, k, 31)
    g, (sx, sy) = group_for(3, X, Y, ptr, col)
    rng = np.random.default_rng(32)
    # writer A: users < 40 and items < 30; writer B: the others -- no row in common, so the order does not matter
    batches = {w: [(rng.integers(lo_u, lo_u + 40, 30), rng.integers(lo_i, lo_i + 30, 30), rng.choice([1.0, 2.0, -1.0], 30).astype(np.float32))
                   for _ in range(10)] for w, (lo_u, lo_i) in enumerate([(0, 0), (40, 30)])}
    run_threads([lambda w=w: [g.set_preferences(*b) for b in batches[w]] for w in (0, 1)])
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    for w in (0, 1):
        for (u, i, v) in batches[w]:
            assert not fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy).any()
    check_group(g, Xo, Yo)
    top_same(g, Xo, Yo, known, np.arange(80))
    assert g.foldin_stats()["applied"] == 600
    g.close()


def test_two_writers_of_the_same_rows_leave_the_members_equal():
    k = 16
    X, Y, ptr, col = model(40, 30, k, 33)
    g, _ = group_for(3, X, Y, ptr, col)
    rng = np.random.default_rng(34)
    batches = {w: [(rng.integers(0, 40, 12), rng.integers(0, 5, 12), rng.choice([1.0, 2.0, -1.0, 0.5], 12).astype(np.float32))
                   for _ in range(50)] for w in (0, 1)}       # every batch hits the same 5 items: the order matters
    run_threads([lambda w=w: [g.set_preferences(*b) for b in batches[w]] for w in (0, 1)])
    Xm = [g.local(m)[0].get_factors(X_) for m in range(3)]
    Ym = [g.local(m)[0].get_factors(Y_) for m in range(3)]
    assert not np.array_equal(Ym[0][:5], Y[:5])
    for m in (1, 2):       # whatever order the two writers got, every member saw the same one
        assert np.array_equal(bits(Xm[m]), bits(Xm[0])) and np.array_equal(bits(Ym[m]), bits(Ym[0]))
    for side, M in ((X_, Xm[0]), (Y_, Ym[0])):
        d, eq = g.replica_digest(side)
        assert eq and int(d[0]) == int(d[1]) == int(d[2]) == pkg.factor_digest_host(M)
    assert g.foldin_stats()["applied"] == 1200
    g.close()


def test_readers_alongside_a_writer_see_whole_models():
    k = 16
    n_users = 48
    X, Y, ptr, col = model(n_users, 400, k, 35, nnz_per_user=2)
    g, (sx, sy) = group_for(3, X, Y, ptr, col)
    rng = np.random.default_rng(36)
    batches = [(rng.integers(0, n_users, 30), rng.integers(0, 400, 30), np.ones(30, np.float32)) for _ in range(20)]
    eu, ei = rng.integers(0, n_users, 8), rng.integers(0, 400, 8)
    Xo, Yo, known = X.copy(), Y.copy(), known_of(ptr, col)
    tops, ests = [], []

    def snapshot():
        tops.append([to.recommend(Yo, Xo[uu], 5, known=sorted(known.get(uu, ()))) for uu in range(n_users)])
        ests.append(bits(fo.estimate_preferences(Xo, Yo, eu, ei)).copy())

    snapshot()
    for (u, i, v) in batches:
        fo.set_preferences(Xo, Yo, known, u, i, v, sx, sy)
        snapshot()                                           # the 21 models a reader may see
    stop = threading.Event()
    bad = []

    def writer():
        try:
            for b in batches:
                g.set_preferences(*b)
        finally:
            stop.set()

    def reader(seed):
        r = np.random.default_rng(seed)
        while True:
            last = stop.is_set()                              # (one more round after the writer is done)
            uu = int(r.integers(0, n_users))
            idx, sc, cnt = g.recommend([uu], 5)
            if not any(np.array_equal(idx[0, :cnt[0]], t[uu][0]) and np.array_equal(bits(sc[0, :cnt[0]]), bits(t[uu][1])) for t in tops):
                bad.append(("recommend", uu))
            e = bits(g.estimate_preferences(eu, ei))
            if not any(np.array_equal(e, x) for x in ests):
                bad.append(("estimate", e.tolist()))
            if last:
                return

    run_threads([writer] + [lambda s=s: reader(s) for s in range(4)])
    assert not bad, bad[:3]
    check_group(g, Xo, Yo)
    g.close()


# ---- 10. the digest on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 30, 50, 64, 128])
def test_device_digest_is_the_host_digest(k):
    rng = np.random.default_rng(k)
    n = 5000
    F = rng.integers(0, 1 << 32, n * k, dtype=np.uint64).astype(np.uint32).view(np.float32).reshape(n, k)   # any bits: NaNs, -0.0
    F[11, 0] = -0.0
    with pkg.ALSCore(k) as c:
        c.set_factor_rows(Y_, n)
        c.set_factors(Y_, F)
        back = c.get_factors(Y_)
        assert np.array_equal(bits(back), bits(F))
        for n_rows in (1, 3, 255, 256, 257, 5000):
            for row_begin in (0, 1, 7):           # row_begin * k * 4 bytes: unaligned heads at k = 1, 2, 30, 50
                rows = min(n_rows, n - row_begin)
                assert c.factor_digest(Y_, row_begin, rows) == pkg.factor_digest_host(back[row_begin:row_begin + rows], row_begin), (n_rows, row_begin)
        assert c.factor_digest(Y_, 9, 0) == 0 and c.factor_digest(Y_, n, 0) == 0
        assert c.factor_digest(Y_) == pkg.factor_digest_host(back)
        with pytest.raises(MalsError):
            c.factor_digest(Y_, n - 1, 2)
        with pytest.raises(MalsError):
            c.factor_digest(Y_, -1, 1)


def test_replica_digest_names_the_member_that_differs():
    k = 30
    X, Y, ptr, col = model(40, 30, k, 41)
    g, _ = group_for(3, X, Y, ptr, col)
    d, eq = g.replica_digest(Y_)
    assert eq and len(set(d.tolist())) == 1
    row = Y[17:18].copy()
    row.view(np.uint32)[0, 29] ^= np.uint32(1)              # one bit, in one member's replica
    g.local(1)[0].set_factors(Y_, row, 17)
    d, eq = g.replica_digest(Y_)
    assert not eq and d[0] == d[2] != d[1]
    assert int(d[0]) == pkg.factor_digest_host(Y)
    Y1 = Y.copy()
    Y1[17] = row[0]
    assert int(d[1]) == pkg.factor_digest_host(Y1)
    # only the band that holds the row differs
    assert g.replica_digest(Y_, 0, 17)[1] and g.replica_digest(Y_, 18)[1] and not g.replica_digest(Y_, 17, 1)[1]
    assert g.local(1)[0].factor_digest(Y_, 17, 1) == pkg.factor_digest_host(row, 17)      # members are allowed
    g.close()


# ---- 11. refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    k = 8
    X, Y, ptr, col = model(10, 20, k, 51)
    g, _ = group_for(2, X, Y, ptr, col)
    for u, i in (([10], [0]), ([0], [20]), ([-1], [0]), ([0], [-1])):          # rows outside the replicas
        with pytest.raises(MalsError) as e:
            g.set_preferences(u, i, [1.0])
        assert e.value.status == _lib.INVALID_ARG
        with pytest.raises(MalsError) as e:
            g.remove_preferences(u, i)
        assert e.value.status == _lib.INVALID_ARG
    with pytest.raises(MalsError) as e:
        g.estimate_preferences([10], [0])
    assert e.value.status == _lib.INVALID_ARG
    with pytest.raises(MalsError, match="only grows") as e:
        g.grow_factor_rows(X_, 5)
    assert e.value.status == _lib.INVALID_ARG
    with pytest.raises(MalsError):
        g.replica_digest(X_, 5, 6)
    check_group(g, X, Y)                                   # none of it touched the model
    m, _ = g.local(0)                                      # the member's handle stays refused on the single-handle calls
    with pytest.raises(MalsError, match="group"):
        m.set_preferences([0], [0], [1.0])
    with pytest.raises(MalsError, match="group"):
        m.estimate_preferences([0], [0])
    with pytest.raises(MalsError, match="group"):
        m.grow_factor_rows(X_, 20)
    g.close()


def _rank_of_two(q):
    """Rank 0 of a world-2 group over the tests' stand-in transport (its communicator comes up without the peer): every twin
    answers from its argument check, before anything would be sent."""
    try:
        import myrrix_recommender_amd as pkg
        from myrrix_recommender_amd import _lib
        from myrrix_recommender_amd.core import MalsError
        pkg.GroupALS.use_transport(MOCK)
        out = []
        with pkg.GroupALS.from_unique_id(8, 0, 2, 0, pkg.GroupALS.unique_id()) as g:
            calls = [lambda: g.set_foldin_solver(pkg.SIDE_X, None), lambda: g.set_foldin_learn_rate(1.0), g.foldin_stats,
                     lambda: g.set_preferences([0], [0], [1.0]), lambda: g.remove_preferences([0], [0]),
                     lambda: g.grow_factor_rows(pkg.SIDE_X, 10), lambda: g.estimate_preferences([0], [0]),
                     lambda: g.anonymous_features([[0]]), lambda: g.recommend_to_anonymous([[0]], 3),
                     lambda: g.estimate_for_anonymous([0], [[0]]),
                     lambda: g._chk(g._L.mals_group_replica_digest(g._g, pkg.SIDE_X, 0, 0, (ctypes.c_uint64 * 1)(), None))]
            for call in calls:
                try:
                    call()
                    out.append((_lib.OK, ""))
                except MalsError as e:
                    out.append((e.status, str(e.message)))
        q.put(("ok", out))
    except Exception as e:  # noqa: BLE001 -- reported to the parent
        q.put(("error", repr(e)))


def test_ranks_of_a_multi_process_group_are_refused():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rank_of_two, args=(q,))
    p.start()
    res = q.get(timeout=120)
    p.join(timeout=60)
    assert res[0] == "ok", res
    assert len(res[1]) == 11
    for code, msg in res[1]:
        assert code == _lib.INVALID_ARG and "several processes" in msg, (code, msg)
