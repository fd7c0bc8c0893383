"""mals_most_popular_items against tests/popular_oracle.py (ServerRecommender.java:611-673): item indices and score bits
are compared array_equal.  Counts are small integers, so nearly every case here has ties at the cut."""
import threading

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib, ingest
from myrrix_recommender_amd.core import HostSolver, MalsError
from tests import popular_oracle as po
from tests.rescorer_oracle import AffineRescorer

pytestmark = pytest.mark.gpu
X_, Y_ = pkg.SIDE_X, pkg.SIDE_Y
K = 4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows]) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, idx.astype(np.int32)


def make_core(n_users, n_items, ptr=None, idx=None, factors_seed=None):
    """a handle whose rows of R are (ptr, idx), or an empty R (the known items then come from set_known_items)"""
    core = pkg.ALSCore(K)
    core.set_factor_rows(X_, n_users)
    core.set_factor_rows(Y_, n_items)
    if ptr is None:
        ptr, idx = np.zeros(n_users + 1, np.int64), np.zeros(0, np.int32)
    core.set_matrix(X_, ptr, idx, np.ones(len(idx), np.float32))
    if factors_seed is not None:
        rng = np.random.default_rng(factors_seed)
        X = (rng.standard_normal((n_users, K)) * 0.3).astype(np.float32)
        Y = (rng.standard_normal((n_items, K)) * 0.3).astype(np.float32)
        core.set_factors(X_, X)
        core.set_factors(Y_, Y)
        core.set_foldin_solver(X_, HostSolver.create(X.astype(np.float64).T @ X.astype(np.float64)))
        core.set_foldin_solver(Y_, HostSolver.create(Y.astype(np.float64).T @ Y.astype(np.float64)))
    return core


def same(got, want, how_many):
    idx, sc, n = got
    oi, ov = want
    assert n == len(oi), (n, len(oi))
    assert np.array_equal(idx[:n], oi), (idx[:n], oi)
    assert np.array_equal(bits(sc[:n]), bits(ov)), (sc[:n], ov)
    assert len(idx) == how_many and np.all(idx[n:] == -1) and np.all(np.isneginf(sc[n:]))


# ---- the small base case ---------------------------------------------------------------------------------------------------
def small_rows():
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 98, 300)
    lens[[3, 50, 298]] = 0                                   # empty rows
    lens[7] = 97                                             # one full row
    lens[0] = 40                                             # (tag users with something to lose)
    lens[17] = 60
    lens[299] = 5
    # popularity falls with the index, so the counts spread and still tie
    p = 1.0 / (1.0 + np.arange(97))
    p /= p.sum()
    return [np.sort(rng.choice(97, int(n), replace=False, p=p if n < 60 else None)) for n in lens]


SMALL = {}


def small_reference():
    if not SMALL:
        rows = small_rows()
        SMALL["rows"] = rows
        SMALL["counts"] = po.counts_from_sets(rows, 97, item_tag_users=[0, 17, 299])
        assert SMALL["counts"].max() > 100 and (np.bincount(SMALL["counts"]) > 1).any()
    return SMALL


@pytest.mark.parametrize("installed", [True, False])
def test_small_base_case(installed):
    ref = small_reference()
    ptr, idx = csr(ref["rows"])
    core = make_core(300, 97) if installed else make_core(300, 97, ptr, idx)
    with core:
        if installed:
            core.set_known_items(ptr, idx)
        core.set_tag_users([0, 17, 299, 300, -1, 5000])      # rows outside the handle's users are ignored
        assert core.tag_user_count() == 3
        core.set_tag_items([5, 96])
        for how_many in (1, 10, 97, 200):
            same(core.most_popular_items(how_many), po.most_popular(ref["counts"], how_many, user_tag_items=[5, 96]), how_many)
        st = core.most_popular_stats()
        assert st["calls"] == 4 and st["recounts"] == 1 and st["overlay_rows"] == 0
        assert st["pairs"] == int(ref["counts"].sum())
        core.set_tag_users(None)                             # n = 0 clears: the three users count again
        assert core.tag_user_count() == 0
        same(core.most_popular_items(97), po.most_popular(po.counts_from_sets(ref["rows"], 97), 97, user_tag_items=[5, 96]), 97)
        assert core.most_popular_stats()["recounts"] == 2


def test_no_known_items_is_invalid():
    with pkg.ALSCore(K) as core:
        core.set_factor_rows(X_, 10)
        core.set_factor_rows(Y_, 10)
        with pytest.raises(MalsError) as e:                  # UnsupportedOperationException (:622)
            core.most_popular_items(3)
        assert e.value.status == _lib.INVALID_ARG
    with make_core(10, 10, *csr([[1]] * 10)) as core:
        for bad in (0, 4097):
            with pytest.raises(MalsError) as e:
                core.most_popular_items(bad)
            assert e.value.status == _lib.INVALID_ARG


# ---- ties: the cut falls inside a block of equal counts -------------------------------------------------------------------
@pytest.mark.parametrize("n_items,n_tied", [(5000, 3000), (70000, 40000)])
def test_ties_at_the_cut(n_items, n_tied):
    rng = np.random.default_rng(n_items)
    perm = rng.permutation(n_items)
    tied, hot = perm[:n_tied], perm[n_tied:n_tied + 40]      # 40 items above the block, the rest unknown to everybody
    # user 0 knows every tied item and nobody else does: count exactly 1; hot[m] is known to m + 2 of the users 1..41
    rows = [np.sort(tied)] + [np.sort(hot[max(0, j - 1):]) for j in range(41)]
    ptr, idx = csr(rows)
    counts = po.counts_from_sets(rows, n_items)
    assert (counts == 1).sum() == n_tied
    with make_core(len(rows), n_items) as core:
        core.set_known_items(ptr, idx)
        got = core.most_popular_items(100)
        same(got, po.most_popular(counts, 100), 100)
        assert np.array_equal(got[0][40:], np.sort(tied)[:60])   # the lowest indices of the block win
        same(core.most_popular_items(4096), po.most_popular(counts, 4096), 4096)


# ---- unsorted rows with repeated items ------------------------------------------------------------------------------------
def test_unsorted_rows_and_repeats_count_once():
    rng = np.random.default_rng(5)
    rows = []
    for u in range(200):
        r = rng.integers(0, 150, int(rng.integers(0, 80)))   # with replacement: repeats, any order
        rows.append(r)
    rows[10] = np.array([7] * 70)                            # one item, seventy times, longer than a wave
    rows[11] = np.arange(149, -1, -1)                        # descending
    ptr, idx = csr(rows)
    counts = po.counts_from_sets(rows, 150)
    assert np.array_equal(counts, po.counts_from_csr(ptr, idx, 150))
    with make_core(200, 150) as core:
        core.set_known_items(ptr, idx)
        for how_many in (5, 150):
            same(core.most_popular_items(how_many), po.most_popular(counts, how_many), how_many)
        assert core.most_popular_stats()["pairs"] == int(counts.sum())
        # items outside the catalogue are ignored, never written: the same rows on a handle of 100 items
    with make_core(200, 100) as core:
        core.set_known_items(ptr, idx)
        same(core.most_popular_items(100), po.most_popular(po.counts_from_sets(rows, 100), 100), 100)


# ---- saturation -----------------------------------------------------------------------------------------------------------
def test_the_value_saturates_at_two_to_the_24():
    n_users = (1 << 24) + 3
    lens = np.ones(n_users, np.int64)
    lens[:5] = 2
    ptr = np.zeros(n_users + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    idx = np.zeros(int(ptr[-1]), np.int32)
    idx[ptr[:5] + 1] = 1                                     # users 0..4: {0, 1}
    counts = np.zeros(8, np.int64)
    counts[0], counts[1] = n_users, 5
    with make_core(n_users, 8) as core:
        core.set_known_items(ptr, idx)
        got = core.most_popular_items(3)
        same(got, po.most_popular(counts, 3), 3)
        assert got[0][:2].tolist() == [0, 1] and got[1][0] == np.float32(16777216.0) and got[1][1] == np.float32(5.0)
        assert core.most_popular_stats()["pairs"] == n_users + 5


# ---- writes ---------------------------------------------------------------------------------------------------------------
def test_writes_move_the_counts_and_only_they_recount():
    rng = np.random.default_rng(21)
    n_users, n_items = 120, 60
    rows = [np.sort(rng.choice(n_items, int(rng.integers(1, 9)), replace=False)) for _ in range(n_users)]
    rows[40] = np.array([13])                                # a user with one item: removing it empties the user
    ptr, idx = csr(rows)
    sets = {u: set(int(i) for i in r) for u, r in enumerate(rows)}
    tag_users, tag_items = [2, 40 + 1], [0]

    def check(core, recounts, overlay_rows=None, rescorer=None, oracle_rescorer=None):
        want = po.most_popular(po.counts_from_sets(sets, n_items, tag_users), 25, tag_items, oracle_rescorer)
        same(core.most_popular_items(25, rescorer), want, 25)
        st = core.most_popular_stats()
        assert st["recounts"] == recounts, st
        if overlay_rows is not None:
            assert st["overlay_rows"] == overlay_rows, st

    with make_core(n_users, n_items, ptr, idx, factors_seed=3) as core:
        core.set_tag_users(tag_users)
        core.set_tag_items(tag_items)
        check(core, 1, 0)
        check(core, 1)                                       # two calls in a row: one recount
        new = int(next(i for i in range(n_items) if i not in sets[5]))
        core.set_preferences([5], [new], [1.0])              # a new pair
        sets[5].add(new)
        check(core, 2, 1)
        core.set_preferences([5], [int(rows[5][0])], [1.0])  # a pair the base row already holds: the set does not change
        check(core, 3, 1)
        core.set_preferences([5], [new], [2.0])              # ... and one an earlier write added
        check(core, 4, 1)
        core.grow_factor_rows(X_, n_users + 2)               # a grown user, written
        core.set_preferences([n_users + 1, n_users + 1], [7, 9], [1.0, 1.0])
        sets[n_users + 1] = {7, 9}
        check(core, 5, 2)                                    # two batches since the last call: one recount
        base = 5
        gone = int(rows[8][0])
        core.remove_preferences([8], [gone])                 # user 8 becomes a replaced set
        sets[8].discard(gone)
        check(core, base + 1, 3)
        removed = core.remove_preferences([40], [13])        # a user's last item
        assert removed.tolist() == [40]
        sets[40] = set()
        check(core, base + 2, 4)
        core.set_preferences([2], [33], [1.0])               # a tag user's write is not counted, before or after
        sets[2].add(33)
        check(core, base + 3, 4)
        # what acts after the count never recounts: the tag items and the rescorer
        tag_items.append(int(po.most_popular(po.counts_from_sets(sets, n_items, tag_users), 1, tag_items)[0][0]))
        core.set_tag_items(tag_items)
        check(core, base + 3)
        with core.rescorer() as r:
            r.set_filter([4, 6])
            check(core, base + 3, rescorer=r, oracle_rescorer=AffineRescorer(filtered=[4, 6]))
            r.set_uniform(2.0, 0.5)
            check(core, base + 3, rescorer=r, oracle_rescorer=AffineRescorer(filtered=[4, 6], scale=2.0, offset=0.5))
        core.set_known_items(ptr, idx)                       # a new generation: the writes are gone with the overlay
        for u, r in enumerate(rows):
            sets[u] = set(int(i) for i in r)
        del sets[n_users + 1]
        check(core, base + 4, 0)


# ---- rescorers ------------------------------------------------------------------------------------------------------------
def test_rescorers():
    ref = small_reference()
    ptr, idx = csr(ref["rows"])
    counts = po.counts_from_sets(ref["rows"], 97)
    rng = np.random.default_rng(8)
    with make_core(300, 97, ptr, idx) as core, core.rescorer() as r:
        plain = core.most_popular_items(30)
        same(core.most_popular_items(30, r), (plain[0][:plain[2]], plain[1][:plain[2]]), 30)   # the identity: the plain call
        same(plain, po.most_popular(counts, 30), 30)
        filt = po.most_popular(counts, 3)[0].tolist() + [50]
        r.set_filter(filt)                                   # the three best and another go
        same(core.most_popular_items(30, r), po.most_popular(counts, 30, rescorer=AffineRescorer(filtered=filt)), 30)
        scale = np.exp(rng.uniform(-6, 6, 97))               # reorders across counts, far outside [2^-20, 2^20] is fine too
        scale[3] = 2.0 ** 40
        scale[4] = 2.0 ** -40
        offset = rng.uniform(-50, 50, 97)
        r.set_weights(scale, offset)
        orc = AffineRescorer(filtered=filt, scale=scale, offset=offset)
        for how_many in (1, 30, 97):
            same(core.most_popular_items(how_many, r), po.most_popular(counts, how_many, rescorer=orc), how_many)
        r.set_filter(None)
        r.set_uniform(0.125, -3.0)                           # uniform: the order of the plain call, other values
        got = core.most_popular_items(97, r)
        same(got, po.most_popular(counts, 97, rescorer=AffineRescorer(scale=0.125, offset=-3.0)), 97)
        assert np.array_equal(got[0], core.most_popular_items(97)[0])
        offset = np.zeros(97)
        offset[[1, 2]] = [1e39, -1e39]                       # (float) of it is infinite: skipped, and the call succeeds
        r.set_weights(None, offset)
        got = core.most_popular_items(97, r)
        same(got, po.most_popular(counts, 97, rescorer=AffineRescorer(offset=offset)), 97)
        assert 1 not in got[0] and 2 not in got[0] and got[2] == int((counts > 0).sum()) - 2
        same(core.most_popular_items(30, None), po.most_popular(counts, 30), 30)
        assert core.most_popular_stats()["recounts"] == 1    # rescorers act after the count
        with make_core(4, 4, *csr([[0]] * 4)) as other, other.rescorer() as r2:
            with pytest.raises(MalsError) as e:              # a rescorer is bound to its handle
                core.most_popular_items(3, r2)
            assert e.value.status == _lib.INVALID_ARG


# ---- threads --------------------------------------------------------------------------------------------------------------
def test_a_call_among_recommend_threads_answers_as_if_alone():
    rng = np.random.default_rng(31)
    n_users, n_items = 400, 3000
    rows = [np.sort(rng.choice(n_items, 20, replace=False)) for _ in range(n_users)]
    ptr, idx = csr(rows)
    with make_core(n_users, n_items, ptr, idx, factors_seed=9) as core:
        alone_top = core.recommend(np.arange(n_users), 10)
        alone = core.most_popular_items(50)
        same(alone, po.most_popular(po.counts_from_sets(rows, n_items), 50), 50)
        stop = threading.Event()
        errors = []

        def recommender(t):
            try:
                while not stop.is_set():
                    u = np.arange(t, n_users, 8)[:16]
                    i, s, _ = core.recommend(u, 10)
                    if not (np.array_equal(i, alone_top[0][u]) and np.array_equal(bits(s), bits(alone_top[1][u]))):
                        errors.append(("recommend", t))
                        return
            except Exception as e:                           # noqa: BLE001 -- reported below
                errors.append(e)

        threads = [threading.Thread(target=recommender, args=(t,)) for t in range(8)]
        for t in threads:
            t.start()
        try:
            for _ in range(20):
                got = core.most_popular_items(50)
                assert got[2] == alone[2] and np.array_equal(got[0], alone[0]) and np.array_equal(bits(got[1]), bits(alone[1]))
        finally:
            stop.set()
            for t in threads:
                t.join()
        assert not errors, errors
        assert core.most_popular_stats()["recounts"] == 1


# ---- install --------------------------------------------------------------------------------------------------------------
def test_ingest_install_hands_the_item_tags_over():
    from oracle import ingest_text_oracle as to
    from tests.test_gpu_ingest_text import build_corpus
    data = build_corpus(41, 3000, 0.05)
    want = to.expected([data])
    uid, iid = want["csr_x"][0], want["csr_y"][0]
    item_tags, user_tags = want["item_tag_ids"], want["user_tag_ids"]
    assert len(item_tags) and len(user_tags)                 # tags in both columns
    tag_users = np.flatnonzero(np.isin(uid, item_tags))      # the itemTagIDs that own a row of R
    tag_items = np.flatnonzero(np.isin(iid, user_tags))
    assert len(tag_users) and len(tag_items)
    kp, ki = want["known_ptr"], want["known_idx"]
    with ingest.Ingest(0) as g, pkg.ALSCore(K) as core:
        g.set_option(_lib.INGEST_OPT_KNOWN_ITEMS, 1)
        g.append_text(data, True)
        g.finish()
        core.set_factor_rows(X_, len(uid))
        core.set_factor_rows(Y_, len(iid))
        g.install(core)
        assert core.tag_user_count() == len(tag_users)
        assert core.tag_item_count() == len(tag_items)
        counts = po.counts_from_csr(kp, ki, len(iid), tag_users)
        for how_many in (10, len(iid)):
            same(core.most_popular_items(how_many), po.most_popular(counts, how_many, user_tag_items=tag_items), how_many)
