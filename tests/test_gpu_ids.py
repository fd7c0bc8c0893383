"""The id directory resident on the handle (mals_ids_set / _lookup / _resolve / _get / _count) against a Python dict: rows,
row -> id, the grown replicas bit for bit, the refusals."""
import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd.core import MalsError, generation_hash_host

pytestmark = pytest.mark.gpu
X_, Y_ = pkg.SIDE_X, pkg.SIDE_Y
K = 8
I64 = np.iinfo(np.int64)
EXTREMES = [0, -1, I64.min, I64.max]


def core_with(n_rows, side=X_, seed=0):
    c = pkg.ALSCore(K)
    c.set_factor_rows(side, n_rows)
    F = (np.random.default_rng(seed).standard_normal((n_rows, K)) * 0.5).astype(np.float32)
    c.set_factors(side, F)
    return c, F


def distinct_ids(rng, n, first=()):
    ids = list(first)[:n]
    while len(ids) < n:
        x = int(rng.integers(I64.min, I64.max, endpoint=True))
        if x not in ids:
            ids.append(x)
    return np.array(ids, np.int64)


def dict_resolve(model, batch):
    rows, n_new = [], 0
    for x in batch:
        x = int(x)
        if x not in model:
            model[x] = len(model)
            n_new += 1
        rows.append(model[x])
    return np.array(rows, np.int64), n_new


def check_resolve(c, side, model, F, batch):
    """one resolve against the dict; -> the replica as it must be afterwards"""
    n_old = len(model)
    digest = c.factor_digest(side, 0, n_old)
    want, want_new = dict_resolve(model, batch)
    rows, n_new = c.rows_of(side, batch, add=True)
    assert n_new == want_new and np.array_equal(rows, want)
    ids = c.ids_of(side)
    assert len(ids) == len(model) and all(model[int(x)] == r for r, x in enumerate(ids))
    assert np.array_equal(c.ids_of(side, n_old, want_new), ids[n_old:])
    assert np.array_equal(c.rows_of(side, ids), np.arange(len(ids)))
    F = np.vstack([F, np.zeros((want_new, K), np.float32)])
    assert np.array_equal(c.get_factors(side).view(np.uint32), F.view(np.uint32))       # grown with zero rows, the old ones kept
    assert c.factor_digest(side, 0, n_old) == digest
    return F


@pytest.mark.parametrize("n", [1, 32, 33, 63, 64, 65])
def test_set_lookup_and_resolve_against_a_dict(n):
    rng = np.random.default_rng(n)
    ids = distinct_ids(rng, n, EXTREMES)
    rng.shuffle(ids)
    c, F = core_with(n, seed=n)
    c.set_ids(X_, ids)
    model = {int(x): r for r, x in enumerate(ids)}
    assert np.array_equal(c.ids_of(X_), ids)
    absent = [x for x in EXTREMES + distinct_ids(rng, 40).tolist() if x not in model]
    probe = np.array(ids.tolist() + absent + ids.tolist()[::-1], np.int64)
    assert np.array_equal(c.rows_of(X_, probe), [model.get(int(x), -1) for x in probe])
    assert len(c.rows_of(X_, [])) == 0
    # all known; all new; one new id 500 times; new and known interleaved with repeats (the extremes among them); two in a row
    F = check_resolve(c, X_, model, F, ids[::-1][:20])
    F = check_resolve(c, X_, model, F, distinct_ids(rng, 40))
    F = check_resolve(c, X_, model, F, np.full(500, int(rng.integers(1, 1 << 40)), np.int64))
    pool = np.array(EXTREMES + distinct_ids(rng, 30).tolist(), np.int64)
    known = np.array(list(model), np.int64)
    batch = np.where(np.arange(400) % 3 > 0, pool[rng.integers(0, len(pool), 400)], known[rng.integers(0, len(known), 400)])
    F = check_resolve(c, X_, model, F, batch)
    F = check_resolve(c, X_, model, F, batch[::-1])
    c.close()


def test_a_batch_larger_than_the_table_rebuilds_it_in_one_call_and_is_repeatable():
    rng = np.random.default_rng(7)
    ids = distinct_ids(rng, 32)
    new = distinct_ids(rng, 300)
    batch = np.concatenate([new[:150], ids[:10], new, new[::-1]])       # 300 new ids into a 32-id (64-slot) directory
    got = []
    for _ in range(2):                                                  # fresh handles: the same rows, whatever the scheduling
        c, F = core_with(32, side=Y_, seed=3)
        c.set_ids(Y_, ids)
        model = {int(x): r for r, x in enumerate(ids)}
        check_resolve(c, Y_, model, F, batch)
        got.append((c.rows_of(Y_, batch), c.ids_of(Y_)))
        c.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][1][32:], new)                          # the order of first appearance


def test_a_family_of_one_home_slot_at_the_tables_end():
    # 12 ids whose home is the last of 64 slots: the chain wraps to slot 0, in the directory and in a resolve's batch table
    fam = []
    x = 1
    while len(fam) < 24:
        if int(generation_hash_host([x])[0]) & 63 == 63:
            fam.append(x)
        x += 1
    fam = np.array(fam, np.int64)
    c, F = core_with(12, seed=5)
    c.set_ids(X_, fam[:12])
    model = {int(v): r for r, v in enumerate(fam[:12])}
    assert np.array_equal(c.rows_of(X_, fam), list(range(12)) + [-1] * 12)
    F = check_resolve(c, X_, model, F, np.concatenate([fam[12:][::-1], fam[:12], fam[12:]]))
    assert np.array_equal(c.rows_of(X_, fam[12:][::-1]), np.arange(12, 24))
    c.close()


def test_set_ids_from_device_memory_duplicates_and_clearing():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    ids = distinct_ids(rng, 65, EXTREMES)
    c, F = core_with(65)
    c.set_ids(X_, torch.from_numpy(ids).cuda())
    assert np.array_equal(c.ids_of(X_), ids)
    before = c.factor_digest(X_)
    twice = ids.copy()
    twice[64] = twice[3]
    twice[40] = twice[50]                                  # rows 50 and 64 repeat earlier rows: 50 is the smaller
    with pytest.raises(MalsError, match=r"row 50 repeats"):
        c.set_ids(X_, twice)
    assert np.array_equal(c.ids_of(X_), ids) and c.factor_digest(X_) == before           # nothing changed
    with pytest.raises(MalsError, match="one id per row"):
        c.set_ids(X_, ids[:64])
    with pytest.raises(MalsError, match="one id per row"):                                # 0 ids clear a side without rows only
        c.set_ids(X_, np.zeros(0, np.int64))
    c.close()
    # a directory of 0 ids: a side without a replica; cleared, and every call says that no row has an id
    c = pkg.ALSCore(K)
    c.set_ids(Y_, np.zeros(0, np.int64))
    for call in (lambda: c.rows_of(Y_, [1]), lambda: c.rows_of(Y_, [1], add=True), lambda: c.ids_of(Y_)):
        with pytest.raises(MalsError, match="no row"):
            call()
    c.close()


def test_refusals_until_the_ids_are_installed_again():
    rng = np.random.default_rng(13)
    ids = distinct_ids(rng, 20)
    c, F = core_with(20)
    every = (lambda: c.rows_of(X_, ids[:3]), lambda: c.rows_of(X_, [5], add=True), lambda: c.ids_of(X_), lambda: c.ids_of(X_, 0, 1))
    for call in every:                                     # never set
        with pytest.raises(MalsError, match=r"rows \[0, 20\) have no id"):
            call()
    c.set_ids(X_, ids)
    assert np.array_equal(c.rows_of(X_, ids), np.arange(20))
    c.grow_factor_rows(X_, 23)                             # grown directly: rows 20..22 have no id
    for call in every:
        with pytest.raises(MalsError, match=r"rows \[20, 23\) have no id"):
            call()
    more = np.concatenate([ids, distinct_ids(rng, 3)])
    c.set_ids(X_, more)
    assert np.array_equal(c.rows_of(X_, more), np.arange(23))
    c.set_factor_rows(X_, 23)                              # a new replica: the directory is dropped
    for call in every:
        with pytest.raises(MalsError, match=r"rows \[0, 23\) have no id"):
            call()
    c.set_ids(X_, more)
    assert np.array_equal(c.ids_of(X_), more)
    c.close()


def test_load_generation_drops_both_directories():
    rng = np.random.default_rng(17)
    uid, iid = distinct_ids(rng, 10), distinct_ids(rng, 6)
    c = pkg.ALSCore(K)
    for side, n in ((X_, 10), (Y_, 6)):
        c.set_factor_rows(side, n)
        c.set_factors(side, rng.standard_normal((n, K)).astype(np.float32))
    c.set_ids(X_, uid)
    c.set_ids(Y_, iid)
    new_u, new_i = np.concatenate([uid[:4], distinct_ids(rng, 2)]), iid[::-1].copy()
    _, (merged_u, merged_i), _ = c.load_generation(uid, iid, new_u, new_i, rng.standard_normal((6, K)).astype(np.float32),
                                                   rng.standard_normal((6, K)).astype(np.float32), keep_not_updated=True)
    for side in (X_, Y_):
        with pytest.raises(MalsError, match="have no id"):
            c.rows_of(side, [1])
    c.set_ids(X_, merged_u)                                 # the caller installs the merged ids the load hands back
    c.set_ids(Y_, merged_i)
    assert np.array_equal(c.rows_of(X_, merged_u), np.arange(len(merged_u)))
    assert np.array_equal(c.rows_of(Y_, iid), [int(np.nonzero(merged_i == x)[0][0]) for x in iid])
    c.close()


def test_a_member_of_a_group_is_refused():
    with pkg.GroupALS.single_process(K, [0], backend=pkg._lib.GROUP_PEER_COPY) as g:
        m, _ = g.local(0)
        for call in (lambda: m.set_ids(X_, [1, 2]), lambda: m.rows_of(X_, [1]), lambda: m.rows_of(X_, [1], add=True), lambda: m.ids_of(X_, 0, 1)):
            with pytest.raises(MalsError, match="group"):
                call()
