"""mals_generation_join_host / mals_generation_hash_host (include/myrrix_als.h, "loading a new generation") against
tests/generation_load_oracle.py on seeded inputs: no GPU, no handle.  The host join fills the same open-addressing table
with the same hash and the same slot rule as the device's, so the colliding set below walks a chain that is longer than a
wave and wraps around the end of the table."""
import numpy as np
import pytest

from myrrix_recommender_amd import _lib
from myrrix_recommender_amd.core import MalsError, generation_hash_host, generation_join_host
from tests import generation_load_oracle as glo

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
EXTREME = [I64_MIN, I64_MAX, -1, 0]


def np_hash(ids):
    """The hash of include/myrrix_als.h in numpy (uint64 arithmetic wraps)."""
    z = np.asarray(ids, dtype=np.int64).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    z ^= z >> np.uint64(32)
    z *= np.uint64(0xD6E8FEB86659FD93)
    z ^= z >> np.uint64(32)
    return z


def table_slots(n):
    s = 64
    while s < 2 * n:
        s <<= 1
    return s


def colliding_ids(n, n_table, seed=5):
    """n distinct ids whose home slot is the LAST slot of the table of n_table ids."""
    slots = table_slots(n_table)
    rng = np.random.default_rng(seed)
    found = np.zeros(0, dtype=np.int64)
    while len(found) < n:
        cand = rng.integers(I64_MIN, I64_MAX, size=1 << 18, dtype=np.int64, endpoint=True)
        hit = cand[(np_hash(cand) & np.uint64(slots - 1)) == np.uint64(slots - 1)]
        found = np.unique(np.concatenate([found, hit]))
    return np.random.default_rng(seed + 1).permutation(found)[:n]


def check(cur, new, recent, keep=False):
    want = glo.join(cur, new, recent, keep)
    flags = _lib.GENERATION_KEEP_NOT_UPDATED if keep else 0
    if want is None:
        with pytest.raises(MalsError) as ei:
            generation_join_host(cur, new, recent, flags)
        assert ei.value.status == _lib.INVALID_ARG
        return None
    got_map, got_counts = generation_join_host(cur, new, recent, flags)
    assert np.array_equal(got_map, want[0]) and got_counts == want[1]
    return got_map


def test_numpy_hash_is_the_librarys():
    rng = np.random.default_rng(0)
    ids = np.concatenate([np.array(EXTREME + [1, 2, 3, 1 << 32, -(1 << 32)], dtype=np.int64),
                          rng.integers(I64_MIN, I64_MAX, size=200, dtype=np.int64, endpoint=True)])
    assert np.array_equal(generation_hash_host(ids), np_hash(ids))


@pytest.mark.parametrize("seed", range(4))
def test_seeded_joins(seed):
    rng = np.random.default_rng(seed)
    pool = rng.permutation(np.unique(rng.integers(-10**12, 10**12, size=4000, dtype=np.int64)))
    n_cur, n_new = int(rng.integers(1, 1500)), int(rng.integers(1, 1500))
    cur = pool[:n_cur]
    shared = rng.permutation(cur)[: int(rng.integers(0, n_cur + 1))][:n_new]
    new = rng.permutation(np.concatenate([shared, pool[n_cur:n_cur + n_new - len(shared)]]))
    recent = rng.integers(0, n_cur, size=int(rng.integers(0, n_cur)))          # repeats allowed
    for keep in (False, True):
        m = check(cur, new, recent, keep)
        assert (m >= 0).sum() == len(set(m[m >= 0].tolist()))                  # no two live rows share a merged row


def test_extreme_ids_together():
    cur = np.array([7] + EXTREME + [8], dtype=np.int64)
    for new in ([I64_MIN, 0, 99], [-1, I64_MAX], EXTREME, [5]):
        for recent in ([], [1, 2, 3, 4], [0, 5]):
            check(cur, np.array(new, dtype=np.int64), recent)
    m = check(cur, np.array([0, I64_MIN], dtype=np.int64), [2, 3])
    assert m.tolist() == [-1, 1, 2, 3, 0, -1]


def test_duplicate_ids_on_either_side():
    assert check([1, 2, 3, 2], [4, 5], []) is None
    assert check([1, 2, 3], [4, 5, 4], [0]) is None
    assert check(EXTREME + [I64_MIN], [4], []) is None
    assert check([1, 2], [0, 0], []) is None                                   # 0 twice: an "empty" key word is an id too
    with pytest.raises(MalsError):
        generation_join_host([1, 2], [3], [2])                                 # a recent row outside the live rows


def test_no_live_rows_and_no_new_rows():
    m, c = generation_join_host([], [3, 1, 2], [])
    assert len(m) == 0 and c == {"n_merged": 3, "n_updated": 0, "n_kept": 0, "n_pruned": 0}
    check([], [3, 1, 2], [])
    check([5, 6, 7], [], [1])
    check([5, 6, 7], [], [], keep=True)


def test_three_hundred_ids_in_the_last_slot():
    new = colliding_ids(300, 300)
    slots = table_slots(300)
    assert slots == 1024 and len(set(new.tolist())) == 300
    home = generation_hash_host(new[:25]) & np.uint64(slots - 1)
    assert (home == np.uint64(slots - 1)).all()                                # the library's hash, not only the numpy copy
    rng = np.random.default_rng(11)
    others = colliding_ids(420, 300, seed=9)
    others = others[~np.isin(others, new)][:100]                               # same home slot, not in the new model: misses that walk the whole chain
    cur = rng.permutation(np.concatenate([new[:150], others, np.array(EXTREME, dtype=np.int64)]))
    recent = rng.permutation(len(cur))[:120]
    m = check(cur, new, recent)
    assert (m[np.isin(cur, new)] < 300).all() and (m[np.isin(cur, new)] >= 0).all()
    check(cur, new, [], keep=True)
