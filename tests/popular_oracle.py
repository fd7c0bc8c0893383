"""TEST INFRASTRUCTURE ONLY -- CPU restatement of ServerRecommender.mostPopularItems (what mals_most_popular_items and
mals_group_most_popular_items must return, bit for bit).

  mostPopularItems         online/src/net/myrrix/online/ServerRecommender.java:611-673
      :622       knownItemIDs == null -> UnsupportedOperationException
      :636-648   for every user of knownItemIDs that is no itemTagID: itemCounts.increment(itemID, 1.0f) per item of its SET
      :657-667   the items that are userTagIDs leave itemCounts
      :672       TopN.selectTopN(new MostPopularItemsIterator(itemCounts, rescorer), howMany)
  MostPopularItemsIterator online/src/net/myrrix/online/MostPopularItemsIterator.java:51-67
      :56-59     a filtered item is skipped
      :60        value = (float) rescorer.rescore(id, value)
      :61-63     a value that is not finite is skipped (no checkState: never an error)

The library's own rule on top: equal values come back in ascending item index (the reference leaves them in hash order).

`most_popular` is the vectorised restatement the GPU tests compare with; `most_popular_literal` transliterates the loops
item by item, float increments included, and pins it (tests/test_popular_oracle.py)."""
import numpy as np

SATURATED = 1 << 24   # fp32: 2^24 + 1.0f rounds back to 2^24, increment(id, 1.0f) stops moving there (:644)


def float_count(counts):
    """the float(s) that `counts` increments by 1.0f reach from 0.0f (FastByIDFloatMap.increment, :644)"""
    return np.minimum(np.asarray(counts, np.int64), SATURATED).astype(np.float32)


def float_count_literal(count, start=np.float32(0.0)):
    """... literally: `count` fp32 additions of 1.0f"""
    v = np.float32(start)
    for _ in range(int(count)):
        v = np.float32(v + np.float32(1.0))
    return v


def counts_from_sets(sets, n_items, item_tag_users=()):
    """count(i) over the users of `sets` (dict user -> iterable of items, or a list indexed by user) that are no
    itemTagIDs (:636-648); a user's items count once each (a FastIDSet), items outside [0, n_items) own no row"""
    skip = set(int(u) for u in item_tag_users)
    items = sets.items() if isinstance(sets, dict) else enumerate(sets)
    counts = np.zeros(n_items, np.int64)
    for u, s in items:
        if int(u) in skip:
            continue
        for i in set(int(i) for i in s):
            if 0 <= i < n_items:
                counts[i] += 1
    return counts


def counts_from_csr(ptr, idx, n_items, item_tag_users=()):
    """the same from a CSR over the users (rows need not be sorted, repeats count once), vectorised"""
    ptr = np.asarray(ptr, np.int64)
    idx = np.asarray(idx, np.int64)
    users = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    keep = (idx >= 0) & (idx < n_items)
    if len(item_tag_users):
        keep &= ~np.isin(users, np.asarray(list(item_tag_users), np.int64))
    users, idx = users[keep], idx[keep]
    ascending = np.all((np.diff(idx) > 0) | (np.diff(users) != 0)) if len(idx) > 1 else True
    if not ascending:                                    # a set per user: (user, item) pairs once
        idx = np.unique(users * np.int64(n_items) + idx) % np.int64(n_items)
    return np.bincount(idx, minlength=n_items).astype(np.int64)


def most_popular(counts, how_many, user_tag_items=(), rescorer=None):
    """(item indices int64, values float32) best first, equal values in ascending index.  rescorer: an object with
    is_filtered / rescore / arrays as tests/rescorer_oracle.AffineRescorer, or None."""
    counts = np.asarray(counts, np.int64)
    n_items = len(counts)
    ok = counts > 0                                      # only the keys of itemCounts are candidates
    tags = np.asarray(list(user_tag_items), np.int64)
    ok[tags[(tags >= 0) & (tags < n_items)]] = False     # :657-667
    value = float_count(counts)
    if rescorer is not None:
        sc, of, filt = rescorer.arrays(n_items)
        with np.errstate(over="ignore", invalid="ignore"):
            r = sc * value.astype(np.float64) + of       # numpy: one rounding per operation, as Java's a * s + b
            value = r.astype(np.float32)                 # :60
        ok &= ~filt & np.isfinite(value)                 # :57, :61
    idx = np.flatnonzero(ok)
    order = np.lexsort((idx, -value[idx].astype(np.float64)))[:how_many]
    return idx[order].astype(np.int64), value[idx][order]


def most_popular_literal(sets, n_items, how_many, item_tag_users=(), user_tag_items=(), rescorer=None):
    """ServerRecommender.java:611-673 and MostPopularItemsIterator.next line by line, with the float increments"""
    if sets is None:
        raise NotImplementedError("UnsupportedOperationException")          # :622
    item_tag_users = set(int(u) for u in item_tag_users)
    user_tag_items = set(int(i) for i in user_tag_items)
    item_counts = {}
    for user, items in (sets.items() if isinstance(sets, dict) else enumerate(sets)):   # :636
        if int(user) in item_tag_users:                                     # :638
            continue
        for item in set(int(i) for i in items):                             # :641-645
            if 0 <= item < n_items:
                item_counts[item] = np.float32(item_counts.get(item, np.float32(0.0)) + np.float32(1.0))
    for item in list(item_counts):                                          # :662-667
        if item in user_tag_items:
            del item_counts[item]
    out = []
    for item, value in item_counts.items():                                 # MostPopularItemsIterator.next
        if rescorer is not None:
            if rescorer.is_filtered(item):                                  # :57
                continue
            with np.errstate(over="ignore", invalid="ignore"):
                value = np.float32(rescorer.rescore(item, float(value)))    # :60
            if not np.isfinite(value):                                      # :61
                continue
        out.append((item, np.float32(value)))
    out.sort(key=lambda t: (-float(t[1]), t[0]))
    out = out[:how_many]
    return np.array([i for i, _ in out], np.int64), np.array([v for _, v in out], np.float32)
