"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the reference's online write path (mals_set_preferences,
mals_remove_preferences, mals_estimate_preferences, mals_anonymous_features, mals_estimate_for_anonymous).  Not product
code: only tests/ and tools/bench_foldin.py may import it.  Updates are applied one at a time, in numpy with explicit
fp32 / fp64 casts; the fold-in solve is the package's host solver (HostSolver.solve_ftod, no GPU needed).

  foldInWeight                online/src/net/myrrix/online/ServerRecommender.java:981-994
  updateFeatures              :865-912 (estimate check :982, w == 0 :870-872, solves :876-885, item loop :888-896,
                              user loop :897-906; norm(userFoldIn) read in both branches)
  setPreference               :770-836 (the known items gain the item after updateFeatures returned)
  removePreference            :1001-1074
  buildAnonymousUserFeatures  :561-609
  estimatePreferences         :690-727
  estimateForAnonymous        :734-759
  SimpleVectorMath.dot / norm common/src/net/myrrix/common/math/SimpleVectorMath.java:34-63
"""
import math

import numpy as np

OK, INVALID_ARG = 0, 2
BIG_FOLDIN_THRESHOLD = 1e4
WHY_ESTIMATE, WHY_ITEM_DELTA, WHY_USER_DELTA, WHY_NO_YTY = 1, 2, 3, 4


def dot(x, y):
    """SimpleVectorMath.dot(float[], float[]): every product rounded to fp32, summed in fp64 from 0.0 in feature order."""
    p = (np.asarray(x, np.float32) * np.asarray(y, np.float32)).astype(np.float32)
    s = 0.0
    for v in p.tolist():
        s += v
    return s


def norm64(x):
    """SimpleVectorMath.norm(double[])."""
    s = 0.0
    for v in np.asarray(x, np.float64).tolist():
        s += v * v
    return math.sqrt(s)


def fold_in_weight(estimate, value, rate=1.0):
    """foldInWeight(double estimate, float value) (:981-994); the caller has checked that estimate is finite."""
    value = float(np.float32(value))
    if value > 0.0 and estimate < 1.0:
        multiplier = 1.0 - max(0.0, estimate)
        w = (1.0 - 1.0 / (1.0 + value)) * multiplier
    elif value < 0.0 and estimate > 0.0:
        multiplier = -min(1.0, estimate)
        w = (1.0 - 1.0 / (1.0 - value)) * multiplier
    else:
        w = 0.0
    return rate * w


def update_features(X, Y, u, i, value, sx, sy, rate=1.0):
    """updateFeatures on X[u], Y[i] in place.  sx / sy: HostSolver of X^T X / Y^T Y or None.  Returns (status, why,
    number of "fold in vector is large" warnings)."""
    xu, yi = X[u], Y[i]
    estimate = dot(xu, yi)
    if not math.isfinite(estimate):
        return INVALID_ARG, WHY_ESTIMATE, 0
    w = fold_in_weight(estimate, value, rate)
    if w == 0.0:
        return OK, 0, 0
    item_fold = sx.solve_ftod(xu.copy()) if sx is not None else None
    user_fold = sy.solve_ftod(yi.copy()) if sy is not None else None
    big = 0
    if item_fold is not None:
        if user_fold is None:   # norm(null): the reference throws before the item loop
            return INVALID_ARG, WHY_NO_YTY, 0
        big += norm64(user_fold) > BIG_FOLDIN_THRESHOLD
        for f in range(len(yi)):
            delta = w * float(item_fold[f])
            if not math.isfinite(delta):
                return INVALID_ARG, WHY_ITEM_DELTA, big
            yi[f] = np.float32(yi[f] + np.float32(delta))
    if user_fold is not None:
        big += norm64(user_fold) > BIG_FOLDIN_THRESHOLD
        for f in range(len(xu)):
            delta = w * float(user_fold[f])
            if not math.isfinite(delta):
                return INVALID_ARG, WHY_USER_DELTA, big
            xu[f] = np.float32(xu[f] + np.float32(delta))
    return OK, 0, big


def set_preferences(X, Y, known, users, items, values, sx, sy, rate=1.0):
    """setPreference for every update in order: X, Y (float32 arrays) and known (dict user -> set of items) in place.
    Returns the per-update status array."""
    st = np.zeros(len(users), np.int32)
    for t, (u, i, v) in enumerate(zip(users, items, values)):
        code, _, _ = update_features(X, Y, int(u), int(i), v, sx, sy, rate)
        st[t] = code
        if code == OK:
            known.setdefault(int(u), set()).add(int(i))
    return st


def remove_preferences(X, known, users, items):
    """removePreference for every pair in order; returns the users removed (their rows of X zeroed)."""
    removed = []
    for u, i in zip(users, items):
        u, i = int(u), int(i)
        s = known.get(u)
        if not s or i not in s:
            continue
        s.discard(i)
        if not s:
            del known[u]
            X[u] = 0.0
            removed.append(u)
    return removed


def anonymous_features(Y, items, values, sy, rate=1.0):
    """buildAnonymousUserFeatures: (features float32, ok).  items: item rows (-1 = no such item)."""
    acc = np.zeros(Y.shape[1], np.float32)
    if sy is None:
        return acc, False
    found = False
    for j, i in enumerate(items):
        if i < 0:
            continue
        found = True
        fold = sy.solve_ftod(Y[int(i)].copy())
        w = fold_in_weight(0.0, 1.0 if values is None else values[j], rate)
        if w != 0.0:
            for f in range(len(acc)):
                acc[f] = np.float32(acc[f] + np.float32(w * float(fold[f])))
    return acc, found


def estimate_preferences(X, Y, users, items):
    out = np.zeros(len(users), np.float32)
    for t, (u, i) in enumerate(zip(users, items)):
        if u >= 0 and i >= 0:
            out[t] = np.float32(dot(X[int(u)], Y[int(i)]))
    return out


def estimate_for_anonymous(Y, to_item, items, values, sy, rate=1.0):
    acc, ok = anonymous_features(Y, items, values, sy, rate)
    return np.float32(dot(acc, Y[int(to_item)])), ok
