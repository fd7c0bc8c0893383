"""Rescored mostSimilarItems on the device (mals_most_similar_items_rescored, include/myrrix_als.h; the filter's bound in
csrc/topn_kernels.h, RESCORED COSINE MODE) against the CPU restatement tests/similar_rescored_oracle.py: indices and score
bits identical in every case, on the dense path and on the filter path -- where mals_similar_stats shows that the filter
answered."""
import os
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd.core import MalsError
from tests import rescorer_oracle as ro
from tests import similar_rescored_cases as cases
from tests import similar_rescored_oracle as sro
from tests import similarity_oracle as so
from tests.test_gpu_similarity import hard_Y, same_ranking, y_core

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_call(core, Y, Yn, queries, how_many, r, o, flag, tags=None, sample=None):
    idx, sc, cnt = core.most_similar_items(queries, how_many, rescorer=r, filter_query_items=flag)
    for q in (range(len(queries)) if sample is None else sample):
        oidx, osc = sro.most_similar(Y, queries[q], how_many, o, flag, tags=tags, Ynorm=Yn)
        same_ranking(idx[q], sc[q], cnt[q], oidx, osc)
    return idx, sc, cnt


# ---- dense path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 30, 64, 100, 128])
def test_dense_path_matches_the_oracle(k):
    n_items = 1000
    Y = hard_Y(n_items, k, 10 + k)
    Y[3] = 0.0                                                      # a zero query item
    tags = [5, 6, 12, 400]
    Yn = so.norms(Y)
    singles = [[11], [0], [3], [7], [999], [100]]
    multi = [[11, 20], [20, 20, 31], [3, 11], [1, 2, 4, 9], [11, 11, 500]]
    with y_core(Y) as core:
        core.set_tag_items(tags)
        before = core.similar_stats()
        n_q = 0
        for kind, spec in cases.rescorer_specs(n_items, 40 + k).items():
            r, o = cases.device_rescorer(core, spec), cases.oracle_rescorer(spec)
            for flag in (False, True):
                for how_many in (1, 10, 100):
                    check_call(core, Y, Yn, singles, how_many, r, o, flag, tags)
                    n_q += len(singles)
                check_call(core, Y, Yn, multi, 64, r, o, flag, tags)
                n_q += len(multi)
            r.close()
        st = core.similar_stats()
        assert st["dense"] - before["dense"] == n_q and st["rescored"] - before["rescored"] == n_q and st["filter"] == before["filter"]


def test_a_rescorer_outside_the_filters_range_is_answered_by_the_dense_path():
    k, n_items = 30, cases.FILTER_ITEMS
    Y = hard_Y(n_items, k, 77)
    Yn = so.norms(Y)
    rng = np.random.default_rng(77)
    with y_core(Y) as core:
        r = core.rescorer()
        # weights far outside the filter's range; r_j overflows fp64 for some items: they are skipped, never an error
        scale = np.exp(rng.uniform(np.log(1e-30), np.log(1e30), n_items))
        offset = rng.standard_normal(n_items) * 1e20
        c11 = so.cosine64(Y, Y[11])                                 # (the queries below are item 11, its scaled copies and its near-copy)
        big = np.flatnonzero(np.abs(c11) > 0.1)[:5000]
        scale[big] = 1.7e308
        offset[big] = np.where(c11[big] > 0, 1.7e308, -1.7e308)     # 1.7e308 (|s| + 1) overflows fp64
        r.set_weights(scale, offset)
        o = ro.AffineRescorer(scale=scale, offset=offset)
        _, ok = sro.scores(Y, [11], o, Ynorm=Yn)
        _, ok_plain = so.most_similar_scores(Y, [11], Yn)
        assert np.sum(ok_plain & ~ok) > 1000                        # the overflowing terms do skip items
        before = core.similar_stats()
        check_call(core, Y, Yn, [[11], [100], [300]], 10, r, o, False)
        check_call(core, Y, Yn, [[11, 300], [11, 11, 137]], 64, r, o, False)
        st = core.similar_stats()
        assert st["dense"] - before["dense"] == 5 and st["filter"] == before["filter"]
        # an offset just past the range (|offset| <= 2^6 scale): dense; just inside: the filter
        r.set_uniform(1.0, 64.5)
        check_call(core, Y, Yn, [[11]], 10, r, ro.AffineRescorer(scale=1.0, offset=64.5), False)
        assert core.similar_stats()["dense"] - st["dense"] == 1
        r.set_uniform(1.0, 64.0)
        check_call(core, Y, Yn, [[11]], 10, r, ro.AffineRescorer(scale=1.0, offset=64.0), False)
        assert core.similar_stats()["filter"] - st["filter"] == 1
        # a few items outside the range stay on the filter path, as candidates of every query: one that wins every query through
        # its scale, one that loses through its offset, one whose terms overflow (skipped), one beside a zero row
        st = core.similar_stats()
        scale, offset = np.ones(n_items), np.zeros(n_items)
        winner = int(np.flatnonzero((c11 > 0.3) & (c11 < 0.99))[0])
        scale[winner], offset[big[0]], scale[big[1]], offset[big[1]] = 2.0 ** 30, -1e10, 1.7e308, np.where(c11[big[1]] > 0, 1.7e308, -1.7e308)
        offset[int(np.flatnonzero(Yn == 0)[0])] = 1e39
        r.set_weights(scale, offset)
        o = ro.AffineRescorer(scale=scale, offset=offset)
        idx, _, _ = check_call(core, Y, Yn, [[11], [100], [11, 300]], 10, r, o, False)
        assert idx[0, 0] == winner
        five = offset.copy()
        five[20000] = 65.0                                           # a fifth: too many, the dense path
        r.set_weights(scale, five)
        check_call(core, Y, Yn, [[11]], 10, r, ro.AffineRescorer(scale=scale, offset=five), False)
        sim = core.similar_stats()
        assert sim["filter"] - st["filter"] == 3 and sim["dense"] - st["dense"] == 1
        r.close()


# ---- filter path ----------------------------------------------------------------------------------------------------------
FULL_RUN = r"""
import sys, pickle, numpy as np
sys.path.insert(0, %r)
import myrrix_recommender_amd as pkg
from tests import similar_rescored_cases as cases
k = %d
Y = cases.filter_catalogue(k)
specs, calls = cases.filter_calls(k)
core = pkg.ALSCore(k); core.set_factor_rows(pkg.SIDE_Y, len(Y)); core.set_factors(pkg.SIDE_Y, Y)
rs = {kind: cases.device_rescorer(core, spec) for kind, spec in specs.items()}
out = [core.most_similar_items(q, hm, rescorer=rs[kind], filter_query_items=flag) for kind, hm, flag, q in calls]
st = core.similar_stats()
assert st["filter"] == 0 and st["empty"] == 0 and st["dense"] == sum(len(c[3]) for c in calls), st
pickle.dump(out, open(%r, "wb"))
for r in rs.values():
    r.close()
core.close()
"""


@pytest.mark.parametrize("k", cases.FILTER_KS)
def test_filter_path_matches_the_oracle_and_the_dense_path_and_never_falls_back(k):
    import pickle
    Y = cases.filter_catalogue(k)
    Yn = so.norms(Y)
    specs, calls = cases.filter_calls(k)
    env = dict(os.environ)
    env.pop("MALS_TOPN_FULL", None)
    assert "MALS_TOPN_FULL" not in os.environ
    with y_core(Y) as core:
        rs = {kind: cases.device_rescorer(core, spec) for kind, spec in specs.items()}
        os_ = {kind: cases.oracle_rescorer(spec) for kind, spec in specs.items()}
        got = []
        n_live = n_dead = 0
        before = core.similar_stats()
        for kind, hm, flag, queries in calls:
            sample = list(range(0, len(queries), 5 if len(queries) < 100 else 25)) + [len(queries) - 1]
            got.append(check_call(core, Y, Yn, queries, hm, rs[kind], os_[kind], flag, sample=sample))
            dead = [flag and any(os_[kind].is_filtered(i) for i in q) for q in queries]
            n_dead += sum(dead)
            n_live += len(queries) - sum(dead)
            assert all(got[-1][2][q] == 0 for q in range(len(queries)) if dead[q])
        st = core.similar_stats()
        # EVERY live query of these calls was answered by the filter path: a silent fallback is a failure
        assert st["dense"] == before["dense"], st
        assert st["filter"] - before["filter"] == n_live and st["empty"] - before["empty"] == n_dead, (st, n_live, n_dead)
        assert st["rescored"] - before["rescored"] == n_live + n_dead
        assert n_dead == 2
        for r in rs.values():
            r.close()
    # the same calls with the filter switched off, in a process of their own: the same bits
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "full.pkl")
        env["MALS_TOPN_FULL"] = "1"
        subprocess.run([sys.executable, "-c", FULL_RUN % (ROOT, k, path)], check=True, env=env, timeout=600)
        full = pickle.load(open(path, "rb"))
    for (idx, sc, cnt), (fidx, fsc, fcnt) in zip(got, full):
        assert np.array_equal(idx, fidx) and np.array_equal(cnt, fcnt)
        assert np.array_equal(sc.view(np.uint32), fsc.view(np.uint32))


# ---- identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [1000, cases.FILTER_ITEMS])
def test_no_rescorer_and_the_identity_rescorer_give_the_plain_bits(n_items):
    k = 30
    Y = hard_Y(n_items, k, 5)
    queries = [[11], [0], [3], [11, 20], [20, 20, 31], [n_items - 1]]
    with y_core(Y) as core:
        plain = core.most_similar_items(queries, 20)
        L = core._L
        import ctypes
        from myrrix_recommender_amd.core import _item_queries
        flat, ptr = _item_queries(queries)
        idx = np.empty((len(queries), 20), np.int64)
        sc = np.empty((len(queries), 20), np.float32)
        cnt = np.empty(len(queries), np.int32)
        for flags in (0, 1):                                        # r = NULL: the plain call, whatever the flags
            assert L.mals_most_similar_items_rescored(core._h, None, flags, flat.ctypes.data_as(ctypes.c_void_p), ptr.ctypes.data_as(ctypes.c_void_p),
                                                      len(queries), 20, idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p),
                                                      cnt.ctypes.data_as(ctypes.c_void_p)) == 0
            assert np.array_equal(idx, plain[0]) and np.array_equal(sc.view(np.uint32), plain[1].view(np.uint32)) and np.array_equal(cnt, plain[2])
        st = core.similar_stats()
        assert st["rescored"] == 0 and st["filter"] + st["dense"] + st["empty"] == 3 * len(queries)
        r = core.rescorer()
        for flag in (False, True):
            got = core.most_similar_items(queries, 20, rescorer=r, filter_query_items=flag)
            assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1].view(np.uint32), plain[1].view(np.uint32)) and np.array_equal(got[2], plain[2])
        assert core.similar_stats()["rescored"] == 2 * len(queries)
        r.close()


def test_a_rescorer_of_another_handle_is_refused():
    Y = hard_Y(500, 8, 1)
    with y_core(Y) as a, y_core(Y) as b:
        r = a.rescorer()
        with pytest.raises(MalsError, match="another handle"):
            b.most_similar_items([1], 5, rescorer=r)
        r.close()


# ---- bad value ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [1000, cases.FILTER_ITEMS])
def test_a_non_finite_result_fails_its_own_call_only(n_items):
    """Item 17 carries offset 1e39: outside the filter's range of weights, but a rescorer with a few such items stays on the
    filter path (they are candidates of every query, topn_kernels.h), so at 150 000 items the calls below ARE folded into
    passes and the failure is one query's of a pass.  At 1000 items the dense path answers, one call at a time: there each call
    fails or succeeds alone."""
    k = 16
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((n_items, k)).astype(np.float32)
    offset = np.zeros(n_items)
    offset[17] = 1e39                                               # finite in fp64, not in fp32
    o = ro.AffineRescorer(offset=offset)
    Yn = so.norms(Y)
    queries = {0: [17], 1: [5], 2: [17, 17]}                        # 17's own queries strike it first; query 1 meets it
    expect = {t: sro.most_similar(Y, queries[t], 10, o, Ynorm=Yn) for t in (0, 2)}
    with pytest.raises(sro.BadSimilarityValue):
        sro.most_similar(Y, [5], 10, o, Ynorm=Yn)
    filter_path = n_items >= 131072
    REPS = 3
    with y_core(Y) as core:
        r = core.rescorer()
        r.set_weights(None, offset)
        idx, sc, cnt = core.most_similar_items([[17]], 10, rescorer=r)
        same_ranking(idx[0], sc[0], cnt[0], *expect[0])
        results, errors, broken = {}, {}, {}
        # a thirteenth thread sends an exclusive ticket every round (the weights of ANOTHER rescorer, milliseconds of upload):
        # while it holds the front the callers' tickets queue up behind it and are folded when it is done
        other = core.rescorer()
        other_scale = np.linspace(0.5, 2.0, n_items)
        barrier = threading.Barrier(13)
        go = [threading.Event() for _ in range(REPS)]
        before, sim_before = core.recommend_front_stats(), core.similar_stats()

        def worker(t):
            try:
                for rep in range(REPS):
                    barrier.wait(timeout=120)                       # every round's calls arrive together
                    if t == 12:
                        go[rep].set()                               # (the callers start once this thread is on its way into the library)
                        other.set_weights(other_scale, None)
                        continue
                    go[rep].wait(timeout=120)
                    try:
                        results[(t, rep)] = core.most_similar_items([queries[t % 3]], 10, rescorer=r)
                    except MalsError as e:
                        errors[(t, rep)] = e
            except Exception as e:   # noqa: BLE001
                broken[t] = e
                barrier.abort()

        th = [threading.Thread(target=worker, args=(t,)) for t in range(13)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        other.close()
        assert not broken, broken
        assert set(errors) == {(t, rep) for t in (1, 4, 7, 10) for rep in range(REPS)}, errors
        for e in errors.values():
            assert "Bad similarity value" in str(e)
        assert len(results) == 8 * REPS
        for (t, rep), (idx, sc, cnt) in results.items():
            same_ranking(idx[0], sc[0], cnt[0], *expect[t % 3])
        st, sim = core.recommend_front_stats(), core.similar_stats()
        if filter_path:
            # every query was answered by a filter pass, and the 36 calls needed at most 24 passes: calls were folded.  Which
            # calls share a pass is the order of arrival; with four of every twelve failing, passes that hold both kinds are the
            # rule, and every succeeding call above has the answer it has alone
            assert sim["dense"] == sim_before["dense"] and sim["filter"] - sim_before["filter"] == 12 * REPS
            assert st["passes"] - before["passes"] <= 8 * REPS, (st, before)
        else:
            assert sim["dense"] - sim_before["dense"] == 12 * REPS and st["passes"] == before["passes"]
        r.close()


# ---- threads --------------------------------------------------------------------------------------------------------------
def test_16_threads_mix_rescored_and_plain_calls_recommend_and_rescorer_updates():
    """threads 0-7: rescored similar calls over two rescorers and both flags (two threads per combination); 8-10: plain similar
    calls; 11-13: recommend_vectors; 14, 15: set_uniform tickets that alternate one rescorer between two known states"""
    from oracle import topn_oracle as to
    k, n_items = 32, cases.FILTER_ITEMS
    rng = np.random.default_rng(12)
    Y = rng.standard_normal((n_items, k)).astype(np.float32)
    Yn = so.norms(Y)
    spec = cases.rescorer_specs(n_items, 61)["combined"]
    filt = spec[0]
    V = (rng.standard_normal((16, k)) * 0.3).astype(np.float32)
    STATES = [(2.0, 0.5), (0.5, -1.0)]
    free = np.setdiff1d(np.arange(n_items), filt)
    items = {t: [int(free[10 * t + 1])] if t % 2 else [int(free[10 * t + 1]), int(free[10 * t + 2])] for t in range(16)}
    items[6] = [int(free[61]), int(filt[0])]                        # a filtered query item: empty with the flag (threads 6, 7: flag 1)
    o_fixed = cases.oracle_rescorer(spec)
    o_moving = [ro.AffineRescorer(filtered=filt, scale=s, offset=f) for s, f in STATES]
    expect = {}
    for t in range(16):
        if t < 8:
            flag = t >= 4
            expect[t] = [sro.most_similar(Y, items[t], 10, o, flag, Ynorm=Yn) for o in ([o_fixed] if t % 4 < 2 else o_moving)]
        elif t < 11:
            expect[t] = [so.most_similar(Y, items[t], 10, Ynorm=Yn)]
        elif t < 14:
            expect[t] = [to.recommend(Y, V[t], 10, None)]
    assert len(expect[6][0][0]) == 0 and len(expect[2][0][0]) == 10
    with y_core(Y) as core:
        fixed = cases.device_rescorer(core, spec)
        moving = core.rescorer()
        moving.set_filter(filt)
        moving.set_uniform(*STATES[0])
        errors, results = {}, {}
        barrier = threading.Barrier(16)
        before = core.recommend_front_stats()
        REPS = 6

        def worker(t):
            try:
                for rep in range(REPS):
                    barrier.wait(timeout=120)                       # every round's calls arrive together: the front has a queue to fold
                    if t < 8:
                        results[(t, rep)] = core.most_similar_items([items[t]], 10, rescorer=fixed if t % 4 < 2 else moving, filter_query_items=t >= 4)
                    elif t < 11:
                        results[(t, rep)] = core.most_similar_items([items[t]], 10)
                    elif t < 14:
                        results[(t, rep)] = core.recommend_vectors(V[t][None], 10)
                    else:
                        moving.set_uniform(*STATES[(rep + t) % 2])
            except Exception as e:   # noqa: BLE001
                errors[t] = e
                barrier.abort()

        th = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errors, errors
        assert len(results) == 14 * REPS
        for (t, rep), (idx, sc, cnt) in results.items():
            ok = False
            for oidx, osc in expect[t]:
                n = len(oidx)
                ok = ok or (cnt[0] == n and np.array_equal(idx[0, :n], oidx) and
                            np.array_equal(sc[0, :n].view(np.uint32), np.asarray(osc, np.float32).view(np.uint32)))
            assert ok, (t, rep, idx[0], sc[0], expect[t])
        st = core.recommend_front_stats()
        assert st["passes"] - before["passes"] < 14 * REPS          # calls were folded into passes
        sim = core.similar_stats()
        assert sim["dense"] == 0 and sim["filter"] + sim["empty"] == 11 * REPS and sim["rescored"] == 8 * REPS
        fixed.close()
        moving.close()
