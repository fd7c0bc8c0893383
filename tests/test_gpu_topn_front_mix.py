"""Every kind of request the serving front takes, alone and from 12 threads at once on one handle: each concurrent answer
-- folded into a shared pass, or queued behind the others as a call of its own -- is array_equal (indices, score bits,
counts) to the answer the same call got alone.  The one-at-a-time answers are tied to the oracle by test_gpu_topn*.py,
test_gpu_similarity.py, test_gpu_rescorer.py and test_gpu_lsh.py; this ties the coalesced and the queued form of every
request kind to them, at a catalogue the dense path answers and at the smallest one the filter path takes, first without
and then with the candidate filter built."""
import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd.core import HostSolver
from tests.test_gpu_topn import big_core
from tests.test_gpu_topn_serving import run_threads

pytestmark = pytest.mark.gpu

K, N_USERS, DEG = 16, 200, 20
N_THREADS, ROUNDS = 12, 3
WRITER = N_USERS - 1          # the user of the write: in none of the compared calls


def bits(out):
    """(indices, score bits, counts) of a top-N answer; similarity_to_item's floats as their bits"""
    if isinstance(out, tuple):
        return out[0].copy(), out[1].view(np.uint32).copy(), out[2].copy()
    return (np.asarray(out, np.float32).view(np.uint32).copy(),)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n_items", [3000, 131072])      # every call on the dense path / the smallest catalogue of the filter path
def test_every_request_kind_alone_and_from_12_threads(n_items):
    core, X, Y, rp, col = big_core(K, n_items, N_USERS, DEG, 4242 + n_items)
    rng = np.random.default_rng(n_items)
    with core:
        # the write below folds the item into the user's vector only: Y stays as it is for every other reader
        core.set_foldin_solver(pkg.SIDE_Y, HostSolver.create(Y.astype(np.float64).T @ Y.astype(np.float64)))
        r = core.rescorer()
        r.set_filter(rng.choice(n_items, n_items // 10, replace=False))
        r.set_weights(rng.uniform(0.5, 2.0, n_items), rng.standard_normal(n_items) * 0.1)
        u1, u2 = np.array([3], np.int64), np.array([17], np.int64)
        u5 = np.array([5, 44, 45, 120, 198], np.int64)
        u70 = np.arange(60, 130, dtype=np.int64)
        ex = col[rp[9]:rp[10]].astype(np.int64)
        it3 = [[10, 11, 12], [n_items - 1, 0, 77], [500, 2999, 1]]
        calls = [
            ("user, known skipped", lambda: core.recommend(u1, 10)),
            ("user, known considered", lambda: core.recommend(u2, 7, consider_known_items=True)),
            ("five users", lambda: core.recommend(u5, 10)),
            ("70 users, exclusive", lambda: core.recommend(u70, 10)),
            ("vectors with exclusions", lambda: core.recommend_vectors(X[9:10], 10, exclude=[ex])),
            ("to many, two vectors", lambda: core.recommend_to_many([X[20:22]], 10)),
            ("similar, one item each", lambda: core.most_similar_items([4, 2500], 10)),
            ("similar, three items each", lambda: core.most_similar_items(it3, 10)),
            ("because", lambda: core.recommended_because(u5, [7, 8, 9, 10, n_items - 2], 5)),
            ("similarity to item", lambda: core.similarity_to_item(42, np.arange(0, 3000, 7))),
            ("user, rescored", lambda: core.recommend(u1, 10, rescorer=r)),
            ("vectors, rescored", lambda: core.recommend_vectors(X[30:32], 10, rescorer=r)),
        ]
        wu = np.array([WRITER], np.int64)
        for lsh in (False, True):
            if lsh:
                rv = np.random.default_rng(7).integers(0, 2, (20, K)).astype(bool)
                core.lsh_build(num_hashes=20, sample_ratio=0.3, random_vectors=rv)
            want = [bits(fn()) for _, fn in calls]
            before = core.recommend_front_stats()
            bits(calls[3][1]())
            assert core.recommend_front_stats()["exclusive"] == before["exclusive"] + 1      # the 70-user call runs alone
            # the write alone: the pair can be estimated, and the item is known to the user from then on
            top = core.recommend(wu, 1)[0][0, :1]
            assert core.set_preferences(wu, top, [1.0]).tolist() == [0]
            assert np.isfinite(core.estimate_preferences(wu, top)[0])
            assert int(top[0]) not in core.recommend(wu, 10)[0][0].tolist()
            bad = []

            def worker(t):
                for rnd in range(ROUNDS):
                    for j in range(len(calls) + 1):
                        c = (j + t + rnd) % (len(calls) + 1)      # the threads are in different kinds of call at any moment
                        if c == len(calls):      # a TOPN_KIND_CALL ticket in the same queue, and a read behind it
                            if core.set_preferences(wu, top, [1.0]).tolist() != [0] or not np.isfinite(core.estimate_preferences(wu, top)[0]):
                                bad.append((lsh, t, rnd, "write"))
                            if int(top[0]) in core.recommend(wu, 10)[0][0].tolist():
                                bad.append((lsh, t, rnd, "read after write"))
                        elif not same(bits(calls[c][1]()), want[c]):
                            bad.append((lsh, t, rnd, calls[c][0]))
            run_threads(N_THREADS, worker)
            assert not bad, bad[:8]
        r.close()
