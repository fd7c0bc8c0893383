#!/usr/bin/env python
"""Top-N scoring on one MI355X: queries/s of mals_recommend for model users
against n_items item vectors resident in HBM, per batch size, + the oracle (numpy restatement of
RecommendIterator + TopN, 1 core) on a few queries.
usage: python tools/bench_topn.py [--items N] [--users U] [--features K] [--how-many N]
       python tools/bench_topn.py --similar [--lib-root DIR]: mostSimilarItems (mals_most_similar_items, one item per
       query) next to recommend in the same run, per batch size; --lib-root imports the package (and its library) from
       another checkout, whose recommend leg alone then runs (an A/B of recommend against an older build)
       python tools/bench_topn.py --rescorer [--how-many 64]: recommend with a rescorer (a 10 %% filter set plus per-item
       scale and offset, mals_recommend_rescored) next to the unrescored leg in the same run, 240-query batches
       python tools/bench_topn.py --lsh 0.3,0.1 [--lib-root DIR]: recommend with the candidate filter (mals_lsh_build,
       LocationSensitiveHash) off and at each sample ratio in the same run, the build time next to its bytes bounds (the
       signatures read Y once, n k 4 bytes; with the mean computed on the device Y is read twice) and how many queries the bf16 filter path / the dense path answered; with --lib-root of a checkout that has
       no candidate filter only the filter-off leg runs (the A/B of unfiltered passes against an older build)
       python tools/bench_topn.py --similar-rescored [--how-many 64] [--lib-root DIR]: one pass of mostSimilarItems per call
       (240 queries at 64 features), plain and with a rescorer (per-item scale and offset, mals_most_similar_items_rescored),
       next to the plain and rescored recommend pass in the same run; with --lib-root of a checkout without the rescored
       call only the plain legs run (the A/B of the unrescored cosine pass against an older build)
       python tools/bench_topn.py --popular [--items 1000000] [--entries 100000000] [--how-many 100]: mostPopularItems
       (mals_most_popular_items) over a seeded known-item CSR resident on the device: the first call (the recount), the
       second (counts cached) and, in the same run, a device-to-device copy of the same index array as the yardstick"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--how-many", type=int, default=10)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--similar", action="store_true")
    ap.add_argument("--similar-rescored", action="store_true")
    ap.add_argument("--label", default=None, help="--similar-rescored: recorded as \"run\" in place of the library's path")
    ap.add_argument("--lib-root", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rescorer", action="store_true")
    ap.add_argument("--lsh", default=None, metavar="RATIOS")
    ap.add_argument("--hashes", type=int, default=20)
    ap.add_argument("--popular", action="store_true")
    ap.add_argument("--entries", type=int, default=100_000_000)
    a = ap.parse_args()
    if a.popular:
        return popular(a)
    if a.lsh:
        return lsh(a)
    if a.similar_rescored:
        return similar_rescored(a)
    if a.similar:
        return similar(a)
    if a.rescorer:
        return rescored(a)
    import numpy as np
    import myrrix_recommender_amd as pkg
    rng = np.random.default_rng(1234567890)
    k = a.features
    Y = (rng.standard_normal((a.items, k)) / np.sqrt(k)).astype(np.float32)
    X = (rng.standard_normal((a.users, k)) / np.sqrt(k)).astype(np.float32)
    deg = 100
    rp = np.arange(a.users + 1, dtype=np.int64) * deg
    col = rng.integers(0, a.items, a.users * deg).astype(np.int32)
    val = np.ones(a.users * deg, np.float32)
    out = {"metric": "top-N queries/s (all items scored in the reference's arithmetic, known items skipped)", "unit": "queries/s", "items": a.items,
           "features": k, "how_many": a.how_many, "batches": {}}
    with pkg.ALSCore(k) as core:
        core.set_factor_rows(pkg.SIDE_X, a.users)
        core.set_factor_rows(pkg.SIDE_Y, a.items)
        core.set_factors(pkg.SIDE_X, X)
        core.set_factors(pkg.SIDE_Y, Y)
        core.set_matrix(pkg.SIDE_X, rp, col, val)
        per_pass = 16 * {1: 16, 2: 15, 3: 10, 4: 7}[(k + 31) // 32]        # queries scored per read of Y (csrc/topn_host.h)
        for batch in (1, 16, 64, per_pass, 1024, 4096):
            users = rng.integers(0, a.users, batch).astype(np.int64)
            core.recommend(users, a.how_many)                          # warm
            reps = max(10, 4096 // batch)
            t0 = time.perf_counter()
            for _ in range(reps):
                core.recommend(users, a.how_many)
            dt = (time.perf_counter() - t0) / reps
            passes = (batch + per_pass - 1) // per_pass
            # bytes that must move: Y once per pass (+ the sample of it); everything else (sample rows, candidates) is
            # hundreds of KB
            y_bytes = passes * a.items * k * 4
            out["batches"][str(batch)] = {"ms_per_call": dt * 1e3, "queries_per_s": batch / dt, "passes": passes,
                                          "Y_GBps": y_bytes / dt / 1e9, "Y_stream_frac": y_bytes / dt / 8e12}
        out["queries_per_pass"] = per_pass
        out["value"] = out["batches"]["4096"]["queries_per_s"]
        big = out["batches"]["4096"]
        # the same 4096 queries with fewer queries per read of Y (MALS_TOPN_QUERIES_PER_PASS, the tuning knob of csrc/topn_host.h):
        # more passes, each nearer the speed of one stream of Y
        out["by_queries_per_pass"] = {}
        users = rng.integers(0, a.users, 4096).astype(np.int64)
        for pp in sorted({64, 128, per_pass}):
            if pp > per_pass:
                continue
            os.environ["MALS_TOPN_QUERIES_PER_PASS"] = str(pp)
            core.recommend(users, a.how_many)
            t0 = time.perf_counter()
            for _ in range(10):
                core.recommend(users, a.how_many)
            dt = (time.perf_counter() - t0) / 10
            passes = (4096 + pp - 1) // pp
            out["by_queries_per_pass"][str(pp)] = {"ms_per_call": dt * 1e3, "queries_per_s": 4096 / dt, "passes": passes, "us_per_pass": dt * 1e6 / passes,
                                                   "Y_GBps": passes * a.items * k * 4 / dt / 1e9, "Y_stream_frac": passes * a.items * k * 4 / dt / 8e12}
        del os.environ["MALS_TOPN_QUERIES_PER_PASS"]
        best = max(out["by_queries_per_pass"].values(), key=lambda d: d["Y_stream_frac"])
        out["roofline"] = {"bound": "hbm", "achieved": big["Y_GBps"], "peak": 8000.0, "unit": "GB/s", "frac": big["Y_stream_frac"],
                           "algorithmic_bytes": "items * 4k per pass of %d queries (Y streamed once per pass; passes overlap on six streams)" % per_pass,
                           "at_64_queries_per_call": out["batches"]["64"]["Y_stream_frac"],
                           "at_one_pass_per_call": out["batches"][str(per_pass)]["Y_stream_frac"],
                           "best_over_queries_per_pass": {"frac": best["Y_stream_frac"], "queries_per_s": best["queries_per_s"],
                                                          "queries_per_pass": [int(kk) for kk, v in out["by_queries_per_pass"].items() if v is best][0]}}
        # ---- the way the reference is entered: request threads, one user per call (ServerRecommender.java:359-441) ----------
        # native threads (tools/topn_callers.cpp) on ONE handle; the library folds the concurrent calls into passes
        import ctypes
        harness = os.path.join(ROOT, "tools", "libtopn_callers.so")
        if os.path.exists(harness):
            H = ctypes.CDLL(harness)
            H.topn_callers_run.restype = ctypes.c_int
            H.topn_callers_run.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]
            out["callers"] = {}

            def run_callers(n_threads, calls):
                lat = np.zeros(n_threads * calls, dtype=np.float64)
                wall, chk = ctypes.c_double(0.0), ctypes.c_int64(0)
                before = core.recommend_front_stats()
                rc = H.topn_callers_run(core._h, n_threads, calls, a.users, a.how_many, 42, lat.ctypes.data_as(ctypes.c_void_p), ctypes.byref(wall),
                                        ctypes.byref(chk))
                assert rc == 0, rc
                st = core.recommend_front_stats()
                passes = st["passes"] - before["passes"]
                n = n_threads * calls
                return {"threads": n_threads, "calls": n, "queries_per_s": n / wall.value, "latency_us": {"p50": float(np.percentile(lat, 50)),
                        "p99": float(np.percentile(lat, 99)), "mean": float(lat.mean())}, "passes": passes, "queries_per_pass": n / max(passes, 1),
                        "us_per_pass": wall.value * 1e6 / max(passes, 1), "Y_stream_frac": passes * a.items * k * 4 / wall.value / 8e12}
            for depth in (1, 2, 3):
                core.recommend_set_depth(depth)
                run_callers(8, 50)                                      # warm
                out["callers"]["depth_%d" % depth] = {str(nt): run_callers(nt, 4000 if nt > 1 else 2000) for nt in (1, 8, 32, 128)}
            core.recommend_set_depth(2)
            # waiting callers that poll for their answer before they block (mals_recommend_set_spin_us)
            out["callers_by_spin_us"] = {}
            for spin in (0, 50, 300):
                core.recommend_set_spin_us(spin)
                out["callers_by_spin_us"][str(spin)] = {str(nt): run_callers(nt, 4000) for nt in (8, 32, 128)}
            core.recommend_set_spin_us(0)
            c32 = out["callers"]["depth_2"]["32"]
            out["roofline_callers"] = {"bound": "hbm", "achieved": c32["Y_stream_frac"] * 8000.0, "peak": 8000.0, "unit": "GB/s", "frac": c32["Y_stream_frac"],
                                       "what": "32 native threads of one-user calls on one handle, 2 passes in flight: reads of Y (items * 4k bytes per "
                                               "coalesced pass) per second of wall time", "queries_per_s": c32["queries_per_s"],
                                       "latency_us": c32["latency_us"], "queries_per_pass": c32["queries_per_pass"]}
    if not a.no_cpu_baseline:
        from oracle import topn_oracle as to
        t0 = time.perf_counter()
        nq = 5
        for u in range(nq):
            to.recommend(Y, X[u], a.how_many, col[rp[u]:rp[u + 1]])
        out["cpu_baseline"] = {"value": nq / (time.perf_counter() - t0), "unit": "queries/s", "cores": 1, "kind": "port",
                               "sample": "%d queries, oracle/topn_oracle.py (numpy)" % nq}
    print(json.dumps(out))


def similar(a):
    """mostSimilarItems against recommend, the same batches in the same run: queries/s and Y_stream_frac (Y read once
    per pass of up to per_pass queries, over 8 TB/s)"""
    if a.lib_root:
        sys.path.insert(0, os.path.abspath(a.lib_root))
    import numpy as np
    import myrrix_recommender_amd as pkg
    rng = np.random.default_rng(1234567890)
    k = a.features
    Y = (rng.standard_normal((a.items, k)) / np.sqrt(k)).astype(np.float32)
    X = (rng.standard_normal((a.users, k)) / np.sqrt(k)).astype(np.float32)
    deg = 100
    rp = np.arange(a.users + 1, dtype=np.int64) * deg
    col = rng.integers(0, a.items, a.users * deg).astype(np.int32)
    per_pass = 16 * {1: 16, 2: 15, 3: 10, 4: 7}[(k + 31) // 32]
    out = {"metric": "mostSimilarItems and recommend queries/s, same run", "unit": "queries/s", "items": a.items, "features": k,
           "how_many": a.how_many, "queries_per_pass": per_pass, "lib": pkg._lib.LIB_PATH, "recommend": {}, "similar": {}}
    with pkg.ALSCore(k) as core:
        core.set_factor_rows(pkg.SIDE_X, a.users)
        core.set_factor_rows(pkg.SIDE_Y, a.items)
        core.set_factors(pkg.SIDE_X, X)
        core.set_factors(pkg.SIDE_Y, Y)
        core.set_matrix(pkg.SIDE_X, rp, col, np.ones(len(col), np.float32))
        legs = {"recommend": lambda q: core.recommend(q, a.how_many)}
        if hasattr(core, "most_similar_items"):
            legs["similar"] = lambda q: core.most_similar_items(q, a.how_many)
        else:
            del out["similar"]
        for batch in (1, 64, per_pass, 4096):
            qs = {"recommend": rng.integers(0, a.users, batch).astype(np.int64), "similar": rng.integers(0, a.items, batch).astype(np.int64)}
            for name, fn in legs.items():
                fn(qs[name])                                            # warm
                reps = max(10, 4096 // batch)
                runs = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        fn(qs[name])
                    runs.append((time.perf_counter() - t0) / reps)
                dt = min(runs)
                passes = (batch + per_pass - 1) // per_pass
                y_bytes = passes * a.items * k * 4
                out[name][str(batch)] = {"ms_per_call": dt * 1e3, "ms_per_call_runs": [r * 1e3 for r in runs], "queries_per_s": batch / dt,
                                         "passes": passes, "Y_stream_frac": y_bytes / dt / 8e12}
        if "similar" in out:
            out["similar_over_recommend"] = {b: out["similar"][b]["queries_per_s"] / out["recommend"][b]["queries_per_s"] for b in out["similar"]}
    out["value"] = out["similar"]["4096"]["queries_per_s"] if "similar" in out else out["recommend"]["4096"]["queries_per_s"]
    print(json.dumps(out))


def rescored(a):
    """recommend with and without a rescorer (10 % of the items filtered, per-item scale in [0.5, 2], offset ~ 0.1 N(0, 1)),
    the same users in the same run: queries/s per batch and their ratio; the filter reads 16 bytes per item more than the
    4k bytes of its row (csrc/topn_kernels.h, RESCORED MODE)"""
    import numpy as np
    import myrrix_recommender_amd as pkg
    rng = np.random.default_rng(1234567890)
    k = a.features
    Y = (rng.standard_normal((a.items, k)) / np.sqrt(k)).astype(np.float32)
    X = (rng.standard_normal((a.users, k)) / np.sqrt(k)).astype(np.float32)
    deg = 100
    rp = np.arange(a.users + 1, dtype=np.int64) * deg
    col = rng.integers(0, a.items, a.users * deg).astype(np.int32)
    per_pass = 16 * {1: 16, 2: 15, 3: 10, 4: 7}[(k + 31) // 32]
    out = {"metric": "recommend queries/s with and without a rescorer, same run", "unit": "queries/s", "items": a.items, "features": k,
           "how_many": a.how_many, "queries_per_pass": per_pass, "filter_bytes_per_item": {"plain": 4 * k, "rescored": 4 * k + 16},
           "plain": {}, "rescored": {}}
    with pkg.ALSCore(k) as core:
        core.set_factor_rows(pkg.SIDE_X, a.users)
        core.set_factor_rows(pkg.SIDE_Y, a.items)
        core.set_factors(pkg.SIDE_X, X)
        core.set_factors(pkg.SIDE_Y, Y)
        core.set_matrix(pkg.SIDE_X, rp, col, np.ones(len(col), np.float32))
        r = core.rescorer()
        r.set_filter(rng.choice(a.items, a.items // 10, replace=False))
        r.set_weights(rng.uniform(0.5, 2.0, a.items), rng.standard_normal(a.items) * 0.1)
        legs = {"plain": None, "rescored": r}
        for batch in (per_pass, 4 * per_pass, 4096):
            users = rng.integers(0, a.users, batch).astype(np.int64)
            for name, rs in legs.items():
                core.recommend(users, a.how_many, rescorer=rs)          # warm
                reps = max(10, 4096 // batch)
                runs = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        core.recommend(users, a.how_many, rescorer=rs)
                    runs.append((time.perf_counter() - t0) / reps)
                dt = min(runs)
                out[name][str(batch)] = {"ms_per_call": dt * 1e3, "ms_per_call_runs": [x * 1e3 for x in runs], "queries_per_s": batch / dt}
        out["rescored_over_plain"] = {b: out["rescored"][b]["queries_per_s"] / out["plain"][b]["queries_per_s"] for b in out["plain"]}
        r.close()
    out["value"] = out["rescored"]["4096"]["queries_per_s"]
    print(json.dumps(out))


def similar_rescored(a):
    """one pass per call (per_pass queries): mostSimilarItems plain and rescored (per-item scale in [0.5, 2], offset ~ 0.1
    N(0, 1): csrc/topn_kernels.h, RESCORED COSINE MODE), recommend plain and rescored with the same weights, same run; every
    leg min and all of --reps runs of 40 calls, and which path answered the similarity queries (mals_similar_stats)"""
    if a.lib_root:
        sys.path.insert(0, os.path.abspath(a.lib_root))
    import numpy as np
    import myrrix_recommender_amd as pkg
    rng = np.random.default_rng(1234567890)
    k = a.features
    Y = (rng.standard_normal((a.items, k)) / np.sqrt(k)).astype(np.float32)
    X = (rng.standard_normal((a.users, k)) / np.sqrt(k)).astype(np.float32)
    per_pass = 16 * {1: 16, 2: 15, 3: 10, 4: 7}[(k + 31) // 32]
    out = {"metric": "us per pass of %d queries: mostSimilarItems and recommend, plain and rescored, same run" % per_pass, "unit": "us", "items": a.items,
           "features": k, "how_many": a.how_many, "queries_per_pass": per_pass, "legs": {}}
    out.update({"run": a.label} if a.label else {"lib": pkg._lib.LIB_PATH})
    with pkg.ALSCore(k) as core:
        core.set_factor_rows(pkg.SIDE_X, a.users)
        core.set_factor_rows(pkg.SIDE_Y, a.items)
        core.set_factors(pkg.SIDE_X, X)
        core.set_factors(pkg.SIDE_Y, Y)
        items = rng.integers(0, a.items, per_pass).astype(np.int64)
        users = rng.integers(0, a.users, per_pass).astype(np.int64)
        legs = {"similar_plain": lambda: core.most_similar_items(items, a.how_many),
                "recommend_plain": lambda: core.recommend(users, a.how_many, consider_known_items=True)}
        r = None
        if hasattr(core, "similar_stats"):
            r = core.rescorer()
            r.set_weights(rng.uniform(0.5, 2.0, a.items), rng.standard_normal(a.items) * 0.1)
            legs["similar_rescored"] = lambda: core.most_similar_items(items, a.how_many, rescorer=r)
            legs["recommend_rescored"] = lambda: core.recommend(users, a.how_many, consider_known_items=True, rescorer=r)
        for name, fn in legs.items():
            fn()                                                        # warm
        for name, fn in legs.items():
            runs = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(40):
                    fn()
                runs.append((time.perf_counter() - t0) / 40 * 1e6)
            out["legs"][name] = {"us_per_pass": min(runs), "us_per_pass_runs": runs, "queries_per_s": per_pass / min(runs) * 1e6}
        if r is not None:
            out["similar_stats"] = core.similar_stats()
            out["similar_rescored_over_plain"] = out["legs"]["similar_rescored"]["us_per_pass"] / out["legs"]["similar_plain"]["us_per_pass"]
            out["recommend_rescored_over_plain"] = out["legs"]["recommend_rescored"]["us_per_pass"] / out["legs"]["recommend_plain"]["us_per_pass"]
            r.close()
    out["value"] = out["legs"]["similar_plain"]["us_per_pass"]
    print(json.dumps(out))


def lsh(a):
    """recommend with the candidate filter off and at each of the given sample ratios (model.lsh.sampleRatio), the same users
    in the same run; the build (mean + signatures of Y) against the time its bytes need at 8 TB/s"""
    if a.lib_root:
        sys.path.insert(0, os.path.abspath(a.lib_root))
    import numpy as np
    import myrrix_recommender_amd as pkg
    rng = np.random.default_rng(1234567890)
    k = a.features
    Y = (rng.standard_normal((a.items, k)) / np.sqrt(k)).astype(np.float32)
    X = (rng.standard_normal((a.users, k)) / np.sqrt(k)).astype(np.float32)
    deg = 100
    rp = np.arange(a.users + 1, dtype=np.int64) * deg
    col = rng.integers(0, a.items, a.users * deg).astype(np.int32)
    per_pass = 16 * {1: 16, 2: 15, 3: 10, 4: 7}[(k + 31) // 32]
    out = {"metric": "recommend queries/s with the candidate filter off and on, same run", "unit": "queries/s", "items": a.items, "features": k,
           "how_many": a.how_many, "queries_per_pass": per_pass, "num_hashes": a.hashes, "package": os.path.dirname(pkg.__file__), "legs": {}}
    with pkg.ALSCore(k) as core:
        core.set_factor_rows(pkg.SIDE_X, a.users)
        core.set_factor_rows(pkg.SIDE_Y, a.items)
        core.set_factors(pkg.SIDE_X, X)
        core.set_factors(pkg.SIDE_Y, Y)
        core.set_matrix(pkg.SIDE_X, rp, col, np.ones(len(col), np.float32))
        ratios = [float(r) for r in a.lsh.split(",") if r != "off"] if hasattr(core, "lsh_build") else []   # "--lsh off": the unfiltered leg alone
        batches = {b: rng.integers(0, a.users, b).astype(np.int64) for b in (per_pass, 4096)}
        for ratio in [None] + ratios:
            leg = {}
            if ratio is not None:
                rv = rng.integers(0, 2, (a.hashes, k)).astype(bool)
                core.lsh_build(num_hashes=a.hashes, sample_ratio=ratio, random_vectors=rv)      # warm (allocations, code load)
                runs = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    core.lsh_build(num_hashes=a.hashes, sample_ratio=ratio, random_vectors=rv)
                    runs.append(time.perf_counter() - t0)
                y_bytes = a.items * k * 4              # the signatures read Y once; so does the mean before them
                leg["build_ms"] = min(runs) * 1e3
                leg["build_ms_runs"] = [x * 1e3 for x in runs]
                leg["signatures_bytes_bound_ms"] = y_bytes / 8e12 * 1e3
                leg["build_bytes_bound_ms"] = 2 * y_bytes / 8e12 * 1e3      # mean + signatures, as timed here
                leg["max_bits_differing"] = core.lsh_info()["max_bits_differing"]
                before = core.lsh_info()
            for batch, users in batches.items():
                core.recommend(users, a.how_many)                          # warm
                reps = max(10, 4096 // batch)
                runs = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        core.recommend(users, a.how_many)
                    runs.append((time.perf_counter() - t0) / reps)
                dt = min(runs)
                leg[str(batch)] = {"ms_per_call": dt * 1e3, "ms_per_call_runs": [x * 1e3 for x in runs], "queries_per_s": batch / dt}
            if ratio is not None:
                after = core.lsh_info()
                leg["filter_queries"] = after["filter_queries"] - before["filter_queries"]
                leg["dense_queries"] = after["dense_queries"] - before["dense_queries"]
            out["legs"]["off" if ratio is None else str(ratio)] = leg
    out["value"] = out["legs"]["off"]["4096"]["queries_per_s"]
    print(json.dumps(out))


def popular(a):
    """mostPopularItems: recount and cached call against a device-to-device copy of the index array (4 bytes per entry read
    and written; the count pass reads them once and adds one atomic per entry)"""
    import numpy as np
    import torch
    import myrrix_recommender_amd as pkg
    deg = 100
    n_users = a.entries // deg
    gen = torch.Generator(device="cuda").manual_seed(1234567890)
    # strictly ascending rows of `deg` items, popularity skewed towards the low indices
    first = (torch.rand((n_users, deg), device="cuda", generator=gen).pow_(2.0) * (a.items - deg)).to(torch.int32)
    col = (torch.sort(first, dim=1).values + torch.arange(deg, device="cuda", dtype=torch.int32)[None, :]).reshape(-1).contiguous()
    del first
    rp = torch.arange(n_users + 1, device="cuda", dtype=torch.int64) * deg
    val = torch.ones(n_users * deg, device="cuda", dtype=torch.float32)
    out = {"metric": "mostPopularItems: recount / cached call / device-to-device copy of the index array, same run", "unit": "ms",
           "items": a.items, "users": n_users, "entries": n_users * deg, "how_many": a.how_many}
    with pkg.ALSCore(4) as core:
        core.set_factor_rows(pkg.SIDE_Y, a.items)
        core.set_matrix(pkg.SIDE_X, rp, col, val)
        t0 = time.perf_counter()
        first_call = core.most_popular_items(a.how_many)
        out["first_call_ms"] = (time.perf_counter() - t0) * 1e3            # with the ascending check and the allocations
        recount, cached, copy = [], [], []
        for _ in range(a.reps):
            core.set_tag_users(None)                                       # forces a recount
            t0 = time.perf_counter()
            again = core.most_popular_items(a.how_many)
            recount.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            core.most_popular_items(a.how_many)
            cached.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(again[0], first_call[0]) and np.array_equal(again[1], first_call[1])
            dst = torch.empty_like(col)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(col)
            torch.cuda.synchronize()
            copy.append((time.perf_counter() - t0) * 1e3)
            del dst
        st = core.most_popular_stats()
        out.update({"recount_ms": min(recount), "recount_ms_runs": recount, "cached_ms": min(cached), "cached_ms_runs": cached,
                    "d2d_copy_ms": min(copy), "d2d_copy_ms_runs": copy, "recount_over_copy": min(recount) / min(copy),
                    "pairs": st["pairs"], "recounts": st["recounts"], "top": first_call[0][:5].tolist(), "top_counts": first_call[1][:5].tolist()})
    out["value"] = out["recount_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
