#!/usr/bin/env python
"""The online write path (mals_set_preferences) on one MI355X: updates/s per batch size for uniform and Zipf(1.1) item
draws, the level count of each batch, single-update latency from 1 and 32 writer threads while 32 threads recommend, and
a CPU baseline (the same updates through HostSolver in one thread, sampled, labelled as such).  One JSON line per leg.
--members N: the same writes on a single-process group of N members ON ONE DEVICE (mals_group_set_preferences): a 1-update
call and a distinct-rows call of --group-batch updates, to price the replication where it cannot spread (N replicas share one
device, so their work adds up; N devices are not measured here).  --digest: mals_factor_digest over the whole X replica.
wall_ms: host wall clock around the synchronous call (level assignment, upload, every level's kernel, status copy, known-item
bookkeeping); device_ms: HIP events around the level kernels (mals_foldin_stats).
usage: python tools/bench_foldin.py [--items N] [--users U] [--features K ...] [--members N ...] [--digest] [--out FILE]"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def zipf_items(rng, n_items, n, s=1.1):
    # inverse-CDF draw over ranks 1..n_items (rank r with probability ~ r^-s); item r - 1 is rank r (item 0 is the hottest)
    import numpy as np
    ranks = np.arange(1, n_items + 1, dtype=np.float64)
    cdf = np.cumsum(ranks ** -s)
    cdf /= cdf[-1]
    r = np.searchsorted(cdf, rng.random(n))
    return r.astype(np.int64)


def group_legs(a, k, pkg, np, torch):
    """mals_group_set_preferences on N members that share device 0: what the replication costs when it cannot spread."""
    gen = torch.Generator(device="cuda").manual_seed(k)
    X = (torch.randn(a.users, k, device="cuda", generator=gen) * (0.3 / k ** 0.5)).float().cpu().numpy()
    Y = (torch.randn(a.items, k, device="cuda", generator=gen) * (0.3 / k ** 0.5)).float().cpu().numpy()
    torch.cuda.empty_cache()
    ptr = np.arange(a.users + 1, dtype=np.int64)
    col = np.random.default_rng(1).integers(0, a.items, a.users).astype(np.int32)
    for members in a.members:
        g = pkg.GroupALS.single_process(k, [0] * members, backend=pkg._lib.GROUP_PEER_COPY)
        g.set_factor_rows(pkg.SIDE_X, a.users)
        g.set_factor_rows(pkg.SIDE_Y, a.items)
        g.set_factors(pkg.SIDE_X, X)
        g.set_factors(pkg.SIDE_Y, Y)
        g.set_matrix(pkg.SIDE_X, ptr, col, np.ones(a.users, np.float32))
        m0, _ = g.local(0)
        sx, _ = m0.recompute_solver(pkg.SIDE_X)
        sy, _ = m0.recompute_solver(pkg.SIDE_Y)
        g.set_foldin_solver(pkg.SIDE_X, sx)
        g.set_foldin_solver(pkg.SIDE_Y, sy)
        rng = np.random.default_rng(k)
        for n in (1, a.group_batch):
            times, dev = [], []
            for rep in range(a.reps + 1):
                u = rng.permutation(a.users)[:n]            # distinct rows: one level
                i = rng.permutation(a.items)[:n]
                v = rng.choice(np.array([1.0, 2.0, -1.0, 0.5], np.float32), n)
                t0 = time.perf_counter()
                g.set_preferences(u, i, v, raise_on_error=False)
                dt = time.perf_counter() - t0
                if rep:
                    times.append(dt)
                    dev.append(g.foldin_stats()["device_ms_last"])
            med = float(np.median(times))
            emit({"leg": "group_set_preferences", "members": members, "devices": 1, "k": k, "items": a.items, "users": a.users,
                  "dist": "distinct", "batch": n, "wall_ms_median": med * 1e3, "wall_ms_min": min(times) * 1e3, "updates_per_s": n / med,
                  "device_ms_median_slowest_member": float(np.median(dev)), "replicas_equal": bool(g.replica_digest(pkg.SIDE_Y)[1]),
                  "reps": a.reps}, a.out)
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--users", type=int, default=10_000_000)
    ap.add_argument("--features", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 4096, 65536])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--latency-calls", type=int, default=300)
    ap.add_argument("--cpu-sample", type=int, default=200)
    ap.add_argument("--members", type=int, nargs="+", default=[], help="group legs: members on one device (replaces the other legs)")
    ap.add_argument("--group-batch", type=int, default=4096)
    ap.add_argument("--digest", action="store_true", help="add the mals_factor_digest leg (single handle)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import myrrix_recommender_amd as pkg
    from tests import foldin_oracle as fo

    for k in a.features if a.members else []:
        group_legs(a, k, pkg, np, torch)
    if a.members:
        return
    for k in a.features:
        g = torch.Generator(device="cuda").manual_seed(k)
        X = (torch.randn(a.users, k, device="cuda", generator=g) * (0.3 / k ** 0.5)).float()
        Y = (torch.randn(a.items, k, device="cuda", generator=g) * (0.3 / k ** 0.5)).float()
        core = pkg.ALSCore(k)
        core.bind_factors(pkg.SIDE_X, X)
        core.bind_factors(pkg.SIDE_Y, Y)
        # one known item per user (the rows of R); the writes add to them
        core.set_matrix(pkg.SIDE_X, np.arange(a.users + 1, dtype=np.int64),
                        np.random.default_rng(1).integers(0, a.items, a.users).astype(np.int32), np.ones(a.users, np.float32))
        sx, _ = core.recompute_solver(pkg.SIDE_X)
        sy, _ = core.recompute_solver(pkg.SIDE_Y)
        core.set_foldin_solver(pkg.SIDE_X, sx)
        core.set_foldin_solver(pkg.SIDE_Y, sy)
        rng = np.random.default_rng(k)
        for dist in ("uniform", "zipf1.1"):
            for n in a.batches:
                times, levels, dev = [], [], []
                for rep in range(a.reps + 1):
                    u = rng.integers(0, a.users, n)
                    i = rng.integers(0, a.items, n) if dist == "uniform" else zipf_items(rng, a.items, n)
                    v = rng.choice(np.array([1.0, 2.0, -1.0, 0.5], np.float32), n)
                    l0 = core.foldin_stats()["levels"]
                    t0 = time.perf_counter()
                    core.set_preferences(u, i, v, raise_on_error=False)
                    dt = time.perf_counter() - t0
                    if rep:   # the first call is warm-up
                        st = core.foldin_stats()
                        times.append(dt)
                        levels.append(st["levels"] - l0)
                        dev.append(st["device_ms_last"])
                med = float(np.median(times))
                dmed = float(np.median(dev))
                emit({"leg": "set_preferences", "k": k, "items": a.items, "users": a.users, "dist": dist, "batch": n,
                      "wall_ms_median": med * 1e3, "wall_ms_min": min(times) * 1e3, "updates_per_s": n / med,
                      "device_ms_median": dmed, "device_updates_per_s": n / (dmed * 1e-3),
                      "levels_median": float(np.median(levels)), "levels_max": int(max(levels)), "reps": a.reps}, a.out)
        if a.digest:
            # one streaming read of the X replica; wall clock around the synchronous call (ticket, launch, 8-byte copy back)
            core.factor_digest(pkg.SIDE_X)
            times = []
            for _ in range(20):
                t0 = time.perf_counter()
                core.factor_digest(pkg.SIDE_X)
                times.append(time.perf_counter() - t0)
            nbytes = 4.0 * a.users * k
            emit({"leg": "factor_digest", "k": k, "rows": a.users, "bytes": nbytes, "wall_ms_min": min(times) * 1e3,
                  "wall_ms_median": float(np.median(times)) * 1e3, "read_TBps_at_min": nbytes / min(times) / 1e12,
                  "read_TBps_at_median": nbytes / float(np.median(times)) / 1e12, "calls": 20}, a.out)
        # single-update latency from 1 and 32 writer threads while 32 threads recommend
        for writers in (1, 32):
            stop = threading.Event()
            lat = []
            lk = threading.Lock()

            def reader(seed):
                r = np.random.default_rng(seed)
                while not stop.is_set():
                    core.recommend(r.integers(0, a.users, 1), 10, consider_known_items=True)

            def writer(seed, calls):
                r = np.random.default_rng(seed)
                mine = []
                for _ in range(calls):
                    t0 = time.perf_counter()
                    core.set_preferences(r.integers(0, a.users, 1), r.integers(0, a.items, 1), np.ones(1, np.float32), raise_on_error=False)
                    mine.append(time.perf_counter() - t0)
                with lk:
                    lat.extend(mine)

            readers = [threading.Thread(target=reader, args=(100 + s,)) for s in range(32)]
            for t in readers:
                t.start()
            ws = [threading.Thread(target=writer, args=(200 + s, max(1, a.latency_calls // writers))) for s in range(writers)]
            for t in ws:
                t.start()
            for t in ws:
                t.join()
            stop.set()
            for t in readers:
                t.join()
            lat = np.array(lat) * 1e6
            emit({"leg": "latency", "k": k, "writer_threads": writers, "reader_threads": 32, "calls": len(lat),
                  "p50_us": float(np.percentile(lat, 50)), "p99_us": float(np.percentile(lat, 99))}, a.out)
        # CPU baseline: the reference's per-update loop on the host -- estimate, HostSolver.solve_ftod twice (the C++ solver
        # through ctypes), the two row updates as numpy vector operations -- one thread, on a sample of rows copied to the host
        n = a.cpu_sample
        u = rng.integers(0, a.users, n)
        i = rng.integers(0, a.items, n)
        Xs = X[torch.as_tensor(u, device="cuda")].cpu().numpy()
        Ys = Y[torch.as_tensor(i, device="cuda")].cpu().numpy()
        t0 = time.perf_counter()
        for t in range(n):
            xu, yi = Xs[t], Ys[t]
            w = fo.fold_in_weight(float(np.sum((xu * yi).astype(np.float64))), 1.0)
            item_fold = sx.solve_ftod(xu)
            user_fold = sy.solve_ftod(yi)
            yi += (w * item_fold).astype(np.float32)
            xu += (w * user_fold).astype(np.float32)
        dt = time.perf_counter() - t0
        emit({"leg": "cpu_baseline", "k": k, "what": "per update: numpy estimate + 2 x HostSolver.solve_ftod (C++, ctypes) + numpy row updates, "
              "1 thread, sampled", "updates": n, "updates_per_s": n / dt}, a.out)
        core.close()
        del X, Y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
