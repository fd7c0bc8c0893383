#!/usr/bin/env python3
"""Time mals_load_generation at the C4 shape: a live handle of --users x --features users and --items items takes a new model
of the same sizes that sits on the device, with --kept live rows per side kept (ids the new model lacks, marked recent).

Steady state: after the first load the handle holds the new rows and the kept ones behind them; every further load gives it
the same new model again with the kept rows marked recent again, so every timed load does the same work (n_new rows updated,
--kept rows kept, none pruned).  Reported, as medians over --reps timed loads after --warmup untimed ones:
  * the per-phase device times of mals_generation_result (join, scan, gather per side), the bytes each phase must move
    (the formulas are below, next to the numbers) and the rate that gives;
  * a device-to-device hipMemcpy of the bytes the gather phase copies (new rows + kept rows), in the same process: the yardstick for
    the head copy and the tail gather;
  * the only route the library had before: mals_set_factors of both sides from host memory plus mals_set_known_items on
    a handle of the merged shape.
--members W loads the same shape through a W-member group on device 0 (peer-copy backend, mals_group_load_generation): the
phase times are then the slowest member's, known_ms is the group's known-item step (the device path for plain kept users and
the assembly of every new owner's CSR).  --live-known-per-user gives every live user a base row of that many items, and
--keep-not-updated keeps every live row the new model lacks, so that the --kept users are plain kept users with real rows.
Prints one JSON line last.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def slots(n):
    s = 64
    while s < 2 * n:
        s <<= 1
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=10_000_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--kept", type=int, default=100_000)
    ap.add_argument("--known-per-user", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-parent-route", action="store_true")
    ap.add_argument("--members", type=int, default=0, help="load through a group of this many members on device 0 (0: one handle)")
    ap.add_argument("--keep-not-updated", action="store_true", help="MALS_GENERATION_KEEP_NOT_UPDATED")
    ap.add_argument("--live-known-per-user", type=int, default=0, help="known items of every live user before the first load")
    a = ap.parse_args()

    import torch
    import myrrix_recommender_amd as pkg
    X_, Y_ = pkg.SIDE_X, pkg.SIDE_Y
    k = a.features
    n = [a.users, a.items]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    # ids: live row r of a side has id r; the new model has the ids [kept, n + kept) in a shuffled order
    new_ids = [(torch.randperm(n[s], device=dev, generator=g) + a.kept).to(torch.int64) for s in range(2)]
    new_rows = [torch.randn((n[s], k), device=dev, generator=g, dtype=torch.float32) * 0.3 for s in range(2)]
    kp = torch.arange(0, (n[0] + 1) * a.known_per_user, a.known_per_user, device=dev, dtype=torch.int64)
    ki = torch.randint(0, n[1], (n[0] * a.known_per_user,), device=dev, generator=g, dtype=torch.int32)

    if a.members > 0:
        from myrrix_recommender_amd import _lib
        core = pkg.GroupALS.single_process(k, [0] * a.members, backend=_lib.GROUP_PEER_COPY)
    else:
        core = pkg.ALSCore(k)
    for s in range(2):
        core.set_factor_rows(s, n[s])
    lk = a.live_known_per_user
    live_ptr = np.arange(0, (n[0] + 1) * lk, max(lk, 1), dtype=np.int64) if lk else np.zeros(n[0] + 1, np.int64)
    live_idx = np.random.default_rng(2).integers(0, n[1], n[0] * lk, dtype=np.int32)
    core.set_matrix(X_, live_ptr, live_idx, np.ones(len(live_idx), np.float32))
    del live_ptr, live_idx
    cur = [torch.arange(n[s], device=dev, dtype=torch.int64) for s in range(2)]
    for s in range(2):
        core.mark_recent(s, np.arange(a.kept, dtype=np.int64))          # ids [0, kept): not in the new model

    results = []
    for it in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        res, ids, _ = core.load_generation(cur[0], cur[1], new_ids[0], new_ids[1], new_rows[0], new_rows[1], new_known=(kp, ki),
                                           keep_not_updated=a.keep_not_updated)
        res["call_ms"] = (time.perf_counter() - t0) * 1e3     # includes the two id / map read-backs of the binding
        assert res["n_kept"] == [a.kept, a.kept], res
        if it >= a.warmup:
            results.append(res)
        cur = [torch.from_numpy(ids[s]).to(dev) for s in range(2)]
        for s in range(2):
            core.mark_recent(s, np.arange(n[s], n[s] + a.kept, dtype=np.int64))   # the kept rows sit behind the new ones

    out = {"tool": "bench_generation_load", "users": n[0], "items": n[1], "features": k, "kept": a.kept, "reps": a.reps, "members": a.members,
           "keep_not_updated": a.keep_not_updated, "live_known_per_user": lk, "phases": {}}
    names = ["users", "items"]
    for s in range(2):
        n_new, n_cur, n_kept = n[s], n[s] + a.kept, a.kept
        # Bytes a phase must move at the least (S = slots of a table = the smallest power of two >= max(64, 2 n); every random
        # access is charged the bytes it asks for, not the cache line it touches; probe chains are charged one slot):
        #   join   both tables zeroed (16 S_new + 16 S_cur); an insert reads its id and swaps one value word (16 n_new + 16 n_cur);
        #          the key pass reads every value word of the new table (8 S_new) and, per taken slot, reads an id and writes a
        #          key (16 n_new); a probe reads its id and one slot and writes map + keep flag (8 + 16 + 12 = 36 n_cur)
        #   scan   (the phase's events also span the map and the copy of the new ids into the merged ids) the keep flags read by
        #          the tile sums and again by the map (8 n_cur); a kept row's map entry, row and id written (24 n_kept); the new
        #          ids read and written (16 n_new)
        #   gather every new row and kept row read and written once (8 k (n_new + n_kept))
        s_new, s_cur = slots(n_new), slots(n_cur)
        must = {"join": 16 * (s_new + s_cur) + 16 * (n_new + n_cur) + 8 * s_new + 16 * n_new + 36 * n_cur,
                "scan": 8 * n_cur + 24 * n_kept + 16 * n_new,
                "gather": 8 * k * (n_new + n_kept)}
        for ph in ("join", "scan", "gather"):
            ms = median([r[ph + "_ms"][s] for r in results])
            out["phases"]["%s_%s" % (ph, names[s])] = {"ms": ms, "bytes": must[ph], "GBps": must[ph] / ms / 1e6 if ms > 0 else None}
    for name in ("sides_ms", "known_ms", "tags_ms", "total_ms", "call_ms"):
        out[name] = median([r[name] for r in results])

    # the yardstick: a device-to-device hipMemcpy of what the gather phase copies, per side (torch's copy of a contiguous tensor
    # of the same dtype on one device is hipMemcpyAsync(..., hipMemcpyDeviceToDevice); timed with events on its stream)
    out["memcpy_dtod"] = {}
    for s in range(2):
        nbytes = 4 * k * (n[s] + a.kept)
        src = torch.empty(nbytes // 4, device=dev, dtype=torch.float32).normal_()
        dst = torch.empty_like(src)
        times = []
        for it in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times.append(e0.elapsed_time(e1))
        ms = median(times)
        out["memcpy_dtod"][names[s]] = {"ms": ms, "bytes_copied": nbytes, "GBps_moved": 2 * nbytes / ms / 1e6}
        del src, dst

    if not a.skip_parent_route and a.members == 0:
        # what a caller had before: every row of both sides from host memory, and the known items, onto the serving handle
        merged = [n[s] + a.kept for s in range(2)]
        host_rows = [np.ascontiguousarray(torch.cat([new_rows[s], torch.zeros((a.kept, k), device=dev)]).cpu().numpy()) for s in range(2)]
        hp = np.concatenate([kp.cpu().numpy(), np.full(a.kept, int(kp[-1]), np.int64)])
        hi = ki.cpu().numpy()
        old = pkg.ALSCore(k)
        for s in range(2):
            old.set_factor_rows(s, merged[s])
        old.set_matrix(X_, np.zeros(merged[0] + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
        times = []
        for it in range(1 + min(a.reps, 3)):
            t0 = time.perf_counter()
            old.set_factors(X_, host_rows[0])
            old.set_factors(Y_, host_rows[1])
            old.set_known_items(hp, hi)
            old.get_rows(X_, [0])                      # (a read that waits for the uploads)
            if it >= 1:
                times.append((time.perf_counter() - t0) * 1e3)
        out["parent_route_ms"] = median(times)
        old.close()
    core.close()

    for key, ph in out["phases"].items():
        print("%-14s %9.3f ms  %8.1f MB must move  %8.1f GB/s" % (key, ph["ms"], ph["bytes"] / 1e6, ph["GBps"] or 0.0))
    for s in names:
        m = out["memcpy_dtod"][s]
        print("memcpy_dtod %-6s %9.3f ms  %8.1f MB copied     %8.1f GB/s moved" % (s, m["ms"], m["bytes_copied"] / 1e6, m["GBps_moved"]))
    print("load: sides %.2f ms, known items %.2f ms, tag sets %.2f ms, ticket %.2f ms, call %.2f ms; parent route %s ms"
          % (out["sides_ms"], out["known_ms"], out["tags_ms"], out["total_ms"], out["call_ms"], out.get("parent_route_ms")))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
