#!/usr/bin/env python
"""Ingest -> CSR throughput on one MI355X: records/s of mals_ingest_finish on a
synthetic record stream already resident in HBM, the algorithmic bytes all passes move, and the oracle
(record-by-record restatement of the reference's maps, pure Python, 1 core) on a bounded sample.
usage: python tools/bench_ingest.py [--records N] [--users U] [--items I] [--removes P]
       python tools/bench_ingest.py --from-text [...]   the same stream as TEXT ("user,item,value\\n" lines, resident in
           HBM) through mals_ingest_append_text + mals_ingest_finish: lines/s of the whole path, the text kernels'
           own rate, and the end-to-end roofline on the bytes that must move (text in + both CSR matrices out)
       python tools/bench_ingest.py --ranks 1,2,4 [--records N]   the same text cut into N shares, one single-process group of N
           members on device 0 (MALS_GROUP_PEER_COPY) and mals_group_ingest_finish: one JSON line per N with the split kernels'
           time, traffic and rate, the device bytes every member's ingest holds afterwards next to one whole-input ingest plus
           mals_ingest_install_group, and the entry imbalance of the X slices
       python tools/bench_ingest.py --live [--live-users U] [--live-items I] [--live-lines N] [--features K] [--repeat R] [--tags]
           the id directory and mals_ingest_apply: (1) mals_ids_resolve on a directory of 1M ids, batches of 1e6 ids of which a
           tenth is new, next to the join of mals_load_generation over as many ids and to one CPU thread with
           std::unordered_map (tools/ubench/ids_map_baseline.cpp, compiled here); (2) R + 1 streams of N lines applied to a
           U x I model with Ingest.apply, and the same records driven by hand (a Python dict, grow_factor_rows,
           set_preferences / remove_preferences run by run) on a second handle: per-stream wall times of both, the spread of
           the by-hand figure, apply's time by stage, and whether the two handles end bit-identical"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000_000)
    ap.add_argument("--users", type=int, default=10_000_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--removes", type=float, default=0.01)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--from-text", action="store_true")
    ap.add_argument("--text-chunk", type=int, default=1 << 25, help="lines formatted per torch pass")
    ap.add_argument("--stream-text", action="store_true",
                    help="--from-text for inputs whose text does not fit beside the ingest (C5: 5e9 lines = 88 GB): every piece of text is "
                         "generated in HBM, handed to mals_ingest_append_text and dropped; times are the library's HIP-event times of its "
                         "kernels (text_info, stats), so the generator between the pieces is not in them; one run, no repeats")
    ap.add_argument("--partition-records", type=int, default=0, help="MALS_INGEST_OPT_PARTITION_RECORDS (0: the library's default)")
    ap.add_argument("--ranks", type=str, default="", help="comma-separated member counts: the sharded ingest (mals_group_ingest_finish)")
    ap.add_argument("--features", type=int, default=32, help="--ranks: k of the group (its factor replicas are declared by the finish)")
    ap.add_argument("--live", action="store_true", help="the id directory and mals_ingest_apply against the same stream driven by hand")
    ap.add_argument("--live-users", type=int, default=1_000_000)
    ap.add_argument("--live-items", type=int, default=100_000)
    ap.add_argument("--live-lines", type=int, default=100_000)
    ap.add_argument("--tags", action="store_true",
                    help="--live: every tenth line of the stream is a tag line (setUserTag / setItemTag by turns, 1000 tags), applied with "
                         "MALS_INGEST_OPT_LIVE_TAGS")
    a = ap.parse_args()
    if a.live:
        return live(a)
    if a.ranks:
        return ranks(a)
    if a.from_text:
        return from_text(a)
    import numpy as np
    import torch
    import myrrix_recommender_amd as pkg
    from myrrix_recommender_amd import ingest
    gen = torch.Generator(device="cuda").manual_seed(1234567890)
    n = a.records
    u = torch.randint(0, a.users, (n,), device="cuda", generator=gen)
    # items: heavy-tailed popularity like synth.torch_problem
    i = (torch.rand(n, device="cuda", generator=gen).pow_(3.0) * a.items).long().clamp_(max=a.items - 1)
    v = torch.randint(1, 6, (n,), device="cuda", generator=gen).float()
    if a.removes > 0:
        v[torch.rand(n, device="cuda", generator=gen) < a.removes] = float("nan")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()   # hand the generator's temporaries back to the driver before the library allocates
    best, workspace_ms = None, 0.0
    with ingest.Ingest(0) as g:
        g.append(u, i, v)
        for _ in range(a.repeat):
            g.finish()
            st = g.stats()
            workspace_ms = max(workspace_ms, st["workspace_ms"])   # paid once, by the first finish
            if best is None or st["finish_ms"] < best["finish_ms"]:
                best = st
        c = g.counts()
    out = {"metric": "ingest records/s (records -> two CSR matrices + id tables, on device)", "value": n / best["finish_ms"] * 1e3,
           "unit": "records/s", "ms": best["finish_ms"], "records": n, "users": c["users"], "items": c["items"], "nnz": c["nnz"],
           "radix_passes": best["radix_passes"], "workspace_alloc_ms": workspace_ms,
           "roofline": {"bound": "hbm", "achieved": best["bytes_moved"] / best["finish_ms"] / 1e6, "peak": 8000.0, "unit": "GB/s",
                        "frac": best["bytes_moved"] / best["finish_ms"] / 1e6 / 8000.0,
                        "algorithmic_bytes": best["bytes_moved"], "bytes_per_record": best["bytes_moved"] / n}}
    if not a.no_cpu_baseline:
        from oracle import ingest_oracle as io
        m = min(n, 2_000_000)
        us, is_, vs = u[:m].cpu().numpy(), i[:m].cpu().numpy(), v[:m].cpu().numpy()
        t0 = time.perf_counter()
        io.read_input_records(us, is_, vs)
        dt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": m / dt, "unit": "records/s", "cores": 1, "kind": "port",
                               "sample": "first %d records, oracle/ingest_oracle.py (pure-Python dict-of-dicts like the reference's map-of-maps)" % m}
    print(json.dumps(out))


def format_lines(torch, u, i, v):
    """(user, item, value | NaN) -> the bytes of "user,item,value\\n" lines (value token empty for a remove), on the device:
    fixed-width digit columns + a mask of the columns that print."""
    m = u.shape[0]
    wu, wi = 8, 7
    cols = wu + 1 + wi + 1 + 1 + 1
    mat = torch.empty((m, cols), dtype=torch.uint8, device=u.device)
    keep = torch.ones((m, cols), dtype=torch.bool, device=u.device)
    for j in range(wu):
        p = 10 ** (wu - 1 - j)
        mat[:, j] = ((u // p) % 10 + 48).to(torch.uint8)
        if p > 1:
            keep[:, j] = u >= p
    mat[:, wu] = 44
    for j in range(wi):
        p = 10 ** (wi - 1 - j)
        mat[:, wu + 1 + j] = ((i // p) % 10 + 48).to(torch.uint8)
        if p > 1:
            keep[:, wu + 1 + j] = i >= p
    mat[:, wu + 1 + wi] = 44
    nan = v != v
    mat[:, wu + wi + 2] = (torch.where(nan, torch.zeros_like(v), v).to(torch.int64) + 48).to(torch.uint8)
    keep[:, wu + wi + 2] = ~nan
    mat[:, wu + wi + 3] = 10
    return mat[keep]


def from_text(a):
    import numpy as np
    import torch
    import myrrix_recommender_amd as pkg
    from myrrix_recommender_amd import _lib, ingest
    assert a.users <= 10 ** 8 and a.items <= 10 ** 7
    gen = torch.Generator(device="cuda").manual_seed(1234567890)
    n = a.records
    texts, n_bytes, sample = [], 0, None

    def pieces():
        nonlocal sample
        for lo in range(0, n, a.text_chunk):
            m = min(a.text_chunk, n - lo)
            u = torch.randint(0, a.users, (m,), device="cuda", generator=gen)
            i = (torch.rand(m, device="cuda", generator=gen).pow_(3.0) * a.items).long().clamp_(max=a.items - 1)
            v = torch.randint(1, 6, (m,), device="cuda", generator=gen).float()
            if a.removes > 0:
                v[torch.rand(m, device="cuda", generator=gen) < a.removes] = float("nan")
            t = format_lines(torch, u, i, v)
            if sample is None:
                sample = (u[:200000].cpu().numpy(), i[:200000].cpu().numpy(), v[:200000].cpu().numpy())
            del u, i, v
            yield t, lo + m >= n
    best = None
    if a.stream_text:
        with ingest.Ingest(0) as g:
            g.set_option(_lib.INGEST_OPT_RESERVE_RECORDS, n)
            if a.partition_records:
                g.set_option(_lib.INGEST_OPT_PARTITION_RECORDS, a.partition_records)
            t0 = time.perf_counter()
            for t, last in pieces():
                n_bytes += t.numel()
                g.append_text(t, last)
                del t
            info = g.text_info()
            wall_text = (time.perf_counter() - t0) * 1e3     # (includes the generator: not a rate of anything)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            g.finish()
            st, c = g.stats(), g.counts()
            best = {"total_ms": info["stage_ms"] + info["parse_ms"] + st["finish_ms"], "parse_ms": info["parse_ms"], "stage_ms": info["stage_ms"],
                    "append_text_wall_ms": wall_text, "finish": st, "info": info, "counts": c, "partitions": g.partitions()}
            hbm = torch.cuda.mem_get_info()
            best["hbm_GB_in_use_after_finish"] = round((hbm[1] - hbm[0]) / 1e9, 1)
    else:
        for t, last in pieces():
            texts.append(t)
            n_bytes += t.numel()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    for rep in range(0 if a.stream_text else a.repeat):
        with ingest.Ingest(0) as g:
            g.set_option(_lib.INGEST_OPT_RESERVE_RECORDS, n)
            if a.partition_records:
                g.set_option(_lib.INGEST_OPT_PARTITION_RECORDS, a.partition_records)
            t0 = time.perf_counter()
            for k, t in enumerate(texts):
                g.append_text(t, k == len(texts) - 1)        # one file in len(texts) pieces: lines straddle the pieces
            info = g.text_info()
            t1 = time.perf_counter()
            g.finish()
            st = g.stats()
            c = g.counts()
            wall_text = (t1 - t0) * 1e3
            total_ms = info["stage_ms"] + info["parse_ms"] + st["finish_ms"]
            if best is None or total_ms < best["total_ms"]:
                best = {"total_ms": total_ms, "parse_ms": info["parse_ms"], "stage_ms": info["stage_ms"], "append_text_wall_ms": wall_text, "finish": st, "info": info,
                        "counts": c, "partitions": g.partitions()}
    assert best["info"]["lines"] == n and best["info"]["records"] == n and best["info"]["bad_lines"] == 0
    csr_out = 2.0 * best["counts"]["nnz"] * 8 + 8.0 * (best["counts"]["users"] + best["counts"]["items"] + 2) \
        + 8.0 * (best["counts"]["users"] + best["counts"]["items"])
    # what the text kernels read and write: the text three times (line count, line starts, parse); per line its start
    # offset (4 written, 8 read), status + parsed fields (21 written), status twice more (summary, compaction), the
    # parsed fields once more (20) and the record (20 written)
    parse_bytes = 3.0 * n_bytes + n * (4 + 8 + 21 + 2 + 20 + 20)
    out = {"metric": "ingest lines/s (text of the input files -> records -> two CSR matrices + id tables, on device)",
           "value": n / best["total_ms"] * 1e3, "unit": "lines/s", "ms": best["total_ms"], "text_ms": best["parse_ms"],
           "block_copy_ms": best["stage_ms"],
           "append_text_wall_ms": best["append_text_wall_ms"], "finish_ms": best["finish"]["finish_ms"], "lines": n, "text_bytes": n_bytes,
           "bytes_per_line": n_bytes / n, "users": best["counts"]["users"], "items": best["counts"]["items"], "nnz": best["counts"]["nnz"],
           "full_parser_lines": best["info"]["full_parser_lines"],
           "data": "synthetic, text resident in HBM" + (" piece by piece (generated, appended, dropped: --stream-text)" if a.stream_text else ""),
           "user_ranges": best["partitions"][0], "item_ranges": best["partitions"][1], "hbm_GB_in_use_after_finish": best.get("hbm_GB_in_use_after_finish"),
           "roofline": {"bound": "hbm", "what": "end to end: text bytes in + both CSR matrices and id tables out",
                        "achieved": (n_bytes + csr_out) / best["total_ms"] / 1e6, "peak": 8000.0, "unit": "GB/s",
                        "frac": (n_bytes + csr_out) / best["total_ms"] / 1e6 / 8000.0, "algorithmic_bytes": n_bytes + csr_out},
           "roofline_text_kernels": {"bound": "hbm", "what": "the text kernels alone, on the bytes their passes read and write",
                                     "achieved": parse_bytes / best["parse_ms"] / 1e6, "peak": 8000.0, "unit": "GB/s",
                                     "frac": parse_bytes / best["parse_ms"] / 1e6 / 8000.0, "bytes": parse_bytes,
                                     "text_GBps": n_bytes / best["parse_ms"] / 1e6},
           "roofline_finish": {"bound": "hbm", "achieved": best["finish"]["bytes_moved"] / best["finish"]["finish_ms"] / 1e6, "peak": 8000.0,
                               "unit": "GB/s", "frac": best["finish"]["bytes_moved"] / best["finish"]["finish_ms"] / 1e6 / 8000.0,
                               "radix_passes": best["finish"]["radix_passes"]}}
    if not a.no_cpu_baseline:
        from oracle import ingest_text_oracle as to
        us, is_, vs = sample
        lines = ["%d,%d,%s" % (x, y, "" if z != z else "%d" % z) for x, y, z in zip(us.tolist(), is_.tolist(), vs.tolist())]
        data = ("\n".join(lines) + "\n").encode()
        t0 = time.perf_counter()
        to.expected([data])
        dt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": len(lines) / dt, "unit": "lines/s", "cores": 1, "kind": "port",
                               "sample": "first %d lines, oracle/ingest_text_oracle.py + ingest_oracle.py (pure Python restatement of "
                                         "InputFilesReader.readInputFiles)" % len(lines)}
    print(json.dumps(out))


def ranks(a):
    """--ranks: the stream of --from-text generated piece by piece; piece p goes to share p * N // pieces (shares in stream
    order, every piece ends at a line end); one single-process group of N members on device 0 finishes it collectively."""
    import torch
    import myrrix_recommender_amd as pkg
    from myrrix_recommender_amd import _lib, ingest
    n, k = a.records, a.features

    def pieces():
        gen = torch.Generator(device="cuda").manual_seed(1234567890)
        n_pieces = (n + a.text_chunk - 1) // a.text_chunk
        for p, lo in enumerate(range(0, n, a.text_chunk)):
            m = min(a.text_chunk, n - lo)
            u = torch.randint(0, a.users, (m,), device="cuda", generator=gen)
            i = (torch.rand(m, device="cuda", generator=gen).pow_(3.0) * a.items).long().clamp_(max=a.items - 1)
            v = torch.randint(1, 6, (m,), device="cuda", generator=gen).float()
            if a.removes > 0:
                v[torch.rand(m, device="cuda", generator=gen) < a.removes] = float("nan")
            t = format_lines(torch, u, i, v)
            del u, i, v
            yield p, n_pieces, t

    def hbm_in_use():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        f, t = torch.cuda.mem_get_info()
        return t - f
    # the whole-input path: one ingest of everything + mals_ingest_install_group (what every rank holds today)
    base0 = hbm_in_use()
    with ingest.Ingest(0) as g, pkg.GroupALS.single_process(k, [0], backend=_lib.GROUP_PEER_COPY) as grp:
        g.set_option(_lib.INGEST_OPT_RESERVE_RECORDS, n)
        for p, n_p, t in pieces():
            g.append_text(t, p == n_p - 1)
            del t
        g.finish()
        g.install_group(grp)
        mem = g.memory()
        c = g.counts()
        whole = {"ingest_bytes_held": mem["work_bytes"] + mem["result_bytes"], "work_bytes": mem["work_bytes"],
                 "result_bytes": mem["result_bytes"], "finish_ms": g.stats()["finish_ms"],
                 "hbm_bytes_in_use_after_install": hbm_in_use() - base0}
    replica_bytes = 4.0 * k * (c["users"] + c["items"])
    for N in [int(x) for x in a.ranks.split(",")]:
        base = hbm_in_use()
        ings = [ingest.Ingest(0) for _ in range(N)]
        with pkg.GroupALS.single_process(k, [0] * N, backend=_lib.GROUP_PEER_COPY) as grp:
            for s, g in enumerate(ings):
                g.set_share(s)
                g.set_option(_lib.INGEST_OPT_RESERVE_RECORDS, (n + N - 1) // N)
            for p, n_p, t in pieces():
                s = p * N // n_p
                last = (p + 1) * N // n_p != s or p == n_p - 1
                ings[s].append_text(t, last)
                del t
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grp.ingest_finish(ings)
            wall_ms = (time.perf_counter() - t0) * 1e3
            in_use = hbm_in_use() - base
            mems = [g.memory() for g in ings]
            x_entries = [g.slice_entries(pkg.SIDE_X) for g in ings]    # entries of every member's X slice
            split_ms = [m["split_ms"] for m in mems]
            split_bytes = [m["split_bytes"] for m in mems]
            held = [m["work_bytes"] + m["result_bytes"] for m in mems]
            cc = ings[0].counts()
            rec = [g.counts()["records"] for g in ings]
            out = {"metric": "sharded ingest (mals_group_ingest_finish), %d members of one single-process group on one MI355X" % N,
                   "ranks": N, "lines": n, "users": cc["users"], "items": cc["items"], "nnz": cc["nnz"],
                   "group_finish_wall_ms": wall_ms,
                   "group_finish_wall_ms_per_member": wall_ms / N,
                   "note": "the members share one device and are finished one after another by one thread: the wall time is the "
                           "sum over members (plus the host merges), not what N devices would take in parallel; the exchange is "
                           "hipMemcpyPeerAsync inside one device, not xGMI",
                   "split": {"ms_per_member": split_ms, "bytes_per_member": split_bytes,
                             "GBps_per_member": [b / t / 1e6 if t > 0 else None for b, t in zip(split_bytes, split_ms)],
                             "what": "count + scatter kernels of both splits (records by user owner, entries by item owner) and their "
                                     "scan; bytes = 50 per record moved (8 B key + 1 B destination in the count pass, 1 + 20 B read and "
                                     "20 B written in the scatter)",
                             "frac_of_6290_GBps_copy": [b / t / 1e6 / 6290.0 if t > 0 else None for b, t in zip(split_bytes, split_ms)]},
                   "records_finished_per_member": rec,
                   "hbm_per_member": {"ingest_bytes_held": held, "work_bytes": [m["work_bytes"] for m in mems],
                                      "work_bytes_at_replicas": [m["work_bytes_at_replicas"] for m in mems],
                                      "replica_bytes_k": replica_bytes,
                                      "bytes_held_incl_replicas_max": max(held) + replica_bytes},
                   "hbm_whole_input_per_rank": dict(whole, replica_bytes_k=replica_bytes,
                                                    bytes_held_incl_replicas=whole["ingest_bytes_held"] + replica_bytes),
                   "hbm_bytes_in_use_after_group_finish_all_members": in_use,
                   "x_slice_entries": x_entries,
                   "x_entry_imbalance_max_over_mean": max(x_entries) / (sum(x_entries) / N) if sum(x_entries) else None,
                   "features": k}
        for g in ings:
            g.close()
        print(json.dumps(out), flush=True)


def live(a):
    import shutil
    import subprocess
    import tempfile
    import numpy as np
    import myrrix_recommender_amd as pkg
    from myrrix_recommender_amd import ingest
    from myrrix_recommender_amd.core import HostSolver
    X_, Y_ = pkg.SIDE_X, pkg.SIDE_Y
    rng = np.random.default_rng(20240607)
    out = {"metric": "id directory and mals_ingest_apply (live ingest)", "features": a.features}

    # ---- 1. resolve rate -----------------------------------------------------------------------------------------------
    n_dir, n_batch, batches = 1_000_000, 1_000_000, 5
    ids = rng.permutation(np.arange(1, 4 * n_dir, dtype=np.int64) * 2654435761)[:n_dir + batches * n_batch // 10]
    dir_ids, fresh = ids[:n_dir], ids[n_dir:]
    with pkg.ALSCore(8) as c:
        c.set_factor_rows(X_, n_dir)
        t0 = time.perf_counter()
        c.set_ids(X_, dir_ids)
        set_ms = (time.perf_counter() - t0) * 1e3
        res_ms, look_ms = [], []
        for b in range(batches):
            batch = dir_ids[rng.integers(0, n_dir, n_batch)]
            where = rng.permutation(n_batch)[:n_batch // 10]
            batch[where] = fresh[b * (n_batch // 10):(b + 1) * (n_batch // 10)]
            t0 = time.perf_counter()
            c.rows_of(X_, batch)
            look_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            rows, n_new = c.rows_of(X_, batch, add=True)
            res_ms.append((time.perf_counter() - t0) * 1e3)
            assert n_new == n_batch // 10 and rows.max() == n_dir + (b + 1) * (n_batch // 10) - 1
        out["resolve"] = {"directory_ids": n_dir, "batch_ids": n_batch, "new_per_batch": n_batch // 10, "set_ids_ms": set_ms,
                          "resolve_ms": res_ms, "lookup_ms": look_ms, "resolve_ids_per_s": n_batch / min(res_ms) * 1e3,
                          "lookup_ids_per_s": n_batch / min(look_ms) * 1e3,
                          "what": "wall time of mals_ids_resolve / mals_ids_lookup with host arrays: 8 MB up, 8 MB down, and for "
                                  "resolve the growth of the k = 8 replica by 100k rows; best of %d batches" % batches}
    with pkg.ALSCore(8) as c:      # the join of mals_load_generation over as many ids: 1M live against 1M new, half of them shared
        c.set_factor_rows(X_, n_dir)
        c.set_factor_rows(Y_, 64)
        new_ids = np.concatenate([dir_ids[:n_dir // 2], fresh[:n_dir // 2]])
        res, _, _ = c.load_generation(dir_ids, np.arange(64, dtype=np.int64), new_ids, np.arange(64, dtype=np.int64),
                                      np.zeros((n_dir, 8), np.float32), np.zeros((64, 8), np.float32), keep_not_updated=True)
        out["load_generation_join"] = {"live_ids": n_dir, "new_ids": n_dir, "join_ms": res["join_ms"][0],
                                       "probed_ids_per_s": n_dir / res["join_ms"][0] * 1e3,
                                       "what": "HIP events around the join of side X: two tables of 1M ids built, 1M ids probed"}
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx:
        with tempfile.TemporaryDirectory() as td:
            exe = os.path.join(td, "ids_map_baseline")
            subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "ubench", "ids_map_baseline.cpp")])
            r = subprocess.run([exe, str(n_dir), str(n_batch), "100", str(batches)], capture_output=True, text=True, check=True)
            out["cpu_baseline"] = {"value": float(r.stdout.split()[0]), "unit": "ids/s", "cores": 1, "kind": "std::unordered_map, one thread, the same batches"}

    # ---- 2. apply against the same stream by hand ---------------------------------------------------------------------------
    U, I, k, N = a.live_users, a.live_items, a.features, a.live_lines
    X = (rng.standard_normal((U, k)) * 0.1).astype(np.float32)
    Y = (rng.standard_normal((I, k)) * 0.1).astype(np.float32)
    uid = np.arange(U, dtype=np.int64) * 7 + 1_000_000_000
    iid = np.arange(I, dtype=np.int64) * 3 + 5
    ptr = np.arange(0, 3 * U + 1, 3, dtype=np.int64)
    col = (rng.integers(0, I - 3, U)[:, None] + np.arange(3)).ravel().astype(np.int32)    # three known items per user
    Ys = Y[:20000].astype(np.float64)
    sx = HostSolver.create(X[:20000].astype(np.float64).T @ X[:20000].astype(np.float64) * (U / 20000) + np.eye(k) * 0.1)
    sy = HostSolver.create(Ys.T @ Ys * (I / 20000) + np.eye(k) * 0.1)

    def handle():
        c = pkg.ALSCore(k)
        c.set_factor_rows(X_, U)
        c.set_factor_rows(Y_, I)
        c.set_factors(X_, X)
        c.set_factors(Y_, Y)
        c.set_matrix(X_, ptr, col, np.ones(len(col), np.float32))
        c.set_foldin_solver(X_, sx)
        c.set_foldin_solver(Y_, sy)
        return c

    def stream(r):
        """N lines: 5 % of the users and 2 % of the items new (ids of this stream alone), a quarter removes, half of them of a
        pair the stream set before"""
        u = uid[rng.integers(0, U, N)]
        i = iid[rng.integers(0, I, N)]
        nu = rng.random(N) < 0.05
        u[nu] = -(r * 10_000_000 + rng.integers(1, N, nu.sum()))
        ni = rng.random(N) < 0.02
        i[ni] = -(r * 10_000_000 + rng.integers(1, N // 4, ni.sum()))
        v = rng.choice(np.array([1.0, 2.0, 3.0, 5.0, -1.0], np.float32), N)
        rem = np.nonzero(rng.random(N) < 0.25)[0]
        v[rem] = np.nan
        back = rem[rng.random(len(rem)) < 0.5]
        src = (back * rng.random(len(back))).astype(np.int64)
        u[back], i[back] = u[src], i[src]
        kd = np.zeros(N, np.uint8)           # 0 a preference, 1 a tag in the user column (setItemTag), 2 in the item column (setUserTag)
        us, its = [str(x) for x in u.tolist()], [str(y) for y in i.tolist()]
        if a.tags:
            at = np.arange(9, N, 10)
            kd[at] = 1 + (at // 10) % 2
            for t, name in zip(at.tolist(), rng.integers(0, 1000, len(at)).tolist()):
                if kd[t] == 1:
                    u[t], us[t] = tag_ids[name], '"tag%d"' % name
                else:
                    i[t], its[t] = tag_ids[name], '"tag%d"' % name
        text = "".join("%s,%s,%s\n" % (x, y, "" if z != z else "%g" % z) for x, y, z in zip(us, its, v.tolist())).encode()
        return u, i, v, kd, text

    tag_ids = [pkg.tag_id("tag%d" % j) for j in range(1000)] if a.tags else []
    ca, ch = handle(), handle()
    ca.set_ids(X_, uid)
    ca.set_ids(Y_, iid)
    urow = {int(x): r for r, x in enumerate(uid.tolist())}
    irow = {int(x): r for r, x in enumerate(iid.tolist())}

    def by_hand(u, i, v, kd):
        keep = (v == v) | (kd == 0)          # a tag remove is ignored altogether
        u, i, v, kd = u[keep], i[keep], v[keep], kd[keep]
        is_set = v == v
        ul, il = u.tolist(), i.tolist()
        for t in np.nonzero(is_set)[0].tolist():
            urow.setdefault(ul[t], len(urow))
            irow.setdefault(il[t], len(irow))
        ch.grow_factor_rows(X_, len(urow))
        ch.grow_factor_rows(Y_, len(irow))
        ur = np.array([urow.get(x, -1) for x in ul], np.int64)
        ir = np.array([irow.get(x, -1) for x in il], np.int64)
        live = is_set | ((ur >= 0) & (ir >= 0))
        ur, ir, vv = ur[live], ir[live], v[live]
        ss = np.where(is_set[live], 1 + kd[live].astype(np.int64), 0)     # a batch of the existing calls holds one kind of write
        cut = np.concatenate([[0], np.nonzero(ss[1:] != ss[:-1])[0] + 1, [len(ss)]])
        calls = 0
        for b, e in zip(cut[:-1].tolist(), cut[1:].tolist()):
            if ss[b]:
                (ch.set_preferences, ch.set_item_tags, ch.set_user_tags)[ss[b] - 1](ur[b:e], ir[b:e], vv[b:e], raise_on_error=False)
            else:
                ch.remove_preferences(ur[b:e], ir[b:e])
            calls += 1
        return calls

    rows = []
    with ingest.Ingest(0) as g:
        if a.tags:
            g.set_option(ingest.INGEST_OPT_LIVE_TAGS, 1)
        for r in range(a.repeat + 1):      # the first stream warms both routes up
            u, i, v, kd, text = stream(r + 1)
            parse0 = g.text_info()["parse_ms"] if r else 0.0
            g.append_text(text)
            parse_ms = g.text_info()["parse_ms"] - parse0
            lev0 = ca.foldin_stats()["device_ms_total"]
            t0 = time.perf_counter()
            st, _ = g.apply(ca, raise_on_error=False)
            apply_ms = (time.perf_counter() - t0) * 1e3
            times = ca.ingest_apply_times()
            levels_ms = ca.foldin_stats()["device_ms_total"] - lev0
            t0 = time.perf_counter()
            calls = by_hand(u, i, v, kd)
            hand_ms = (time.perf_counter() - t0) * 1e3
            same = all(ca.factor_digest(s) == ch.factor_digest(s) for s in (X_, Y_))
            rows.append({"apply_ms": apply_ms, "by_hand_ms": hand_ms, "parse_ms": parse_ms, "ids_ms": times["ids_ms"], "plan_ms": times["plan_ms"],
                         "writes_ms": times["writes_ms"], "level_kernels_ms": levels_ms, "write_calls": st["write_calls"],
                         "by_hand_calls": calls, "new_users": st["new_users"], "new_items": st["new_items"], "bit_identical": same})
            if a.tags:
                rows[-1]["tag_stats"] = ca.ingest_apply_tag_stats()
                same_sets = all(np.array_equal(ca.tag_rows(s), ch.tag_rows(s)) for s in (X_, Y_))
                rows[-1]["bit_identical"] = same and same_sets
    timed = rows[1:]
    hand = np.array([x["by_hand_ms"] for x in timed])
    app = np.array([x["apply_ms"] for x in timed])
    out["apply"] = {"users": U, "items": I, "lines": N, "tag_lines": bool(a.tags), "streams": timed, "warm_up": rows[0],
                    "apply_ms_median": float(np.median(app)), "apply_ms_min": float(app.min()), "apply_ms_max": float(app.max()),
                    "by_hand_ms_median": float(np.median(hand)), "by_hand_ms_min": float(hand.min()), "by_hand_ms_max": float(hand.max()),
                    "by_hand_spread_ms": float(hand.max() - hand.min()),
                    "apply_slower_than_by_hand_beyond_spread": bool(np.median(app) > np.median(hand) + (hand.max() - hand.min())),
                    "all_bit_identical": all(x["bit_identical"] for x in rows),
                    "what": "wall ms per stream; apply starts from the parsed records in the ingest (parse_ms: HIP events of the text "
                            "kernels, outside apply_ms), by hand from the same records as numpy arrays; ids_ms: HIP events on the "
                            "handle's stream around gather, resolve and lookup; plan_ms, writes_ms: host clock inside the ticket; "
                            "level_kernels_ms: HIP events around the update kernels (mals_foldin_stats)"}
    ca.close()
    ch.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
