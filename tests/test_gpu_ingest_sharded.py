"""The sharded ingest (mals_group_ingest_finish): every member of a group ingests one SHARE of the input stream, and the
collective finish leaves every member exactly its slices of what ONE ingest of the whole stream builds -- bit for bit against
oracle/ingest_text_oracle.expected on the whole stream -- with the text counters, the header rule and the abort rule of the
whole stream, then factorizes like any other upload.  Shares are cut at random line starts (an empty share 0 and a share 0
that holds only the header line included), and read from a directory by mals_ingest_read_dir_share."""
import gzip
import multiprocessing as mp
import os
import zipfile

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib, ingest
from oracle import ingest_text_oracle as to
from oracle import oracle, topn_oracle
from tests import text_corpus
from tests.test_gpu_ingest_group import corpus

pytestmark = pytest.mark.gpu
REL_TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "cpp", "libmock_rccl.so")
X, Y = pkg.SIDE_X, pkg.SIDE_Y


def rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / max(np.linalg.norm(b.astype(np.float64)), 1e-30))


def line_starts(data):
    """byte offsets at which a line starts ('\\n', lone '\\r' terminators), the end of the data included"""
    out = [0]
    for i, b in enumerate(data):
        if b == 10 or (b == 13 and (i + 1 >= len(data) or data[i + 1] != 10)):
            out.append(i + 1)
    if out[-1] != len(data):
        out.append(len(data))
    return sorted(set(out))


def cut(data, n, seed, first=None):
    """n shares of data cut at random line starts; first: 'empty' or 'header' pins share 0"""
    rng = np.random.default_rng(seed)
    starts = line_starts(data)
    inner = starts[1:-1]
    fixed = []
    if first == "empty":
        fixed = [0]
    elif first == "header":
        fixed = [starts[1]]
    k = n - 1 - len(fixed)
    pts = sorted(fixed + sorted(rng.choice(inner, size=k, replace=False).tolist())) if k > 0 else fixed
    b = [0] + pts + [len(data)]
    return [data[b[i]:b[i + 1]] for i in range(n)]


def whole_counters(data):
    with ingest.Ingest(0) as g:
        g.append_text(data, True)
        g.finish()
        t = g.text_info()
    return t["lines"], t["bad_lines"], t["header_lines"]


def check_slices(grp, ings, want, counters):
    (uid, rp, col, val), (iid, cp, ccol, cval) = want["csr_x"], want["csr_y"]
    bx, by = grp.bounds(X), grp.bounds(Y)
    assert bx[0] == 0 and bx[-1] == len(uid) and by[-1] == len(iid)
    for i, g in enumerate(ings):
        _, rank = grp.local(i)
        c = g.counts()
        assert (c["users"], c["items"], c["nnz"]) == (len(uid), len(iid), len(col))
        assert np.array_equal(g.ids(X), uid) and np.array_equal(g.ids(Y), iid)
        for side, (p, cc, vv), b in ((X, (rp, col, val), bx), (Y, (cp, ccol, cval), by)):
            b0, n = g.slice(side)
            assert (b0, n) == (b[rank], b[rank + 1] - b[rank])
            srp, scol, sval = g.csr(side)
            e0, e1 = p[b0], p[b0 + n]
            assert np.array_equal(srp, p[b0:b0 + n + 1] - e0), (rank, side)
            assert np.array_equal(scol, cc[e0:e1]) and np.array_equal(sval.view(np.uint32), vv[e0:e1].view(np.uint32)), (rank, side)
        kp, ki = g.known_items()
        b0, n = g.slice(X)
        k0, k1 = want["known_ptr"][b0], want["known_ptr"][b0 + n]
        assert np.array_equal(kp, want["known_ptr"][b0:b0 + n + 1] - k0) and np.array_equal(ki, want["known_idx"][k0:k1])
        assert np.array_equal(g.tag_ids(_lib.ITEM_TAG_IDS), want["item_tag_ids"])
        assert np.array_equal(g.tag_ids(_lib.USER_TAG_IDS), want["user_tag_ids"])
        t = g.text_info()
        assert (t["lines"], t["bad_lines"], t["header_lines"]) == counters
        assert t["lines"] == want["lines"] and t["bad_lines"] == want["bad_lines"]
        assert g.memory()["work_bytes"] == 0       # records, text buffers, workspace: all released


def factorize_and_check(grp, want, k, users_per_member=6):
    (uid, rp, col, val), (iid, cp, ccol, cval) = want["csr_x"], want["csr_y"]
    Y0 = (np.random.default_rng(k).standard_normal((len(iid), k)) / np.sqrt(k)).astype(np.float32)
    grp.set_factors(Y, Y0)
    grp.iterate(2)
    Xg = grp.get_factors(X, 0, len(uid))
    Yg = grp.get_factors(Y, 0, len(iid))
    Xo, Yo = None, Y0
    for _ in range(2):
        Xo = oracle.half_iteration(rp, col, val, Yo, threads=4)
        Yo = oracle.half_iteration(cp, ccol, cval, Xo, threads=4)
    assert rel(Xg, Xo) < REL_TOL and rel(Yg, Yo) < REL_TOL, (rel(Xg, Xo), rel(Yg, Yo))
    tags = want["user_tag_ids"]
    tag_idx = np.searchsorted(iid, tags)
    tag_idx = tag_idx[(tag_idx < len(iid)) & (iid[np.minimum(tag_idx, len(iid) - 1)] == tags)]
    bx = grp.bounds(X)
    for r in range(len(bx) - 1):
        users = np.arange(bx[r], bx[r + 1], dtype=np.int64)[:users_per_member]
        if len(users) == 0:
            continue
        idx, sc, cnt = grp.recommend(users, 8)
        for q, u in enumerate(users):
            known = want["known_idx"][want["known_ptr"][u]:want["known_ptr"][u + 1]]
            oidx, osc = topn_oracle.recommend(Yg, Xg[u], 8, known, tag_idx)
            assert cnt[q] == len(oidx) and np.array_equal(idx[q, :cnt[q]], oidx), (r, u)
            assert np.array_equal(sc[q, :cnt[q]].view(np.uint32), np.asarray(osc, np.float32).view(np.uint32))


def run_sharded(world, shares, backend, k=32, part=0, known=True):
    ings = [ingest.Ingest(0) for _ in range(world)]
    grp = pkg.GroupALS.single_process(k, [0] * world, backend=backend, exchange_chunks=2)
    for s, (g, piece) in enumerate(zip(ings, shares)):
        g.set_share(s)
        if known:
            g.set_option(_lib.INGEST_OPT_KNOWN_ITEMS, 1)
        if part:
            g.set_option(_lib.INGEST_OPT_PARTITION_RECORDS, part)
        g.append_text(piece, True)
    grp.ingest_finish(ings)
    return grp, ings


CASES = [(2, None, 0), (3, "empty", 0), (4, "header", 0), (3, None, 300)]


def _case(world, first, part, backend, seed):
    data = corpus(900 + seed, 700, 260, 9000)
    want = to.expected([data])
    counters = whole_counters(data)
    grp, ings = run_sharded(world, cut(data, world, seed, first), backend, part=part)
    with grp:
        check_slices(grp, ings, want, counters)
        factorize_and_check(grp, want, 32)
    for g in ings:
        g.close()


@pytest.mark.parametrize("world,first,part", CASES)
def test_sharded_slices_bit_exact_peer_copy(world, first, part):
    _case(world, first, part, _lib.GROUP_PEER_COPY, world * 10 + part)


def _mock_worker(q):
    try:
        pkg.GroupALS.use_transport(MOCK)
        for world, first, part in CASES[:3]:
            _case(world, first, part, _lib.GROUP_RCCL, 50 + world)
        q.put("ok")
    except BaseException as e:   # noqa: BLE001 -- the parent reports it
        import traceback
        q.put("".join(traceback.format_exception(type(e), e, e.__traceback__)))


def test_sharded_slices_bit_exact_rccl_mock():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_mock_worker, args=(q,))
    p.start()
    p.join(240)
    if p.is_alive():
        p.kill()
        p.join()
        pytest.fail("the mock-RCCL run did not finish in time")
    assert p.exitcode == 0 and q.get(timeout=5) == "ok"


def _mixed_dir(path, seed):
    """several .csv files (one CRLF, one lone-CR), a .csv.gz, a .csv.zip and a large file the byte balance cuts"""
    os.makedirs(path, exist_ok=True)
    files = {
        "a.csv": corpus(seed, 300, 120, 3000),
        "b.csv": text_corpus.corpus(seed + 1, 400, p_odd=0.0, terminators=("\r\n",)),
        "c.csv": text_corpus.corpus(seed + 2, 400, p_odd=0.0, terminators=("\r",)),
        "d.csv": text_corpus.corpus(seed + 3, 3000, p_odd=0.0, terminators=("\n", "\r\n", "\r")),
    }
    for name, b in files.items():
        with open(os.path.join(path, name), "wb") as f:
            f.write(b)
    with gzip.open(os.path.join(path, "e.csv.gz"), "wb") as f:
        f.write(text_corpus.corpus(seed + 4, 500, p_odd=0.0))
    with zipfile.ZipFile(os.path.join(path, "f.csv.zip"), "w") as z:
        z.writestr("f.csv", text_corpus.corpus(seed + 5, 50, p_odd=0.0))
    t = 1_600_000_000
    for i, name in enumerate(sorted(os.listdir(path))):
        os.utime(os.path.join(path, name), (t + i, t + i))
    return path


def test_read_dir_share_cut_rule(tmp_path):
    d = _mixed_dir(str(tmp_path / "in"), 7)
    want = to.read_input_files(d)
    with ingest.Ingest(0) as whole:
        whole.read_dir(d)
        lines = whole.text_info()["lines"]
    assert lines == want["lines"]
    for n in range(1, 6):
        per = []
        for s in range(n):
            with ingest.Ingest(0) as g:
                g.read_dir_share(d, s, n)
                per.append(g.text_info()["lines"])
        assert sum(per) == lines, (n, per)
    # the group result of 4 shares read from the directory equals the one-ingest result
    exp = to.expected([to.file_bytes(p) for p in to.list_input_files(d)])
    ings = [ingest.Ingest(0) for _ in range(4)]
    with pkg.GroupALS.single_process(16, [0] * 4, backend=_lib.GROUP_PEER_COPY) as grp:
        for s, g in enumerate(ings):
            g.set_option(_lib.INGEST_OPT_KNOWN_ITEMS, 1)
            g.read_dir_share(d, s, 4)
        grp.ingest_finish(ings)
        t = ings[0].text_info()
        check_slices(grp, ings, exp, (t["lines"], t["bad_lines"], t["header_lines"]))
        assert t["lines"] == lines
    for g in ings:
        g.close()


def _errors(world, shares):
    """status of every member's finish (each share's own read errors ignored: it still enters the collective)"""
    ings = [ingest.Ingest(0) for _ in range(world)]
    codes = []
    with pkg.GroupALS.single_process(8, [0] * world, backend=_lib.GROUP_PEER_COPY) as grp:
        for s, (g, piece) in enumerate(zip(ings, shares)):
            g.set_share(s)
            try:
                g.append_text(piece, True)
            except pkg.MalsError:
                pass
        try:
            grp.ingest_finish(ings)
            codes.append(_lib.OK)
        except pkg.MalsError as e:
            codes.append(e.status)
    for g in ings:
        g.close()
    return codes[0]


def test_errors_agree():
    good = b"".join(b"%d,%d,1\n" % (u, i) for u in range(5) for i in range(4))
    bad = b"x,y,z\n"
    # 101 bad lines, no share holds 101 of them, lines after them
    s = [good + bad * 40, bad * 40 + good, bad * 21 + good]
    assert _errors(3, s) == _lib.IO_ERROR
    # exactly 101 bad lines, the 101st the last line of the stream: accepted
    s = [good + bad * 40, bad * 40, bad * 21]
    assert _errors(3, s) == _lib.OK
    # a lone-quote token in share 2 only
    s = [good, good, b'1,"\n' + good]
    assert _errors(3, s) == _lib.INVALID_ARG


def test_memory_released_before_replicas():
    data = corpus(5, 800, 300, 20000)
    grp, ings = run_sharded(2, cut(data, 2, 3), _lib.GROUP_PEER_COPY, k=16)
    with grp:
        for g in ings:
            m = g.memory()
            assert m["work_bytes"] == 0 and m["result_bytes"] > 0
            assert m["work_bytes_at_replicas"] == 0          # nothing of the work was held when the replicas were declared
            assert m["split_bytes"] > 0
        assert grp.local(0)[0].get_factors(X).shape[0] == ings[0].counts()["users"]
    for g in ings:
        g.close()


def test_spent_ingests_are_refused():
    """after a group finish (successful or not) an ingest holds slices or nothing: append / finish / install refuse it"""
    data = corpus(6, 200, 80, 3000)
    grp, ings = run_sharded(2, cut(data, 2, 4), _lib.GROUP_PEER_COPY, k=8)
    with grp:
        for g in ings:
            for call in (g.finish, lambda: g.append([1], [2], [1.0]), lambda: g.append_text(b"1,2,3\n"),
                         lambda: g.install_group(grp)):
                with pytest.raises(pkg.MalsError) as e:
                    call()
                assert e.value.status == _lib.INVALID_ARG
    for g in ings:
        g.close()
    # a failed group finish (a lone quote in share 1): the records are gone, a finish is refused instead of reading them
    ings = [ingest.Ingest(0) for _ in range(2)]
    with pkg.GroupALS.single_process(8, [0, 0], backend=_lib.GROUP_PEER_COPY) as grp:
        ings[0].append_text(b"1,2,3\n", True)
        ings[1].set_share(1)
        with pytest.raises(pkg.MalsError):
            ings[1].append_text(b'1,"\n', True)
        with pytest.raises(pkg.MalsError):
            grp.ingest_finish(ings)
        for g in ings:
            assert g.memory()["work_bytes"] == 0
            with pytest.raises(pkg.MalsError) as e:
                g.finish()
            assert e.value.status == _lib.INVALID_ARG
    for g in ings:
        g.close()


def test_empty_slices_and_a_share_that_stopped_on_its_own():
    # 2 users, 3 ranks: duplicate splitters, at least one empty X slice
    data = b"1,10,1\n2,11,1\n1,11,2\n2,12,1\n"
    want = to.expected([data])
    grp, ings = run_sharded(3, cut(data, 3, 1), _lib.GROUP_PEER_COPY, k=8)
    with grp:
        bx = grp.bounds(X)
        assert bx[-1] == 2 and (np.diff(bx) == 0).any()
        check_slices(grp, ings, want, whole_counters(data))
        factorize_and_check(grp, want, 8)
    for g in ings:
        g.close()
    # share 1 alone reaches 101 bad lines with lines after them: it stops parsing, every rank returns MALS_IO_ERROR
    good = b"1,2,1\n"
    assert _errors(3, [good, b"x,y,z\n" * 102 + good, good]) == _lib.IO_ERROR


def test_cut_rule_in_one_file_with_mixed_line_ends(tmp_path):
    """one small file, '\n', '\r\n' and lone '\r' mixed: every share count 1..5, lines add up and the group result is the
    one-ingest result"""
    d = tmp_path / "one"
    d.mkdir()
    data = text_corpus.corpus(11, 300, p_odd=0.0, terminators=("\n", "\r\n", "\r"))
    (d / "a.csv").write_bytes(data)
    want = to.expected([data])
    counters = whole_counters(data)
    for n in range(1, 6):
        ings = [ingest.Ingest(0) for _ in range(n)]
        with pkg.GroupALS.single_process(8, [0] * n, backend=_lib.GROUP_PEER_COPY) as grp:
            for s, g in enumerate(ings):
                g.set_option(_lib.INGEST_OPT_KNOWN_ITEMS, 1)
                g.read_dir_share(str(d), s, n)
            per = [g.text_info()["lines"] for g in ings]
            assert sum(per) == counters[0], (n, per)
            grp.ingest_finish(ings)
            check_slices(grp, ings, want, counters)
        for g in ings:
            g.close()


def test_many_tiles_equal_one_ingest():
    """10M records through the record path, 4 shares: every split has more tile x bucket counts than one scan tile holds;
    the slices equal one ingest of the same records bit for bit"""
    rng = np.random.default_rng(3)
    n = 10_000_000
    u = rng.integers(0, 200_000, n).astype(np.int64) * 5 + 7
    i = (rng.random(n) ** 3 * 50_000).astype(np.int64)
    v = rng.integers(1, 6, n).astype(np.float32)
    v[rng.random(n) < 0.01] = np.nan
    with ingest.Ingest(0) as whole:
        whole.append(u, i, v)
        whole.finish()
        ids = (whole.ids(X), whole.ids(Y))
        csr = (whole.csr(X), whole.csr(Y))
    world = 4
    cuts = np.linspace(0, n, world + 1).astype(np.int64)
    ings = [ingest.Ingest(0) for _ in range(world)]
    with pkg.GroupALS.single_process(16, [0] * world, backend=_lib.GROUP_PEER_COPY) as grp:
        for s, g in enumerate(ings):
            g.set_share(s)
            g.append(u[cuts[s]:cuts[s + 1]], i[cuts[s]:cuts[s + 1]], v[cuts[s]:cuts[s + 1]])
        grp.ingest_finish(ings)
        for k, g in enumerate(ings):
            _, rank = grp.local(k)
            assert np.array_equal(g.ids(X), ids[0]) and np.array_equal(g.ids(Y), ids[1])
            for side in (X, Y):
                b0, m = g.slice(side)
                rp, col, val = csr[side]
                srp, scol, sval = g.csr(side)
                e0, e1 = rp[b0], rp[b0 + m]
                assert np.array_equal(srp, rp[b0:b0 + m + 1] - e0)
                assert np.array_equal(scol, col[e0:e1]) and np.array_equal(sval.view(np.uint32), val[e0:e1].view(np.uint32))
            assert g.memory()["split_bytes"] > 0
        # every record was finished by exactly one rank
        assert sum(g.counts()["records"] for g in ings) == n
    for g in ings:
        g.close()


def _one_rank_share(rank, world, k, d, scenarios, uid_q, out_q):
    """one process per rank (mals_group_create_rank over the stand-in transport): every scenario on a fresh group"""
    try:
        pkg.GroupALS.use_transport(MOCK)
        res = {}
        for name, shares in scenarios:
            if rank == 0:
                uid = pkg.GroupALS.unique_id()
                for _ in range(world - 1):
                    uid_q.put(uid)
            else:
                uid = uid_q.get(timeout=120)
            with ingest.Ingest(0) as g, pkg.GroupALS.from_unique_id(k, 0, world, rank, uid, exchange_chunks=2) as grp:
                g.set_option(_lib.INGEST_OPT_KNOWN_ITEMS, 1)
                try:
                    if shares is None:
                        g.read_dir_share(d, rank, world)
                    else:
                        g.set_share(rank)
                        g.append_text(shares[rank], True)
                except pkg.MalsError:
                    pass                                    # the share still enters the collective
                try:
                    grp.ingest_finish([g])
                except pkg.MalsError as e:
                    res[name] = (e.status,)
                    continue
                if shares is not None:
                    res[name] = (_lib.OK,)
                    continue
                c = g.counts()
                Y0 = (np.random.default_rng(k).standard_normal((c["items"], k)) / np.sqrt(k)).astype(np.float32)
                slices = {side: (g.slice(side), g.csr(side)) for side in (X, Y)}
                known = g.known_items()
                ids = (g.ids(X), g.ids(Y))
                grp.set_factors(Y, Y0)
                grp.iterate(2)
                core = grp.local(0)[0]
                res[name] = (_lib.OK, slices, known, ids, grp.bounds(X).tolist(), grp.bounds(Y).tolist(),
                             core.get_factors(X), core.get_factors(Y), g.text_info()["lines"])
        out_q.put((rank, "ok", res))
    except Exception as e:  # noqa: BLE001
        import traceback
        out_q.put((rank, "error", traceback.format_exc()))


def _terminated(data, terminators):
    """the lines of a '\n'-terminated corpus with the terminators cycled"""
    lines = data.split(b"\n")[:-1]
    return b"".join(l + terminators[j % len(terminators)] for j, l in enumerate(lines))


def _factorizable_dir(path, seed):
    """_mixed_dir's layout (CRLF, lone CR, mixed, .gz, .zip, a file the byte balance cuts) with reference-shaped numeric lines
    that factorize without near-singular rows"""
    os.makedirs(path, exist_ok=True)
    files = {
        "a.csv": corpus(seed, 300, 120, 3000),
        "b.csv": _terminated(corpus(seed + 1, 300, 120, 2000, tags=False), (b"\r\n",)),
        "c.csv": _terminated(corpus(seed + 2, 300, 120, 2000, tags=False), (b"\r",)),
        "d.csv": _terminated(corpus(seed + 3, 300, 120, 12000, tags=False), (b"\n", b"\r\n", b"\r")),
    }
    for name, b in files.items():
        with open(os.path.join(path, name), "wb") as f:
            f.write(b)
    with gzip.open(os.path.join(path, "e.csv.gz"), "wb") as f:
        f.write(corpus(seed + 4, 300, 120, 2000, tags=False))
    with zipfile.ZipFile(os.path.join(path, "f.csv.zip"), "w") as z:
        z.writestr("f.csv", corpus(seed + 5, 300, 120, 500, tags=False))
    t = 1_600_000_000
    for i, name in enumerate(sorted(os.listdir(path))):
        os.utime(os.path.join(path, name), (t + i, t + i))
    return path


def test_one_process_per_rank(tmp_path):
    world, k = 3, 16
    d = _factorizable_dir(str(tmp_path / "in"), 13)
    good = b"".join(b"%d,%d,1\n" % (u, i) for u in range(5) for i in range(4))
    bad = b"x,y,z\n"
    scenarios = [("dir", None),
                 ("abort", [good + bad * 40, bad * 40 + good, bad * 21 + good]),
                 ("exact101", [good + bad * 40, bad * 40, bad * 21]),
                 ("quote", [good, good, b'1,"\n' + good])]
    ctx = mp.get_context("spawn")
    uid_q, out_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_one_rank_share, args=(r, world, k, d, scenarios, uid_q, out_q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [out_q.get(timeout=300) for _ in range(world)]
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.kill()
                p.join()
    assert all(r[1] == "ok" for r in res), [r[2] for r in res if r[1] != "ok"]
    res = [r[2] for r in sorted(res, key=lambda r: r[0])]
    assert [r["abort"][0] for r in res] == [_lib.IO_ERROR] * world
    assert [r["exact101"][0] for r in res] == [_lib.OK] * world
    assert [r["quote"][0] for r in res] == [_lib.INVALID_ARG] * world
    want = to.expected([to.file_bytes(p) for p in to.list_input_files(d)])
    (uid, rp, col, val), (iid, cp, ccol, cval) = want["csr_x"], want["csr_y"]
    Xo, Yo = None, (np.random.default_rng(k).standard_normal((len(iid), k)) / np.sqrt(k)).astype(np.float32)
    for _ in range(2):
        Xo = oracle.half_iteration(rp, col, val, Yo, threads=4)
        Yo = oracle.half_iteration(cp, ccol, cval, Xo, threads=4)
    for rank, r in enumerate(res):
        _, slices, (kp, ki), ids, bx, by, Xg, Yg, lines = r["dir"]
        assert lines == want["lines"] and bx == res[0]["dir"][4] and by == res[0]["dir"][5]
        assert np.array_equal(ids[0], uid) and np.array_equal(ids[1], iid)
        for side, (p, cc, vv), b in ((X, (rp, col, val), bx), (Y, (cp, ccol, cval), by)):
            (b0, n), (srp, scol, sval) = slices[side]
            assert (b0, n) == (b[rank], b[rank + 1] - b[rank])
            e0, e1 = p[b0], p[b0 + n]
            assert np.array_equal(srp, p[b0:b0 + n + 1] - e0) and np.array_equal(scol, cc[e0:e1])
            assert np.array_equal(sval.view(np.uint32), vv[e0:e1].view(np.uint32))
        b0, n = slices[X][0]
        k0, k1 = want["known_ptr"][b0], want["known_ptr"][b0 + n]
        assert np.array_equal(kp, want["known_ptr"][b0:b0 + n + 1] - k0) and np.array_equal(ki, want["known_idx"][k0:k1])
        assert rel(Xg, Xo) < REL_TOL and rel(Yg, Yo) < REL_TOL, (rank, rel(Xg, Xo), rel(Yg, Yo))
