"""setUserTag / setItemTag on the device (mals_set_user_tags, mals_set_item_tags, their group twins) and the tag lines of
mals_ingest_apply with MALS_INGEST_OPT_LIVE_TAGS, against tests/tags_live_oracle.py.  Everything exact: X and Y as uint32,
the tag sets and the known items as sets, the counters as numbers."""
import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib
from myrrix_recommender_amd.core import HostSolver, MalsError
from myrrix_recommender_amd.ingest import INGEST_OPT_LIVE_TAGS, Ingest
from tests import tags_live_oracle as tlo

pytestmark = pytest.mark.gpu
X_, Y_ = pkg.SIDE_X, pkg.SIDE_Y
STAT_KEYS = Ingest.APPLY_STATS


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Model:
    """n_users x n_items: factors, three known items per user, the solvers of (M^T M + I / 10), ids = pools' heads"""

    def __init__(self, k, n_users, n_items, seed):
        rng = np.random.default_rng(seed)
        self.k, self.n_users, self.n_items = k, n_users, n_items
        self.X = (rng.standard_normal((n_users, k)) * 0.3).astype(np.float32)
        self.Y = (rng.standard_normal((n_items, k)) * 0.3).astype(np.float32)
        rows = [np.sort(rng.choice(n_items, 3, replace=False)) for _ in range(n_users)]
        self.ptr = np.arange(0, 3 * n_users + 1, 3, dtype=np.int64)
        self.col = np.concatenate(rows).astype(np.int32)
        self.known = {u: set(rows[u].tolist()) for u in range(n_users)}
        self.uid = np.array([1000 + 37 * j for j in range(n_users)], np.int64)
        self.iid = np.array([-5 + 11 * j for j in range(n_items)], np.int64)
        self.sx = HostSolver.create(self.X.astype(np.float64).T @ self.X.astype(np.float64) + np.eye(k) * 0.1)
        self.sy = HostSolver.create(self.Y.astype(np.float64).T @ self.Y.astype(np.float64) + np.eye(k) * 0.1)

    def fill(self, c):
        c.set_factor_rows(X_, self.n_users)
        c.set_factor_rows(Y_, self.n_items)
        c.set_factors(X_, self.X)
        c.set_factors(Y_, self.Y)
        c.set_matrix(X_, self.ptr, self.col, np.ones(len(self.col), np.float32))
        c.set_foldin_solver(X_, self.sx)
        c.set_foldin_solver(Y_, self.sy)
        return c

    def core(self):
        c = self.fill(pkg.ALSCore(self.k))
        c.set_known_items(self.ptr, self.col)
        c.set_ids(X_, self.uid)
        c.set_ids(Y_, self.iid)
        return c

    def oracle(self):
        return tlo.TagModel(self.X, self.Y, self.known, self.uid, self.iid, self.sx, self.sy)


MODELS = {}


def model(k, n_users=12, n_items=9, seed=1):
    key = (k, n_users, n_items, seed)
    if key not in MODELS:
        MODELS[key] = Model(*key)
    return MODELS[key]


def candidates(c, users):
    """per user, the items recommend (known items skipped) can return: everything with how_many = all items"""
    n_items = c.factor_device_ptr(Y_)[1]
    idx, _, cnt = c.recommend(users, n_items)
    return [set(idx[q, :cnt[q]].tolist()) for q in range(len(users))]


def popular_by_hand(o, how_many):
    """mostPopularItems of the oracle's model: users that are item tags are not counted, items that are user tags are struck"""
    count = np.zeros(len(o.Y), np.int64)
    for u, s in o.known.items():
        if u not in o.item_tag_rows:
            for i in s:
                count[i] += 1
    order = [i for i in np.lexsort((np.arange(len(count)), -count)) if count[i] > 0 and i not in o.user_tag_rows]
    return [int(i) for i in order[:how_many]], [float(count[i]) for i in order[:how_many]]


def check_against(c, o, skip_users=()):
    """factors, ids (if the handle has them), tag sets, known items and every reader's view of the tag rows"""
    Xo, Yo = o.arrays()
    assert np.array_equal(bits(c.get_factors(X_)), bits(Xo)) and np.array_equal(bits(c.get_factors(Y_)), bits(Yo))
    n_users, n_items = len(Xo), len(Yo)
    assert c.tag_rows(Y_).tolist() == sorted(o.user_tag_rows) and c.tag_item_count() == len(o.user_tag_rows)
    assert c.tag_rows(X_).tolist() == sorted(o.item_tag_rows) and c.tag_user_count() == len(o.item_tag_rows)
    users = [u for u in range(n_users) if u not in skip_users]
    # the known items are what they were: a tag write adds none, so the candidates are all items but the known and the tags
    for u, got in zip(users, candidates(c, users)):
        assert got == set(range(n_items)) - o.known.get(u, set()) - o.user_tag_rows, u
    tags = o.user_tag_rows
    idx, _, cnt = c.recommend(users, n_items, consider_known_items=True)
    assert all(cnt[q] == n_items - len(tags) and not (set(idx[q, :cnt[q]].tolist()) & tags) for q in range(len(users)))
    idx, _, cnt = c.most_similar_items(list(range(min(n_items, 6))), n_items)
    assert all(cnt[q] > 0 and not (set(idx[q, :cnt[q]].tolist()) & tags) for q in range(len(cnt)))
    idx, sc, cnt = c.most_popular_items(n_items)
    want_i, want_s = popular_by_hand(o, n_items)
    assert idx[:cnt].tolist() == want_i and sc[:cnt].tolist() == want_s


# ---- 1. the direct calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 64])
def test_a_batch_of_130_user_tags_then_item_tags(k):
    m = model(k, 140, 150, seed=3)
    n_tags = 130
    with m.fill(pkg.ALSCore(k)) as c:
        c.set_known_items(m.ptr, m.col)
        o = m.oracle()
        # user 100's row is not finite: its estimate is not, its update fails before anything changes -- the mark stays
        bad = m.X[100].copy()
        bad[0] = np.nan
        c.set_factors(X_, bad[None, :], row_begin=100)
        o.X[100] = bad.copy()
        c.grow_factor_rows(Y_, 150 + n_tags)
        o.grow(140, 150 + n_tags)
        c.set_preferences([5, 6], [7, 7], [2.0, 1.0])                  # item 7 is an ordinary item, written as one ...
        assert o.apply_records(m.uid[[5, 6]], m.iid[[7, 7]], [2.0, 1.0])[0]["sets_failed"] == 0
        rng = np.random.default_rng(k)
        users = np.arange(n_tags)
        rows = 150 + np.arange(n_tags)                                 # one new tag per update: level 1 fills two workgroups ...
        rows[[0, 20, 40, 60, 80]] = 150                                # ... but one tag hit 5 times: 5 levels
        rows[[10, 11]] = 7                                             # ... and the tag whose row is item 7's
        rows[[30, 31]] = 160                                           # (a repeat the count must not see twice)
        values = rng.choice(np.array([1.0, 2.0, 0.5, -1.0, 3.0], np.float32), n_tags)
        values[50] = np.nan                                            # weight 0: the mark alone
        before = c.foldin_stats()
        st = c.set_user_tags(users, rows, values, raise_on_error=False)
        want = o.set_user_tags(users, rows, values)
        assert st.tolist() == want and st[100] == _lib.INVALID_ARG and (st != 0).sum() == 1
        after = c.foldin_stats()
        assert after["levels"] - before["levels"] == 5 and after["failed"] - before["failed"] == 1
        assert o.user_tag_rows == set(rows.tolist()) and len(o.user_tag_rows) == n_tags - 4 - 1 - 1 and 150 + 100 in o.user_tag_rows
        check_against(c, o, skip_users={100})
        # with an X^T X solver alone every update whose weight is not 0 fails (the item branch reads a null userFoldIn): the mark stays
        c.set_foldin_solver(Y_, None)
        o.sy = None
        st = c.set_user_tags([1, 2], [9, 9], [1.0, 2.0], raise_on_error=False)
        assert st.tolist() == o.set_user_tags([1, 2], [9, 9], [1.0, 2.0]) == [_lib.INVALID_ARG] * 2 and 9 in o.user_tag_rows
        with pytest.raises(MalsError):
            c.set_user_tags([1], [9], [1.0])
        check_against(c, o, skip_users={100})
        c.set_foldin_solver(Y_, m.sy)
        o.sy = m.sy
        # setItemTag: 130 updates again; the tags are new rows of X, one of them hit 5 times, and one is an ordinary user (3)
        c.grow_factor_rows(X_, 140 + n_tags)
        o.grow(140 + n_tags, 150 + n_tags)
        trows = 140 + np.arange(n_tags)
        trows[[1, 21, 41, 61, 81]] = 140
        trows[[12, 13]] = 3
        items = rng.integers(0, 150, n_tags)
        items[100] = 150 + 100
        values = rng.choice(np.array([1.0, 2.0, 0.5, -1.0], np.float32), n_tags)
        values[7] = np.nan
        st = c.set_item_tags(trows, items, values)
        assert st.tolist() == o.set_item_tags(trows, items, values) == [0] * n_tags
        assert o.item_tag_rows == set(trows.tolist()) and len(o.item_tag_rows) == n_tags - 5 - 1 and 3 in o.item_tag_rows
        check_against(c, o, skip_users={100})
        assert set(c.get_recent(Y_).tolist()) >= o.user_tag_rows and set(c.get_recent(X_).tolist()) >= o.item_tag_rows


def test_the_edges_of_the_mask():
    """63 rows of Y and no mask; row 64 after a grow lies in a new word and, past the even-word rounding, in a new pair;
    rows 31 and 32 are neighbours in two words"""
    m = model(8, 12, 63, seed=5)
    with m.fill(pkg.ALSCore(8)) as c:
        c.set_known_items(m.ptr, m.col)
        o = m.oracle()
        assert c.tag_item_count() == 0 and len(c.tag_rows(Y_)) == 0
        steps = [([0], [62], [1.0]), None, ([1], [64], [2.0]), ([2, 3, 2], [31, 32, 31], [1.0, 1.0, 0.5])]
        for step in steps:
            if step is None:
                c.grow_factor_rows(Y_, 65)
                o.grow(12, 65)
            else:
                assert c.set_user_tags(*step).tolist() == o.set_user_tags(*step)
            check_against(c, o)
        assert c.tag_rows(Y_).tolist() == [31, 32, 62, 64]
        # a bad row is refused whole
        with pytest.raises(MalsError):
            c.set_user_tags([0], [65], [1.0])
        with pytest.raises(MalsError):
            c.set_item_tags([12], [0], [1.0])
        check_against(c, o)


# ---- 2. tag lines in apply ----------------------------------------------------------------------------------------------
TAG_WORDS = ["rock", "jazz", "é", "\U0001F3B8x", "pop", "a b", "k" * 70]
USER_POOL = np.array([1000 + 37 * j for j in range(30)], np.int64)
ITEM_POOL = np.array([-5 + 11 * j for j in range(20)], np.int64)


def tagged_stream(seed):
    """about 200 lines: sets and removes of 30 users x 20 items (the model knows 12 x 9), a fifth tag lines of both kinds,
    some of them removes; rock's and jazz's hashes also stand as plain numbers in the column their tags stand in"""
    rng = np.random.default_rng(seed)
    rock, jazz = tlo.tag_id("rock"), tlo.tag_id("jazz")
    L = ["%d,%d,2" % (USER_POOL[1], rock),                    # the item whose id is rock's hash: an ordinary item, until ...
         '%d,"rock",1.5' % USER_POOL[2],                      # ... the same run tags its row
         "%d,%d,1" % (jazz, ITEM_POOL[3]),                    # likewise a user whose id is jazz's hash
         '"jazz",%d,0.5' % ITEM_POOL[3],
         "%d,%d,1" % (USER_POOL[4], ITEM_POOL[1]),
         '"never set",%d,' % ITEM_POOL[1],                    # a tag remove between two sets of one run: creates nothing, cuts nothing
         "%d,%d,3" % (USER_POOL[4], ITEM_POOL[2]),
         '"rock","jazz",1',                                   # two tags: a bad line
         '%d,"pop",' % USER_POOL[0]]                          # a tag remove of a tag that is set later
    pairs = []
    while len(L) < 200:
        u, i = int(rng.choice(USER_POOL)), int(rng.choice(ITEM_POOL))
        r = rng.random()
        tag = TAG_WORDS[int(rng.integers(len(TAG_WORDS)))]
        if r < 0.08:
            L.append('"%s",%d,%s' % (tag, i, rng.choice(["1", "2.5", "-1", ""])))
        elif r < 0.2:
            L.append('%d,"%s"%s' % (u, tag, rng.choice([",1", ",0.5", ",-2", ",", ""])))
        elif r < 0.4:
            if pairs and rng.random() < 0.7:
                u, i = pairs[int(rng.integers(len(pairs)))]
            L.append("%d,%d," % (u, i))
        else:
            pairs.append((u, i))
            L.append("%d,%d,%s" % (u, i, rng.choice(["1", "2.0", "0.5", "-1", "3.5"])))
    return ("\n".join(L) + "\n").encode()


def check_live(c, o):
    check_against(c, o)
    assert np.array_equal(c.ids_of(X_), o.user_ids) and np.array_equal(c.ids_of(Y_), o.item_ids)


@pytest.mark.parametrize("k", [8, 64])
def test_a_stream_with_tag_lines_whole_and_in_three_pieces(k):
    m = model(k)
    text = tagged_stream(k)
    users, items, values, kinds, lines, bad, _ = tlo.parse_text(text)
    o = m.oracle()
    st_o, removed_o, _, tg_o = o.apply_text(text)
    assert lines == 200 and bad == 1 and st_o["removes"] > 10 and st_o["new_users"] > 10 and st_o["new_items"] > 10
    assert tg_o["item_tag_sets"] > 5 and tg_o["user_tag_sets"] > 10 and tg_o["tag_removes_ignored"] > 5 and tg_o["rows_marked"] >= 8
    assert o.irow[tlo.tag_id("rock")] in o.user_tag_rows and o.urow[tlo.tag_id("jazz")] in o.item_tag_rows
    assert tlo.tag_id("never set") not in o.urow and st_o["write_calls"] < st_o["sets"]
    with m.core() as whole, m.core() as pieces:
        with Ingest() as g:
            g.set_option(INGEST_OPT_LIVE_TAGS, 1)
            g.append_text(text)
            st, removed = g.apply(whole)
        assert {key: st[key] for key in STAT_KEYS} == st_o and removed.tolist() == removed_o
        assert whole.ingest_apply_tag_stats() == tg_o
        check_live(whole, o)
        # three pieces, the first cut inside a tag token, an apply after each
        cut1 = text.index(b'"jazz"') + 3
        cuts = [0, cut1, text.index(b"\n", len(text) // 2) + 4, len(text)]
        op, at = m.oracle(), 0
        with Ingest() as g:
            g.set_option(INGEST_OPT_LIVE_TAGS, 1)
            for a, b in zip(cuts[:-1], cuts[1:]):
                g.append_text(text[a:b], end_of_file=(b == len(text)))
                st, removed = g.apply(pieces)
                n = st["records"]
                st_p, rem_p, _, tg_p = op.apply_records(users[at:at + n], items[at:at + n], values[at:at + n], kinds[at:at + n])
                assert {key: st[key] for key in STAT_KEYS} == st_p and removed.tolist() == rem_p and pieces.ingest_apply_tag_stats() == tg_p
                at += n
            assert at == len(users) and g.text_info()["lines"] == 200
        check_live(pieces, o)
        for side in (X_, Y_):
            assert whole.factor_digest(side) == pieces.factor_digest(side)


def test_a_set_of_the_empty_tag_fails_the_text_and_its_remove_is_ignored():
    m = model(8)
    u, i = m.uid.tolist(), m.iid.tolist()
    head = "%d,%d,1\n%d,%d,2\n" % (u[0], i[0], u[1], i[1])
    with m.core() as c:
        before = (c.factor_digest(X_), c.factor_digest(Y_))
        for tok in ('"é', '""', '"a'):
            with Ingest() as g:
                g.set_option(INGEST_OPT_LIVE_TAGS, 1)
                g.append_text(head.encode())
                with pytest.raises(MalsError, match="line 3.*empty tag"):
                    g.append_text(("%s,%d,1\n%d,%d,1\n" % (tok, i[2], u[2], i[2])).encode())
                with pytest.raises(MalsError, match="text has failed"):
                    g.apply(c)
                assert g.counts_records() == 2 and (c.factor_digest(X_), c.factor_digest(Y_)) == before
                assert c.factor_device_ptr(X_)[1] == 12 and len(c.tag_rows(X_)) == 0
        # the same with an empty value: a tag remove, ignored
        text = (head + '"é,%d,\n%d,%d,1\n' % (i[2], u[2], i[2])).encode()
        o = m.oracle()
        st_o, _, _, tg_o = o.apply_text(text)
        with Ingest() as g:
            g.set_option(INGEST_OPT_LIVE_TAGS, 1)
            g.append_text(text)
            st, _ = g.apply(c)
        assert {key: st[key] for key in STAT_KEYS} == st_o and st["records"] == 4 and st["sets"] == 3 and st["write_calls"] == 1
        assert c.ingest_apply_tag_stats() == tg_o == dict(item_tag_sets=0, user_tag_sets=0, tag_removes_ignored=1, rows_marked=0)
        check_live(c, o)
        # the option is chosen before the first append
        with Ingest() as g:
            g.append_text(head.encode())
            with pytest.raises(MalsError, match="before the first"):
                g.set_option(INGEST_OPT_LIVE_TAGS, 1)


# ---- 3. a group ----------------------------------------------------------------------------------------------------------
def test_the_group_calls_leave_every_member_what_one_handle_holds():
    m = model(8, 40, 30, seed=7)
    rng = np.random.default_rng(11)
    with pkg.GroupALS.single_process(8, [0, 0], backend=_lib.GROUP_PEER_COPY) as g, m.fill(pkg.ALSCore(8)) as one:
        m.fill(g)
        o = m.oracle()
        for w in (g, one):
            w.grow_factor_rows(X_, 44)
            w.grow_factor_rows(Y_, 36)
        o.grow(44, 36)
        ut = (rng.integers(0, 40, 20), np.concatenate([30 + rng.integers(0, 6, 18), [4, 4]]), rng.choice(np.array([1.0, 2.0, -1.0], np.float32), 20))
        it = (np.concatenate([40 + rng.integers(0, 4, 10), [2, 25]]), rng.integers(0, 30, 12), rng.choice(np.array([1.0, 0.5], np.float32), 12))
        for w in (g, one):
            assert w.set_user_tags(*ut).tolist() == [0] * 20 and w.set_item_tags(*it).tolist() == [0] * 12
        o.set_user_tags(*ut)
        o.set_item_tags(*it)
        Xo, Yo = o.arrays()
        bounds = g.bounds(X_)
        for side, M in ((X_, Xo), (Y_, Yo)):
            d, eq = g.replica_digest(side)
            assert eq and len(d) == 2 and int(d[0]) == one.factor_digest(side) == pkg.factor_digest_host(M)
        owned = []
        for r in range(2):
            member, _ = g.local(r)
            assert np.array_equal(bits(member.get_factors(X_)), bits(Xo)) and np.array_equal(bits(member.get_factors(Y_)), bits(Yo))
            assert member.tag_rows(Y_).tolist() == sorted(o.user_tag_rows) == one.tag_rows(Y_).tolist()
            owned += member.tag_rows(X_).tolist()
        # every tag user with its owner: user 2 in the first slice, user 25 and the grown rows with the last rank
        assert owned == sorted(o.item_tag_rows) == one.tag_rows(X_).tolist() and 2 < bounds[1] <= 25
        users = np.arange(40)
        idx, _, cnt = g.recommend(users, 36)
        for q in users:
            assert set(idx[q, :cnt[q]].tolist()) == set(range(36)) - o.known[q] - o.user_tag_rows
        want_i, want_s = popular_by_hand(o, 36)
        for w in (g, one):
            idx, sc, cnt = w.most_popular_items(36)
            assert idx[:cnt].tolist() == want_i and sc[:cnt].tolist() == want_s
        with pytest.raises(MalsError, match="group"):
            g.local(0)[0].set_user_tags([0], [0], [1.0])


# ---- 4. a generation load keeps the tag row and its mark ---------------------------------------------------------------
def test_a_load_after_a_tag_write_keeps_the_vector_and_the_mark():
    m = model(8)
    with m.core() as c:
        o = m.oracle()
        rock, new = tlo.tag_id("rock"), tlo.tag_id("new")
        (ir,), _ = c.rows_of(Y_, [rock], add=True)
        (ur,), _ = c.rows_of(X_, [new], add=True)
        o.apply_records([m.uid[0], new], [rock, m.iid[1]], [2.0, 1.0], [tlo.USER_TAG, tlo.ITEM_TAG])
        assert c.set_user_tags([0], [ir], [2.0]).tolist() == [0] and c.set_item_tags([ur], [1], [1.0]).tolist() == [0]
        check_live(c, o)
        y_rock, x_new = c.get_factors(Y_)[ir].copy(), c.get_factors(X_)[ur].copy()
        assert y_rock.any() and x_new.any()
        # a new model that knows neither tag: users 0..9 and items 0..7 of the old one, two new of each
        rng = np.random.default_rng(4)
        nu = np.concatenate([m.uid[:10], [5, 6]]).astype(np.int64)
        ni = np.concatenate([m.iid[:8], [7, 8]]).astype(np.int64)
        nX = (rng.standard_normal((12, 8)) * 0.3).astype(np.float32)
        nY = (rng.standard_normal((10, 8)) * 0.3).astype(np.float32)
        known = (np.arange(0, 13, dtype=np.int64), np.arange(12, dtype=np.int32) % 10)
        _, (uids, iids), (umap, imap) = c.load_generation(c.ids_of(X_), c.ids_of(Y_), nu, ni, nX, nY, new_known=known)
        assert imap[ir] >= 0 and umap[ur] >= 0 and iids[imap[ir]] == rock and uids[umap[ur]] == new
        assert np.array_equal(bits(c.get_factors(Y_)[imap[ir]]), bits(y_rock)) and np.array_equal(bits(c.get_factors(X_)[umap[ur]]), bits(x_new))
        assert c.tag_rows(Y_).tolist() == [imap[ir]] and c.tag_rows(X_).tolist() == [umap[ur]] and c.tag_item_count() == 1
        idx, _, cnt = c.recommend(np.arange(len(uids)), len(iids), consider_known_items=True)
        assert all(imap[ir] not in idx[q, :cnt[q]].tolist() for q in range(len(uids)))
