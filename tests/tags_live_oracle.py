"""TEST INFRASTRUCTURE ONLY -- CPU restatement of ServerRecommender.setUserTag / setItemTag (online/src/net/myrrix/online/
ServerRecommender.java:1076-1165) and of the tag lines of ingest(Reader) (:268-298), as mals_set_user_tags,
mals_set_item_tags and mals_ingest_apply with MALS_INGEST_OPT_LIVE_TAGS serve them.  Built on tests/foldin_oracle
.update_features (the one update every write is), oracle/ingest_text_oracle.parse_line (the parser the device restates)
and the LiveModel of tests/ingest_live_oracle.py.  Not product code: only tests/ and tools/bench_ingest.py may import it.

  setUserTag(userID, tag, value): tagID = toLongID(tag); userTagIDs.add(tagID); the user's row of X and the tag's row of Y
    (zero rows if new); updateFeatures(x_user, y_tag, value).  No known item.
  setItemTag(tag, itemID, value): itemTagIDs.add(tagID); the tag's row of X, the item's row of Y;
    updateFeatures(x_tag, y_item, value).  No known item.
Both mark before the update and whatever becomes of it.

ingest, line by line: two tags on a line are a bad line (the parser's); a tag line whose value is empty (a remove) is
ignored altogether -- no row, no mark, and it stands between no two writes; any other tag line is a setItemTag (tag in
the user column) or a setUserTag (tag in the item column), and both throw for the empty tag (a tag token of two chars).
The library's documented difference stays: what throws out of ingest fails the text BEFORE anything is applied."""
import numpy as np

from oracle import ingest_text_oracle as ito
from tests import foldin_oracle as fo
from tests import ingest_live_oracle as lo

PREF, ITEM_TAG, USER_TAG = 0, 1, 2           # a record's kind: a tag in the user column is an item tag (setItemTag)
EMPTY_TAG_ID = ito.to_long_id([])


class EmptyTag(Exception):
    """checkArgument(!tag.isEmpty()) of setUserTag / setItemTag"""


def tag_id(tag):
    """tagHasher.toLongID of a str"""
    return ito.to_long_id(ito.java_utf8_decode(tag.encode("utf-8")))


def parse_text(data, first_line=1, bad_before=0, tabs=False):
    """ingest_live_oracle.parse_text with the tag lines kept: (users, items, values, kinds, lines, bad lines, header lines)"""
    if tabs:
        data = bytes(data).replace(b"\t", b",")
    users, items, values, kinds = [], [], [], []
    lines, bad, header = first_line - 1, bad_before, 0
    for line in ito.read_lines(ito.java_utf8_decode(data)):
        if bad > 100:
            raise ito.TooManyBadLines("Too many bad lines; aborting")
        lines += 1
        st, u, i, v, ut, it = ito.parse_line(line, lines)
        if st == ito.FATAL:
            raise ito.UncaughtStringIndexOutOfBounds()
        bad += st == ito.BAD
        header += st == ito.HEADER
        if st != ito.RECORD:
            continue
        if (ut and u == EMPTY_TAG_ID or it and i == EMPTY_TAG_ID) and v != ito.NAN_BITS:
            raise EmptyTag("line %d" % lines)
        users.append(u)
        items.append(i)
        values.append(v)
        kinds.append(ITEM_TAG if ut else USER_TAG if it else PREF)
    return (np.array(users, np.int64), np.array(items, np.int64), np.array(values, np.uint32).view(np.float32), np.array(kinds, np.uint8),
            lines, bad, header)


class TagModel(lo.LiveModel):
    """LiveModel + userTagIDs (rows of Y) and itemTagIDs (rows of X)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.user_tag_rows, self.item_tag_rows = set(), set()

    def set_user_tags(self, user_rows, tag_item_rows, values):
        """by ROW, as mals_set_user_tags: -> the status of every update"""
        out = []
        for u, i, v in zip(user_rows, tag_item_rows, values):
            self.user_tag_rows.add(int(i))
            out.append(int(fo.update_features(self.X, self.Y, int(u), int(i), v, self.sx, self.sy, self.rate)[0]))
        return out

    def set_item_tags(self, tag_user_rows, item_rows, values):
        out = []
        for u, i, v in zip(tag_user_rows, item_rows, values):
            self.item_tag_rows.add(int(u))
            out.append(int(fo.update_features(self.X, self.Y, int(u), int(i), v, self.sx, self.sy, self.rate)[0]))
        return out

    def grow(self, n_users, n_items):
        """mals_grow_factor_rows by hand: zero rows whose ids are their row numbers' negatives (never looked up)"""
        while len(self.X) < n_users:
            self._row(self.urow, self.user_ids, self.X, -10**9 - len(self.X))
        while len(self.Y) < n_items:
            self._row(self.irow, self.item_ids, self.Y, -10**9 - len(self.Y))

    def apply_records(self, users, items, values, kinds=None):
        """-> (stats as mals_ingest_apply's, removed user ids, status of every set, tag stats as mals_ingest_apply_tag_stats)"""
        if kinds is None:
            kinds = np.zeros(len(users), np.uint8)
        st = dict(records=len(users), sets=0, removes=0, removes_dropped=0, sets_failed=0, new_users=0, new_items=0, write_calls=0)
        tg = dict(item_tag_sets=0, user_tag_sets=0, tag_removes_ignored=0, rows_marked=0)
        marked = len(self.user_tag_rows) + len(self.item_tag_rows)
        removed, statuses, last = [], [], None
        users, items, values = np.asarray(users, np.int64), np.asarray(items, np.int64), np.asarray(values, np.float32)
        kinds = np.asarray(kinds, np.uint8)
        is_set = ~np.isnan(values)               # (a tag remove is no set either: it creates nothing)
        seen_u = set(self.urow) | set(users[is_set].tolist())
        seen_i = set(self.irow) | set(items[is_set].tolist())
        for u, i, v, kd in zip(users.tolist(), items.tolist(), values, kinds.tolist()):
            if np.isnan(v):
                if kd != PREF:
                    tg["tag_removes_ignored"] += 1    # cuts nothing: `last` stays
                    continue
                if u not in seen_u or i not in seen_i:
                    st["removes_dropped"] += 1
                    continue
                st["removes"] += 1
                st["write_calls"] += last != "remove"
                last = "remove"
                if u not in self.urow or i not in self.irow:
                    continue
                for r in fo.remove_preferences(self.X, self.known, [self.urow[u]], [self.irow[i]]):
                    self.X[r] = np.zeros(self.k, np.float32)
                    removed.append(self.user_ids[r])
                continue
            st["sets"] += 1
            st["write_calls"] += last != "set"
            last = "set"
            ur, nu = self._row(self.urow, self.user_ids, self.X, u)
            ir, ni = self._row(self.irow, self.item_ids, self.Y, i)
            st["new_users"] += nu
            st["new_items"] += ni
            if kd == PREF:
                code = int(fo.set_preferences(self.X, self.Y, self.known, [ur], [ir], [v], self.sx, self.sy, self.rate)[0])
            elif kd == USER_TAG:
                tg["user_tag_sets"] += 1
                code = self.set_user_tags([ur], [ir], [v])[0]
            else:
                tg["item_tag_sets"] += 1
                code = self.set_item_tags([ur], [ir], [v])[0]
            statuses.append(code)
            st["sets_failed"] += code != fo.OK
        tg["rows_marked"] = len(self.user_tag_rows) + len(self.item_tag_rows) - marked
        return st, removed, statuses, tg

    def apply_text(self, data, tabs=False):
        u, i, v, kd, _, _, _ = parse_text(data, tabs=tabs)
        return self.apply_records(u, i, v, kd)
