"""TEST INFRASTRUCTURE ONLY -- CPU restatement of ServerRecommender.ingest(Reader) (online/src/net/myrrix/online/
ServerRecommender.java:204-309) as mals_ingest_apply serves it: lines and tokens from oracle/ingest_text_oracle.py (the
parser the device restates), setPreference / removePreference from tests/foldin_oracle.py, and a plain dict as the id
directory.  Not product code: only tests/ and tools/bench_ingest.py may import it.

One line at a time, as the reference does it (:268-298):
  * a line whose value token is empty is a remove, any other record a set;
  * a set looks its user and its item up and gives an unknown id the next row (getFeatures :838-863: a zero vector), so new
    rows are numbered in the order their ids first appear among the SETS of the stream;
  * a remove of a user or an item without a row does nothing (:1033-1042) and creates no row (whether the library counts it
    as dropped or as passed on depends on the sets of the same call, see apply_records; the model is the same);
  * a user that a remove empties keeps its id and its zeroed row; a later set finds that row.
What the library does not serve is an exception here: a tag in either column (NotServed), more than 100 bad lines and a
lone-quote token (the text oracle's exceptions) -- raised BEFORE anything is applied, which is the library's documented
difference from the reference."""
import numpy as np

from oracle import ingest_text_oracle as ito
from tests import foldin_oracle as fo


class NotServed(Exception):
    pass


def parse_text(data, first_line=1, bad_before=0, tabs=False):
    """The records of a text (bytes), in line order: (users, items, values float32 with NaN = remove, lines, bad lines,
    header lines).  Raises like the library refuses.  tabs: ServerRecommender.ingest's splitter (DELIMITER, :95: commas and
    tabs) in place of the input-file reader's (commas): with every tab read as a comma the two split alike."""
    if tabs:
        data = bytes(data).replace(b"\t", b",")
    users, items, values = [], [], []
    lines, bad, header = first_line - 1, bad_before, 0
    for line in ito.read_lines(ito.java_utf8_decode(data)):
        if bad > 100:
            raise ito.TooManyBadLines("Too many bad lines; aborting")
        lines += 1
        st, u, i, v, ut, it = ito.parse_line(line, lines)
        if st == ito.FATAL:
            raise ito.UncaughtStringIndexOutOfBounds()
        if st == ito.BAD:
            bad += 1
        if st == ito.HEADER:
            header += 1
        if st != ito.RECORD:
            continue
        if ut or it:
            raise NotServed("tag line %d" % lines)
        users.append(u)
        items.append(i)
        values.append(v)
    return (np.array(users, np.int64), np.array(items, np.int64), np.array(values, np.uint32).view(np.float32), lines, bad, header)


class LiveModel:
    """X, Y (float32), known items by user ROW, the two directories."""

    def __init__(self, X, Y, known, user_ids, item_ids, sx=None, sy=None, rate=1.0):
        self.X = [np.array(r, np.float32) for r in X]
        self.Y = [np.array(r, np.float32) for r in Y]
        self.k = np.asarray(X).shape[1]
        self.known = {int(u): set(int(i) for i in s) for u, s in known.items()}
        self.user_ids = [int(x) for x in user_ids]
        self.item_ids = [int(x) for x in item_ids]
        self.urow = {x: r for r, x in enumerate(self.user_ids)}
        self.irow = {x: r for r, x in enumerate(self.item_ids)}
        assert len(self.urow) == len(self.X) and len(self.irow) == len(self.Y)
        self.sx, self.sy, self.rate = sx, sy, rate

    def _row(self, table, ids, F, key):
        r = table.get(key)
        if r is None:
            r = table[key] = len(ids)
            ids.append(key)
            F.append(np.zeros(self.k, np.float32))
            return r, 1
        return r, 0

    def apply_records(self, users, items, values):
        """-> (stats dict as mals_ingest_apply's, removed user ids, status of every set)"""
        st = dict(records=len(users), sets=0, removes=0, removes_dropped=0, sets_failed=0, new_users=0, new_items=0, write_calls=0)
        removed, statuses, last = [], [], None
        users, items, values = np.asarray(users, np.int64), np.asarray(items, np.int64), np.asarray(values, np.float32)
        # the library resolves the ids of ALL the sets of a call before it looks the removes' ids up: a remove whose id only a
        # LATER set of the same call creates is passed on (and then finds nothing to remove: the same model) instead of dropped
        is_set = ~np.isnan(values)
        seen_u = set(self.urow) | set(users[is_set].tolist())
        seen_i = set(self.irow) | set(items[is_set].tolist())
        for u, i, v in zip(users.tolist(), items.tolist(), values):
            if np.isnan(v):
                if u not in seen_u or i not in seen_i:
                    st["removes_dropped"] += 1
                    continue
                st["removes"] += 1
                st["write_calls"] += last != "remove"
                last = "remove"
                if u not in self.urow or i not in self.irow:
                    continue
                for r in fo.remove_preferences(self.X, self.known, [self.urow[u]], [self.irow[i]]):
                    self.X[r] = np.zeros(self.k, np.float32)   # (the oracle's X[r] = 0.0 replaced the list's element)
                    removed.append(self.user_ids[r])
                continue
            st["sets"] += 1
            st["write_calls"] += last != "set"
            last = "set"
            ur, nu = self._row(self.urow, self.user_ids, self.X, u)
            ir, ni = self._row(self.irow, self.item_ids, self.Y, i)
            st["new_users"] += nu
            st["new_items"] += ni
            code = int(fo.set_preferences(self.X, self.Y, self.known, [ur], [ir], [v], self.sx, self.sy, self.rate)[0])
            statuses.append(code)
            st["sets_failed"] += code != fo.OK
        return st, removed, statuses

    def apply_text(self, data, tabs=False):
        u, i, v, _, _, _ = parse_text(data, tabs=tabs)
        return self.apply_records(u, i, v)

    def arrays(self):
        return np.array(self.X, np.float32).reshape(len(self.X), self.k), np.array(self.Y, np.float32).reshape(len(self.Y), self.k)
