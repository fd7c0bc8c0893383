"""ctypes binding of the mals_group_* entry points: the multi-GPU half-iteration below the C-ABI
(csrc/mals_group.cpp).  Two constructors:

  GroupALS.single_process(features, devices, ...)   one process drives all GPUs (ncclCommInitAll, or
                                                    peer copies with backend=GROUP_PEER_COPY)
  GroupALS.from_torch_distributed(features, ...)    one process per GPU: the RCCL unique id is broadcast
                                                    with torch.distributed (plumbing: rendezvous only);
                                                    every collective afterwards is the library's own

Every method is a single C-ABI call; in multi-process groups the calls are collective.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import MEM_DEVICE, MEM_HOST, SIDE_X, SIDE_Y
from .core import ALSCore, Cancelled, MalsError, SingularSystem, _host, _item_queries, _load_generation


def generation_plan_host(world, features, new_known_ptr, kept_sizes, kept_rows, old_bounds, n_new=None):
    """mals_group_generation_plan_host: who owns which merged user after GroupALS.load_generation.  new_known_ptr: n_new + 1
    offsets or None (then n_new says how many new users); kept_rows: the kept users' live rows, ascending; kept_sizes:
    their set sizes; old_bounds: world + 1 or None.  Returns (bounds[world + 1], moves[world][world][2]): moves[m][j] = the run
    of old member m's own kept list that new member j gets.  Host only."""
    L = _lib.load()
    rp = np.ascontiguousarray(new_known_ptr, dtype=np.int64) if new_known_ptr is not None else None
    n_new = len(rp) - 1 if rp is not None else int(n_new or 0)
    ks = np.ascontiguousarray(kept_sizes, dtype=np.int64)
    kr = np.ascontiguousarray(kept_rows, dtype=np.int64)
    ob = np.ascontiguousarray(old_bounds, dtype=np.int64) if old_bounds is not None else None
    assert len(ks) == len(kr) and (ob is None or len(ob) == world + 1)
    bounds = np.zeros(world + 1, dtype=np.int64)
    moves = np.zeros((world, world, 2), dtype=np.int64)
    rc = L.mals_group_generation_plan_host(int(world), int(features), n_new, rp.ctypes.data_as(ctypes.c_void_p) if rp is not None else None,
                                           len(ks), ks.ctypes.data_as(ctypes.c_void_p) if len(ks) else None,
                                           kr.ctypes.data_as(ctypes.c_void_p) if len(kr) else None,
                                           ob.ctypes.data_as(ctypes.c_void_p) if ob is not None else None,
                                           bounds.ctypes.data_as(ctypes.c_void_p), moves.ctypes.data_as(ctypes.c_void_p))
    if rc != _lib.OK:
        raise MalsError(rc, "mals_group_generation_plan_host")
    return bounds, moves


def plan_shards(row_ptr, world, features, row_cost=-1.0):
    """mals_plan_shards: contiguous slices of equal cost (entries + row_cost per row).  Host only."""
    L = _lib.load()
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    out = np.zeros(world + 1, dtype=np.int64)
    rc = L.mals_plan_shards(rp.ctypes.data_as(ctypes.c_void_p), len(rp) - 1, int(world), float(row_cost), int(features),
                            out.ctypes.data_as(ctypes.c_void_p))
    if rc != _lib.OK:
        raise MalsError(rc, "mals_plan_shards")
    return out


class _MemberCore(ALSCore):
    """ALSCore view of a group member's handle (owned by the group: never destroyed here)."""

    def __init__(self, L, handle, features):   # noqa: D107 -- no mals_create
        self._L = L
        self._h = handle
        self._keep = {}
        self.features = features
        self.chunk_rows = 0

    def close(self):
        self._h = ctypes.c_void_p()

    def __del__(self):
        pass


class GroupALS:
    def __init__(self, features, handle, world):
        self._L = _lib.load()
        self._g = handle
        self.features = int(features)
        self.world = int(world)
        self._keep = {}

    @staticmethod
    def _config(L, features, alpha, lam, flags, device, segment_nnz, singularity_threshold, gramian_mode, solve_mode):
        cfg = _lib.Config()
        L.mals_default_config(ctypes.byref(cfg))
        cfg.features, cfg.alpha, cfg.lam, cfg.flags = int(features), float(alpha), float(lam), int(flags)
        cfg.device, cfg.segment_nnz = int(device), int(segment_nnz)
        cfg.singularity_threshold = float(singularity_threshold)
        cfg.gramian_mode, cfg.solve_mode = int(gramian_mode), int(solve_mode)
        return cfg

    @classmethod
    def single_process(cls, features, devices, backend=_lib.GROUP_RCCL, alpha=1.0, lam=0.1, flags=0, segment_nnz=0,
                       singularity_threshold=1e-5, gramian_mode=0, solve_mode=0, exchange_chunks=4):
        L = _lib.load()
        cfg = cls._config(L, features, alpha, lam, flags, devices[0], segment_nnz, singularity_threshold, gramian_mode, solve_mode)
        devs = (ctypes.c_int32 * len(devices))(*devices)
        g = ctypes.c_void_p()
        rc = L.mals_group_create(ctypes.byref(cfg), devs, len(devices), int(backend), ctypes.byref(g))
        if rc != _lib.OK:
            raise MalsError(rc, "mals_group_create failed (devices %s): %s" % (list(devices), _lib.create_error()))
        self = cls(features, g, len(devices))
        self._chk(L.mals_group_set_exchange_chunks(g, int(exchange_chunks)))
        return self

    def set_alternate_streams(self, on):
        """mals_group_set_alternate_streams: consecutive chunks of a half-iteration on two alternating compute streams
        (default on) or on one (A/B)."""
        self._chk(self._L.mals_group_set_alternate_streams(self._g, 1 if on else 0))

    @staticmethod
    def use_transport(library_path):
        """mals_group_use_transport: the shared library to load as RCCL (None = librccl.so.1), once per process and
        before the first group / unique id.  The tests point it at their stand-in transport."""
        L = _lib.load()
        rc = L.mals_group_use_transport(library_path.encode() if library_path else None)
        if rc != _lib.OK:
            raise MalsError(rc, "mals_group_use_transport: a transport is already loaded in this process")

    def comm_info(self, i=0):
        """What the communicator reports for local member i: {"comm_size", "comm_rank", "hip_device", "pci_bus_id"}."""
        n, r, d = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        buf = ctypes.create_string_buffer(32)
        self._chk(self._L.mals_group_comm_info(self._g, int(i), ctypes.byref(n), ctypes.byref(r), ctypes.byref(d), buf, 32))
        return {"comm_size": n.value, "comm_rank": r.value, "hip_device": d.value, "pci_bus_id": buf.value.decode("ascii", "replace")}

    @staticmethod
    def unique_id():
        """mals_group_unique_id: the 128-byte RCCL unique id rank 0 creates and hands to the other ranks."""
        L = _lib.load()
        buf = (ctypes.c_uint8 * 128)()
        rc = L.mals_group_unique_id(buf)
        if rc != _lib.OK:
            raise MalsError(rc, "mals_group_unique_id failed (is librccl.so.1 loadable?)")
        return bytes(buf)

    @classmethod
    def from_unique_id(cls, features, device, world, rank, uid, alpha=1.0, lam=0.1, flags=0, segment_nnz=0,
                       singularity_threshold=1e-5, gramian_mode=0, solve_mode=0, exchange_chunks=4):
        """One rank per process (mals_group_create_rank); `uid` = unique_id() of rank 0, carried by whatever
        the application has (MPI, a socket, torch.distributed); None with world == 1 = no communicator at all."""
        L = _lib.load()
        cfg = cls._config(L, features, alpha, lam, flags, device, segment_nnz, singularity_threshold, gramian_mode, solve_mode)
        buf = (ctypes.c_uint8 * 128)(*uid) if uid is not None else None
        g = ctypes.c_void_p()
        rc = L.mals_group_create_rank(ctypes.byref(cfg), int(world), int(rank), buf, ctypes.byref(g))
        if rc != _lib.OK:
            raise MalsError(rc, "mals_group_create_rank failed (rank %d of %d): %s" % (rank, world, _lib.create_error()))
        self = cls(features, g, world)
        self._chk(L.mals_group_set_exchange_chunks(g, int(exchange_chunks)))
        return self

    @classmethod
    def from_torch_distributed(cls, features, device, alpha=1.0, lam=0.1, flags=0, segment_nnz=0, singularity_threshold=1e-5,
                               gramian_mode=0, solve_mode=0, exchange_chunks=4, world=None, rank=None, one_rank_communicator=False):
        """One rank per process.  torch.distributed (already initialised unless world == 1) only carries
        the 128-byte RCCL unique id from rank 0 to the others."""
        if world is None:
            import torch.distributed as dist
            world, rank = dist.get_world_size(), dist.get_rank()
        uid = None
        if world > 1 or one_rank_communicator:
            uid = cls.unique_id() if rank == 0 else bytes(128)
            if world > 1:
                import torch
                import torch.distributed as dist
                # a CPU tensor under gloo (single-device test runs), a device tensor under RCCL
                dev = torch.device("cuda", device) if dist.get_backend() == "nccl" else torch.device("cpu")
                t = torch.tensor(list(uid), dtype=torch.uint8, device=dev)
                dist.broadcast(t, 0)
                uid = bytes(t.cpu().tolist())
        return cls.from_unique_id(features, device, world, rank, uid, alpha=alpha, lam=lam, flags=flags, segment_nnz=segment_nnz,
                                  singularity_threshold=singularity_threshold, gramian_mode=gramian_mode, solve_mode=solve_mode,
                                  exchange_chunks=exchange_chunks)

    # -- lifecycle --------------------------------------------------------------------------------
    def close(self):
        if self._g is not None and self._g.value:
            self._L.mals_group_destroy(self._g)
            self._g = ctypes.c_void_p()
            self._keep.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc == _lib.OK:
            return
        msg = (self._L.mals_group_last_error(self._g) or b"").decode("utf-8", "replace")
        if rc == _lib.SINGULAR:
            side, row, rank = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
            self._L.mals_group_singular_info(self._g, ctypes.byref(side), ctypes.byref(row), ctypes.byref(rank))
            raise SingularSystem(rc, msg, side.value, row.value, rank.value)
        if rc == _lib.CANCELLED:
            raise Cancelled(rc, msg)
        raise MalsError(rc, msg)

    def set_refine_limit(self, limit):
        """mals_group_set_refine_limit: see mals_set_refine_limit (every local member)."""
        self._chk(self._L.mals_group_set_refine_limit(self._g, float(limit)))

    def local(self, i=0):
        """(ALSCore view, rank) of local member i -- stats, top-N, reconstruction error per GPU."""
        h, r = ctypes.c_void_p(), ctypes.c_int32()
        self._chk(self._L.mals_group_local(self._g, int(i), ctypes.byref(h), ctypes.byref(r)))
        return _MemberCore(self._L, h, self.features), r.value

    # -- data -------------------------------------------------------------------------------------
    def set_factor_rows(self, side, n_rows_total):
        self._chk(self._L.mals_group_set_factor_rows(self._g, side, int(n_rows_total)))

    def set_factors(self, side, rows, row_begin=0):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        self._chk(self._L.mals_group_set_factors(self._g, side, int(row_begin), rows.shape[0], rows.ctypes.data_as(ctypes.c_void_p)))

    def get_factors(self, side, row_begin, n_rows):
        out = np.empty((n_rows, self.features), dtype=np.float32)
        self._chk(self._L.mals_group_get_factors(self._g, side, int(row_begin), int(n_rows), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def set_matrix(self, side, row_ptr, col_idx, val):
        """The FULL matrix of a side (numpy arrays, or torch CUDA tensors of this process's device)."""
        if type(row_ptr).__module__.startswith("torch"):
            row_ptr, col_idx, val = row_ptr.contiguous(), col_idx.contiguous(), val.contiguous()
            self._keep[("M", side)] = (row_ptr, col_idx, val)
            self._chk(self._L.mals_group_set_matrix(self._g, side, int(row_ptr.shape[0]) - 1, int(col_idx.shape[0]),
                                                    ctypes.c_void_p(row_ptr.data_ptr()), ctypes.c_void_p(col_idx.data_ptr()),
                                                    ctypes.c_void_p(val.data_ptr()), MEM_DEVICE))
        else:
            rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
            c = np.ascontiguousarray(col_idx, dtype=np.int32)
            v = np.ascontiguousarray(val, dtype=np.float32)
            self._chk(self._L.mals_group_set_matrix(self._g, side, len(rp) - 1, len(c), rp.ctypes.data_as(ctypes.c_void_p),
                                                    c.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p), MEM_HOST))

    def set_matrix_chunked(self, side, row_ptr, col_idx, val, rows_per_piece):
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        c = np.ascontiguousarray(col_idx, dtype=np.int32)
        v = np.ascontiguousarray(val, dtype=np.float32)
        n = len(rp) - 1
        self._chk(self._L.mals_group_begin_matrix(self._g, side, n, rp.ctypes.data_as(ctypes.c_void_p)))
        for r0 in range(0, n, rows_per_piece):
            r1 = min(n, r0 + rows_per_piece)
            cc = np.ascontiguousarray(c[rp[r0]:rp[r1]])
            vv = np.ascontiguousarray(v[rp[r0]:rp[r1]])
            self._chk(self._L.mals_group_append_rows(self._g, side, r1 - r0, cc.ctypes.data_as(ctypes.c_void_p), vv.ctypes.data_as(ctypes.c_void_p)))
        self._chk(self._L.mals_group_end_matrix(self._g, side))

    def ingest_finish(self, ingests):
        """mals_group_ingest_finish: ingests[i] holds share `rank of local member i` of the input on that member's device;
        collective.  Afterwards every ingest holds its member's slices, which the members borrow: the ingests are kept alive
        here."""
        arr = (ctypes.c_void_p * len(ingests))(*[g._g.value for g in ingests])
        self._chk(self._L.mals_group_ingest_finish(self._g, arr, len(ingests), 0))
        self._keep_ingest = list(ingests)

    def recommend(self, user_idx, how_many, consider_known_items=False):
        """ServerRecommender.recommend on the group: every query answered by the member that holds the user's row."""
        u = np.ascontiguousarray(user_idx, dtype=np.int64)
        idx = np.empty((len(u), how_many), dtype=np.int64)
        sc = np.empty((len(u), how_many), dtype=np.float32)
        cnt = np.empty(len(u), dtype=np.int32)
        self._chk(self._L.mals_group_recommend(self._g, u.ctypes.data_as(ctypes.c_void_p), len(u), int(how_many), 1 if consider_known_items else 0,
                                               idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p)))
        return idx, sc, cnt

    def most_similar_items(self, items, how_many):
        """mostSimilarItems on the group (any local member: the Y replicas are complete)."""
        flat, ptr = _item_queries(items)
        idx = np.empty((len(ptr) - 1, how_many), dtype=np.int64)
        sc = np.empty((len(ptr) - 1, how_many), dtype=np.float32)
        cnt = np.empty(len(ptr) - 1, dtype=np.int32)
        self._chk(self._L.mals_group_most_similar_items(self._g, flat.ctypes.data_as(ctypes.c_void_p), ptr.ctypes.data_as(ctypes.c_void_p),
                                                        len(ptr) - 1, int(how_many), idx.ctypes.data_as(ctypes.c_void_p),
                                                        sc.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p)))
        return idx, sc, cnt

    def similarity_to_item(self, to_item, items):
        ii = np.ascontiguousarray(items, dtype=np.int64)
        out = np.empty(len(ii), dtype=np.float32)
        self._chk(self._L.mals_group_similarity_to_item(self._g, int(to_item), ii.ctypes.data_as(ctypes.c_void_p), len(ii),
                                                        out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def recommended_because(self, users, items, how_many):
        """recommendedBecause on the group: every query answered by the member that holds the user's row."""
        u = np.ascontiguousarray(users, dtype=np.int64)
        ii = np.ascontiguousarray(items, dtype=np.int64)
        assert len(u) == len(ii)
        idx = np.empty((len(u), how_many), dtype=np.int64)
        sc = np.empty((len(u), how_many), dtype=np.float32)
        cnt = np.empty(len(u), dtype=np.int32)
        self._chk(self._L.mals_group_recommended_because(self._g, u.ctypes.data_as(ctypes.c_void_p), ii.ctypes.data_as(ctypes.c_void_p), len(u),
                                                         int(how_many), idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p),
                                                         cnt.ctypes.data_as(ctypes.c_void_p)))
        return idx, sc, cnt

    def set_tag_users(self, user_idx):
        """itemTagIDs as global user rows: every member keeps those it owns; None or empty clears."""
        uu = np.ascontiguousarray(user_idx if user_idx is not None else [], dtype=np.int64)
        self._chk(self._L.mals_group_set_tag_users(self._g, len(uu), uu.ctypes.data_as(ctypes.c_void_p) if len(uu) else None))

    def most_popular_items(self, how_many):
        """mostPopularItems on the group: every member counts its own users, one member adds the counts and selects.
        Returns what ALSCore.most_popular_items returns on one handle holding the whole model."""
        idx = np.empty(int(how_many), dtype=np.int64)
        sc = np.empty(int(how_many), dtype=np.float32)
        cnt = ctypes.c_int32(0)
        self._chk(self._L.mals_group_most_popular_items(self._g, int(how_many), idx.ctypes.data_as(ctypes.c_void_p),
                                                        sc.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cnt)))
        return idx, sc, cnt.value

    # -- the online write path on the group (the mals_group_* twins of ALSCore's methods of the same names) -------
    # Writes go to every local member (replicated, in one order); a user's known items stay with the member that owns the
    # user; the reads rotate over the members.  Signatures and return values are ALSCore's.
    def set_foldin_solver(self, side, solver):
        self._chk(self._L.mals_group_set_foldin_solver(self._g, side, solver._s if solver is not None else None))

    def set_foldin_learn_rate(self, rate):
        self._chk(self._L.mals_group_set_foldin_learn_rate(self._g, float(rate)))

    def foldin_stats(self):
        """The group's writes counted once (not once per member); the device times are the slowest member's."""
        o = np.zeros(6, dtype=np.int64)
        self._chk(self._L.mals_group_foldin_stats(self._g, o.ctypes.data_as(ctypes.c_void_p)))
        return {"applied": int(o[0]), "failed": int(o[1]), "big_foldin": int(o[2]), "levels": int(o[3]),
                "device_ms_total": o[4] * 1e-6, "device_ms_last": o[5] * 1e-6}

    def set_preferences(self, users, items, values, raise_on_error=True):
        u, i, v = _host(users, np.int64), _host(items, np.int64), _host(values, np.float32)
        assert len(u) == len(i) == len(v)
        st = np.zeros(len(u), dtype=np.int32)
        rc = self._L.mals_group_set_preferences(self._g, len(u), u.ctypes.data_as(ctypes.c_void_p), i.ctypes.data_as(ctypes.c_void_p),
                                                v.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p))
        if raise_on_error or rc not in (_lib.OK, _lib.INVALID_ARG) or not st.any():
            self._chk(rc)
        return st

    def _set_tags(self, fn, users, items, values, raise_on_error):
        u, i, v = _host(users, np.int64), _host(items, np.int64), _host(values, np.float32)
        assert len(u) == len(i) == len(v)
        st = np.zeros(len(u), dtype=np.int32)
        rc = fn(self._g, len(u), u.ctypes.data_as(ctypes.c_void_p), i.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p),
                st.ctypes.data_as(ctypes.c_void_p))
        if raise_on_error or rc not in (_lib.OK, _lib.INVALID_ARG) or not st.any():
            self._chk(rc)
        return st

    def set_user_tags(self, users, tag_items, values, raise_on_error=True):
        """setUserTag on every member (ALSCore.set_user_tags): tag_items are the tags' rows of Y."""
        return self._set_tags(self._L.mals_group_set_user_tags, users, tag_items, values, raise_on_error)

    def set_item_tags(self, tag_users, items, values, raise_on_error=True):
        """setItemTag on every member (ALSCore.set_item_tags): tag_users are the tags' rows of X."""
        return self._set_tags(self._L.mals_group_set_item_tags, tag_users, items, values, raise_on_error)

    def remove_preferences(self, users, items):
        u, i = _host(users, np.int64), _host(items, np.int64)
        assert len(u) == len(i)
        out = np.zeros(max(len(u), 1), dtype=np.int64)
        n = ctypes.c_int64(0)
        self._chk(self._L.mals_group_remove_preferences(self._g, len(u), u.ctypes.data_as(ctypes.c_void_p), i.ctypes.data_as(ctypes.c_void_p),
                                                        out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)))
        return out[:n.value].copy()

    def grow_factor_rows(self, side, n_rows_total):
        self._chk(self._L.mals_group_grow_factor_rows(self._g, side, int(n_rows_total)))

    def estimate_preferences(self, users, items):
        u, i = _host(users, np.int64), _host(items, np.int64)
        out = np.empty(len(u), dtype=np.float32)
        self._chk(self._L.mals_group_estimate_preferences(self._g, len(u), u.ctypes.data_as(ctypes.c_void_p), i.ctypes.data_as(ctypes.c_void_p),
                                                          out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def anonymous_features(self, queries, values=None, raise_on_error=True):
        flat, ptr, vals = ALSCore._anon_args(queries, values)
        nq = len(ptr) - 1
        out = np.zeros((nq, self.features), dtype=np.float32)
        st = np.zeros(nq, dtype=np.int32)
        rc = self._L.mals_group_anonymous_features(self._g, nq, ptr.ctypes.data_as(ctypes.c_void_p), flat.ctypes.data_as(ctypes.c_void_p),
                                                   vals.ctypes.data_as(ctypes.c_void_p) if vals is not None else None,
                                                   out.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p))
        if raise_on_error or not st.any():
            self._chk(rc)
        return out, st

    def recommend_to_anonymous(self, queries, how_many, values=None):
        flat, ptr, vals = ALSCore._anon_args(queries, values)
        nq = len(ptr) - 1
        idx = np.empty((nq, how_many), dtype=np.int64)
        sc = np.empty((nq, how_many), dtype=np.float32)
        cnt = np.empty(nq, dtype=np.int32)
        st = np.zeros(nq, dtype=np.int32)
        rc = self._L.mals_group_recommend_to_anonymous(self._g, nq, ptr.ctypes.data_as(ctypes.c_void_p), flat.ctypes.data_as(ctypes.c_void_p),
                                                       vals.ctypes.data_as(ctypes.c_void_p) if vals is not None else None, int(how_many),
                                                       idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p),
                                                       cnt.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p))
        if not st.any():
            self._chk(rc)
        return idx, sc, cnt, st

    def estimate_for_anonymous(self, to_items, queries, values=None):
        flat, ptr, vals = ALSCore._anon_args(queries, values)
        nq = len(ptr) - 1
        to = _host(to_items, np.int64)
        assert len(to) == nq
        out = np.zeros(nq, dtype=np.float32)
        st = np.zeros(nq, dtype=np.int32)
        rc = self._L.mals_group_estimate_for_anonymous(self._g, nq, to.ctypes.data_as(ctypes.c_void_p), ptr.ctypes.data_as(ctypes.c_void_p),
                                                       flat.ctypes.data_as(ctypes.c_void_p),
                                                       vals.ctypes.data_as(ctypes.c_void_p) if vals is not None else None,
                                                       out.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p))
        if not st.any():
            self._chk(rc)
        return out, st

    # -- a new generation into the live group (the mals_group_* twins of ALSCore's methods of the same names) ------
    def mark_recent(self, side, rows):
        """mals_group_mark_recent: global rows of `side` written elsewhere since the last load."""
        r = _host(rows, np.int64)
        self._chk(self._L.mals_group_mark_recent(self._g, side, len(r), r.ctypes.data_as(ctypes.c_void_p) if len(r) else None))

    def get_recent(self, side):
        """mals_group_get_recent: the global rows of `side` written since the last load (the group's writes and
        mark_recent), ascending."""
        n = ctypes.c_int64(0)
        self._chk(self._L.mals_group_get_recent(self._g, side, None, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.int64)
        if n.value:
            self._chk(self._L.mals_group_get_recent(self._g, side, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)))
        return out[:n.value]

    def load_generation(self, cur_user_ids, cur_item_ids, new_user_ids, new_item_ids, new_X, new_Y, new_known=None,
                        item_tag_ids=None, user_tag_ids=None, keep_not_updated=False, recompute_solvers=False):
        """mals_group_load_generation: ALSCore.load_generation for the group -- the same arguments (the new model WHOLE; torch
        CUDA tensors on the first local member's device) and the same return shape.  Afterwards bounds(SIDE_X) is the new
        ownership plan."""
        out = _load_generation(self.features, lambda L, R: self._chk(self._L.mals_group_load_generation(self._g, L, R)),
                               lambda side, p: self._chk(self._L.mals_group_generation_get_ids(self._g, side, p)),
                               lambda side, p: self._chk(self._L.mals_group_generation_get_map(self._g, side, p)),
                               cur_user_ids, cur_item_ids, new_user_ids, new_item_ids, new_X, new_Y, new_known, item_tag_ids, user_tag_ids,
                               keep_not_updated, recompute_solvers)
        for side in (SIDE_X, SIDE_Y):     # the members' matrices are released: nothing of the caller's is borrowed any more
            self._keep.pop(("M", side), None)
        return out

    def replica_digest(self, side, row_begin=0, n_rows=None):
        """mals_group_replica_digest: (uint64 digest of the range on every local member, whether they all agree), taken
        between the same two group writes on every member.  n_rows None: to the end of the replica."""
        m, _ = self.local(0)
        if n_rows is None:
            n_rows = m.factor_device_ptr(side)[1] - int(row_begin)
        n_local = self._n_local()
        out = np.zeros(n_local, dtype=np.uint64)
        eq = ctypes.c_int32(0)
        self._chk(self._L.mals_group_replica_digest(self._g, side, int(row_begin), int(n_rows), out.ctypes.data_as(ctypes.c_void_p),
                                                    ctypes.byref(eq)))
        return out, bool(eq.value)

    def _n_local(self):
        n = 0
        h, r = ctypes.c_void_p(), ctypes.c_int32()
        while self._L.mals_group_local(self._g, n, ctypes.byref(h), ctypes.byref(r)) == _lib.OK:
            n += 1
        return n

    def bounds(self, side):
        out = np.zeros(self.world + 1, dtype=np.int64)
        self._chk(self._L.mals_group_bounds(self._g, side, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    # -- compute ----------------------------------------------------------------------------------
    def half_iteration(self, side):
        self._chk(self._L.mals_group_half_iteration(self._g, side))

    def iterate(self, n=1):
        for _ in range(n):
            self.half_iteration(SIDE_X)
            self.half_iteration(SIDE_Y)

    def exchange_only(self, side):
        self._chk(self._L.mals_group_exchange_only(self._g, side))

    def synchronize(self):
        self._chk(self._L.mals_group_synchronize(self._g))

    def factorize(self, convergence_threshold, max_iterations, random_y, iterate, test_users, test_items):
        tu = np.ascontiguousarray(test_users, dtype=np.int64)
        ti = np.ascontiguousarray(test_items, dtype=np.int64)
        it, conv = ctypes.c_int32(0), ctypes.c_double(float("nan"))
        self._chk(self._L.mals_group_factorize(self._g, float(convergence_threshold), int(max_iterations), int(bool(random_y)),
                                               int(bool(iterate)), tu.ctypes.data_as(ctypes.c_void_p), len(tu),
                                               ti.ctypes.data_as(ctypes.c_void_p), len(ti), ctypes.byref(it), ctypes.byref(conv)))
        return it.value, conv.value


__all__ = ["GroupALS", "plan_shards", "generation_plan_host", "SIDE_X", "SIDE_Y"]
