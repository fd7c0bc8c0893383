"""ALSCore: thin object wrapper over one mals_handle (one GPU).  Pure plumbing: every method is a
single C-ABI call (include/myrrix_als.h); arrays are numpy (host) or torch CUDA tensors (device,
borrowed -- a reference is kept so they stay alive)."""
import ctypes

import numpy as np

from . import _lib
from ._lib import (FLAG_LOSS_IGNORES_UNSPECIFIED, FLAG_RECONSTRUCT_R, MEM_DEVICE, MEM_HOST, SIDE_X,
                   SIDE_Y)


class MalsError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s: %s" % (_lib.STATUS_NAMES.get(status, status), message))
        self.status = status
        self.message = message


class SingularSystem(MalsError):
    """MALS_SINGULAR: the reference throws SingularMatrixSolverException here (CMLSS:46-54)."""

    def __init__(self, status, message, side, row, apparent_rank):
        super().__init__(status, message)
        self.side = side
        self.row = row
        self.apparent_rank = apparent_rank


class Cancelled(MalsError):
    pass


class IllConditioned(MalsError):
    """MALS_ILL_CONDITIONED: IllConditionedSolverException (Generation.java:150-153)."""

    def __init__(self, status, message, inf_norm):
        super().__init__(status, message)
        self.inf_norm = inf_norm


class HostSolver:
    """One mals_solver: the fp64 pivoted-QR factorization of a k x k matrix (Solver.java:35-41)."""

    def __init__(self, L, handle):
        self._L, self._s = L, handle
        self.n = L.mals_solver_dim(handle)

    @classmethod
    def create(cls, A, singularity_threshold=1e-5):
        """MatrixUtils.getSolver(A) (MU:137, CMLSS:37-55); raises SingularSystem with the rank."""
        L = _lib.load()
        A = _host(A, np.float64)
        assert A.ndim == 2 and A.shape[0] == A.shape[1]
        s, rank = ctypes.c_void_p(), ctypes.c_int32(0)
        rc = L.mals_solver_create(A.ctypes.data_as(ctypes.c_void_p), A.shape[0], float(singularity_threshold),
                                  ctypes.byref(s), ctypes.byref(rank))
        if rc == _lib.SINGULAR:
            raise SingularSystem(rc, "Apparent rank: %d" % rank.value, -1, -1, rank.value)
        if rc != _lib.OK:
            raise MalsError(rc, "mals_solver_create failed")
        return cls(L, s)

    def solve_dtof(self, b):
        b = _host(b, np.float64)
        assert b.shape == (self.n,)
        x = np.empty(self.n, dtype=np.float32)
        rc = self._L.mals_solver_solve_dtof(self._s, b.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p))
        if rc != _lib.OK:
            raise MalsError(rc, "mals_solver_solve_dtof failed")
        return x

    def solve_ftod(self, b):
        b = _host(b, np.float32)
        assert b.shape == (self.n,)
        x = np.empty(self.n, dtype=np.float64)
        rc = self._L.mals_solver_solve_ftod(self._s, b.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p))
        if rc != _lib.OK:
            raise MalsError(rc, "mals_solver_solve_ftod failed")
        return x

    def close(self):
        if getattr(self, "_s", None) is not None and self._s.value:
            self._L.mals_solver_destroy(self._s)
            self._s = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _host(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _item_queries(items):
    """mostSimilarItems queries as CSR: a sequence of ints is one item per query, a list of sequences several per query."""
    items = list(items)
    if items and all(np.ndim(q) == 0 for q in items):
        flat = np.ascontiguousarray(np.asarray(items, dtype=np.int64))
        return flat, np.arange(len(flat) + 1, dtype=np.int64)
    qs = [np.asarray(q, dtype=np.int64).ravel() for q in items]
    ptr = np.zeros(len(qs) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(q) for q in qs])
    flat = np.ascontiguousarray(np.concatenate(qs)) if ptr[-1] else np.zeros(0, np.int64)
    return flat, ptr


def factor_digest_host(rows, row_begin=0):
    """mals_factor_digest_host: the digest mals_factor_digest gives for rows [row_begin, row_begin + len(rows)) of a replica
    that holds `rows` (n x features float32) there.  Host only: no handle, no device."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] < 1:
        raise ValueError("rows must be n x features")
    out = ctypes.c_uint64(0)
    rc = _lib.load().mals_factor_digest_host(rows.ctypes.data_as(ctypes.c_void_p), rows.shape[1], int(row_begin), rows.shape[0], ctypes.byref(out))
    if rc != _lib.OK:
        raise MalsError(rc, "mals_factor_digest_host: bad arguments")
    return out.value


def generation_hash_host(ids):
    """mals_generation_hash_host of every id (int64) as uint64: the home slot of an id in the join's table is
    hash & (slots - 1), slots = the smallest power of two >= max(64, 2 * n_new).  Host only."""
    L = _lib.load()
    return np.array([L.mals_generation_hash_host(int(i)) for i in np.asarray(ids, dtype=np.int64).ravel()], dtype=np.uint64)


def generation_join_host(cur_ids, new_ids, recent_rows=(), flags=0):
    """mals_generation_join_host: the id join of mals_load_generation on the host.  Returns (map int64 [n_cur]: live row ->
    merged row, -1 = pruned; counts dict).  Raises MalsError(INVALID_ARG) for a duplicate id.  Host only."""
    cur, new, rec = _host(cur_ids, np.int64), _host(new_ids, np.int64), _host(recent_rows, np.int64)
    out = np.empty(len(cur), dtype=np.int64)
    counts = np.zeros(4, dtype=np.int64)
    rc = _lib.load().mals_generation_join_host(cur.ctypes.data_as(ctypes.c_void_p), len(cur), new.ctypes.data_as(ctypes.c_void_p), len(new),
                                               rec.ctypes.data_as(ctypes.c_void_p), len(rec), int(flags),
                                               out.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p))
    if rc != _lib.OK:
        raise MalsError(rc, "mals_generation_join_host: a duplicate id, or a recent row outside the live rows")
    return out, {"n_merged": int(counts[0]), "n_updated": int(counts[1]), "n_kept": int(counts[2]), "n_pruned": int(counts[3])}


def lsh_max_bits_differing(sample_ratio, num_hashes=20):
    """maxBitsDiffering of LocationSensitiveHash (LocationSensitiveHash.java:98-108) for model.lsh.sampleRatio and
    model.lsh.numHashes; may be -1.  Host only: no handle, no device."""
    out = ctypes.c_int32(0)
    rc = _lib.load().mals_lsh_max_bits_differing(float(sample_ratio), int(num_hashes), ctypes.byref(out))
    if rc != _lib.OK:
        raise MalsError(rc, "lsh_max_bits_differing: sample_ratio in (0, 1], num_hashes in 1..64")
    return out.value


class Rescorer:
    """RecommendIterator's IDRescorer in the form the device runs (include/myrrix_als.h, "rescorers"): a filter set of
    item indices and rescore(i, sum) = fl(fl(scale_i * sum) + offset_i) in fp64, applied to the sum of the dots before the
    division by the query's vector count.  Made by ALSCore.rescorer(); bound to that handle."""

    def __init__(self, core):
        self._core = core
        self._h = ctypes.c_void_p()
        core._chk(core._L.mals_rescorer_create(core._h, ctypes.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def set_filter(self, items):
        """isFiltered: these dense item indices are skipped; None or empty clears."""
        ii = _host(items if items is not None else [], np.int64)
        self._core._chk(self._core._L.mals_rescorer_set_filter(self._h, len(ii), ii.ctypes.data_as(ctypes.c_void_p) if len(ii) else None, MEM_HOST))

    def set_weights(self, scale=None, offset=None):
        """Per-item fp64 weights of rows [0, len): scale_i > 0 and finite, offset_i finite; either may be None (1 / 0).
        Rows past the arrays have scale 1 and offset 0."""
        sc = None if scale is None else _host(scale, np.float64)
        of = None if offset is None else _host(offset, np.float64)
        n = len(sc) if sc is not None else len(of) if of is not None else 0
        if sc is not None and of is not None and len(sc) != len(of):
            raise ValueError("scale and offset cover different rows (%d, %d)" % (len(sc), len(of)))
        self._core._chk(self._core._L.mals_rescorer_set_weights(
            self._h, sc.ctypes.data_as(ctypes.c_void_p) if sc is not None and n else None,
            of.ctypes.data_as(ctypes.c_void_p) if of is not None and n else None, n, MEM_HOST))

    def set_uniform(self, scale=1.0, offset=0.0):
        """The same weights for every item (replaces per-item weights)."""
        self._core._chk(self._core._L.mals_rescorer_set_uniform(self._h, float(scale), float(offset)))

    def close(self):
        if self._h is not None and self._h.value:
            self._core._L.mals_rescorer_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _load_generation(features, load, get_ids, get_map, cur_user_ids, cur_item_ids, new_user_ids, new_item_ids, new_X, new_Y, new_known,
                     item_tag_ids, user_tag_ids, keep_not_updated, recompute_solvers):
    """The argument marshalling and the return shape of ALSCore.load_generation and GroupALS.load_generation: load(L, R) makes
    the C call (and raises), get_ids / get_map(side, pointer) fetch the merged ids and the maps."""

    arrays = [new_user_ids, new_item_ids, new_X, new_Y] + (list(new_known) if new_known is not None else []) + \
             [a for a in (item_tag_ids, user_tag_ids) if a is not None]
    device = any(_is_torch(a) for a in arrays)
    keep = []

    def ptr(a, dtype):
        if a is None:
            return None, 0
        if device:
            assert _is_torch(a) and a.is_cuda and str(a.dtype) == "torch." + np.dtype(dtype).name, "the new model: all device or all host"
            a = a.contiguous()
            keep.append(a)
            return (ctypes.c_void_p(a.data_ptr()) if a.numel() else None), int(a.shape[0])
        a = _host(a, dtype)
        keep.append(a)
        return (a.ctypes.data_as(ctypes.c_void_p) if a.size else None), int(a.shape[0])

    cur_device = _is_torch(cur_user_ids)
    if cur_device:     # the live ids on the device too (both)
        assert _is_torch(cur_item_ids) and cur_user_ids.is_cuda and cur_item_ids.is_cuda and str(cur_user_ids.dtype) == str(cur_item_ids.dtype) == "torch.int64"
        cur = [cur_user_ids.contiguous(), cur_item_ids.contiguous()]
    else:
        cur = [_host(cur_user_ids, np.int64), _host(cur_item_ids, np.int64)]
    L = _lib.GenerationLoad()
    L.struct_size = ctypes.sizeof(_lib.GenerationLoad)
    L.flags = (_lib.GENERATION_KEEP_NOT_UPDATED if keep_not_updated else 0) | (_lib.GENERATION_RECOMPUTE_SOLVERS if recompute_solvers else 0)
    L.features = features
    L.cur_mem_kind = MEM_DEVICE if cur_device else MEM_HOST
    L.new_mem_kind = MEM_DEVICE if device else MEM_HOST
    for s, (ids, rows) in enumerate(((new_user_ids, new_X), (new_item_ids, new_Y))):
        if not len(cur[s]):
            L.cur_ids[s] = None
        else:
            L.cur_ids[s] = ctypes.c_void_p(cur[s].data_ptr()) if cur_device else cur[s].ctypes.data_as(ctypes.c_void_p)
        L.n_cur[s] = len(cur[s])
        L.new_ids[s], L.n_new[s] = ptr(ids, np.int64)
        p, n = ptr(rows, np.float32)
        if n != L.n_new[s] or (n and tuple(keep[-1].shape) != (n, features)):
            raise ValueError("load_generation: the new rows must be n_new x features")
        L.new_rows[s] = p
    if new_known is not None:
        L.new_known_ptr, n = ptr(new_known[0], np.int64)
        if n != L.n_new[0] + 1:
            raise ValueError("load_generation: new_known[0] holds n_new users + 1 offsets")
        L.new_known_idx, _ = ptr(new_known[1], np.int32)
    L.item_tag_ids, L.n_item_tag_ids = ptr(item_tag_ids, np.int64)
    L.user_tag_ids, L.n_user_tag_ids = ptr(user_tag_ids, np.int64)
    R = _lib.GenerationResult()
    R.struct_size = ctypes.sizeof(_lib.GenerationResult)
    load(ctypes.byref(L), ctypes.byref(R))
    res = {name: (list(getattr(R, name)) if hasattr(getattr(R, name), "__len__") else getattr(R, name))
           for name, _ in _lib.GenerationResult._fields_ if name != "struct_size"}
    ids, maps = [], []
    for side in (SIDE_X, SIDE_Y):
        i = np.empty(int(R.n_merged[side]), dtype=np.int64)
        m = np.empty(len(cur[side]), dtype=np.int64)
        get_ids(side, i.ctypes.data_as(ctypes.c_void_p))
        if len(m):
            get_map(side, m.ctypes.data_as(ctypes.c_void_p))
        ids.append(i)
        maps.append(m)
    return res, tuple(ids), tuple(maps)


class ALSCore:
    def __init__(self, features, alpha=1.0, lam=0.1, flags=0, device=0, segment_nnz=0,
                 singularity_threshold=1e-5, chunk_rows=0, gramian_mode=0, solve_mode=0):
        self._L = _lib.load()
        cfg = _lib.Config()
        self._L.mals_default_config(ctypes.byref(cfg))
        cfg.features = int(features)
        cfg.alpha = float(alpha)
        cfg.lam = float(lam)
        cfg.flags = int(flags)
        cfg.device = int(device)
        cfg.segment_nnz = int(segment_nnz)
        cfg.chunk_rows = int(chunk_rows)
        cfg.gramian_mode = int(gramian_mode)
        cfg.solve_mode = int(solve_mode)
        self.chunk_rows = max(0, int(chunk_rows))
        cfg.singularity_threshold = float(singularity_threshold)
        self.features = int(features)
        self._h = ctypes.c_void_p()
        self._keep = {}
        rc = self._L.mals_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc != _lib.OK:
            self._h = ctypes.c_void_p()
            raise MalsError(rc, "mals_create failed (features=%d, device=%d): a HIP device is "
                                "required, there is no CPU fallback" % (features, device))

    # -- lifecycle --------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.mals_destroy(self._h)
            self._h = ctypes.c_void_p()
            self._keep.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc == _lib.OK:
            return
        msg = (self._L.mals_last_error(self._h) or b"").decode("utf-8", "replace")
        if rc == _lib.SINGULAR:
            side, row, rank = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
            self._L.mals_singular_info(self._h, ctypes.byref(side), ctypes.byref(row), ctypes.byref(rank))
            raise SingularSystem(rc, msg, side.value, row.value, rank.value)
        if rc == _lib.CANCELLED:
            raise Cancelled(rc, msg)
        raise MalsError(rc, msg)

    # -- configuration ----------------------------------------------------------------------------
    def set_stream(self, hip_stream_ptr):
        self._chk(self._L.mals_set_stream(self._h, ctypes.c_void_p(int(hip_stream_ptr or 0))))

    def set_factor_rows(self, side, n_rows_total):
        self._keep.pop(("F", side), None)
        self._chk(self._L.mals_set_factor_rows(self._h, side, int(n_rows_total)))

    def bind_factors(self, side, tensor):
        """tensor: contiguous fp32 torch CUDA tensor [n_rows_total, features]."""
        assert _is_torch(tensor) and tensor.is_cuda and tensor.is_contiguous()
        assert tensor.dim() == 2 and tensor.shape[1] == self.features and str(tensor.dtype) == "torch.float32"
        self._keep[("F", side)] = tensor
        self._chk(self._L.mals_bind_factors(self._h, side, ctypes.c_void_p(tensor.data_ptr()),
                                            int(tensor.shape[0])))

    def factor_device_ptr(self, side):
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._chk(self._L.mals_factor_device_ptr(self._h, side, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def set_matrix(self, side, row_ptr, col_idx, val, row_offset=0):
        if _is_torch(row_ptr):
            assert row_ptr.is_cuda and col_idx.is_cuda and val.is_cuda
            assert str(row_ptr.dtype) == "torch.int64" and str(col_idx.dtype) == "torch.int32" \
                and str(val.dtype) == "torch.float32"
            row_ptr, col_idx, val = row_ptr.contiguous(), col_idx.contiguous(), val.contiguous()
            self._keep[("M", side)] = (row_ptr, col_idx, val)
            n_rows, nnz = int(row_ptr.shape[0]) - 1, int(col_idx.shape[0])
            self._chk(self._L.mals_set_matrix(
                self._h, side, int(row_offset), n_rows, nnz, ctypes.c_void_p(row_ptr.data_ptr()),
                ctypes.c_void_p(col_idx.data_ptr()), ctypes.c_void_p(val.data_ptr()), MEM_DEVICE))
        else:
            row_ptr = _host(row_ptr, np.int64)
            col_idx = _host(col_idx, np.int32)
            val = _host(val, np.float32)
            self._keep.pop(("M", side), None)
            n_rows, nnz = len(row_ptr) - 1, len(col_idx)
            self._chk(self._L.mals_set_matrix(
                self._h, side, int(row_offset), n_rows, nnz, row_ptr.ctypes.data_as(ctypes.c_void_p),
                col_idx.ctypes.data_as(ctypes.c_void_p), val.ctypes.data_as(ctypes.c_void_p), MEM_HOST))

    def set_matrix_chunked(self, side, row_ptr, col_idx, val, rows_per_chunk, row_offset=0):
        """Same as set_matrix (host arrays) through the begin/append/end entry points."""
        row_ptr = _host(row_ptr, np.int64)
        col_idx = _host(col_idx, np.int32)
        val = _host(val, np.float32)
        n_rows, nnz = len(row_ptr) - 1, len(col_idx)
        self._chk(self._L.mals_begin_matrix(self._h, side, int(row_offset), n_rows, nnz))
        for r0 in range(0, max(n_rows, 1), rows_per_chunk):
            r1 = min(n_rows, r0 + rows_per_chunk)
            rp = np.ascontiguousarray(row_ptr[r0:r1 + 1] - row_ptr[r0])
            c = np.ascontiguousarray(col_idx[row_ptr[r0]:row_ptr[r1]])
            v = np.ascontiguousarray(val[row_ptr[r0]:row_ptr[r1]])
            self._chk(self._L.mals_append_rows(
                self._h, side, r1 - r0, rp.ctypes.data_as(ctypes.c_void_p),
                c.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p)))
        self._chk(self._L.mals_end_matrix(self._h, side))

    def value_bound(self, side):
        v = ctypes.c_float(0.0)
        self._chk(self._L.mals_get_value_bound(self._h, side, ctypes.byref(v)))
        return v.value

    def set_value_bound(self, side, max_abs_value):
        self._chk(self._L.mals_set_value_bound(self._h, side, float(max_abs_value)))

    def value_stats(self, side):
        """(largest |value|, sum of |value|, number of entries) of the local rows."""
        m, sm, n = ctypes.c_float(0.0), ctypes.c_double(0.0), ctypes.c_int64(0)
        self._chk(self._L.mals_get_value_stats(self._h, side, ctypes.byref(m), ctypes.byref(sm), ctypes.byref(n)))
        return m.value, sm.value, n.value

    def set_value_stats(self, side, max_abs_value, mean_abs_value):
        self._chk(self._L.mals_set_value_stats(self._h, side, float(max_abs_value), float(mean_abs_value)))

    # -- factors ----------------------------------------------------------------------------------
    def set_factors(self, side, rows, row_begin=0):
        rows = _host(rows, np.float32)
        assert rows.ndim == 2 and rows.shape[1] == self.features
        self._chk(self._L.mals_set_factors(self._h, side, int(row_begin), rows.shape[0],
                                           rows.ctypes.data_as(ctypes.c_void_p)))

    def get_factors(self, side, row_begin=0, n_rows=None):
        if n_rows is None:
            n_rows = self.factor_device_ptr(side)[1] - row_begin
        out = np.empty((n_rows, self.features), dtype=np.float32)
        self._chk(self._L.mals_get_factors(self._h, side, int(row_begin), int(n_rows),
                                           out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def get_rows(self, side, idx):
        idx = _host(idx, np.int64)
        out = np.empty((len(idx), self.features), dtype=np.float32)
        self._chk(self._L.mals_get_rows(self._h, side, idx.ctypes.data_as(ctypes.c_void_p), len(idx),
                                        out.ctypes.data_as(ctypes.c_void_p)))
        return out

    # -- compute ----------------------------------------------------------------------------------
    def gramian(self, side, fetch=False):
        if fetch:
            G = np.empty((self.features, self.features), dtype=np.float64)
            self._chk(self._L.mals_gramian(self._h, side, G.ctypes.data_as(ctypes.c_void_p)))
            return G
        self._chk(self._L.mals_gramian(self._h, side, None))
        return None

    def gramian_partial(self, side, row_begin, n_rows, out_tensor):
        assert _is_torch(out_tensor) and out_tensor.is_cuda and str(out_tensor.dtype) == "torch.float64"
        assert out_tensor.numel() == self.features * self.features and out_tensor.is_contiguous()
        self._chk(self._L.mals_gramian_partial(self._h, side, int(row_begin), int(n_rows),
                                               ctypes.c_void_p(out_tensor.data_ptr())))

    def set_gramian(self, side, G):
        if _is_torch(G):
            assert G.is_cuda and str(G.dtype) == "torch.float64" and G.is_contiguous()
            self._chk(self._L.mals_set_gramian(self._h, side, ctypes.c_void_p(G.data_ptr()), MEM_DEVICE))
        else:
            G = _host(G, np.float64)
            self._chk(self._L.mals_set_gramian(self._h, side, G.ctypes.data_as(ctypes.c_void_p), MEM_HOST))

    def solve_side(self, side):
        self._chk(self._L.mals_solve_side(self._h, side))

    def solve_chunk(self, side, chunk):
        self._chk(self._L.mals_solve_chunk(self._h, side, int(chunk)))

    def num_chunks(self, side):
        n = ctypes.c_int32()
        self._chk(self._L.mals_num_chunks(self._h, side, ctypes.byref(n)))
        return n.value

    def check(self):
        self._chk(self._L.mals_check(self._h))

    def half_iteration(self, side):
        self._chk(self._L.mals_half_iteration(self._h, side))

    def factorize(self, convergence_threshold, max_iterations, random_y, test_users, test_items,
                  iterate=True):
        tu = _host(test_users, np.int64)
        ti = _host(test_items, np.int64)
        iters, conv = ctypes.c_int32(0), ctypes.c_double(float("nan"))
        rc = self._L.mals_factorize(self._h, float(convergence_threshold), int(max_iterations),
                                    1 if random_y else 0, 1 if iterate else 0,
                                    tu.ctypes.data_as(ctypes.c_void_p), len(tu),
                                    ti.ctypes.data_as(ctypes.c_void_p), len(ti),
                                    ctypes.byref(iters), ctypes.byref(conv))
        self._chk(rc)
        return iters.value, conv.value

    def set_iteration_callback(self, fn):
        """mals_set_iteration_callback: fn(info: dict) after every iteration of factorize() -- iteration, avg_abs_difference,
        seconds, x_rows, y_rows, entries_gathered, algorithmic_bytes, devices (what call() logs per iteration, ALS:241-246,
        351-358); None removes it."""
        if fn is None:
            self._iter_cb = None
            self._chk(self._L.mals_set_iteration_callback(self._h, None, None))
            return

        def tramp(_user, info):
            i = info.contents
            fn({name: getattr(i, name) for name, _ in _lib.IterationInfo._fields_ if name not in ("struct_size", "reserved")})
        self._iter_cb = _lib.ITERATION_FN(tramp)      # keep the trampoline alive as long as the library may call it
        self._chk(self._L.mals_set_iteration_callback(self._h, ctypes.cast(self._iter_cb, ctypes.c_void_p), None))

    def cancel(self):
        self._chk(self._L.mals_cancel(self._h))

    def rescorer(self):
        """A new Rescorer bound to this handle (the identity until it is set)."""
        return Rescorer(self)

    def recommend(self, user_idx, how_many, consider_known_items=False, rescorer=None):
        """ServerRecommender.recommend for model users (dense indices): (item_idx [q][how_many] int64,
        scores float32, counts).  rescorer: a Rescorer of this handle (None: none)."""
        u = _host(user_idx, np.int64)
        idx = np.empty((len(u), how_many), dtype=np.int64)
        sc = np.empty((len(u), how_many), dtype=np.float32)
        cnt = np.empty(len(u), dtype=np.int32)
        args = (u.ctypes.data_as(ctypes.c_void_p), len(u), int(how_many), 1 if consider_known_items else 0,
                idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p))
        if rescorer is None:
            self._chk(self._L.mals_recommend(self._h, *args))
        else:
            self._chk(self._L.mals_recommend_rescored(self._h, rescorer.handle, *args))
        return idx, sc, cnt

    def recommend_vectors(self, vectors, how_many, exclude=None, rescorer=None):
        """Top-N for caller-supplied query vectors; exclude: optional list of item-index lists; rescorer: a Rescorer."""
        v = _host(vectors, np.float32)
        assert v.ndim == 2 and v.shape[1] == self.features
        idx = np.empty((len(v), how_many), dtype=np.int64)
        sc = np.empty((len(v), how_many), dtype=np.float32)
        cnt = np.empty(len(v), dtype=np.int32)
        ep = ei = None
        if exclude is not None:
            ptr = np.zeros(len(v) + 1, dtype=np.int64)
            ptr[1:] = np.cumsum([len(e) for e in exclude])
            flat = np.ascontiguousarray(np.concatenate([np.asarray(e, np.int64) for e in exclude]) if ptr[-1] else np.zeros(0, np.int64))
            ep, ei = ptr.ctypes.data_as(ctypes.c_void_p), flat.ctypes.data_as(ctypes.c_void_p)
            self._keep[("excl",)] = (ptr, flat)
        if rescorer is None:
            self._chk(self._L.mals_recommend_vectors(self._h, v.ctypes.data_as(ctypes.c_void_p), len(v), int(how_many), ep, ei,
                                                     idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p),
                                                     cnt.ctypes.data_as(ctypes.c_void_p)))
        else:
            self._chk(self._L.mals_recommend_to_many_rescored(self._h, rescorer.handle, v.ctypes.data_as(ctypes.c_void_p), None, len(v),
                                                              int(how_many), ep, ei, idx.ctypes.data_as(ctypes.c_void_p),
                                                              sc.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p)))
        return idx, sc, cnt

    def lsh_build(self, num_hashes=20, sample_ratio=None, max_bits_differing=None, random_vectors=None, mean=None, seed=None):
        """Build the reference's candidate filter (LocationSensitiveHash.java:89-152) over the rows of Y: from then on every
        recommend call only sees a query's LSH candidates and the rows of Y grown later.  sample_ratio
        (model.lsh.sampleRatio) or max_bits_differing sets the threshold; random_vectors: [num_hashes][features] booleans
        (None: drawn hash-major with random_mt.MersenneTwister(seed).nextBoolean(), as LSH:113-119 draws them from
        RandomManager.getRandom()); mean: features doubles (None: the mean of Y's rows, computed on the device).  Returns
        the random vectors used."""
        from . import random_mt
        H = int(num_hashes)
        if max_bits_differing is None:
            if sample_ratio is None:
                raise ValueError("lsh_build: give sample_ratio or max_bits_differing")
            max_bits_differing = lsh_max_bits_differing(sample_ratio, H)
        if random_vectors is None:
            rng = random_mt.MersenneTwister(seed)
            random_vectors = np.array([[rng.nextBoolean() for _ in range(self.features)] for _ in range(H)], dtype=bool).reshape(H, self.features)
        rv = np.ascontiguousarray(np.asarray(random_vectors, dtype=bool).astype(np.uint8))
        if rv.shape != (H, self.features):
            raise ValueError("lsh_build: random_vectors must be [num_hashes][features], got %s" % (rv.shape,))
        m = None if mean is None else _host(mean, np.float64)
        if m is not None and m.shape != (self.features,):
            raise ValueError("lsh_build: mean must hold features doubles")
        self._chk(self._L.mals_lsh_build(self._h, H, int(max_bits_differing), rv.ctypes.data_as(ctypes.c_void_p),
                                         m.ctypes.data_as(ctypes.c_void_p) if m is not None else None))
        return rv.astype(bool)

    def lsh_clear(self):
        """Back to every item a candidate."""
        self._chk(self._L.mals_lsh_clear(self._h))

    def lsh_info(self):
        o = np.zeros(6, dtype=np.int64)
        self._chk(self._L.mals_lsh_info(self._h, o.ctypes.data_as(ctypes.c_void_p)))
        return {"num_hashes": int(o[0]), "max_bits_differing": int(o[1]), "rows_signed": int(o[2]), "rows_now": int(o[3]),
                "filter_queries": int(o[4]), "dense_queries": int(o[5])}

    def lsh_get(self, row_begin=0, n_rows=None):
        """(mean float64 [features], signatures uint64 [n_rows]) of the built filter: rows [row_begin, row_begin + n_rows)
        of the rows signed at build time (None: all from row_begin)."""
        if n_rows is None:
            n_rows = self.lsh_info()["rows_signed"] - int(row_begin)
        mean = np.empty(self.features, dtype=np.float64)
        sig = np.empty(int(n_rows), dtype=np.uint64)
        self._chk(self._L.mals_lsh_get(self._h, mean.ctypes.data_as(ctypes.c_void_p), int(row_begin), int(n_rows),
                                       sig.ctypes.data_as(ctypes.c_void_p) if n_rows else None))
        return mean, sig

    def lsh_signatures(self, vectors):
        """toBitSignature (LocationSensitiveHash.java:169-190) of caller vectors with the built mean and random vectors."""
        v = _host(vectors, np.float32)
        assert v.ndim == 2 and v.shape[1] == self.features
        out = np.empty(len(v), dtype=np.uint64)
        self._chk(self._L.mals_lsh_signatures(self._h, v.ctypes.data_as(ctypes.c_void_p), len(v), out.ctypes.data_as(ctypes.c_void_p) if len(v) else None))
        return out

    def set_known_items(self, row_ptr, item_idx):
        """knownItemIDs as a CSR over the local user rows (generation.getKnownItemIDs()); None, None: back to the rows of R."""
        if row_ptr is None:
            self._chk(self._L.mals_set_known_items(self._h, 0, None, None, MEM_HOST))
            return
        rp = _host(row_ptr, np.int64)
        ii = _host(item_idx, np.int32)
        self._chk(self._L.mals_set_known_items(self._h, len(rp) - 1, rp.ctypes.data_as(ctypes.c_void_p), ii.ctypes.data_as(ctypes.c_void_p), MEM_HOST))

    def set_tag_items(self, item_idx):
        """userTagIDs as dense item indices: rows of Y that no recommend call returns (RecommendIterator.java:72); None or
        empty clears."""
        ii = _host(item_idx if item_idx is not None else [], np.int64)
        self._chk(self._L.mals_set_tag_items(self._h, len(ii), ii.ctypes.data_as(ctypes.c_void_p) if len(ii) else None, MEM_HOST))

    def tag_item_count(self):
        n = ctypes.c_int64(0)
        self._chk(self._L.mals_get_tag_item_count(self._h, ctypes.byref(n)))
        return n.value

    def set_tag_users(self, user_idx):
        """itemTagIDs as global user rows: "users" that are tags of items, which most_popular_items does not count
        (ServerRecommender.java:631-638); rows outside this handle's users are ignored; None or empty clears."""
        uu = _host(user_idx if user_idx is not None else [], np.int64)
        self._chk(self._L.mals_set_tag_users(self._h, len(uu), uu.ctypes.data_as(ctypes.c_void_p) if len(uu) else None, MEM_HOST))

    def tag_user_count(self):
        n = ctypes.c_int64(0)
        self._chk(self._L.mals_get_tag_user_count(self._h, ctypes.byref(n)))
        return n.value

    def most_popular_items(self, how_many, rescorer=None):
        """mostPopularItems (ServerRecommender.java:611-673): the items most users know, best first, ties in ascending item
        index.  Returns (item_idx [how_many] int64, scores float32 -- the user counts, or their rescored values -- and the
        number of results); padding -1 / -inf.  rescorer: a Rescorer of this handle (None: none)."""
        idx = np.empty(int(how_many), dtype=np.int64)
        sc = np.empty(int(how_many), dtype=np.float32)
        cnt = ctypes.c_int32(0)
        self._chk(self._L.mals_most_popular_items(self._h, rescorer.handle if rescorer is not None else None, int(how_many),
                                                  idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cnt)))
        return idx, sc, cnt.value

    def most_popular_stats(self):
        """{calls, recounts, overlay_rows, pairs}: the last two describe the last recount."""
        o = np.zeros(4, dtype=np.int64)
        self._chk(self._L.mals_most_popular_stats(self._h, o.ctypes.data_as(ctypes.c_void_p)))
        return {"calls": int(o[0]), "recounts": int(o[1]), "overlay_rows": int(o[2]), "pairs": int(o[3])}

    def recommend_front_stats(self):
        """{calls, queries, passes, exclusive} of the serving front since the handle was created."""
        o = np.zeros(4, dtype=np.int64)
        self._chk(self._L.mals_recommend_front_stats(self._h, o.ctypes.data_as(ctypes.c_void_p)))
        return {"calls": int(o[0]), "queries": int(o[1]), "passes": int(o[2]), "exclusive": int(o[3])}

    def recommend_set_depth(self, passes_in_flight):
        self._chk(self._L.mals_recommend_set_depth(self._h, int(passes_in_flight)))

    def recommend_set_spin_us(self, spin_us):
        self._chk(self._L.mals_recommend_set_spin_us(self._h, int(spin_us)))

    def recommend_to_many(self, queries, how_many, exclude=None, rescorer=None):
        """recommendToMany (ServerRecommender.java:366-441): queries = list of (n_j x features) arrays, one per query; the
        score of an item is the mean of its dots with the query's vectors (RecommendIterator.java:93-104)."""
        qs = [np.ascontiguousarray(np.atleast_2d(_host(q, np.float32))) for q in queries]
        assert all(q.shape[1] == self.features for q in qs)
        vptr = np.zeros(len(qs) + 1, dtype=np.int64)
        vptr[1:] = np.cumsum([len(q) for q in qs])
        flatv = np.ascontiguousarray(np.concatenate(qs, axis=0)) if qs else np.zeros((0, self.features), np.float32)
        idx = np.empty((len(qs), how_many), dtype=np.int64)
        sc = np.empty((len(qs), how_many), dtype=np.float32)
        cnt = np.empty(len(qs), dtype=np.int32)
        ep = ei = None
        if exclude is not None:
            ptr = np.zeros(len(qs) + 1, dtype=np.int64)
            ptr[1:] = np.cumsum([len(e) for e in exclude])
            flat = np.ascontiguousarray(np.concatenate([np.asarray(e, np.int64) for e in exclude]) if ptr[-1] else np.zeros(0, np.int64))
            ep, ei = ptr.ctypes.data_as(ctypes.c_void_p), flat.ctypes.data_as(ctypes.c_void_p)
            self._keep[("excl",)] = (ptr, flat)
        args = (flatv.ctypes.data_as(ctypes.c_void_p), vptr.ctypes.data_as(ctypes.c_void_p), len(qs), int(how_many), ep, ei,
                idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p))
        if rescorer is None:
            self._chk(self._L.mals_recommend_to_many(self._h, *args))
        else:
            self._chk(self._L.mals_recommend_to_many_rescored(self._h, rescorer.handle, *args))
        return idx, sc, cnt

    def most_similar_items(self, items, how_many, rescorer=None, filter_query_items=False):
        """mostSimilarItems (ServerRecommender.java:1171-1266): items = a sequence of item indices (one item per query) or a
        list of sequences (several items per query); the score is the mean cosine to the query's items
        (MostSimilarItemIterator.java:73-120).  Returns (item_idx [q][how_many] int64, scores float32, counts).
        rescorer: a Rescorer of this handle used as the Rescorer<LongPair> (None: none): a candidate in its filter set is
        skipped -- with filter_query_items also every candidate of a query that has a filtered query item ("either end of the
        pair") -- and every cosine is rescored scale_c * s + offset_c before the mean."""
        flat, ptr = _item_queries(items)
        idx = np.empty((len(ptr) - 1, how_many), dtype=np.int64)
        sc = np.empty((len(ptr) - 1, how_many), dtype=np.float32)
        cnt = np.empty(len(ptr) - 1, dtype=np.int32)
        args = (flat.ctypes.data_as(ctypes.c_void_p), ptr.ctypes.data_as(ctypes.c_void_p), len(ptr) - 1, int(how_many),
                idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p))
        if rescorer is None:
            self._chk(self._L.mals_most_similar_items(self._h, *args))
        else:
            flags = _lib.SIMILAR_FILTER_QUERY_ITEMS if filter_query_items else 0
            self._chk(self._L.mals_most_similar_items_rescored(self._h, rescorer.handle, flags, *args))
        return idx, sc, cnt

    def similar_stats(self):
        """{filter, dense, empty, rescored}: mostSimilarItems queries answered by the filter path, by the dense path, answered
        empty by a filter pass before scoring, and the rescored ones among them, since the handle was created."""
        o = np.zeros(4, dtype=np.int64)
        self._chk(self._L.mals_similar_stats(self._h, o.ctypes.data_as(ctypes.c_void_p)))
        return {"filter": int(o[0]), "dense": int(o[1]), "empty": int(o[2]), "rescored": int(o[3])}

    def similarity_to_item(self, to_item, items):
        """similarityToItem (ServerRecommender.java:1268-1304): the cosine of every item to to_item, NaN as NaN."""
        ii = _host(items, np.int64)
        out = np.empty(len(ii), dtype=np.float32)
        self._chk(self._L.mals_similarity_to_item(self._h, int(to_item), ii.ctypes.data_as(ctypes.c_void_p), len(ii),
                                                  out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def recommended_because(self, users, items, how_many):
        """recommendedBecause (ServerRecommender.java:1324-1376): per query (users[q], items[q]) the user's known items most
        similar to the item, best first.  Returns (item_idx, scores, counts)."""
        u = _host(users, np.int64)
        ii = _host(items, np.int64)
        assert len(u) == len(ii)
        idx = np.empty((len(u), how_many), dtype=np.int64)
        sc = np.empty((len(u), how_many), dtype=np.float32)
        cnt = np.empty(len(u), dtype=np.int32)
        self._chk(self._L.mals_recommended_because(self._h, u.ctypes.data_as(ctypes.c_void_p), ii.ctypes.data_as(ctypes.c_void_p), len(u),
                                                   int(how_many), idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p),
                                                   cnt.ctypes.data_as(ctypes.c_void_p)))
        return idx, sc, cnt

    # -- the online write path (setPreference / removePreference and the fold-in reads) ---------------------------
    def set_foldin_solver(self, side, solver):
        """The generation's solver of side's M^T M (HostSolver, or None to clear) for the writes and fold-in reads."""
        self._chk(self._L.mals_set_foldin_solver(self._h, side, solver._s if solver is not None else None))

    def set_foldin_learn_rate(self, rate):
        self._chk(self._L.mals_set_foldin_learn_rate(self._h, float(rate)))

    def foldin_stats(self):
        """Counters of mals_set_preferences since the handle was created; device_ms: HIP-event time of the level kernels (all
        calls / the last call)."""
        o = np.zeros(6, dtype=np.int64)
        self._chk(self._L.mals_foldin_stats(self._h, o.ctypes.data_as(ctypes.c_void_p)))
        return {"applied": int(o[0]), "failed": int(o[1]), "big_foldin": int(o[2]), "levels": int(o[3]),
                "device_ms_total": o[4] * 1e-6, "device_ms_last": o[5] * 1e-6}

    def foldin_solve(self, side, b):
        """Solver.solveFToD on the device with side's fold-in solver, for the rows of b (n x features float32)."""
        b = np.ascontiguousarray(np.atleast_2d(_host(b, np.float32)))
        x = np.empty(b.shape, dtype=np.float64)
        self._chk(self._L.mals_foldin_solve(self._h, side, b.ctypes.data_as(ctypes.c_void_p), len(b), x.ctypes.data_as(ctypes.c_void_p)))
        return x

    def set_preferences(self, users, items, values, raise_on_error=True):
        """setPreference for each (users[t], items[t], values[t]) in order.  Returns the per-update status array; raises on
        the first failed update unless raise_on_error is False."""
        u, i, v = _host(users, np.int64), _host(items, np.int64), _host(values, np.float32)
        assert len(u) == len(i) == len(v)
        st = np.zeros(len(u), dtype=np.int32)
        rc = self._L.mals_set_preferences(self._h, len(u), u.ctypes.data_as(ctypes.c_void_p), i.ctypes.data_as(ctypes.c_void_p),
                                          v.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p))
        if raise_on_error or rc not in (_lib.OK, _lib.INVALID_ARG) or not st.any():
            self._chk(rc)
        return st

    def _set_tags(self, fn, users, items, values, raise_on_error):
        u, i, v = _host(users, np.int64), _host(items, np.int64), _host(values, np.float32)
        assert len(u) == len(i) == len(v)
        st = np.zeros(len(u), dtype=np.int32)
        rc = fn(self._h, len(u), u.ctypes.data_as(ctypes.c_void_p), i.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p),
                st.ctypes.data_as(ctypes.c_void_p))
        if raise_on_error or rc not in (_lib.OK, _lib.INVALID_ARG) or not st.any():
            self._chk(rc)
        return st

    def set_user_tags(self, users, tag_items, values, raise_on_error=True):
        """setUserTag for each (users[t], tag_items[t], values[t]) in order: tag_items are the tags' rows of Y (the row of
        tag_id(tag) on side Y).  The rows join the userTagIDs whatever their updates' statuses; no known item is added."""
        return self._set_tags(self._L.mals_set_user_tags, users, tag_items, values, raise_on_error)

    def set_item_tags(self, tag_users, items, values, raise_on_error=True):
        """setItemTag for each (tag_users[t], items[t], values[t]) in order: tag_users are the tags' rows of X."""
        return self._set_tags(self._L.mals_set_item_tags, tag_users, items, values, raise_on_error)

    def tag_rows(self, side):
        """The tag sets as they stand, ascending: SIDE_Y the userTagIDs as rows of Y, SIDE_X the itemTagIDs as user rows."""
        n = ctypes.c_int64(0)
        self._chk(self._L.mals_get_tag_rows(self._h, side, None, 0, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.int64)
        if n.value:
            self._chk(self._L.mals_get_tag_rows(self._h, side, out.ctypes.data_as(ctypes.c_void_p), len(out), ctypes.byref(n)))
        return out[:n.value]

    def remove_preferences(self, users, items):
        """removePreference for each pair in order.  Returns the user rows that lost their last known item (zeroed)."""
        u, i = _host(users, np.int64), _host(items, np.int64)
        assert len(u) == len(i)
        out = np.zeros(max(len(u), 1), dtype=np.int64)
        n = ctypes.c_int64(0)
        self._chk(self._L.mals_remove_preferences(self._h, len(u), u.ctypes.data_as(ctypes.c_void_p), i.ctypes.data_as(ctypes.c_void_p),
                                                  out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)))
        return out[:n.value].copy()

    def grow_factor_rows(self, side, n_rows_total):
        self._chk(self._L.mals_grow_factor_rows(self._h, side, int(n_rows_total)))

    def set_ids(self, side, ids):
        """mals_ids_set: the ids of rows [0, n) of `side` (numpy, or a torch int64 CUDA tensor), one per row of its replica; an
        empty array clears the side.  A duplicate id raises (the message names the row) and nothing changes."""
        if _is_torch(ids):
            assert ids.is_cuda and str(ids.dtype) == "torch.int64"
            d = ids.contiguous()
            self._chk(self._L.mals_ids_set(self._h, side, int(d.numel()), ctypes.c_void_p(d.data_ptr()) if d.numel() else None, MEM_DEVICE))
        else:
            a = _host(ids, np.int64)
            self._chk(self._L.mals_ids_set(self._h, side, len(a), a.ctypes.data_as(ctypes.c_void_p) if len(a) else None, MEM_HOST))

    def rows_of(self, side, ids, add=False):
        """The row of each id (-1: unknown).  add=True (mals_ids_resolve): an unknown id gets a new row, numbered in order of
        first appearance in `ids`, and the replica grows; returns (rows, rows added)."""
        a = _host(ids, np.int64)
        rows = np.empty(len(a), dtype=np.int64)
        if not add:
            self._chk(self._L.mals_ids_lookup(self._h, side, len(a), a.ctypes.data_as(ctypes.c_void_p), rows.ctypes.data_as(ctypes.c_void_p)))
            return rows
        n_new = ctypes.c_int64(0)
        self._chk(self._L.mals_ids_resolve(self._h, side, len(a), a.ctypes.data_as(ctypes.c_void_p), rows.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.byref(n_new)))
        return rows, n_new.value

    def ids_of(self, side, row_begin=0, n=None):
        """The ids of rows [row_begin, row_begin + n) (n=None: to the last row)."""
        if n is None:
            c = ctypes.c_int64(0)
            self._chk(self._L.mals_ids_count(self._h, side, ctypes.byref(c)))
            n = c.value - int(row_begin)
        out = np.empty(max(int(n), 0), dtype=np.int64)
        self._chk(self._L.mals_ids_get(self._h, side, int(row_begin), int(n), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def ingest_apply_times(self):
        """mals_ingest_apply_times: ms of the last Ingest.apply on this handle, by stage."""
        out = np.zeros(4, dtype=np.float64)
        self._chk(self._L.mals_ingest_apply_times(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return dict(zip(("ids_ms", "plan_ms", "writes_ms", "total_ms"), out.tolist()))

    def ingest_apply_tag_stats(self):
        """mals_ingest_apply_tag_stats: the tag lines of the last Ingest.apply on this handle."""
        out = np.zeros(4, dtype=np.int64)
        self._chk(self._L.mals_ingest_apply_tag_stats(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return dict(zip(("item_tag_sets", "user_tag_sets", "tag_removes_ignored", "rows_marked"), (int(x) for x in out)))

    def estimate_preferences(self, users, items):
        u, i = _host(users, np.int64), _host(items, np.int64)
        out = np.empty(len(u), dtype=np.float32)
        self._chk(self._L.mals_estimate_preferences(self._h, len(u), u.ctypes.data_as(ctypes.c_void_p), i.ctypes.data_as(ctypes.c_void_p),
                                                    out.ctypes.data_as(ctypes.c_void_p)))
        return out

    @staticmethod
    def _anon_args(queries, values):
        flat, ptr = _item_queries(queries)
        vals = None
        if values is not None:
            vals = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float32).ravel() for v in values]) if len(flat) else np.zeros(0, np.float32))
            assert len(vals) == len(flat)
        return flat, ptr, vals

    def anonymous_features(self, queries, values=None, raise_on_error=True):
        """buildAnonymousUserFeatures per query (a list of item-row lists, -1 = unknown item): (features [q][k], status)."""
        flat, ptr, vals = self._anon_args(queries, values)
        nq = len(ptr) - 1
        out = np.zeros((nq, self.features), dtype=np.float32)
        st = np.zeros(nq, dtype=np.int32)
        rc = self._L.mals_anonymous_features(self._h, nq, ptr.ctypes.data_as(ctypes.c_void_p), flat.ctypes.data_as(ctypes.c_void_p),
                                             vals.ctypes.data_as(ctypes.c_void_p) if vals is not None else None,
                                             out.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p))
        if raise_on_error or not st.any():
            self._chk(rc)
        return out, st

    def recommend_to_anonymous(self, queries, how_many, values=None, rescorer=None):
        """recommendToAnonymous: (item_idx, scores, counts, status) per query; rescorer: a Rescorer."""
        flat, ptr, vals = self._anon_args(queries, values)
        nq = len(ptr) - 1
        idx = np.empty((nq, how_many), dtype=np.int64)
        sc = np.empty((nq, how_many), dtype=np.float32)
        cnt = np.empty(nq, dtype=np.int32)
        st = np.zeros(nq, dtype=np.int32)
        args = (nq, ptr.ctypes.data_as(ctypes.c_void_p), flat.ctypes.data_as(ctypes.c_void_p),
                vals.ctypes.data_as(ctypes.c_void_p) if vals is not None else None, int(how_many),
                idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p),
                cnt.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p))
        if rescorer is None:
            rc = self._L.mals_recommend_to_anonymous(self._h, *args)
        else:
            rc = self._L.mals_recommend_to_anonymous_rescored(self._h, rescorer.handle, *args)
        if not st.any():
            self._chk(rc)
        return idx, sc, cnt, st

    def estimate_for_anonymous(self, to_items, queries, values=None):
        """estimateForAnonymous per query: (float32 estimates, status)."""
        flat, ptr, vals = self._anon_args(queries, values)
        nq = len(ptr) - 1
        to = _host(to_items, np.int64)
        assert len(to) == nq
        out = np.zeros(nq, dtype=np.float32)
        st = np.zeros(nq, dtype=np.int32)
        rc = self._L.mals_estimate_for_anonymous(self._h, nq, to.ctypes.data_as(ctypes.c_void_p), ptr.ctypes.data_as(ctypes.c_void_p),
                                                 flat.ctypes.data_as(ctypes.c_void_p), vals.ctypes.data_as(ctypes.c_void_p) if vals is not None else None,
                                                 out.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p))
        if not st.any():
            self._chk(rc)
        return out, st

    # -- a new generation into the live handle (GenerationLoader.loadModel) -----------------------------------------
    def mark_recent(self, side, rows):
        """mals_mark_recent: rows of `side` written elsewhere since the last load (recentlyActiveUsers / Items)."""
        r = _host(rows, np.int64)
        self._chk(self._L.mals_mark_recent(self._h, side, len(r), r.ctypes.data_as(ctypes.c_void_p) if len(r) else None))

    def get_recent(self, side):
        """mals_get_recent: the rows of `side` written since the last load, ascending."""
        n = ctypes.c_int64(0)
        self._chk(self._L.mals_get_recent(self._h, side, None, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.int64)
        if n.value:
            self._chk(self._L.mals_get_recent(self._h, side, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)))
        return out[:n.value]

    def load_generation(self, cur_user_ids, cur_item_ids, new_user_ids, new_item_ids, new_X, new_Y, new_known=None,
                        item_tag_ids=None, user_tag_ids=None, keep_not_updated=False, recompute_solvers=False):
        """mals_load_generation: merge a new model into the generation this handle serves, by id, keeping the live rows
        written since the last load.  cur_*_ids: the id of every live row (both numpy, or both torch CUDA int64).  The new model -- ids, X, Y, new_known =
        (row_ptr, item_idx) over the new users or None, the two updated tag-id sets -- is all numpy or all torch CUDA
        tensors (int64 ids and offsets, float32 rows, int32 item indices).  Returns (result dict, (merged user ids, merged
        item ids), (user map, item map)): map[r] = the merged row of live row r, -1 = pruned."""
        out = _load_generation(self.features, lambda L, R: self._chk(self._L.mals_load_generation(self._h, L, R)),
                               lambda side, p: self._chk(self._L.mals_generation_get_ids(self._h, side, p)),
                               lambda side, p: self._chk(self._L.mals_generation_get_map(self._h, side, p)),
                               cur_user_ids, cur_item_ids, new_user_ids, new_item_ids, new_X, new_Y, new_known, item_tag_ids, user_tag_ids,
                               keep_not_updated, recompute_solvers)
        for side in (SIDE_X, SIDE_Y):     # the replicas and matrices are the library's own from here on
            self._keep.pop(("F", side), None)
            self._keep.pop(("M", side), None)
        return out

    def factor_digest(self, side, row_begin=0, n_rows=None):
        """mals_factor_digest: the 64-bit digest of rows [row_begin, row_begin + n_rows) of side's replica, computed on the
        device between two writes (n_rows None: to the end).  Equals factor_digest_host of the same rows."""
        if n_rows is None:
            n_rows = self.factor_device_ptr(side)[1] - int(row_begin)
        out = ctypes.c_uint64(0)
        self._chk(self._L.mals_factor_digest(self._h, side, int(row_begin), int(n_rows), ctypes.byref(out)))
        return out.value

    def reconstruction_error(self):
        """ReconstructionEvaluator's sum and count over the local user rows (mean = sum / count)."""
        sm, cnt = ctypes.c_double(0.0), ctypes.c_int64(0)
        self._chk(self._L.mals_reconstruction_error(self._h, ctypes.byref(sm), ctypes.byref(cnt)))
        return sm.value, cnt.value

    def recompute_solver(self, side):
        """Generation.recomputeSolver (Generation.java:142-158) for `side`'s factors.  Returns
        (HostSolver or None for an empty side, norm)."""
        s, norm = ctypes.c_void_p(), ctypes.c_double(0.0)
        rc = self._L.mals_recompute_solver(self._h, side, ctypes.byref(s), ctypes.byref(norm))
        if rc == _lib.ILL_CONDITIONED:
            msg = (self._L.mals_last_error(self._h) or b"").decode("utf-8", "replace")
            raise IllConditioned(rc, msg, norm.value)
        self._chk(rc)
        return (HostSolver(self._L, s) if s.value else None), norm.value

    # -- stats ------------------------------------------------------------------------------------
    def enable_timing(self, on=True):
        self._chk(self._L.mals_enable_timing(self._h, 1 if on else 0))

    def reset_stats(self):
        self._chk(self._L.mals_reset_stats(self._h))

    def sample_dots(self, test_users, test_items):
        """est[i, j] = SimpleVectorMath.dot(X[test_users[i]], Y[test_items[j]]) from the resident factors."""
        tu = _host(test_users, np.int64)
        ti = _host(test_items, np.int64)
        out = np.empty((len(tu), len(ti)), dtype=np.float64)
        self._chk(self._L.mals_sample_dots(self._h, tu.ctypes.data_as(ctypes.c_void_p), len(tu), ti.ctypes.data_as(ctypes.c_void_p),
                                           len(ti), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def timeline(self):
        """mals_get_timeline: host microseconds [first kernel of the half-iteration enqueued, eigendecomposition begin, end, -]."""
        out = (ctypes.c_double * 4)()
        self._chk(self._L.mals_get_timeline(self._h, out))
        return list(out)

    def gather_scale(self):
        """mals_get_gather_scale: [S, 1/S^2, range flag, bound on |y| used] of the last half-iteration's split-precision gather."""
        out = (ctypes.c_float * 4)()
        self._chk(self._L.mals_get_gather_scale(self._h, out))
        return list(out)

    def set_refine_limit(self, limit):
        """mals_set_refine_limit: conditioning estimate above which a row is re-solved with fp64 residuals (0 = never)."""
        self._chk(self._L.mals_set_refine_limit(self._h, float(limit)))

    def stats(self):
        st = _lib.Stats()
        self._chk(self._L.mals_get_stats(self._h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in _lib.Stats._fields_ if name not in ("struct_size", "reserved")}


__all__ = ["ALSCore", "HostSolver", "factor_digest_host", "generation_hash_host", "generation_join_host", "MalsError", "SingularSystem", "Cancelled", "IllConditioned", "SIDE_X", "SIDE_Y",
           "FLAG_RECONSTRUCT_R", "FLAG_LOSS_IGNORES_UNSPECIFIED"]
