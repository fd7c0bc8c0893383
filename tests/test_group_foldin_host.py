"""The host side of the group write path: the replica digest's definition (include/myrrix_als.h) pinned against a numpy
restatement, and the argument checks of every new entry point that need no device."""
import ctypes

import numpy as np
import pytest

import myrrix_recommender_amd as pkg
from myrrix_recommender_amd import _lib

M64 = (1 << 64) - 1
C_INDEX = np.uint64(0x9E3779B97F4A7C15)
C_MIX = np.uint64(0xD6E8FEB86659FD93)


def digest_numpy(rows, row_begin=0):
    """The header's formula, element by element in uint64 arithmetic (numpy wraps modulo 2^64)."""
    rows = np.ascontiguousarray(rows, np.float32)
    k = rows.shape[1]
    bits = rows.view(np.uint32).ravel().astype(np.uint64)
    j = np.arange(rows.size, dtype=np.uint64) + np.uint64(row_begin * k)
    with np.errstate(over="ignore"):
        z = j * C_INDEX + bits
        z ^= z >> np.uint64(32)
        z *= C_MIX
        z ^= z >> np.uint64(32)
        return int(z.sum(dtype=np.uint64))


def from_bits(bits, k):
    return np.asarray(bits, np.uint32).view(np.float32).reshape(-1, k)


@pytest.mark.parametrize("k", [1, 2, 30, 50, 64, 128])
def test_host_digest_is_the_headers_formula(k):
    rng = np.random.default_rng(k)
    rows = from_bits(rng.integers(0, 1 << 32, 37 * k, dtype=np.uint64).astype(np.uint32), k)   # random bits: NaNs, denormals, all of it
    assert pkg.factor_digest_host(rows) == digest_numpy(rows)
    for row_begin in (1, 3, 7, 1001):                                                           # row_begin * k no multiple of 4 at k = 1, 2, 30, 50
        assert pkg.factor_digest_host(rows, row_begin) == digest_numpy(rows, row_begin), row_begin
    assert pkg.factor_digest_host(rows, 3) != pkg.factor_digest_host(rows, 0)
    assert pkg.factor_digest_host(rows[:0]) == 0


def test_host_digest_sees_signed_zeros_nan_payloads_and_infinities():
    special = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800000, 0xFF800000, 0x7F800001], np.uint32)
    rows = from_bits(special, 2)
    assert pkg.factor_digest_host(rows) == digest_numpy(rows)
    seen = set()
    for b in special:                                    # the same place, another bit pattern: another digest
        one = rows.copy()
        one.view(np.uint32)[1, 1] = b
        seen.add(pkg.factor_digest_host(one))
    assert len(seen) == len(special)


def test_ranges_add_up_and_rows_have_places():
    rng = np.random.default_rng(1)
    k = 30
    rows = rng.standard_normal((41, k)).astype(np.float32)
    whole = pkg.factor_digest_host(rows, 5)
    for cut in (0, 1, 17, 40, 41):
        assert (pkg.factor_digest_host(rows[:cut], 5) + pkg.factor_digest_host(rows[cut:], 5 + cut)) & M64 == whole
    swapped = rows.copy()
    swapped[[3, 29]] = swapped[[29, 3]]
    assert not np.array_equal(swapped[3], swapped[29])
    assert pkg.factor_digest_host(swapped, 5) != whole


def test_every_single_bit_flip_changes_the_digest():
    rng = np.random.default_rng(2)
    rows = rng.standard_normal((7, 30)).astype(np.float32)
    base = pkg.factor_digest_host(rows)
    bits = rows.view(np.uint32)
    flips = 0
    for r in range(7):
        for f in range(30):
            for b in range(32):
                bits[r, f] ^= np.uint32(1 << b)
                assert pkg.factor_digest_host(rows) != base, (r, f, b)
                bits[r, f] ^= np.uint32(1 << b)
                flips += 1
    assert flips == 6720 and pkg.factor_digest_host(rows) == base


def test_null_handles_are_refused_without_a_device():
    L = _lib.load()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    out64 = ctypes.c_uint64(0)
    n64 = ctypes.c_int64(0)
    eq = ctypes.c_int32(0)
    calls = {
        "mals_group_set_foldin_solver": (None, 0, None),
        "mals_group_set_foldin_learn_rate": (None, 1.0),
        "mals_group_foldin_stats": (None, p),
        "mals_group_set_preferences": (None, 1, p, p, p, p),
        "mals_group_remove_preferences": (None, 1, p, p, p, ctypes.byref(n64)),
        "mals_group_grow_factor_rows": (None, 0, 10),
        "mals_group_estimate_preferences": (None, 1, p, p, p),
        "mals_group_anonymous_features": (None, 1, p, p, p, p, p),
        "mals_group_recommend_to_anonymous": (None, 1, p, p, p, 1, p, p, p, p),
        "mals_group_estimate_for_anonymous": (None, 1, p, p, p, p, p, p),
        "mals_factor_digest": (None, 0, 0, 1, ctypes.byref(out64)),
        "mals_group_replica_digest": (None, 0, 0, 1, p, ctypes.byref(eq)),
    }
    for name, args in calls.items():
        assert getattr(L, name)(*args) == _lib.INVALID_ARG, name
    # the host digest has no handle: its own argument checks
    assert L.mals_factor_digest_host(None, 4, 0, 1, ctypes.byref(out64)) == _lib.INVALID_ARG
    assert L.mals_factor_digest_host(p, 0, 0, 1, ctypes.byref(out64)) == _lib.INVALID_ARG
    assert L.mals_factor_digest_host(p, 4, -1, 1, ctypes.byref(out64)) == _lib.INVALID_ARG
    assert L.mals_factor_digest_host(p, 4, 0, 1, None) == _lib.INVALID_ARG
    assert set(calls) | {"mals_factor_digest_host"} <= set(_lib.SYMBOLS)
