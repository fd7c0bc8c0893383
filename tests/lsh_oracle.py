"""CPU restatement of the reference's candidate filter, LocationSensitiveHash (online/src/net/myrrix/online/candidate/
LocationSensitiveHash.java), written from the Java text: what mals_lsh_* (include/myrrix_als.h, csrc/lsh_kernels.h) must
reproduce bit for bit.  numpy fp64 performs the same IEEE additions and subtractions, in the same order, as the Java."""
import math

import numpy as np


def max_bits_differing(sample_ratio, num_hashes):
    """LSH:98-108.  ArithmeticUtils.binomialCoefficientDouble(n, k) is the exact binomial for n <= 66, as a double."""
    cumulative = 0.0
    denominator = 2.0 ** num_hashes
    bits = -1
    while bits < num_hashes and cumulative < sample_ratio:
        bits += 1
        cumulative += float(math.comb(num_hashes, bits)) / denominator
    return bits - 1


def find_mean(Y):
    """LSH:154-167 with the rows in index order (the reference's order is its hash map's): fp64 sums of the fp32 rows,
    divided by the row count."""
    Y = np.asarray(Y, np.float32)
    total = np.zeros(Y.shape[1], np.float64)
    for row in Y:
        total += row.astype(np.float64)
    return total / float(len(Y))


def totals(vectors, random_vectors, mean):
    """The `total` of toBitSignature (LSH:172-182) per (vector, hash): starts at 0.0; per feature, in order,
    delta = (double) v[f] - mean[f], then total += delta or total -= delta."""
    V = np.asarray(vectors, np.float32)
    rv = np.asarray(random_vectors, bool)
    mean = np.asarray(mean, np.float64)
    delta = V.astype(np.float64) - mean[None, :]                     # [n][features]
    tot = np.zeros((len(V), len(rv)), np.float64)
    for f in range(V.shape[1]):
        d = delta[:, f][:, None]
        tot = np.where(rv[None, :, f], tot + d, tot - d)
    return tot


def signatures(vectors, random_vectors, mean):
    """toBitSignature (LSH:169-190): per hash in order l = (l << 1) | (total > 0.0) -- hash 0 ends up the most
    significant of the num_hashes bits."""
    tot = totals(vectors, random_vectors, mean)
    sig = np.zeros(len(tot), np.uint64)
    for h in range(tot.shape[1]):
        sig = (sig << np.uint64(1)) | (tot[:, h] > 0.0).astype(np.uint64)
    return sig


def popcount(x):
    x = np.asarray(x, np.uint64)
    out = np.zeros(x.shape, np.int64)
    for b in range(64):
        out += ((x >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return out


def candidates(item_signatures, query_signatures, max_bits, n_items=None):
    """getCandidateIterator (LSH:193-216): item i is a candidate iff bitCount(sig_i ^ sig_j) <= maxBitsDiffering for ANY of
    the query's signatures; the items past the signed ones (new items, LSH:208-213) always are.  Returns a bool mask over
    n_items (default: the signed items)."""
    isig = np.asarray(item_signatures, np.uint64)
    n_items = len(isig) if n_items is None else n_items
    ok = np.zeros(n_items, bool)
    for s in np.atleast_1d(np.asarray(query_signatures, np.uint64)):
        ok[:len(isig)] |= popcount(isig ^ s) <= max_bits
    ok[len(isig):] = True
    return ok


def non_candidates(item_signatures, query_signatures, max_bits, n_items=None):
    """The items a query does NOT see, as indices: what a test adds to the exclusions of oracle.topn_oracle.recommend."""
    return np.flatnonzero(~candidates(item_signatures, query_signatures, max_bits, n_items))
