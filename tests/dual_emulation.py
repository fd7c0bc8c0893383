"""numpy restatement of the dual ("short row") solve path of csrc/dual_kernels.h, arithmetic step by step:
fp64 eigendecomposition of G, fp32 rotated rows, the d_f(n) table, the power-of-two operand scale, operands split
into two f16 halves (both rounded to nearest, as v_cvt_pk_f16_f32 does in the kernel), S = I + Z Z^T from the three
exact products in fp32, fp32 Cholesky + solves, x' = D^1/2 Z^T v, x = Q x'.  Test infrastructure (CPU): checked
against the oracle in tests/test_dual_emulation.py so that the ALGORITHM is validated without a GPU.

The two rotations exist in every arithmetic the library can run them in (prepare_dual_host, csrc/mals_api.hip):
  forward  "fp64" (rotate_rows_kernel<T,false,true>, the default here), "fp32" (rotate_rows_kernel<T,false,false>),
           "split" (rotate_rows_split_kernel<T,false>);
  back     "fp64" (no kernel: the default here, as before), "fp32" (rotate_rows_kernel<T,true,false>),
           "split" (rotate_rows_split_kernel<T,true>, its operand scale from the largest |x'| of the rows it takes together).
tests/test_dual_cases.py derives the bar of tests/test_gpu_dual_exact.py from these."""
import numpy as np

FORWARD = ("fp64", "fp32", "split")
BACK = ("fp64", "fp32", "split")


def split22(z):
    """z (fp32) -> (hi, lo): hi = z rounded to f16, lo = the exact residual z - hi rounded to f16 (pk_rn16 in the kernels;
    the operand scale keeps both inside f16's normal range)."""
    z = z.astype(np.float32)
    hi = z.astype(np.float16).astype(np.float32)
    lo = (z - hi).astype(np.float32).astype(np.float16).astype(np.float32)
    return hi, lo


def split_toward_zero(v):
    """v (fp32) -> (hi, lo) as split_rotation_operand (csrc/mals_api.hip) splits Q: hi = v rounded to f16 TOWARD ZERO, lo = the
    residual rounded to nearest."""
    v = v.astype(np.float32)
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v)
    hi = (h.view(np.uint16) - over.astype(np.uint16)).view(np.float16).astype(np.float32)   # f16 magnitudes order like their bits
    lo = (v - hi).astype(np.float32).astype(np.float16).astype(np.float32)
    return hi, lo


def power_below_2_14(bound, clamp):
    """pw with bound * 2^pw < 2^14 (the kernels read the exponent field: bound < 2^e), 0 for no bound."""
    bound = np.float32(bound)
    if not bound > 0:
        return 0
    _, e = np.frexp(bound)
    return int(np.clip(14 - int(e), -clamp, clamp))


def rotate(A, B, mode, bound=None):
    """rows A (fp32 [R, k]) times B (fp64 [k, k]), rounded to fp32, in one of the three arithmetics.
    "fp32": fp32 operands, one rounding per product added (v_mfma_f32_16x16x4_f32 up to the order inside a step);
    "split": rows times 2^pw below 2^14 as two f16 halves, B times 2^13 as two f16 halves (hi toward zero), the three
    exact products summed into an fp32 result (rotate_rows_split_kernel); bound: a bound on |A|."""
    A = A.astype(np.float32)
    if mode == "fp64":
        return (A.astype(np.float64) @ B).astype(np.float32)
    if mode == "fp32":
        Bf = B.astype(np.float32).astype(np.float64)
        acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
        for f in range(A.shape[1]):
            acc = (acc.astype(np.float64) + A[:, f:f + 1].astype(np.float64) * Bf[f][None, :]).astype(np.float32)
        return acc
    if mode == "split":
        pw = power_below_2_14(bound, 100)
        ah, al = (h.astype(np.float64) for h in split22(A * np.float32(2.0 ** pw)))
        bh, bl = (h.astype(np.float64) for h in split_toward_zero((B * 8192.0).astype(np.float32)))
        acc = (ah @ bh + ah @ bl + al @ bh).astype(np.float32)
        return (acc * np.float32(2.0 ** (-pw - 13))).astype(np.float32)
    raise KeyError(mode)


def prepare(M, alpha, lam, eigh=np.linalg.eigh, forward="fp64"):
    """Once per half-iteration: G = M^T M (fp64), its eigendecomposition, the rotated copy, the z bound."""
    G = M.astype(np.float64).T @ M.astype(np.float64)
    L, Q = eigh(G)
    L = np.maximum(L, 0.0)
    # the split rotation's bound on |y|: sqrt(max_f G_ff), known to the host
    Mr = rotate(M, Q, forward, bound=np.float32(np.sqrt(np.diag(G).max())) if len(M) else None)
    dmax = (1.0 / np.sqrt(L + lam * alpha)).astype(np.float32)
    zbound = np.float32(np.max(np.abs(Mr) * dmax[None, :])) if len(M) else np.float32(0)
    return {"G": G, "L": L.astype(np.float32), "Q": Q, "Mr": Mr, "zbound": zbound}


def solve_row_rotated(prep, cols, vals, alpha, lam, w_max_sqrt, drop_low_half=False):
    """x' (fp32 [k], the rotated coordinates als_dual_kernel stores) of one row with n <= k entries.
    drop_low_half: the S products on zh alone -- what a kernel that lost the low f16 half of Z would form."""
    n = len(cols)
    k = prep["Mr"].shape[1]
    if n == 0:
        return np.zeros(k, dtype=np.float32)
    d = (np.float32(1.0) / np.sqrt(prep["L"] + np.float32(lam * alpha) * np.float32(n))).astype(np.float32)
    ar = (np.float32(alpha) * np.abs(vals.astype(np.float32))).astype(np.float32)
    w = np.sqrt(ar).astype(np.float32)
    cb = np.where(vals > 0, np.float32(1) + ar, np.float32(0)).astype(np.float32)
    q = np.where(w > 0, cb / np.where(w > 0, w, 1), 0).astype(np.float32)
    bound = np.float32(prep["zbound"]) * np.float32(w_max_sqrt)
    pw = 0 if not bound > 0 else int(np.clip(14 - int(np.floor(np.log2(bound)) + 1), -60, 60))
    sc = np.float32(2.0 ** pw)
    Y = prep["Mr"][cols]
    Z = ((Y * d[None, :]).astype(np.float32) * (w * sc)[:, None]).astype(np.float32)
    zh, zl = split22(Z)
    zh64, zl64 = zh.astype(np.float64), zl.astype(np.float64)
    if drop_low_half:
        S = (zh64 @ zh64.T).astype(np.float32)
    else:
        S = (zh64 @ zh64.T + zh64 @ zl64.T + zl64 @ zh64.T).astype(np.float32)       # exact products, fp32 result
    S = (S * np.float32(2.0 ** (-2 * pw))).astype(np.float32) + np.eye(n, dtype=np.float32)
    Lc = np.linalg.cholesky(S.astype(np.float32)).astype(np.float32)
    v = np.linalg.solve(Lc.astype(np.float32), q).astype(np.float32)
    v = np.linalg.solve(Lc.T.astype(np.float32), v).astype(np.float32)
    return (((zh + zl).astype(np.float32).T @ v).astype(np.float32) * d * np.float32(2.0 ** (-pw))).astype(np.float32)


def solve_row(prep, cols, vals, alpha, lam, w_max_sqrt):
    """One row with n <= k entries."""
    xp = solve_row_rotated(prep, cols, vals, alpha, lam, w_max_sqrt)
    return (prep["Q"] @ xp.astype(np.float64)).astype(np.float32)


def solve_rows(prep, rows, alpha, lam, w_max_sqrt, back="fp64", drop_low_half=False):
    """rows: list of (cols, vals), un-rotated TOGETHER (one launch of the un-rotation: one operand scale).  fp32 [R, k]."""
    Xp = np.stack([solve_row_rotated(prep, c, v, alpha, lam, w_max_sqrt, drop_low_half) for c, v in rows])
    return rotate(Xp, prep["Q"].T, back, bound=np.float32(np.abs(Xp).max()))
