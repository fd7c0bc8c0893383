// foldin_kernels.h -- gfx950 kernels of the online write path (mals_set_preferences, mals_anonymous_features,
// mals_estimate_preferences; include/myrrix_als.h): ServerRecommender.updateFeatures (online/src/net/myrrix/online/
// ServerRecommender.java:865-912), buildAnonymousUserFeatures (:561-609) and estimatePreferences (:690-727), in the
// reference's arithmetic, bit for bit.
//
// The fold-in solve x = A^-1 b of a generation's solver (Solver.solveFToD) restates mals::PivotedQR::solve
// (host_solver.h) operation for operation: the reflectors H_j in order (tau_j == 0 skipped), every sum in ascending row
// order, back substitution with the same division, then the pivot scatter.  hipcc contracts a*b + c into v_fma_f64 on the
// device unless told otherwise; the host build of PivotedQR cannot fuse (x86-64 baseline), so every function below runs
// with contraction off.  The only v_fma_f64 left are the ones inside the correctly rounded fp64 division sequence
// (v_div_scale_f64 .. v_div_fixup_f64), which tests/test_foldin_isa.py checks.
//
// Layout: ONE update (or anonymous query) per lane.  A solve is a serial chain of ~k^2 dependent fp64 adds, so the
// parallelism is across updates, never inside one.  The lane's vector lives in LDS, column per lane (element r of lane l
// at [r * 64 + l]: a wave's access is 512 contiguous bytes, no bank conflict), which keeps any k <= 128 in one kernel with
// plain loops and no private (scratch) arrays; the factors of the solver are read with wave-uniform addresses (scalar
// loads).  Registers cannot hold it: 128 doubles are all 256 architected VGPRs of a lane.  The two solves of an update run
// one after the other in ONE vector of LDS per lane (k * 512 bytes per wave: 32 KiB at k = 64, five waves per CU; 64 KiB
// at k = 128, two), the first solution parked in a global workspace of the batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mals {

constexpr int FOLDIN_LANES = 64;  // one wave per workgroup

// Status word of one update (foldin_update_kernel): low byte the MALS_* code, then why it failed, then how many times
// the reference would have logged "fold in vector is large" (0..2)
enum { FOLDIN_WHY_ESTIMATE = 1, FOLDIN_WHY_ITEM_DELTA = 2, FOLDIN_WHY_USER_DELTA = 3, FOLDIN_WHY_NO_YTY = 4 };
__host__ __device__ inline int foldin_status(int code, int why, int big) { return code | (why << 8) | (big << 16); }

// one generation solver on the device: column-major reflectors / R (n x n), tau, and the inverse of the pivot
// permutation (ipiv[f] = j with piv[j] = f: the scatter x[piv[j]] = y[j] read as x[f] = y[ipiv[f]])
struct FoldinSolverView {
  const double* a;
  const double* tau;
  const int32_t* ipiv;
};

// ServerRecommender.foldInWeight (:981-994), FOLDIN_LEARN_RATE = rate; the caller has checked that estimate is finite
__device__ inline double foldin_weight(double estimate, float value, double rate) {
#pragma clang fp contract(off)
  double w;
  if (value > 0.0f && estimate < 1.0) {
    const double multiplier = 1.0 - (estimate > 0.0 ? estimate : 0.0);   // FastMath.max(0.0, estimate)
    w = (1.0 - 1.0 / (1.0 + (double)value)) * multiplier;
  } else if (value < 0.0f && estimate > 0.0) {
    const double multiplier = -(estimate < 1.0 ? estimate : 1.0);        // -FastMath.min(1.0, estimate)
    w = (1.0 - 1.0 / (1.0 - (double)value)) * multiplier;
  } else {
    w = 0.0;
  }
  return rate * w;
}

// PivotedQR::solve for NV (1 or 2) right-hand sides at once, each with its own solver, up to the scatter: on entry y[v]
// (this lane's column: element r at y[v][r * FOLDIN_LANES]) holds b, on return the permuted solution (x[f] =
// y[v][ipiv[f] * FOLDIN_LANES]).  n, the solvers and the loop bounds are wave-uniform.
template <int NV>
__device__ inline void foldin_qr_solve(const FoldinSolverView* S, double* const* y, int n) {
#pragma clang fp contract(off)
  constexpr int L = FOLDIN_LANES;
  for (int j = 0; j < n; ++j) {  // y <- H_j y
    double s[NV], tj[NV];
    const double* vj[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      tj[v] = S[v].tau[j];
      vj[v] = S[v].a + (size_t)j * n;
      s[v] = y[v][j * L];
    }
    for (int r = j + 1; r < n; ++r) {
#pragma unroll
      for (int v = 0; v < NV; ++v) s[v] += vj[v][r] * y[v][r * L];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (tj[v] == 0.0) continue;  // (wave-uniform)
      s[v] *= tj[v];
      y[v][j * L] -= s[v];
      for (int r = j + 1; r < n; ++r) y[v][r * L] -= s[v] * vj[v][r];
    }
  }
  for (int r = n - 1; r >= 0; --r) {  // R z = y
    double s[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) s[v] = y[v][r * L];
    for (int c = r + 1; c < n; ++c) {
#pragma unroll
      for (int v = 0; v < NV; ++v) s[v] -= S[v].a[(size_t)c * n + r] * y[v][c * L];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) y[v][r * L] = s[v] / S[v].a[(size_t)r * n + r];
  }
}

// The device solve alone (tests: against mals_solver_solve_ftod): x[q] = A^-1 (double) b[q] for n_rhs float vectors
__global__ __launch_bounds__(64) void foldin_solve_kernel(FoldinSolverView S, int n, const float* __restrict__ b, int n_rhs,
                                                          double* __restrict__ x) {
#pragma clang fp contract(off)
  extern __shared__ double foldin_lds[];
  const int lane = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * FOLDIN_LANES + lane;
  const bool active = q < n_rhs;
  double* y = foldin_lds + lane;
  for (int f = 0; f < n; ++f) y[f * FOLDIN_LANES] = active ? (double)b[q * n + f] : 0.0;
  double* ys[1] = {y};
  foldin_qr_solve<1>(&S, ys, n);
  if (active)
    for (int f = 0; f < n; ++f) x[q * n + f] = y[S.ipiv[f] * FOLDIN_LANES];
}

// One level of mals_set_preferences: updates [u0, u1) of the level-ordered batch touch pairwise distinct rows of X and
// of Y, so they run side by side; levels run one after another (kernel boundaries on one stream).  Update t, from the
// rows as they stand (ServerRecommender.updateFeatures, :865-912):
//   estimate = dot(x_u, y_i) (fp32 products, fp64 sum in feature order); not finite: fails, nothing changes (:982)
//   w = foldInWeight(estimate, value); w == 0: nothing changes (:870-872)
//   itemFoldIn = solveFToD_XTX(x_u), userFoldIn = solveFToD_YTY(y_i), both from the rows BEFORE the update
//   XTX solver without YTY solver: the item branch reads norm(userFoldIn) of a null vector -- the reference throws
//     before anything changes (:889); the update fails
//   item branch (XTX solver): y_i[f] += (float)(w * itemFoldIn[f]) in feature order, a non-finite delta stops there
//     (:893: the earlier elements keep their new values, x_u is not touched)
//   user branch (YTY solver): x_u[f] += (float)(w * userFoldIn[f]), likewise (:903)
//   each branch counts norm(userFoldIn) > BIG_FOLDIN_THRESHOLD the way the reference's code reads it (:889, :899);
//   sqrt(total) > 1e4 is decided as total >= big_total (the smallest double whose correctly rounded root exceeds 1e4,
//   found on the host), which is the same predicate without a device square root
__global__ __launch_bounds__(64) void foldin_update_kernel(float* __restrict__ X, float* __restrict__ Y, int k,
                                                           const int64_t* __restrict__ urow, const int64_t* __restrict__ irow,
                                                           const float* __restrict__ value, int64_t u0, int64_t u1,
                                                           FoldinSolverView SX, FoldinSolverView SY, int has_xtx, int has_yty,
                                                           double rate, double big_total, double* __restrict__ user_fold,
                                                           int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  extern __shared__ double foldin_lds[];
  constexpr int L = FOLDIN_LANES;
  const int lane = threadIdx.x;
  const int64_t t = u0 + (int64_t)blockIdx.x * L + lane;
  const bool active = t < u1;
  float* xu = active ? X + (size_t)urow[t] * k : nullptr;
  float* yi = active ? Y + (size_t)irow[t] * k : nullptr;
  double* buf = foldin_lds + lane;  // y_i -> userFoldIn (Y^T Y), then x_u -> itemFoldIn (X^T X)
  double estimate = 0.0;
  for (int f = 0; f < k; ++f) {
    const float xf = active ? xu[f] : 0.f, yf = active ? yi[f] : 0.f;
    estimate += (double)(xf * yf);
    buf[f * L] = (double)yf;
  }
  bool big = false;
  double* uf = user_fold + (size_t)(active ? t : 0) * k;  // userFoldIn of this update, in feature order
  if (has_yty) {
    double* ys[1] = {buf};
    foldin_qr_solve<1>(&SY, ys, k);
    double total = 0.0;
    for (int f = 0; f < k; ++f) {
      const double d = buf[SY.ipiv[f] * L];
      total += d * d;
      if (active) uf[f] = d;
    }
    big = total >= big_total;
  }
  if (has_xtx) {
    for (int f = 0; f < k; ++f) buf[f * L] = active ? (double)xu[f] : 0.0;
    double* ys[1] = {buf};
    foldin_qr_solve<1>(&SX, ys, k);
  }
  if (!active) return;
  if (!__builtin_isfinite(estimate)) {
    status[t] = foldin_status(2 /* MALS_INVALID_ARG */, FOLDIN_WHY_ESTIMATE, 0);
    return;
  }
  const double w = foldin_weight(estimate, value[t], rate);
  if (w == 0.0) {
    status[t] = 0;
    return;
  }
  if (has_xtx && !has_yty) {
    status[t] = foldin_status(2, FOLDIN_WHY_NO_YTY, 0);
    return;
  }
  int n_big = 0;
  if (has_xtx) {
    n_big += big;
    for (int f = 0; f < k; ++f) {
      const double delta = w * buf[SX.ipiv[f] * L];
      if (!__builtin_isfinite(delta)) {
        status[t] = foldin_status(2, FOLDIN_WHY_ITEM_DELTA, n_big);
        return;
      }
      yi[f] = yi[f] + (float)delta;
    }
  }
  if (has_yty) {
    n_big += big;
    for (int f = 0; f < k; ++f) {
      const double delta = w * uf[f];
      if (!__builtin_isfinite(delta)) {
        status[t] = foldin_status(2, FOLDIN_WHY_USER_DELTA, n_big);
        return;
      }
      xu[f] = xu[f] + (float)delta;
    }
  }
  status[t] = foldin_status(0, 0, n_big);
}

// buildAnonymousUserFeatures (:561-609) for one query per lane: over the query's items in order, rows -1 skipped,
// userFoldIn = solveFToD_YTY(y_item), w = foldInWeight(0.0, value or 1), acc[f] += (float)(w * userFoldIn[f]) in fp32
// (w == 0 adds nothing).  found[q] = 0: no item of the query has a row (NoSuchItemException).  to_row (optional):
// dot_out[q] = (float)dot(acc, Y[to_row[q]]) (estimateForAnonymous, :734-759).  max_len[block]: the longest query of
// each block of 64 (the item loop is wave-uniform; shorter queries idle).
__global__ __launch_bounds__(64) void foldin_anonymous_kernel(const float* __restrict__ Y, int k, const int64_t* __restrict__ item_ptr,
                                                              const int64_t* __restrict__ item_row, const float* __restrict__ values,
                                                              int n_queries, const int32_t* __restrict__ max_len, FoldinSolverView SY,
                                                              double rate, float* __restrict__ out, int32_t* __restrict__ found,
                                                              const int64_t* __restrict__ to_row, float* __restrict__ dot_out) {
#pragma clang fp contract(off)
  extern __shared__ double foldin_lds[];
  constexpr int L = FOLDIN_LANES;
  const int lane = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * L + lane;
  const bool active = q < n_queries;
  double* by = foldin_lds + lane;
  float* acc = reinterpret_cast<float*>(foldin_lds + (size_t)k * L) + lane;
  for (int f = 0; f < k; ++f) acc[f * L] = 0.f;
  const int64_t p0 = active ? item_ptr[q] : 0, len = active ? item_ptr[q + 1] - p0 : 0;
  bool any = false;
  const int m_max = max_len[blockIdx.x];
  for (int m = 0; m < m_max; ++m) {
    const int64_t row = m < len ? item_row[p0 + m] : -1;
    for (int f = 0; f < k; ++f) by[f * L] = row >= 0 ? (double)Y[(size_t)row * k + f] : 0.0;
    double* ys[1] = {by};
    foldin_qr_solve<1>(&SY, ys, k);
    if (row < 0) continue;
    any = true;
    const double w = foldin_weight(0.0, values ? values[p0 + m] : 1.0f, rate);
    if (w != 0.0)
      for (int f = 0; f < k; ++f) acc[f * L] = acc[f * L] + (float)(w * by[SY.ipiv[f] * L]);
  }
  if (!active) return;
  for (int f = 0; f < k; ++f) out[q * k + f] = acc[f * L];
  found[q] = any ? 1 : 0;
  if (to_row) {
    double d = 0.0;
    const float* yt = Y + (size_t)to_row[q] * k;
    for (int f = 0; f < k; ++f) d += (double)(acc[f * L] * yt[f]);
    dot_out[q] = (float)d;
  }
}

// estimatePreferences (:690-727): out[t] = (float)dot(x_u, y_i) (fp32 products, fp64 sum in feature order); a row of
// -1 (unknown user or item) gives 0.0f
__global__ __launch_bounds__(256) void foldin_estimate_kernel(const float* __restrict__ X, const float* __restrict__ Y, int k,
                                                              const int64_t* __restrict__ urow, const int64_t* __restrict__ irow, int64_t n,
                                                              float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t u = urow[t], i = irow[t];
  if (u < 0 || i < 0) {
    out[t] = 0.f;
    return;
  }
  const float* x = X + (size_t)u * k;
  const float* y = Y + (size_t)i * k;
  double d = 0.0;
  for (int f = 0; f < k; ++f) d += (double)(y[f] * x[f]);
  out[t] = (float)d;
}

// zero rows of a factor replica (removePreference dropping a user: a later setPreference recreates it from zeros)
__global__ void foldin_zero_rows_kernel(float* __restrict__ F, int k, const int64_t* __restrict__ rows, int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n * k) F[(size_t)rows[t / k] * k + (size_t)(t % k)] = 0.f;
}

// setUserTag's userTagIDs.add(tagID) (:1094) for a batch: the item row of every update whose kind is FOLDIN_KIND_USER_TAG
// is ORed into the mask that top-N, similarity and popular read (topn_tagged), and *n_set counts the bits that were clear
// before -- the old word decides, so a row repeated within the batch counts once.  n_items bounds the mask's words.
enum : uint8_t { FOLDIN_KIND_PREF = 0, FOLDIN_KIND_ITEM_TAG = 1, FOLDIN_KIND_USER_TAG = 2 };
__global__ __launch_bounds__(256) void foldin_tag_mark_kernel(const int64_t* __restrict__ irow, const uint8_t* __restrict__ kind, int64_t n,
                                                              int64_t n_items, uint32_t* __restrict__ bits, unsigned long long* __restrict__ n_set) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n || kind[t] != FOLDIN_KIND_USER_TAG) return;
  const int64_t it = irow[t];
  if (it < 0 || it >= n_items) return;
  const uint32_t bit = 1u << (it & 31);
  if ((atomicOr(&bits[it >> 5], bit) & bit) == 0u) atomicAdd(n_set, 1ull);
}

}  // namespace mals
