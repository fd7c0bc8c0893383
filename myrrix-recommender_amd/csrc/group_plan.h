// group_plan.h -- the arithmetic of a multi-GPU group (mals_group.cpp) that needs no device: who owns a row, what a rank's
// slice and its exchange chunks are, which member answers a run of queries.  Host code only, no HIP and no RCCL include;
// tests/cpp/test_group_host.cpp restates every function here by brute force.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace mals {

// mals_plan_shards (include/myrrix_als.h): `world` consecutive row ranges of nearly equal cost, a row costing its entries plus
// row_cost (< 0: the default, features^2 / 200).  bounds_out: world + 1.  false: bad arguments.
inline bool plan_shards(const int64_t* row_ptr, int64_t n_rows, int32_t world, double row_cost, int32_t features, int64_t* bounds_out) {
  if (!row_ptr || !bounds_out || n_rows < 0 || world <= 0) return false;
  if (row_cost < 0.0) row_cost = features > 0 ? (double)features * features / 200.0 : 0.0;
  const double total = (double)(row_ptr[n_rows] - row_ptr[0]) + row_cost * (double)n_rows;
  bounds_out[0] = 0;
  int64_t r = 0;
  for (int j = 1; j < world; ++j) {
    const double target = total * (double)j / (double)world;
    // first r with cost(rows [0, r)) >= target, then the closer of r-1 and r
    auto cost = [&](int64_t rr) { return (double)(row_ptr[rr] - row_ptr[0]) + row_cost * (double)rr; };
    int64_t lo = r, hi = n_rows;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (cost(mid) >= target) hi = mid; else lo = mid + 1;
    }
    int64_t b = lo;
    if (b > r && target - cost(b - 1) < cost(b) - target) b = b - 1;
    bounds_out[j] = std::max(b, r);
    r = bounds_out[j];
  }
  bounds_out[world] = n_rows;
  return true;
}

// the rank that holds user u's known items: the slice with its row; users past the installed matrix (rows the replicas
// grew by, mals_group_grow_factor_rows) are the last rank's
inline int owner_of(const std::vector<int64_t>& bounds, int64_t u) {
  const int world = (int)bounds.size() - 1;
  return std::min(world - 1, (int)(std::upper_bound(bounds.begin(), bounds.end(), u) - bounds.begin()) - 1);
}

// rows per exchange chunk of the slice [b0, b1) cut into `chunks`
inline int64_t chunk_rows_of(int64_t b0, int64_t b1, int chunks) { return std::max<int64_t>(1, (b1 - b0 + chunks - 1) / chunks); }

// rows [lo, hi) (global) of chunk c of that slice; empty past the slice's end
inline void chunk_range(int64_t b0, int64_t b1, int chunks, int c, int64_t* lo, int64_t* hi) {
  const int64_t cr = chunk_rows_of(b0, b1, chunks);
  *lo = std::min(b1, b0 + (int64_t)c * cr);
  *hi = std::min(b1, b0 + (int64_t)(c + 1) * cr);
}

// rows [r0, r1) of a CSR as a matrix of their own: its entries are [e0, e1) of the source's, its row pointers start at 0
struct CsrSlice {
  int64_t r0, r1, e0, e1;
  std::vector<int64_t> local;   // r1 - r0 + 1
  int64_t rows() const { return r1 - r0; }
  int64_t entries() const { return e1 - e0; }
};
inline CsrSlice csr_slice(const int64_t* row_ptr, int64_t r0, int64_t r1) {
  CsrSlice s{r0, r1, row_ptr[r0], row_ptr[r1], std::vector<int64_t>((size_t)(r1 - r0) + 1)};
  for (int64_t r = r0; r <= r1; ++r) s.local[(size_t)(r - r0)] = row_ptr[r] - s.e0;
  return s;
}

// The run of consecutive queries from q0 on that one rank answers: [q0, *q1) and its owner.  A one-user call is one run.
// false: a negative user, or one at or past max(bounds.back(), users_end) (users_end: the rows of the X replicas).
inline bool owner_run(const std::vector<int64_t>& bounds, int64_t users_end, const int64_t* user_idx, int32_t n_queries, int32_t q0,
                      int32_t* q1, int* owner) {
  const int64_t limit = std::max(bounds.back(), users_end);
  auto valid = [&](int64_t u) { return u >= 0 && u < limit; };
  if (!valid(user_idx[q0])) return false;
  *owner = owner_of(bounds, user_idx[q0]);
  int32_t q = q0 + 1;
  while (q < n_queries && valid(user_idx[q]) && owner_of(bounds, user_idx[q]) == *owner) ++q;
  *q1 = q;
  return true;
}

}  // namespace mals
