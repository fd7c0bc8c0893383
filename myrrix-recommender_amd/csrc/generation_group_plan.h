// generation_group_plan.h -- who owns which user after mals_group_load_generation (include/myrrix_als.h), and which part of
// every old owner's kept users moves to which new owner.  Host code only, no HIP include and no handle;
// tests/cpp/test_generation_group_plan.cpp restates it by brute force.
//
// The merged user order is the new model's rows, then the kept live rows in live order.  Its known-item row pointer is the new
// model's (new_known_ptr, or all zeros) followed by the running sum of the kept users' set sizes; the new bounds are
// plan_shards (group_plan.h, default row cost) over it.  Kept users are a tail of the merged order and appear in the old
// owners' rank order (grown users last, on the last rank), so what old owner m hands to new owner j is ONE contiguous run of
// m's kept list, and the runs of m follow each other in j order.
#pragma once
#include "group_plan.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace mals {

struct GenGroupPlan {
  std::vector<int64_t> bounds;       // world + 1: the new bounds[X], last = n_merged
  std::vector<int64_t> kept_start;   // world + 1: old owner m's kept users are kept_start[m] .. kept_start[m + 1] of the kept list
  std::vector<int64_t> move;         // [old m][new j][2]: the run [begin, end) of m's OWN kept list (0 = its first) that j gets
  std::vector<int64_t> row_ptr;      // n_merged + 1: the concatenated row pointer the bounds were planned over
  const int64_t* run(int world, int m, int j) const { return &move[((size_t)m * (size_t)world + (size_t)j) * 2]; }
};

// old owner m's run of the kept list, out[m] .. out[m + 1] (out: world + 1), by owner_of's rule: a row at or past the last bound
// is the last rank's; without old bounds every kept user is
inline void generation_group_kept_start(int32_t world, int64_t n_kept, const int64_t* kept_rows, const int64_t* old_bounds, int64_t* out) {
  out[0] = 0;
  for (int m = 1; m < world; ++m)
    out[m] = std::max(out[m - 1], old_bounds ? (int64_t)(std::lower_bound(kept_rows, kept_rows + n_kept, old_bounds[m]) - kept_rows) : (int64_t)0);
  out[world] = n_kept;
}

// kept_rows: the kept users' live rows, strictly ascending; old_bounds: the old bounds[X] (world + 1), or NULL for a group
// without a user-side matrix (every kept user is then the last rank's, as grown users are).  false: bad arguments.
inline bool generation_group_plan(int32_t world, int32_t features, int64_t n_new, const int64_t* new_known_ptr, int64_t n_kept,
                                  const int64_t* kept_sizes, const int64_t* kept_rows, const int64_t* old_bounds, GenGroupPlan& p) {
  if (world <= 0 || n_new < 0 || n_kept < 0 || (n_kept > 0 && (!kept_sizes || !kept_rows))) return false;
  for (int64_t i = 0; i < n_kept; ++i)
    if (kept_sizes[i] < 0 || kept_rows[i] < 0 || (i > 0 && kept_rows[i] <= kept_rows[i - 1])) return false;
  for (int m = 0; old_bounds && m < world; ++m)
    if (old_bounds[m] > old_bounds[m + 1]) return false;
  const int64_t n_merged = n_new + n_kept;
  p.row_ptr.assign((size_t)n_merged + 1, 0);
  if (new_known_ptr)
    for (int64_t r = 0; r <= n_new; ++r) {
      if (r > 0 && new_known_ptr[r] < new_known_ptr[r - 1]) return false;
      p.row_ptr[(size_t)r] = new_known_ptr[r] - new_known_ptr[0];
    }
  for (int64_t i = 0; i < n_kept; ++i) p.row_ptr[(size_t)(n_new + i + 1)] = p.row_ptr[(size_t)(n_new + i)] + kept_sizes[i];
  p.bounds.assign((size_t)world + 1, 0);
  if (!plan_shards(p.row_ptr.data(), n_merged, world, -1.0, features, p.bounds.data())) return false;
  // the old owners' runs of the kept list: owner_of's rule (a row at or past the last bound is the last rank's)
  p.kept_start.assign((size_t)world + 1, 0);
  generation_group_kept_start(world, n_kept, kept_rows, old_bounds, p.kept_start.data());
  p.move.assign((size_t)world * (size_t)world * 2, 0);
  for (int m = 0; m < world; ++m) {
    const int64_t lo = n_new + p.kept_start[(size_t)m], hi = n_new + p.kept_start[(size_t)m + 1];   // m's kept users as merged rows
    for (int j = 0; j < world; ++j) {
      const int64_t b = std::min(std::max(p.bounds[(size_t)j], lo), hi), e = std::min(std::max(p.bounds[(size_t)j + 1], lo), hi);
      int64_t* r = &p.move[((size_t)m * (size_t)world + (size_t)j) * 2];
      r[0] = b - lo;
      r[1] = std::max(e, b) - lo;
    }
  }
  return true;
}

}  // namespace mals
