// The ownership plan of mals_group_load_generation (csrc/generation_group_plan.h) with no device.  Stand-alone host program,
// built with -fsanitize=address,undefined by tests/test_generation_group_plan.py.  usage: test_generation_group_plan <seed>
//
// Seeded cases over world 1..8, the named shapes among them -- an empty new model, no kept users, everything kept (no new
// model and every live user kept), a member whose new slice is empty (two new users, eight members), all kept users from one
// old owner, grown users past the old bounds (the last rank's), no old bounds at all -- each checked by brute force:
//   * the bounds are monotone, start at 0 and end at n_merged, and equal plan_shards over the concatenated row pointer, which
//     the test builds itself;
//   * kept_start follows owner-by-scan of every kept user (rows at or past the last old bound: the last rank);
//   * every kept user is assigned exactly once: walking old member m's runs in new-member order covers m's kept list from its
//     first to its last user without a gap or an overlap (so every run is contiguous and the runs are in order), and a user of
//     run (m, j) is a merged row inside new member j's bounds;
//   * bad arguments are refused: world 0, descending kept rows, a negative size, descending old bounds, a descending row pointer.
#include "../../myrrix-recommender_amd/csrc/generation_group_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

using namespace mals;

static int failures = 0, checks = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++checks;                                             \
    if (!(cond)) {                                        \
      if (++failures <= 20) {                             \
        std::fprintf(stderr, "FAIL %s: ", #cond);         \
        std::fprintf(stderr, __VA_ARGS__);                \
        std::fprintf(stderr, "\n");                       \
      }                                                   \
    }                                                     \
  } while (0)

struct Case {
  int world = 1, features = 8;
  std::vector<int64_t> new_ptr;      // empty: NULL (no known items), n_new says how many new users
  int64_t n_new = 0;
  std::vector<int64_t> kept_rows, kept_sizes, old_bounds;   // old_bounds empty: NULL
};

static int old_owner_by_scan(const Case& c, int64_t row) {
  if (c.old_bounds.empty()) return c.world - 1;
  for (int r = 0; r < c.world; ++r)
    if (c.old_bounds[(size_t)r] <= row && row < c.old_bounds[(size_t)r + 1]) return r;
  return c.world - 1;   // past the installed matrix (or in no slice): the last rank's, as owner_of says
}

static void check_case(const Case& c, const char* name) {
  GenGroupPlan p;
  const int64_t n_kept = (int64_t)c.kept_rows.size();
  const bool ok = generation_group_plan(c.world, c.features, c.n_new, c.new_ptr.empty() ? nullptr : c.new_ptr.data(), n_kept, c.kept_sizes.data(),
                                        c.kept_rows.data(), c.old_bounds.empty() ? nullptr : c.old_bounds.data(), p);
  CHECK(ok, "%s: the plan refused a good case", name);
  if (!ok) return;
  const int64_t n_merged = c.n_new + n_kept;
  // the concatenated row pointer, restated
  std::vector<int64_t> cat((size_t)n_merged + 1, 0);
  for (int64_t r = 0; r < c.n_new; ++r) cat[(size_t)r + 1] = c.new_ptr.empty() ? 0 : c.new_ptr[(size_t)r + 1] - c.new_ptr[0];
  for (int64_t i = 0; i < n_kept; ++i) cat[(size_t)(c.n_new + i + 1)] = cat[(size_t)(c.n_new + i)] + c.kept_sizes[(size_t)i];
  CHECK(p.row_ptr == cat, "%s: the concatenated row pointer differs", name);
  std::vector<int64_t> want((size_t)c.world + 1, -1);
  CHECK(plan_shards(cat.data(), n_merged, c.world, -1.0, c.features, want.data()), "%s: plan_shards refused", name);
  CHECK(p.bounds == want, "%s: the bounds are not plan_shards' over the concatenated row pointer", name);
  CHECK(p.bounds.size() == (size_t)c.world + 1 && p.bounds.front() == 0 && p.bounds.back() == n_merged, "%s: bounds do not span [0, n_merged]", name);
  for (int j = 0; j < c.world; ++j) CHECK(p.bounds[(size_t)j] <= p.bounds[(size_t)j + 1], "%s: bounds descend at %d", name, j);
  // the old owners' runs of the kept list
  CHECK(p.kept_start.size() == (size_t)c.world + 1 && p.kept_start.front() == 0 && p.kept_start.back() == n_kept, "%s: kept_start does not span the kept list", name);
  for (int64_t i = 0; i < n_kept; ++i) {
    int m = 0;
    while (m + 1 < c.world && p.kept_start[(size_t)m + 1] <= i) ++m;
    const int scan = old_owner_by_scan(c, c.kept_rows[(size_t)i]);
    CHECK(m == scan, "%s: kept user %lld (row %lld) is member %d's, by scan %d's", name, (long long)i, (long long)c.kept_rows[(size_t)i], m, scan);
  }
  // every kept user exactly once
  std::vector<int> seen((size_t)n_kept, 0);
  CHECK(p.move.size() == (size_t)c.world * (size_t)c.world * 2, "%s: move has the wrong size", name);
  for (int m = 0; m < c.world; ++m) {
    const int64_t n_m = p.kept_start[(size_t)m + 1] - p.kept_start[(size_t)m];
    int64_t next = 0;
    for (int j = 0; j < c.world; ++j) {
      const int64_t* run = p.run(c.world, m, j);
      CHECK(run[0] <= run[1] && run[0] >= 0 && run[1] <= n_m, "%s: run (%d, %d) = [%lld, %lld) outside the member's %lld kept users", name, m, j,
            (long long)run[0], (long long)run[1], (long long)n_m);
      if (run[1] > run[0]) {
        CHECK(run[0] == next, "%s: run (%d, %d) starts at %lld, the runs before it end at %lld", name, m, j, (long long)run[0], (long long)next);
        next = run[1];
      }
      for (int64_t i = run[0]; i < run[1] && i < n_m; ++i) {
        const int64_t kept = p.kept_start[(size_t)m] + i, u = c.n_new + kept;
        ++seen[(size_t)kept];
        CHECK(p.bounds[(size_t)j] <= u && u < p.bounds[(size_t)j + 1], "%s: merged user %lld of run (%d, %d) is outside member %d's bounds", name, (long long)u,
              m, j, j);
      }
    }
    CHECK(next == n_m, "%s: member %d's runs end at %lld of %lld kept users", name, m, (long long)next, (long long)n_m);
  }
  for (int64_t i = 0; i < n_kept; ++i) CHECK(seen[(size_t)i] == 1, "%s: kept user %lld assigned %d times", name, (long long)i, seen[(size_t)i]);
}

// old bounds without empty slices in the middle of occupied ones are not required: any monotone bounds
static std::vector<int64_t> random_bounds(std::mt19937_64& rng, int world, int64_t rows) {
  std::vector<int64_t> cut((size_t)world - 1);
  for (auto& v : cut) v = rows > 0 ? (int64_t)(rng() % (uint64_t)(rows + 1)) : 0;
  std::sort(cut.begin(), cut.end());
  std::vector<int64_t> b(1, 0);
  b.insert(b.end(), cut.begin(), cut.end());
  b.push_back(rows);
  return b;
}

static Case random_case(std::mt19937_64& rng, int world, int shape) {
  Case c;
  c.world = world;
  c.features = 1 + (int)(rng() % 64);
  const int64_t n_live = 1 + (int64_t)(rng() % 300), n_grown = shape == 5 ? 1 + (int64_t)(rng() % 20) : (int64_t)(rng() % 3 == 0 ? rng() % 10 : 0);
  c.old_bounds = random_bounds(rng, world, n_live);
  c.n_new = (int64_t)(rng() % 200);
  if (shape == 0 || shape == 2) c.n_new = 0;   // an empty new model; everything kept
  if (shape == 3) c.n_new = 2;                 // a member whose new slice is empty (world > 2)
  const bool known = rng() % 4 != 0;
  if (known) {
    c.new_ptr.assign((size_t)c.n_new + 1, (int64_t)(rng() % 5));   // (a row pointer need not start at 0)
    for (int64_t r = 0; r < c.n_new; ++r) c.new_ptr[(size_t)r + 1] = c.new_ptr[(size_t)r] + (int64_t)(rng() % 7 == 0 ? rng() % 400 : rng() % 12);
  }
  int one_owner = shape == 4 ? (int)(rng() % (uint64_t)world) : -1;
  for (int64_t r = 0; r < n_live + n_grown; ++r) {
    bool keep = shape == 2 || rng() % 3 == 0;
    if (shape == 1) keep = false;   // no kept users
    if (one_owner >= 0) keep = r >= c.old_bounds[(size_t)one_owner] && r < c.old_bounds[(size_t)one_owner + 1] && r < n_live && rng() % 2 == 0;
    if (shape == 5 && r >= n_live) keep = true;   // grown users on the last rank
    if (keep) {
      c.kept_rows.push_back(r);
      c.kept_sizes.push_back(known ? (int64_t)(rng() % 9 == 0 ? rng() % 300 : rng() % 10) : 0);
    }
  }
  if (rng() % 11 == 0) c.old_bounds.clear();   // a group without a user-side matrix
  return c;
}

static void test_named() {
  {  // two old owners of three users each, four new users with 1 entry each, sizes 1: cost is rows + entries, cut in the middle
    Case c;
    c.world = 2;
    c.features = 1;   // row cost 1 / 200
    c.n_new = 4;
    c.new_ptr = {0, 1, 2, 3, 4};
    c.kept_rows = {0, 2, 3, 5};
    c.kept_sizes = {1, 1, 1, 1};
    c.old_bounds = {0, 3, 6};
    check_case(c, "named: even");
    GenGroupPlan p;
    generation_group_plan(c.world, c.features, c.n_new, c.new_ptr.data(), 4, c.kept_sizes.data(), c.kept_rows.data(), c.old_bounds.data(), p);
    CHECK(p.bounds == (std::vector<int64_t>{0, 4, 8}), "named: even: bounds");
    CHECK(p.kept_start == (std::vector<int64_t>{0, 2, 4}), "named: even: kept_start");
    // old member 0's two kept users and old member 1's two all go to new member 1
    CHECK(p.move == (std::vector<int64_t>{0, 0, 0, 2, 0, 0, 0, 2}), "named: even: moves");
  }
  {  // a heavy kept user pulls the cut into the kept tail: old member 0's users split between the new members
    Case c;
    c.world = 2;
    c.features = 1;
    c.n_new = 1;
    c.new_ptr = {0, 2};
    c.kept_rows = {0, 1, 2, 7};
    c.kept_sizes = {2, 2, 2, 4};   // entries 2 | 2 2 2 4 = 12, half = 6 -> the cut after three rows
    c.old_bounds = {0, 3, 5};
    check_case(c, "named: split");
    GenGroupPlan p;
    generation_group_plan(c.world, c.features, c.n_new, c.new_ptr.data(), 4, c.kept_sizes.data(), c.kept_rows.data(), c.old_bounds.data(), p);
    CHECK(p.bounds == (std::vector<int64_t>{0, 3, 5}), "named: split: bounds %lld", (long long)p.bounds[1]);
    CHECK(p.kept_start == (std::vector<int64_t>{0, 3, 4}), "named: split: kept_start");   // row 7 is past the old bounds: the last rank's
    CHECK(p.move == (std::vector<int64_t>{0, 2, 2, 3, 0, 0, 0, 1}), "named: split: moves");
  }
  {  // refusals
    GenGroupPlan p;
    const int64_t rows[] = {3, 2}, sizes[] = {1, 1}, neg[] = {1, -1}, up[] = {2, 3}, ob[] = {0, 5, 4}, bad_ptr[] = {0, 3, 2};
    CHECK(!generation_group_plan(0, 8, 0, nullptr, 0, nullptr, nullptr, nullptr, p), "world 0 accepted");
    CHECK(!generation_group_plan(2, 8, 0, nullptr, 2, sizes, rows, nullptr, p), "descending kept rows accepted");
    CHECK(!generation_group_plan(2, 8, 0, nullptr, 2, neg, up, nullptr, p), "a negative size accepted");
    CHECK(!generation_group_plan(2, 8, 0, nullptr, 2, sizes, up, ob, p), "descending old bounds accepted");
    CHECK(!generation_group_plan(2, 8, 2, bad_ptr, 0, nullptr, nullptr, nullptr, p), "a descending row pointer accepted");
    CHECK(!generation_group_plan(2, 8, 0, nullptr, 2, nullptr, up, nullptr, p), "null sizes accepted");
  }
}

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
  std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + 7);
  test_named();
  static const char* const shape_name[] = {"empty new model", "no kept users", "everything kept", "two new users", "one old owner", "grown users", "random"};
  for (int world = 1; world <= 8; ++world)
    for (int shape = 0; shape < 7; ++shape)
      for (int t = 0; t < 12; ++t) {
        const Case c = random_case(rng, world, shape);
        check_case(c, (std::string(shape_name[shape]) + ", world " + std::to_string(world)).c_str());
      }
  std::printf("checks %d failures %d\n", checks, failures);
  return failures == 0 ? 0 : 1;
}
