// The host arithmetic of a multi-GPU group (csrc/group_plan.h) and the convergence loop (csrc/convergence.h) with no device.
// Stand-alone host program, built with -fsanitize=address,undefined by tests/test_group_host.py.  usage: test_group_host <seed>
//
// Checked by brute-force restatement, on the named edge cases and on seeded random inputs:
//   * owner_of: a user belongs to the one non-empty slice that holds its row (bounds with empty slices, [0,0,2,2,5] among
//     them); users at and past bounds.back() belong to the last rank;
//   * chunk ranges: for slices of 0, 1, chunks-1, chunks, chunks+1 (and random) rows and 1-5 chunks, the ranges of c = 0 ..
//     chunks-1 tile [b0, b1) exactly and in order; chunks past the slice's end are empty (a 0-row slice has none that is not);
//   * csr_slice: local[0] == 0, every difference is the source's, e1 - e0 == local.back();
//   * owner runs: they cover [0, n) in order, one owner per run, adjacent runs differ in owner; a negative user or one at or
//     past max(bounds.back(), users_end) is refused wherever it stands (interleaved owners, one query, the grown range);
//   * plan_shards: monotone bounds from 0 to n_rows, every cut the closest row boundary to its cost target; bad arguments;
//   * DoubleWeightedMean: (2,4) weighted (1,3) -> 3.5; a zero-weight first datum is replaced; empty -> NaN; update_estimates
//     equals the increment loop in table order, bit for bit;
//   * factorize_loop over a scripted driver: stops at max_iterations, on a non-finite mean, never at iteration 1 with
//     random_y, else at the first mean below the threshold; a cancellation before either half returns MALS_CANCELLED with
//     iterations_out at the completed count; the callback sees the mean before the stop rules apply, and is read once per
//     iteration; bad arguments fail before anything runs; iterate == 0 is one X half.
#include "../../myrrix-recommender_amd/csrc/convergence.h"
#include "../../myrrix-recommender_amd/csrc/group_plan.h"

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

// `world` slices over up to max_rows rows, empty ones likely
static std::vector<int64_t> random_bounds(std::mt19937_64& rng, int world, int64_t max_rows) {
  std::vector<int64_t> b((size_t)world + 1, 0);
  for (int j = 1; j <= world; ++j) b[(size_t)j] = b[(size_t)j - 1] + (rng() % 3 == 0 ? 0 : (int64_t)(rng() % (uint64_t)(max_rows / world + 1)));
  return b;
}

static int owner_by_scan(const std::vector<int64_t>& b, int64_t u) {
  const int world = (int)b.size() - 1;
  for (int r = 0; r < world; ++r)
    if (b[(size_t)r] <= u && u < b[(size_t)r + 1]) return r;
  return world - 1;   // past the installed matrix
}

static void test_owner_of(std::mt19937_64& rng) {
  const std::vector<int64_t> named = {0, 0, 2, 2, 5};
  const int expect[] = {1, 1, 3, 3, 3, 3, 3, 3};   // users 0 .. 7
  for (int u = 0; u < 8; ++u) CHECK(owner_of(named, u) == expect[u], "named bounds, user %d: %d", u, owner_of(named, u));
  for (int t = 0; t < 200; ++t) {
    const int world = 1 + (int)(rng() % 6);
    const std::vector<int64_t> b = random_bounds(rng, world, 40);
    for (int64_t u = 0; u < b.back() + 5; ++u) CHECK(owner_of(b, u) == owner_by_scan(b, u), "world %d user %lld", world, (long long)u);
  }
}

static void check_chunks(int64_t b0, int64_t n, int chunks) {
  const int64_t b1 = b0 + n;
  int64_t next = b0;
  int non_empty = 0;
  for (int c = 0; c < chunks; ++c) {
    int64_t lo = -1, hi = -1;
    chunk_range(b0, b1, chunks, c, &lo, &hi);
    CHECK(lo == next && hi >= lo && hi <= b1, "slice %lld+%lld, %d chunks, chunk %d: [%lld, %lld), expected a start at %lld", (long long)b0,
          (long long)n, chunks, c, (long long)lo, (long long)hi, (long long)next);
    CHECK(hi - lo <= chunk_rows_of(b0, b1, chunks), "chunk %d longer than chunk_rows_of", c);
    if (hi > lo) {
      CHECK(non_empty == c, "an empty chunk before chunk %d", c);   // the empty ones are the last ones
      ++non_empty;
    }
    next = hi;
  }
  CHECK(next == b1, "slice %lld+%lld, %d chunks: the chunks end at %lld", (long long)b0, (long long)n, chunks, (long long)next);
  if (n == 0) CHECK(non_empty == 0, "a 0-row slice with a non-empty chunk");
  CHECK(chunk_rows_of(b0, b1, chunks) >= 1, "chunk_rows_of below 1");
}

static void test_chunks(std::mt19937_64& rng) {
  for (int chunks = 1; chunks <= 5; ++chunks) {
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)chunks - 1, (int64_t)chunks, (int64_t)chunks + 1}) check_chunks(7, n, chunks);
    for (int t = 0; t < 50; ++t) check_chunks((int64_t)(rng() % 1000), (int64_t)(rng() % 200), chunks);
  }
}

static std::vector<int64_t> random_row_ptr(std::mt19937_64& rng, int64_t n_rows, int64_t first) {
  std::vector<int64_t> rp((size_t)n_rows + 1, first);
  for (int64_t r = 0; r < n_rows; ++r) rp[(size_t)r + 1] = rp[(size_t)r] + (rng() % 4 == 0 ? 0 : (int64_t)(rng() % 9));
  return rp;
}

static void test_csr_slice(std::mt19937_64& rng) {
  for (int t = 0; t < 200; ++t) {
    const int64_t n = (int64_t)(rng() % 60);
    const std::vector<int64_t> rp = random_row_ptr(rng, n, 0);
    const int64_t r0 = (int64_t)(rng() % (uint64_t)(n + 1)), r1 = r0 + (int64_t)(rng() % (uint64_t)(n - r0 + 1));
    const CsrSlice s = csr_slice(rp.data(), r0, r1);
    CHECK(s.r0 == r0 && s.r1 == r1 && s.e0 == rp[(size_t)r0] && s.e1 == rp[(size_t)r1], "slice [%lld, %lld): ends", (long long)r0, (long long)r1);
    CHECK((int64_t)s.local.size() == r1 - r0 + 1 && s.local[0] == 0, "slice [%lld, %lld): local[0]", (long long)r0, (long long)r1);
    for (int64_t r = r0; r < r1; ++r)
      CHECK(s.local[(size_t)(r - r0) + 1] - s.local[(size_t)(r - r0)] == rp[(size_t)r + 1] - rp[(size_t)r], "row %lld: length", (long long)r);
    CHECK(s.e1 - s.e0 == s.local.back() && s.entries() == s.local.back() && s.rows() == r1 - r0, "slice [%lld, %lld): entries", (long long)r0, (long long)r1);
  }
}

// all runs of a query list, or false on a refusal
static bool all_runs(const std::vector<int64_t>& b, int64_t users_end, const std::vector<int64_t>& users, std::vector<int32_t>* starts, std::vector<int>* owners) {
  const int32_t n = (int32_t)users.size();
  for (int32_t q0 = 0, q1 = 0; q0 < n; q0 = q1) {
    int owner = -1;
    if (!owner_run(b, users_end, users.data(), n, q0, &q1, &owner)) return false;
    CHECK(q1 > q0 && q1 <= n, "run [%d, %d) of %d", q0, q1, n);
    if (q1 <= q0) return false;
    starts->push_back(q0);
    owners->push_back(owner);
  }
  starts->push_back(n);
  return true;
}

static void check_runs(const std::vector<int64_t>& b, int64_t users_end, const std::vector<int64_t>& users) {
  const int64_t limit = std::max(b.back(), users_end);
  bool valid = true;
  for (int64_t u : users) valid = valid && u >= 0 && u < limit;
  std::vector<int32_t> starts;
  std::vector<int> owners;
  const bool ok = all_runs(b, users_end, users, &starts, &owners);
  CHECK(ok == valid, "%zu queries: accepted %d, valid %d", users.size(), (int)ok, (int)valid);
  if (!ok || !valid) return;
  CHECK(starts.front() == 0 && starts.back() == (int32_t)users.size(), "the runs do not cover the queries");
  for (size_t r = 0; r < owners.size(); ++r) {
    for (int32_t q = starts[r]; q < starts[r + 1]; ++q)
      CHECK(owner_by_scan(b, users[(size_t)q]) == owners[r], "query %d (user %lld) in a run of owner %d", q, (long long)users[(size_t)q], owners[r]);
    if (r > 0) CHECK(owners[r] != owners[r - 1], "adjacent runs %zu and %zu share owner %d", r - 1, r, owners[r]);
  }
}

static void test_owner_runs(std::mt19937_64& rng) {
  const std::vector<int64_t> b = {0, 3, 3, 7, 10};
  check_runs(b, 0, {0, 3, 1, 7, 2, 9});           // interleaved owners: six runs
  check_runs(b, 0, {5});                          // a single query
  check_runs(b, 14, {9, 10, 13, 0, 12});          // users in the grown range: the last rank's
  check_runs(b, 14, {9, 14});                     // at the limit: refused
  check_runs(b, 0, {9, 10});                      // no growth: bounds.back() is the limit
  check_runs(b, 14, {9, 12, -1, 12});             // a negative user inside a run
  check_runs(b, 14, {9, 12, 15});                 // past the limit inside a run of the last rank
  check_runs(b, 14, {-1});
  check_runs(b, 14, {});
  {
    std::vector<int32_t> starts;
    std::vector<int> owners;
    CHECK(all_runs(b, 0, {0, 3, 1, 7, 2, 9}, &starts, &owners) && owners == std::vector<int>({0, 2, 0, 3, 0, 3}), "interleaved owners");
    starts.clear(), owners.clear();
    CHECK(all_runs(b, 14, {9, 10, 13, 0, 12}, &starts, &owners) && owners == std::vector<int>({3, 0, 3}) &&
              starts == std::vector<int32_t>({0, 3, 4, 5}), "grown range");
  }
  for (int t = 0; t < 300; ++t) {
    const int world = 1 + (int)(rng() % 5);
    std::vector<int64_t> rb = random_bounds(rng, world, 30);
    if (rb.back() == 0) rb.back() = 1;
    const int64_t users_end = rng() % 2 ? 0 : rb.back() + (int64_t)(rng() % 6);
    const int64_t limit = std::max(rb.back(), users_end);
    std::vector<int64_t> users((size_t)(rng() % 12));
    for (int64_t& u : users) u = (int64_t)(rng() % (uint64_t)limit);
    if (!users.empty() && t % 5 == 0) users[(size_t)(rng() % users.size())] = rng() % 2 ? -1 - (int64_t)(rng() % 3) : limit + (int64_t)(rng() % 3);
    check_runs(rb, users_end, users);
  }
}

static void test_plan_shards(std::mt19937_64& rng) {
  int64_t out[8];
  const int64_t rp1[] = {0, 1};
  CHECK(!plan_shards(nullptr, 1, 2, -1.0, 8, out) && !plan_shards(rp1, 1, 2, -1.0, 8, nullptr) && !plan_shards(rp1, -1, 2, -1.0, 8, out) &&
            !plan_shards(rp1, 1, 0, -1.0, 8, out), "bad arguments accepted");
  for (int t = 0; t < 200; ++t) {
    const int64_t n = (int64_t)(rng() % 80);
    const std::vector<int64_t> rp = random_row_ptr(rng, n, (int64_t)(rng() % 3));
    const int world = 1 + (int)(rng() % 7);
    const int features = (int)(rng() % 3) * 20;
    const double given = rng() % 2 ? -1.0 : (double)(rng() % 5);
    const double row_cost = given < 0.0 ? (features > 0 ? (double)features * features / 200.0 : 0.0) : given;
    std::vector<int64_t> b((size_t)world + 1, -1);
    CHECK(plan_shards(rp.data(), n, world, given, features, b.data()), "plan refused");
    CHECK(b[0] == 0 && b[(size_t)world] == n, "plan ends: %lld .. %lld of %lld", (long long)b[0], (long long)b[(size_t)world], (long long)n);
    auto cost = [&](int64_t r) { return (double)(rp[(size_t)r] - rp[0]) + row_cost * (double)r; };
    for (int j = 1; j < world; ++j) {
      CHECK(b[(size_t)j] >= b[(size_t)j - 1] && b[(size_t)j] <= n, "bound %d not monotone", j);
      // no row boundary at or behind the previous cut is closer to the target than the chosen one
      const double target = cost(n) * (double)j / (double)world, chosen = std::fabs(cost(b[(size_t)j]) - target);
      for (int64_t r = b[(size_t)j - 1]; r <= n; ++r)
        CHECK(chosen <= std::fabs(cost(r) - target) * (1.0 + 1e-12) + 1e-9, "bound %d = %lld: row %lld is closer to the target", j, (long long)b[(size_t)j], (long long)r);
    }
  }
}

static void test_weighted_mean(std::mt19937_64& rng) {
  double tw = 0.0, mean = std::numeric_limits<double>::quiet_NaN();
  dwm_increment(tw, mean, 2.0, 1.0);
  dwm_increment(tw, mean, 4.0, 3.0);
  CHECK(mean == 3.5 && tw == 4.0, "(2,4) weighted (1,3): %g", mean);
  tw = 0.0, mean = std::numeric_limits<double>::quiet_NaN();
  dwm_increment(tw, mean, 5.0, 0.0);
  dwm_increment(tw, mean, 1.0, 2.0);
  CHECK(mean == 1.0, "a zero-weight first datum stays: %g", mean);
  std::vector<double> none, none_fresh;
  CHECK(std::isnan(update_estimates(none, none_fresh)), "empty sample");
  {  // est (0, 0) <- fresh (1, 3): data (1, 3), weights (1, 3) -> 1 * 1 / 4 + 3 * 3 / 4; then est == fresh -> 0
    std::vector<double> est = {0.0, 0.0}, fresh = {1.0, 3.0};
    CHECK(update_estimates(est, fresh) == 2.5 && est == fresh, "two-entry table");
    CHECK(update_estimates(est, fresh) == 0.0, "unchanged estimates");
  }
  std::uniform_real_distribution<double> u(-1.0, 2.0);
  for (int t = 0; t < 100; ++t) {
    const size_t n = (size_t)(rng() % 40);
    std::vector<double> est(n), fresh(n);
    for (size_t i = 0; i < n; ++i) est[i] = u(rng), fresh[i] = u(rng);
    double w = 0.0, m = std::numeric_limits<double>::quiet_NaN();
    for (size_t i = 0; i < n; ++i) {   // the expression of DoubleWeightedMean.increment, written out
      const double datum = std::fabs(fresh[i] - est[i]), weight = fresh[i] > 0.0 ? fresh[i] : 0.0, old = w;
      w += weight;
      m = old <= 0 ? datum : m * old / w + datum * weight / w;
    }
    const double got = update_estimates(est, fresh);
    CHECK(std::memcmp(&got, &m, sizeof(double)) == 0 && est == fresh, "table of %zu: %.17g against %.17g", n, got, m);
  }
}

// ---- the loop over a scripted driver ----
// Iteration i (from 1) yields the one-entry sample value[i - 1]: the mean is |value[i - 1] - value[i - 2]| (the table starts at 0).
struct Script {
  std::vector<double> value;
  int cancel_before_half = -1;   // the cancelled() call (counted from 0, two per iteration) that reports a cancellation
  bool has_callback = true;
  // what happened
  std::string log;               // c = cancelled(), X / Y = half-iteration, s = sample, 0 / 1 = count, r = report, ! = callback
  int cancel_calls = 0, samples = 0, callbacks = 0, callback_reads = 0;
  std::vector<double> seen_mean;
  std::vector<int> seen_iteration;
  std::string failure;
  bool cancel_cleared = false;

  int fail(int code, const char* msg) { failure = msg; return code; }
  void clear_cancel() { cancel_cleared = true; }
  int cancelled() { log += 'c'; return cancel_calls++ == cancel_before_half ? MALS_CANCELLED : MALS_OK; }
  int half_iteration(int side) { log += side == MALS_SIDE_X ? 'X' : 'Y'; return MALS_OK; }
  int sample_dots(const int64_t*, int32_t n_users, const int64_t*, int32_t n_items, double* out) {
    log += 's';
    for (int i = 0; i < n_users * n_items; ++i) out[i] = value[(size_t)samples];
    ++samples;
    return MALS_OK;
  }
  static void on_iteration(void* user, const mals_iteration_info* info) {
    Script* s = static_cast<Script*>(user);
    s->log += '!';
    ++s->callbacks;
    s->seen_mean.push_back(info->avg_abs_difference);
    s->seen_iteration.push_back(info->iteration);
    CHECK(info->struct_size == (int32_t)sizeof(*info) && info->devices == 7 && info->x_rows == 11 && info->seconds >= 0.0, "report fields");
  }
  mals_iteration_fn callback(void** user) {
    ++callback_reads;
    *user = this;
    return has_callback ? &Script::on_iteration : nullptr;
  }
  void count(int point) { log += (char)('0' + point); }
  void report(mals_iteration_info* info) { log += 'r'; info->devices = 7; info->x_rows = 11; }
};

struct Outcome {
  int rc, iterations;
  double convergence;
};
static Outcome run_loop(Script& s, double threshold, int max_iterations, int random_y, int iterate = 1) {
  const int64_t user = 0, item = 0;
  int32_t it = -1;
  double conv = -1.0;
  const int rc = factorize_loop(s, threshold, max_iterations, random_y, iterate, &user, 1, &item, 1, &it, &conv);
  return {rc, it, conv};
}

static void test_loop() {
  {  // the mean never falls below the threshold: max_iterations ends it
    Script s;
    s.value = {1, 2, 3, 4, 5, 6};
    const Outcome o = run_loop(s, 0.5, 4, 0);
    CHECK(o.rc == MALS_OK && o.iterations == 4 && o.convergence == 1.0 && s.samples == 4, "max_iterations: rc %d, %d iterations", o.rc, o.iterations);
    CHECK(s.log == "0cX1cYsr!0cX1cYsr!0cX1cYsr!0cX1cYsr!", "order of an iteration: %s", s.log.c_str());
    CHECK(s.callback_reads == 4 && s.cancel_cleared, "the callback is read once per iteration (%d reads)", s.callback_reads);
  }
  {  // a non-finite mean ends it (before max_iterations, and although NaN < threshold is false)
    Script s;
    s.value = {1, std::numeric_limits<double>::infinity(), 3, 4};
    const Outcome o = run_loop(s, 0.5, 0, 0);
    CHECK(o.rc == MALS_OK && o.iterations == 2 && !std::isfinite(o.convergence), "non-finite mean: %d iterations", o.iterations);
  }
  {  // the first mean is below the threshold: random_y goes on to the next one, which stops
    Script s;
    s.value = {0.01, 0.02, 5, 6};
    const Outcome o = run_loop(s, 0.5, 0, 1);
    CHECK(o.rc == MALS_OK && o.iterations == 2 && o.convergence == 0.01, "random_y: %d iterations, mean %g", o.iterations, o.convergence);
    Script t;
    t.value = s.value;
    const Outcome p = run_loop(t, 0.5, 0, 0);
    CHECK(p.rc == MALS_OK && p.iterations == 1 && p.convergence == 0.01, "not random_y: %d iterations", p.iterations);
  }
  {  // ... but max_iterations = 1 holds with random_y too
    Script s;
    s.value = {0.01, 0.02};
    CHECK(run_loop(s, 0.5, 1, 1).iterations == 1, "random_y with max_iterations 1");
  }
  {  // the first mean below the threshold stops, not an earlier or a later one; the callback saw every mean, the last included
    Script s;
    s.value = {4, 2, 1, 0.75, 0.7, 0.69};
    const Outcome o = run_loop(s, 0.3, 0, 0);
    CHECK(o.rc == MALS_OK && o.iterations == 4 && o.convergence == 0.25, "threshold: %d iterations, mean %g", o.iterations, o.convergence);
    CHECK(s.seen_mean == std::vector<double>({4, 2, 1, 0.25}) && s.seen_iteration == std::vector<int>({1, 2, 3, 4}), "the callback's means");
  }
  {  // no callback: no counters are read, nothing is reported
    Script s;
    s.has_callback = false;
    s.value = {1, 1};
    const Outcome o = run_loop(s, 0.5, 0, 0);
    CHECK(o.iterations == 2 && s.log == "cXcYscXcYs" && s.callbacks == 0, "without a callback: %s", s.log.c_str());
  }
  for (int at = 0; at < 4; ++at) {  // cancelled before the X or the Y half of iteration 1 or 2: the completed count stays
    Script s;
    s.value = {1, 2, 3};
    s.cancel_before_half = at;
    const Outcome o = run_loop(s, 0.5, 0, 0);
    CHECK(o.rc == MALS_CANCELLED && o.iterations == at / 2 && s.samples == at / 2, "cancel at check %d: rc %d, %d iterations", at, o.rc, o.iterations);
    CHECK(s.log.back() == 'c' && (at % 2 == 0 || s.log[s.log.size() - 3] == 'X'), "cancel at check %d: %s", at, s.log.c_str());
    if (at < 2) CHECK(std::isnan(o.convergence), "no iteration completed: convergence %g", o.convergence);
    else CHECK(o.convergence == 1.0, "convergence of the completed iteration: %g", o.convergence);
  }
  {  // arguments: refused before anything runs, outputs at their initial values
    for (double bad : {0.0, 1.0, -0.1, std::numeric_limits<double>::quiet_NaN()}) {
      Script s;
      const Outcome o = run_loop(s, bad, 3, 0);
      CHECK(o.rc == MALS_INVALID_ARG && o.iterations == 0 && std::isnan(o.convergence) && s.log.empty() && s.failure == "threshold must be in (0,1)",
            "threshold %g: rc %d", bad, o.rc);
    }
    Script s;
    int32_t it = -1;
    const int64_t item = 0;
    CHECK(factorize_loop(s, 0.5, 3, 0, 1, nullptr, 1, &item, 1, &it, nullptr) == MALS_INVALID_ARG && s.failure == "bad convergence sample" && it == 0, "null users");
    CHECK(factorize_loop(s, 0.5, 3, 0, 1, nullptr, -1, &item, 1, nullptr, nullptr) == MALS_INVALID_ARG, "negative sample size");
  }
  {  // iterate == 0: one X half, nothing else
    Script s;
    const Outcome o = run_loop(s, 0.5, 3, 0, 0);
    CHECK(o.rc == MALS_OK && o.iterations == 0 && s.log == "X" && s.cancel_cleared, "iterate 0: %s", s.log.c_str());
  }
  {  // an empty sample: the mean is NaN, which ends the run after one iteration
    Script s;
    int32_t it = -1;
    double conv = 0.0;
    CHECK(factorize_loop(s, 0.5, 0, 0, 1, nullptr, 0, nullptr, 0, &it, &conv) == MALS_OK && it == 1 && std::isnan(conv), "empty sample: %d", it);
  }
  CHECK(should_stop(3, 0.9, 0.5, 3, false) && !should_stop(2, 0.9, 0.5, 3, false) && !should_stop(1, 0.1, 0.5, 0, true) && should_stop(2, 0.1, 0.5, 0, true) &&
            !should_stop(5, 0.5, 0.5, 0, false), "stop rules");
}

int main(int argc, char** argv) {
  const unsigned long seed = argc > 1 ? std::strtoul(argv[1], nullptr, 10) : 1;
  std::mt19937_64 rng(seed);
  test_owner_of(rng);
  test_chunks(rng);
  test_csr_slice(rng);
  test_owner_runs(rng);
  test_plan_shards(rng);
  test_weighted_mean(rng);
  test_loop();
  std::printf("checks %d failures %d\n", checks, failures);
  return failures ? 1 : 0;
}
