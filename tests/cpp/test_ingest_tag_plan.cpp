// The host logic of mals_ingest_apply with MALS_INGEST_OPT_LIVE_TAGS (csrc/ingest_live_plan.h: live_classify_kinds,
// live_run_kinds, and live_cut over their classes) with no device.  Stand-alone host program, built with
// -fsanitize=address,undefined by tests/test_tags_live_host.py.  usage: test_ingest_tag_plan <seed>
//
// Checked against a naive restatement written here -- ServerRecommender.ingest line by line: a tag record (kind 1 or 2) whose
// value is NaN does nothing; any other record with a NaN value is a remove, which does nothing either when its user or item
// has no row; everything else is a set; a write call begins wherever the kind of write changes -- on seeded streams of 0, 1,
// 2, 7, 64 and 300 records with no, a tenth, half and only tag records, NaN on none, a third and all of them:
//   * the set and remove positions, the kinds of the sets and the three tag counts;
//   * the runs expanded back to records are the naive list of writes, in order, and the number of runs its write calls;
//   * live_run_kinds is nullptr exactly for a run without a tag, else points at the run's first kind.
// PINNED: set, ignored tag remove, set is ONE run; remove, ignored tag remove, remove is ONE run; with all kinds 0 the classes
// are live_classify's.
#include "../../myrrix-recommender_amd/csrc/ingest_live_plan.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

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

static const float NaN = std::numeric_limits<float>::quiet_NaN();

struct Write {
  bool is_set;
  int64_t pos;   // the record
  bool operator==(const Write& o) const { return is_set == o.is_set && pos == o.pos; }
};

// known[t]: a remove's user and item have rows
static void check_stream(const std::vector<float>& value, const std::vector<uint8_t>& kind, const std::vector<char>& known, const char* what) {
  const int64_t n = (int64_t)value.size();
  // line by line
  std::vector<Write> want;
  std::vector<uint8_t> want_kind;
  std::vector<int64_t> sp, rp;
  int64_t want_calls = 0, item_tags = 0, user_tags = 0, ignored = 0, dropped = 0;
  int last = -1;
  for (int64_t t = 0; t < n; ++t) {
    const bool nan = value[(size_t)t] != value[(size_t)t];
    if (nan && kind[(size_t)t] != 0) {
      ++ignored;
      continue;
    }
    if (nan) {
      rp.push_back(t);
      if (!known[(size_t)t]) {
        ++dropped;
        continue;
      }
    } else {
      sp.push_back(t);
      want_kind.push_back(kind[(size_t)t]);
      item_tags += kind[(size_t)t] == 1;
      user_tags += kind[(size_t)t] == 2;
    }
    want.push_back({!nan, t});
    want_calls += last != (nan ? 0 : 1);
    last = nan ? 0 : 1;
  }
  LiveClasses c;
  std::vector<uint8_t> set_kind;
  LiveTagCounts tags;
  live_classify_kinds(n, value.data(), kind.data(), c, set_kind, tags);
  CHECK(c.set_pos == sp && c.rem_pos == rp && set_kind == want_kind, "%s n %lld: classes", what, (long long)n);
  CHECK(tags.item_tag_sets == item_tags && tags.user_tag_sets == user_tags && tags.removes_ignored == ignored, "%s n %lld: tag counts", what, (long long)n);
  std::vector<int64_t> ru(rp.size()), ri(rp.size());
  for (size_t j = 0; j < rp.size(); ++j) {
    const bool k = known[(size_t)rp[j]] != 0;
    ru[j] = k ? (int64_t)(j % 5) : (j % 2 ? -1 : 3);
    ri[j] = k ? (int64_t)(j % 3) : (j % 2 ? 2 : -1);
  }
  LivePlan p;
  live_cut(c, ru.data(), ri.data(), p);
  CHECK(p.dropped == dropped && (int64_t)p.runs.size() == want_calls, "%s n %lld: %lld runs (want %lld), %lld dropped (want %lld)", what, (long long)n,
        (long long)p.runs.size(), (long long)want_calls, (long long)p.dropped, (long long)dropped);
  std::vector<Write> got;
  for (size_t r = 0; r < p.runs.size(); ++r) {
    const LiveRun& run = p.runs[r];
    CHECK(run.begin < run.end && (r == 0 || p.runs[r - 1].is_set != run.is_set), "%s: run %zu", what, r);
    bool any_tag = false;
    for (int64_t j = run.begin; j < run.end; ++j) {
      got.push_back({run.is_set, run.is_set ? c.set_pos[(size_t)j] : c.rem_pos[(size_t)p.rem_keep[(size_t)j]]});
      any_tag = any_tag || (run.is_set && set_kind[(size_t)j] != 0);
    }
    if (run.is_set) {
      const uint8_t* rk = live_run_kinds(set_kind, run.begin, run.end);
      CHECK(any_tag ? rk == set_kind.data() + run.begin : rk == nullptr, "%s: kinds of run %zu", what, r);
    }
  }
  CHECK(got == want, "%s n %lld: the writes", what, (long long)n);
}

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
  std::mt19937_64 rng(seed);
  auto coin = [&](double p) { return std::uniform_real_distribution<double>(0.0, 1.0)(rng) < p; };
  // pinned
  check_stream({1.f, NaN, 2.f}, {0, 1, 0}, {1, 1, 1}, "set, tag remove, set");
  check_stream({NaN, NaN, NaN}, {0, 2, 0}, {1, 1, 1}, "remove, tag remove, remove");
  check_stream({1.f, NaN, NaN, 1.f}, {2, 2, 1, 1}, {1, 1, 1, 1}, "tag sets around tag removes");
  check_stream({NaN, NaN}, {1, 2}, {1, 1}, "only tag removes");
  {
    LiveClasses a, b;
    std::vector<uint8_t> sk;
    LiveTagCounts tg;
    const std::vector<float> v = {1.f, NaN, 0.f, NaN, -1.f};
    const std::vector<uint8_t> k(5, 0);
    live_classify(5, v.data(), a);
    live_classify_kinds(5, v.data(), k.data(), b, sk, tg);
    CHECK(a.set_pos == b.set_pos && a.rem_pos == b.rem_pos && sk == std::vector<uint8_t>(3, 0), "kinds all 0");
    CHECK(tg.item_tag_sets == 0 && tg.user_tag_sets == 0 && tg.removes_ignored == 0, "kinds all 0: counts");
  }
  for (int rep = 0; rep < 40; ++rep)
    for (int64_t n : {0, 1, 2, 7, 64, 300})
      for (double p_tag : {0.0, 0.1, 0.5, 1.0})
        for (double p_nan : {0.0, 1.0 / 3, 1.0})
          for (double p_unknown : {0.0, 1.0 / 3}) {
            std::vector<float> value((size_t)n);
            std::vector<uint8_t> kind((size_t)n);
            std::vector<char> known((size_t)n);
            for (int64_t t = 0; t < n; ++t) {
              value[(size_t)t] = coin(p_nan) ? NaN : (float)(t % 5) - 1.f;
              kind[(size_t)t] = coin(p_tag) ? (uint8_t)(1 + (int)coin(0.5)) : (uint8_t)0;
              known[(size_t)t] = coin(p_unknown) ? 0 : 1;
            }
            check_stream(value, kind, known, "seeded");
          }
  std::printf("checks %d failures %d\n", checks, failures);
  return failures ? 1 : 0;
}
