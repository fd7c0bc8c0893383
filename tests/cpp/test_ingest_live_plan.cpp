// The host logic of mals_ingest_apply (csrc/ingest_live_plan.h) and the slot functions of the id directory
// (csrc/ids_kernels.h, which a host compiler sees without its kernels) with no device.  Stand-alone host program, built
// with -fsanitize=address,undefined by tests/test_ingest_live_plan_host.py.  usage: test_ingest_live_plan <seed>
//
// Checked against naive restatements written here:
//   * the classification and the cut into runs, on seeded streams of 0, 1, 2, 7, 64 and 300 records with no, a quarter, half
//     and only removes, strictly alternating single records, and unknown rows on none, a third or all of the removes: the runs
//     expanded back to records are the stream without its dropped removes, in order; neighbouring runs differ in kind;
//     a set run is contiguous in the set records and a remove run in the removes passed on; the dropped count is right.
//     PINNED: a dropped remove between two set runs cuts nothing -- set, dropped remove, set is ONE run.
//   * the directory built from the slot functions (find, the batch's claim, first position, distinct insert, grown slots) as
//     the host driver of ids_host.h uses them, single-threaded, against std::unordered_map: ids 0, -1, INT64_MIN, INT64_MAX;
//     a family of 10 ids whose home is the LAST slot, found by searching with the hash, so that their chain wraps to slot 0;
//     directories of 1, 32, 33, 63, 64, 65 ids (32 -> 64 slots, 33 -> 128); a resolve into a directory of exactly 2 n = slots
//     that rebuilds at 128 slots, and one of 300 new ids into 32 that lands at 1024; seeded batches of known and new ids
//     with repeats.  After every resolve every id ever seen is found at its row, absent ids are not, row -> id agrees.
//   * first-appearance numbering under EVERY order of inserting a batch's positions (7 positions, 5040 orders, repeats and a
//     known id among them): the rows never differ from the sequential dictionary's.
#include "../../myrrix-recommender_amd/csrc/ids_kernels.h"
#include "../../myrrix-recommender_amd/csrc/ingest_live_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <random>
#include <unordered_map>

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

// ---- the cut ------------------------------------------------------------------------------------------------------------------
// value: NaN = remove; known[t]: the remove's user and item have rows
static void check_cut(const std::vector<float>& value, const std::vector<char>& known, const char* what) {
  const int64_t n = (int64_t)value.size();
  LiveClasses c;
  live_classify(n, value.data(), c);
  // the classes, naively
  std::vector<int64_t> sp, rp;
  for (int64_t t = 0; t < n; ++t) (value[(size_t)t] != value[(size_t)t] ? rp : sp).push_back(t);
  CHECK(c.set_pos == sp && c.rem_pos == rp, "%s n %lld: classes", what, (long long)n);
  std::vector<int64_t> ru(rp.size()), ri(rp.size());
  for (size_t j = 0; j < rp.size(); ++j) {
    const bool k = known[(size_t)rp[j]] != 0;
    ru[j] = k ? (int64_t)(j % 5) : (j % 2 ? -1 : 3);   // an unknown remove lacks its user, or its item, or both
    ri[j] = k ? (int64_t)(j % 3) : (j % 2 ? 2 : -1);
    if (!k && j % 7 == 0) ru[j] = ri[j] = -1;
  }
  LivePlan p;
  live_cut(c, ru.data(), ri.data(), p);
  // the stream without its dropped removes, naively: (kind, record)
  std::vector<std::pair<bool, int64_t>> want;
  int64_t dropped = 0;
  for (int64_t t = 0; t < n; ++t) {
    const bool is_set = value[(size_t)t] == value[(size_t)t];
    if (!is_set && !known[(size_t)t]) {
      ++dropped;
      continue;
    }
    want.push_back({is_set, t});
  }
  CHECK(p.dropped == dropped, "%s n %lld: dropped %lld, want %lld", what, (long long)n, (long long)p.dropped, (long long)dropped);
  std::vector<std::pair<bool, int64_t>> got;
  int64_t next_set = 0, next_rem = 0;
  size_t want_runs = 0;
  for (size_t j = 0; j < want.size(); ++j) want_runs += j == 0 || want[j].first != want[j - 1].first ? 1 : 0;
  for (size_t r = 0; r < p.runs.size(); ++r) {
    const LiveRun& run = p.runs[r];
    CHECK(run.begin < run.end, "%s: an empty run", what);
    CHECK(r == 0 || p.runs[r - 1].is_set != run.is_set, "%s: neighbouring runs of one kind", what);
    int64_t& next = run.is_set ? next_set : next_rem;
    CHECK(run.begin == next, "%s: run %zu begins at %lld, the kind's next is %lld", what, r, (long long)run.begin, (long long)next);
    next = run.end;
    for (int64_t j = run.begin; j < run.end; ++j) {
      if (run.is_set) {
        if (j < (int64_t)c.set_pos.size()) got.push_back({true, c.set_pos[(size_t)j]});
      } else if (j < (int64_t)p.rem_keep.size() && p.rem_keep[(size_t)j] < (int64_t)c.rem_pos.size()) {
        got.push_back({false, c.rem_pos[(size_t)p.rem_keep[(size_t)j]]});
      }
    }
  }
  CHECK(got == want, "%s n %lld: the runs are not the stream", what, (long long)n);
  CHECK(p.runs.size() == want_runs, "%s n %lld: %zu runs, maximal runs are %zu", what, (long long)n, p.runs.size(), want_runs);
  CHECK(next_set == (int64_t)c.set_pos.size() && next_rem == (int64_t)p.rem_keep.size(), "%s: records left over", what);
}

static void test_cut(std::mt19937_64& rng) {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (int64_t n : {0, 1, 2, 7, 64, 300})
    for (double p_rem : {0.0, 0.25, 0.5, 1.0})
      for (int unknown : {0, 3, 1}) {   // none / a third / all of the removes name an unknown id
        std::vector<float> v((size_t)n);
        std::vector<char> known((size_t)n, 1);
        for (int64_t t = 0; t < n; ++t) {
          v[(size_t)t] = std::uniform_real_distribution<double>(0, 1)(rng) < p_rem ? nan : (float)(t % 5) - 1.0f;
          if (unknown) known[(size_t)t] = (rng() % (uint64_t)unknown) != 0 ? 1 : 0;
        }
        check_cut(v, known, "seeded");
      }
  {   // alternating single records
    std::vector<float> v(41);
    for (size_t t = 0; t < v.size(); ++t) v[t] = t % 2 ? nan : 1.0f;
    check_cut(v, std::vector<char>(v.size(), 1), "alternating");
    LiveClasses c;
    live_classify((int64_t)v.size(), v.data(), c);
    std::vector<int64_t> rows(c.rem_pos.size(), 0);
    LivePlan p;
    live_cut(c, rows.data(), rows.data(), p);
    CHECK(p.runs.size() == v.size(), "alternating: %zu runs of %zu records", p.runs.size(), v.size());
  }
  {   // PINNED: set, dropped remove, set -> one set run; with the remove known -> three runs
    const float v[5] = {1.0f, 2.0f, nan, 3.0f, 0.0f};
    LiveClasses c;
    live_classify(5, v, c);
    const int64_t no = -1, yes = 4;
    LivePlan p;
    live_cut(c, &no, &yes, p);
    CHECK(p.runs.size() == 1 && p.runs[0].is_set && p.runs[0].begin == 0 && p.runs[0].end == 4 && p.dropped == 1 && p.rem_keep.empty(),
          "a dropped remove must not cut the set run (%zu runs)", p.runs.size());
    live_cut(c, &yes, &no, p);
    CHECK(p.runs.size() == 1 && p.dropped == 1, "a remove without an item row is dropped too");
    live_cut(c, &yes, &yes, p);
    CHECK(p.runs.size() == 3 && p.runs[1].is_set == false && p.runs[1].begin == 0 && p.runs[1].end == 1 && p.runs[2].begin == 2 && p.runs[2].end == 4,
          "a known remove cuts");
  }
}

// ---- the directory, as ids_host.h drives the slot functions ---------------------------------------------------------------------
struct Dir {
  std::vector<unsigned long long> table;
  uint64_t slots = 0;
  std::vector<int64_t> row_id;
};

// mals_ids_set; -1 or the smallest row that repeats an earlier one
static int64_t dir_set(Dir& d, const std::vector<int64_t>& ids) {
  const int64_t n = (int64_t)ids.size();
  Dir nd;
  nd.slots = gen_table_slots(n);
  nd.table.assign((size_t)(2 * nd.slots), 0ull);
  std::vector<uint64_t> slot((size_t)n);
  for (int64_t t = n - 1; t >= 0; --t) slot[(size_t)t] = ids_batch_claim(nd.table.data(), nd.slots - 1, ids.data(), t);   // (back to front: any order does)
  for (int64_t t = 0; t < n; ++t)
    if (ids_batch_first_pos(nd.table.data(), slot[(size_t)t]) != t) return t;
  for (uint64_t s = 0; s < nd.slots; ++s)   // gen_fill_keys_kernel
    if (nd.table[2 * s + 1]) nd.table[2 * s] = (unsigned long long)ids[(size_t)(nd.table[2 * s + 1] - 1)];
  nd.row_id = ids;
  d = nd;
  return -1;
}

// mals_ids_resolve with the batch's positions visited in `order`; -> rows added
static int64_t dir_resolve(Dir& d, const std::vector<int64_t>& ids, const std::vector<int64_t>& order, std::vector<int64_t>& rows, int* rebuilt) {
  const int64_t n = (int64_t)ids.size();
  const uint64_t bslots = gen_table_slots(n);
  std::vector<unsigned long long> batch((size_t)(2 * bslots), 0ull);
  std::vector<uint64_t> slot((size_t)n, IDS_NO_SLOT);
  rows.assign((size_t)n, -2);
  for (int64_t t : order) {   // PROBE
    const int64_t r = ids_find(d.table.data(), d.slots - 1, ids[(size_t)t]);
    rows[(size_t)t] = r;
    slot[(size_t)t] = r >= 0 ? IDS_NO_SLOT : ids_batch_claim(batch.data(), bslots - 1, ids.data(), t);
  }
  std::vector<unsigned> first((size_t)n);
  for (int64_t t = 0; t < n; ++t) first[(size_t)t] = slot[(size_t)t] != IDS_NO_SLOT && ids_batch_first_pos(batch.data(), slot[(size_t)t]) == t;
  const int64_t n_rows = (int64_t)d.row_id.size();
  int64_t rank = 0;
  for (int64_t t = 0; t < n; ++t)   // SCAN + ASSIGN
    if (first[(size_t)t]) {
      rows[(size_t)t] = n_rows + rank++;
      d.row_id.push_back(ids[(size_t)t]);
    }
  for (int64_t t : order)   // FOLLOW
    if (slot[(size_t)t] != IDS_NO_SLOT && !first[(size_t)t]) rows[(size_t)t] = rows[(size_t)ids_batch_first_pos(batch.data(), slot[(size_t)t])];
  const uint64_t new_slots = ids_grown_slots(d.slots, n_rows + rank);
  int64_t from = n_rows;
  if (new_slots != d.slots) {
    d.table.assign((size_t)(2 * new_slots), 0ull);
    d.slots = new_slots;
    from = 0;
    if (rebuilt) ++*rebuilt;
  }
  for (int64_t r = n_rows + rank - 1; r >= from; --r) ids_insert_distinct(d.table.data(), d.slots - 1, d.row_id[(size_t)r], r);   // INSERT
  return rank;
}

static std::vector<int64_t> iota_order(size_t n) {
  std::vector<int64_t> o(n);
  std::iota(o.begin(), o.end(), 0);
  return o;
}

// every id of the model is found at its row, row -> id agrees, the probes of absent ids miss, the table is at most half full
static void check_dir(const Dir& d, const std::unordered_map<int64_t, int64_t>& model, const std::vector<int64_t>& absent, const char* what) {
  CHECK(d.row_id.size() == model.size(), "%s: %zu rows, the model has %zu", what, d.row_id.size(), model.size());
  CHECK(2 * (uint64_t)d.row_id.size() <= d.slots && (d.slots & (d.slots - 1)) == 0 && d.slots >= 64, "%s: %zu ids in %llu slots", what, d.row_id.size(),
        (unsigned long long)d.slots);
  uint64_t taken = 0;
  for (uint64_t s = 0; s < d.slots; ++s) taken += d.table[2 * s + 1] != 0 ? 1 : 0;
  CHECK(taken == d.row_id.size(), "%s: %llu slots taken for %zu ids", what, (unsigned long long)taken, d.row_id.size());
  for (const auto& kv : model) {
    const int64_t r = ids_find(d.table.data(), d.slots - 1, kv.first);
    CHECK(r == kv.second, "%s: id %lld at row %lld, want %lld", what, (long long)kv.first, (long long)r, (long long)kv.second);
    CHECK(kv.second >= 0 && kv.second < (int64_t)d.row_id.size() && d.row_id[(size_t)kv.second] == kv.first, "%s: row -> id of row %lld", what,
          (long long)kv.second);
  }
  for (int64_t id : absent)
    if (!model.count(id)) CHECK(ids_find(d.table.data(), d.slots - 1, id) == -1, "%s: absent id %lld found", what, (long long)id);
}

// a resolve against the sequential dictionary
static void check_resolve(Dir& d, std::unordered_map<int64_t, int64_t>& model, const std::vector<int64_t>& ids, const std::vector<int64_t>& order,
                          const char* what, int* rebuilt = nullptr) {
  std::vector<int64_t> want(ids.size());
  int64_t want_new = 0;
  for (size_t t = 0; t < ids.size(); ++t) {
    auto it = model.find(ids[t]);
    if (it == model.end()) {
      it = model.emplace(ids[t], (int64_t)model.size()).first;
      ++want_new;
    }
    want[t] = it->second;
  }
  std::vector<int64_t> rows;
  const int64_t got_new = dir_resolve(d, ids, order, rows, rebuilt);
  CHECK(got_new == want_new, "%s: %lld new rows, want %lld", what, (long long)got_new, (long long)want_new);
  CHECK(rows == want, "%s: the rows differ from the sequential dictionary's", what);
}

static std::vector<int64_t> family_of_home(uint64_t slots, uint64_t home, size_t count, int64_t from) {
  std::vector<int64_t> f;
  for (int64_t id = from; f.size() < count; ++id)
    if ((gen_hash(id) & (slots - 1)) == home) f.push_back(id);
  return f;
}

static void test_directory(std::mt19937_64& rng) {
  const int64_t lo = std::numeric_limits<int64_t>::min(), hi = std::numeric_limits<int64_t>::max();
  const std::vector<int64_t> extremes = {0, -1, lo, hi};
  CHECK(gen_table_slots(32) == 64 && gen_table_slots(33) == 128 && ids_grown_slots(64, 32) == 64 && ids_grown_slots(64, 33) == 128 &&
            ids_grown_slots(64, 332) == 1024 && ids_grown_slots(0, 1) == 64,
        "slot counts");
  for (int64_t n : {1, 32, 33, 63, 64, 65}) {
    std::vector<int64_t> ids;
    std::unordered_map<int64_t, int64_t> model;
    for (int64_t id : extremes)
      if ((int64_t)ids.size() < n) ids.push_back(id);
    while ((int64_t)ids.size() < n) {
      const int64_t id = (int64_t)rng();
      if (std::find(ids.begin(), ids.end(), id) == ids.end()) ids.push_back(id);
    }
    std::shuffle(ids.begin(), ids.end(), rng);
    for (size_t r = 0; r < ids.size(); ++r) model[ids[r]] = (int64_t)r;
    Dir d;
    CHECK(dir_set(d, ids) == -1, "set of %lld distinct ids refused", (long long)n);
    CHECK(d.slots == gen_table_slots(n), "set: slots");
    std::vector<int64_t> absent = extremes;
    for (int j = 0; j < 50; ++j) absent.push_back((int64_t)rng());
    check_dir(d, model, absent, "after set");
    // a duplicate: the smallest row that repeats an earlier one
    if (n >= 3) {
      std::vector<int64_t> twice = ids;
      const int64_t mid = std::min<int64_t>(n / 2 + 1, n - 1);
      twice[(size_t)n - 1] = twice[0];
      twice[(size_t)mid] = twice[1];   // rows mid and n - 1 repeat rows 1 and 0: mid is the smaller
      Dir e;
      CHECK(dir_set(e, twice) == mid, "set with a duplicate names row %lld", (long long)mid);
    }
    // resolves: all known, all new, one new id many times, interleaved with repeats, the extremes
    std::vector<int64_t> batch(ids.begin(), ids.begin() + std::min<int64_t>(n, 20));
    check_resolve(d, model, batch, iota_order(batch.size()), "all known");
    batch.clear();
    for (int j = 0; j < 40; ++j) batch.push_back((int64_t)rng());
    check_resolve(d, model, batch, iota_order(batch.size()), "all new");
    batch.assign(500, (int64_t)rng());
    check_resolve(d, model, batch, iota_order(batch.size()), "one new id 500 times");
    batch.clear();
    std::vector<int64_t> pool = extremes;
    for (int j = 0; j < 30; ++j) pool.push_back((int64_t)rng());
    for (int j = 0; j < 200; ++j) batch.push_back(j % 3 ? pool[rng() % pool.size()] : d.row_id[rng() % d.row_id.size()]);
    std::vector<int64_t> order = iota_order(batch.size());
    std::shuffle(order.begin(), order.end(), rng);
    check_resolve(d, model, batch, order, "interleaved");
    check_dir(d, model, absent, "after the resolves");
  }
  {   // exactly 2 n = slots, then one more id: a rebuild at 128; then 300 new ids into 32: 1024 slots at once
    for (int big = 0; big < 2; ++big) {
      std::vector<int64_t> ids;
      std::unordered_map<int64_t, int64_t> model;
      for (int64_t r = 0; r < 32; ++r) {
        ids.push_back(1000 + 7 * r);
        model[ids.back()] = r;
      }
      Dir d;
      CHECK(dir_set(d, ids) == -1 && d.slots == 64, "32 ids: 64 slots");
      int rebuilt = 0;
      check_resolve(d, model, {ids[5], ids[31]}, {1, 0}, "known ids at 2 n = slots", &rebuilt);
      CHECK(rebuilt == 0 && d.slots == 64, "no rebuild at exactly half full");
      std::vector<int64_t> batch;
      for (int j = 0; j < (big ? 300 : 1); ++j) batch.push_back(-5000 - j);
      check_resolve(d, model, batch, iota_order(batch.size()), "past half full", &rebuilt);
      CHECK(rebuilt == 1 && d.slots == (big ? 1024u : 128u), "rebuilt to %llu slots", (unsigned long long)d.slots);
      check_dir(d, model, {0, -1, 999, 1001}, "after the rebuild");
    }
  }
  {   // a family whose home is the last slot: the chain wraps to slot 0; in the directory and in the batch's table
    const std::vector<int64_t> fam = family_of_home(64, 63, 10, 1);
    std::unordered_map<int64_t, int64_t> model;
    for (size_t r = 0; r < fam.size(); ++r) model[fam[r]] = (int64_t)r;
    Dir d;
    CHECK(dir_set(d, fam) == -1 && d.slots == 64, "the family installs");
    CHECK(d.table[2 * 63 + 1] != 0 && d.table[1] != 0 && d.table[2 * 8 + 1] != 0 && d.table[2 * 9 + 1] == 0, "the chain wraps past the last slot");
    const std::vector<int64_t> more = family_of_home(64, 63, 18, fam.back() + 1);   // same home in the batch's table (64 slots for <= 32)
    check_dir(d, model, more, "wrapped family");
    std::vector<int64_t> batch;
    for (int j = 0; j < 30; ++j) batch.push_back(j % 2 ? more[(size_t)(j / 2) % more.size()] : fam[(size_t)j % fam.size()]);
    std::vector<int64_t> order = iota_order(batch.size());
    std::shuffle(order.begin(), order.end(), rng);
    check_resolve(d, model, batch, order, "wrapped family, resolve");
    check_dir(d, model, {0, -1}, "wrapped family, after the resolve");
  }
}

// ---- every order ----------------------------------------------------------------------------------------------------------------
static void test_every_order() {
  const std::vector<int64_t> base = {11, 22, 33};
  const std::vector<int64_t> batch = {70, 80, 70, -1, 80, 22, 90};   // a, b, a, c, b, known, d
  const std::vector<int64_t> want = {3, 4, 3, 5, 4, 1, 6};
  std::vector<int64_t> order = iota_order(batch.size());
  int64_t orders = 0;
  do {
    Dir d;
    dir_set(d, base);
    std::vector<int64_t> rows;
    const int64_t n_new = dir_resolve(d, batch, order, rows, nullptr);
    CHECK(n_new == 4 && rows == want, "order %lld: the rows depend on the order", (long long)orders);
    CHECK(d.row_id == std::vector<int64_t>({11, 22, 33, 70, 80, -1, 90}), "order %lld: row -> id", (long long)orders);
    ++orders;
  } while (std::next_permutation(order.begin(), order.end()));
  CHECK(orders == 5040, "orders");
}

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
  std::mt19937_64 rng(seed);
  test_cut(rng);
  test_directory(rng);
  test_every_order();
  std::printf("checks %d failures %d\n", checks, failures);
  return failures ? 1 : 0;
}
