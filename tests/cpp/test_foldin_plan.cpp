// The host logic of the online write path (csrc/foldin_plan.h) with no device: the level plan of a batch, the known-item
// overlay, the status word of an update.  Stand-alone host program, built with -fsanitize=address,undefined by
// tests/test_foldin_plan_host.py.  usage: test_foldin_plan <seed>
//
// Checked against naive restatements written here, on seeded random inputs:
//   * the level plan, for batches of 1, 2, 7, 8, 9, 63, 64, 65 and 1000 updates whose rows come from 1, 3 or 50 distinct users
//     and items (chains as deep as the batch, or nearly flat), small rows and rows up to 2^40 (the hash): `order` is a
//     permutation of [0, n); level(t) = 1 + the larger level of the last earlier update of the same user row and of the same
//     item row (0: none), by a quadratic scan; `off` is the exclusive prefix sum of the level sizes; within a level no two
//     updates share a user row or an item row, and the batch order ascends; n_levels is the largest level; a second plan
//     through a used scratch equals the plan through a fresh one.  Rows are >= 0 only: -1 is the table's empty key, and a
//     batch that reaches the plan has passed the pair check, which lets no negative row through.
//   * the overlay, against a std::map<int64_t, std::set<int32_t>> (a row's whole set once it has one) beside a multiset of
//     additions, over 20 local rows of which the last 5 lie at or past base_rows: after every add, install-then-remove and
//     view, every row's view (additions, possibly repeated, or the whole set; the drop flag) is the model's with the base row
//     folded in; remove answers not-known / removed / emptied as the model does; the override rows are sorted, distinct and
//     exactly the rows the model says differ from their base; clear returns the object to its first answers.
//   * status words: every (code, why, big) with code in 0..2, why in 0..5, big in 0..3 round-trips; a `why` outside the table
//     has the empty text.
#include "../../myrrix-recommender_amd/csrc/foldin_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>

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

// ---- the level plan ---------------------------------------------------------------------------------------------------------
static bool same_plan(const FoldinPlan& a, const FoldinPlan& b) { return a.n_levels == b.n_levels && a.off == b.off && a.order == b.order; }

static void check_plan(FoldinPlanScratch& used, const std::vector<int64_t>& u, const std::vector<int64_t>& i, const char* what) {
  const int64_t n = (int64_t)u.size();
  FoldinPlan p;
  foldin_set_plan(used, n, u.data(), i.data(), p);
  // the definition, by a quadratic scan
  std::vector<uint32_t> level((size_t)n, 0);
  uint32_t deepest = 0;
  for (int64_t t = 0; t < n; ++t) {
    uint32_t lu = 0, li = 0;
    for (int64_t s = t - 1; s >= 0 && !lu; --s)
      if (u[(size_t)s] == u[(size_t)t]) lu = level[(size_t)s];
    for (int64_t s = t - 1; s >= 0 && !li; --s)
      if (i[(size_t)s] == i[(size_t)t]) li = level[(size_t)s];
    level[(size_t)t] = 1 + std::max(lu, li);
    deepest = std::max(deepest, level[(size_t)t]);
  }
  CHECK(p.n_levels == deepest, "%s n %lld: n_levels %u, the deepest level is %u", what, (long long)n, p.n_levels, deepest);
  CHECK((int64_t)p.order.size() == n && p.off.size() == (size_t)p.n_levels + 2, "%s n %lld: sizes", what, (long long)n);
  if ((int64_t)p.order.size() != n || p.off.size() != (size_t)p.n_levels + 2 || p.n_levels != deepest) return;
  std::vector<char> seen((size_t)n, 0);
  for (int64_t t : p.order) {
    CHECK(t >= 0 && t < n && !seen[(size_t)t], "%s n %lld: order is no permutation at %lld", what, (long long)n, (long long)t);
    if (t >= 0 && t < n) seen[(size_t)t] = 1;
  }
  CHECK(p.off[0] == 0 && p.off[1] == 0 && p.off.back() == n, "%s n %lld: off runs from %lld to %lld", what, (long long)n, (long long)p.off[0], (long long)p.off.back());
  for (uint32_t l = 1; l <= p.n_levels; ++l) {
    int64_t size = 0;
    for (int64_t t = 0; t < n; ++t) size += level[(size_t)t] == l;
    CHECK(p.off[l + 1] - p.off[l] == size, "%s n %lld level %u: %lld updates, expected %lld", what, (long long)n, l, (long long)(p.off[l + 1] - p.off[l]), (long long)size);
    if (p.off[l] < 0 || p.off[l + 1] > n || p.off[l + 1] < p.off[l]) continue;
    std::set<int64_t> users, items;
    for (int64_t j = p.off[l]; j < p.off[l + 1]; ++j) {
      const int64_t t = p.order[(size_t)j];
      if (t < 0 || t >= n) continue;
      CHECK(level[(size_t)t] == l, "%s n %lld: update %lld of level %u stands in level %u", what, (long long)n, (long long)t, level[(size_t)t], l);
      CHECK(users.insert(u[(size_t)t]).second, "%s n %lld level %u: user row %lld twice", what, (long long)n, l, (long long)u[(size_t)t]);
      CHECK(items.insert(i[(size_t)t]).second, "%s n %lld level %u: item row %lld twice", what, (long long)n, l, (long long)i[(size_t)t]);
      if (j > p.off[l]) CHECK(p.order[(size_t)j - 1] < t, "%s n %lld level %u: the batch order does not ascend at %lld", what, (long long)n, l, (long long)j);
    }
  }
  FoldinPlanScratch fresh;
  FoldinPlan q;
  foldin_set_plan(fresh, n, u.data(), i.data(), q);
  CHECK(same_plan(p, q), "%s n %lld: a used scratch plans otherwise than a fresh one", what, (long long)n);
}

static void test_plan(std::mt19937_64& rng) {
  FoldinPlanScratch used;   // one scratch through every batch, large and small in turn
  for (int round = 0; round < 6; ++round)
    for (int64_t n : {1, 2, 7, 8, 9, 63, 64, 65, 1000})
      for (int distinct : {1, 3, 50})
        for (int wide = 0; wide < 2; ++wide) {
          // `distinct` row values per side: small ones, or spread up to 2^40
          std::vector<int64_t> uval((size_t)distinct), ival((size_t)distinct);
          for (int d = 0; d < distinct; ++d) {
            uval[(size_t)d] = wide ? (int64_t)(rng() % ((uint64_t)1 << 40)) : (int64_t)d;
            ival[(size_t)d] = wide ? (int64_t)(rng() % ((uint64_t)1 << 40)) : (int64_t)(distinct - 1 - d);
          }
          if (wide) uval[0] = ((int64_t)1 << 40), ival[0] = 0;
          std::vector<int64_t> u((size_t)n), i((size_t)n);
          for (int64_t t = 0; t < n; ++t) {
            u[(size_t)t] = uval[(size_t)(rng() % (uint64_t)distinct)];
            i[(size_t)t] = ival[(size_t)(rng() % (uint64_t)distinct)];
          }
          check_plan(used, u, i, wide ? "wide rows" : "small rows");
        }
  // named: one row on both sides is a chain as deep as the batch; distinct rows are one level
  std::vector<int64_t> same(9, 5), iota(9);
  for (int t = 0; t < 9; ++t) iota[(size_t)t] = t;
  FoldinPlan p;
  foldin_set_plan(used, 9, same.data(), iota.data(), p);
  CHECK(p.n_levels == 9, "one user, nine items: %u levels", p.n_levels);
  foldin_set_plan(used, 9, iota.data(), iota.data(), p);
  CHECK(p.n_levels == 1 && p.order == iota, "nine distinct pairs: %u levels", p.n_levels);
}

// ---- the overlay ------------------------------------------------------------------------------------------------------------
static const int64_t ROWS = 20, BASE_ROWS = 15;
static const int32_t ITEMS = 12;

struct OverlayModel {
  std::map<int64_t, std::set<int32_t>> base;        // what the base CSR holds (rows < BASE_ROWS), never written
  std::map<int64_t, std::multiset<int32_t>> added;  // rows without a whole set: what the writes added
  std::map<int64_t, std::set<int32_t>> whole;       // rows with a whole set
  std::set<int32_t> current(int64_t r) const {
    if (whole.count(r)) return whole.at(r);
    std::set<int32_t> s = base.count(r) ? base.at(r) : std::set<int32_t>();
    if (added.count(r)) s.insert(added.at(r).begin(), added.at(r).end());
    return s;
  }
};

static void check_overlay(const KnownOverlay& ov, const OverlayModel& m, const char* after) {
  bool any = false;
  std::vector<int64_t> differ;
  for (int64_t r = 0; r < ROWS; ++r) {
    std::vector<int64_t> got;
    const bool drop = ov.view(r, BASE_ROWS, got);
    const bool whole = m.whole.count(r) != 0;
    CHECK(drop == (whole || r >= BASE_ROWS), "after %s, row %lld: drop %d", after, (long long)r, (int)drop);
    CHECK(ov.has_set(r) == whole, "after %s, row %lld: has_set", after, (long long)r);
    std::multiset<int64_t> g(got.begin(), got.end()), e;
    if (whole)
      e.insert(m.whole.at(r).begin(), m.whole.at(r).end());
    else if (m.added.count(r))
      e.insert(m.added.at(r).begin(), m.added.at(r).end());
    CHECK(g == e, "after %s, row %lld: the view holds %zu items, the model %zu", after, (long long)r, g.size(), e.size());
    // with the base row folded in as a reader does: the row's current set
    std::set<int32_t> folded(got.begin(), got.end());
    if (!drop && m.base.count(r)) folded.insert(m.base.at(r).begin(), m.base.at(r).end());
    CHECK(folded == m.current(r), "after %s, row %lld: the folded set differs", after, (long long)r);
    if (whole || (m.added.count(r) && !m.added.at(r).empty())) differ.push_back(r);
    any = any || whole || (m.added.count(r) && !m.added.at(r).empty());
  }
  CHECK(ov.any() == any, "after %s: any() %d", after, (int)ov.any());
  const std::vector<int64_t> rows = ov.override_rows();
  CHECK(rows == differ, "after %s: %zu override rows, the model has %zu", after, rows.size(), differ.size());   // (differ ascends, distinct)
}

static void test_overlay(std::mt19937_64& rng) {
  for (int round = 0; round < 40; ++round) {
    KnownOverlay ov;
    OverlayModel m;
    for (int64_t r = 0; r < BASE_ROWS; ++r)
      for (int32_t it = 0; it < ITEMS; ++it)
        if (rng() % 4 == 0) m.base[r].insert(it);
    check_overlay(ov, m, "construction");
    for (int step = 0; step < 60; ++step) {
      const int64_t r = (int64_t)(rng() % (uint64_t)ROWS);
      const int32_t it = (int32_t)(rng() % (uint64_t)ITEMS);
      switch (rng() % 4) {
        case 0:
        case 1: {   // add (twice now and then: the chain repeats, the whole set does not)
          const int times = 1 + (int)(rng() % 2);
          for (int k = 0; k < times; ++k) {
            ov.add(r, it);
            if (m.whole.count(r)) m.whole[r].insert(it); else m.added[r].insert(it);
          }
          check_overlay(ov, m, "add");
          break;
        }
        case 2: {   // install-then-remove, as foldin_remove_decide does: a row without a whole set gets its current one first
          if (!ov.has_set(r)) {
            const std::set<int32_t> cur = m.current(r);
            std::vector<int32_t> set(cur.begin(), cur.end());
            ov.install(r, set);
            m.whole[r] = cur;
            m.added.erase(r);
            check_overlay(ov, m, "install");
          }
          std::set<int32_t>& s = m.whole[r];
          const KnownOverlay::Removal expect = !s.count(it) ? KnownOverlay::NOT_KNOWN : s.size() == 1 ? KnownOverlay::EMPTIED : KnownOverlay::REMOVED;
          const KnownOverlay::Removal got = ov.remove(r, it);
          s.erase(it);
          CHECK(got == expect, "remove(%lld, %d): %d, the model says %d", (long long)r, (int)it, (int)got, (int)expect);
          check_overlay(ov, m, "remove");
          break;
        }
        default: {   // remove on a row without a whole set is not-known and changes nothing
          if (!ov.has_set(r)) CHECK(ov.remove(r, it) == KnownOverlay::NOT_KNOWN, "remove on row %lld without a whole set", (long long)r);
          check_overlay(ov, m, "view");
        }
      }
    }
    // whole sets swapped in for rows that have none (a loaded generation's kept users)
    if (round % 4 == 0) {
      ov.clear();
      m.added.clear();
      m.whole.clear();
      KnownOverlay::Sets sets;
      sets[17] = {1, 4};
      sets[19] = {};
      ov.install_all(sets);
      m.whole[17] = {1, 4};
      m.whole[19] = {};
      check_overlay(ov, m, "install_all");
      CHECK(ov.remove(17, 4) == KnownOverlay::REMOVED && ov.remove(17, 1) == KnownOverlay::EMPTIED && ov.remove(19, 1) == KnownOverlay::NOT_KNOWN, "kept sets");
    }
    ov.clear();
    m.added.clear();
    m.whole.clear();
    check_overlay(ov, m, "clear");
  }
}

// ---- status words -----------------------------------------------------------------------------------------------------------
static void test_status() {
  for (int code = 0; code <= 2; ++code)
    for (int why = 0; why <= 5; ++why)
      for (int big = 0; big <= 3; ++big) {
        const FoldinStatus st = foldin_status_decode((int32_t)(code | (why << 8) | (big << 16)));
        CHECK(st.code == code && st.why == why && st.big == big, "(%d, %d, %d) decodes to (%d, %d, %d)", code, why, big, st.code, st.why, st.big);
      }
  CHECK(std::strlen(foldin_why_text(0)) == 0, "why 0 has a text");
  for (int why = 1; why <= 4; ++why) CHECK(std::strlen(foldin_why_text(why)) > 0, "why %d has no text", why);
  CHECK(std::strstr(foldin_why_text(1), "estimate is not finite") != nullptr, "why 1: %s", foldin_why_text(1));
  CHECK(std::strstr(foldin_why_text(4), "without a Y^T Y solver") != nullptr, "why 4: %s", foldin_why_text(4));
  for (int why : {5, 6, 255, -1}) CHECK(std::strlen(foldin_why_text(why)) == 0, "why %d outside the table has a text", why);
}

int main(int argc, char** argv) {
  std::mt19937_64 rng(argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1);
  test_plan(rng);
  test_overlay(rng);
  test_status();
  std::printf("checks %d failures %d\n", checks, failures);
  return failures ? 1 : 0;
}
