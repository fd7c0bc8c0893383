// ingest_live_plan.h -- the host logic of mals_ingest_apply (ids_host.h) that needs no device: which records of a stream are
// sets and which removes, and the cut of the stream into the ordered batches the write drivers take.  Host code only, no
// HIP include and no handle; tests/cpp/test_ingest_live_plan.cpp restates live_classify and live_cut naively,
// tests/cpp/test_ingest_tag_plan.cpp the functions that take the records' kinds (MALS_INGEST_OPT_LIVE_TAGS).
//
// ServerRecommender.ingest (ServerRecommender.java:268-298) applies its lines one by one.  A batch of mals_set_preferences
// equals its updates applied one by one (the level plan, foldin_plan.h), and so does a batch of mals_remove_preferences, but
// a set and a remove of one user do not commute: the stream is cut into MAXIMAL RUNS of sets and of removes, in order.  A
// remove whose user or item has no row does nothing in the reference (:1033-1042); it is dropped BEFORE the cut, so the set
// runs on either side of it are one run (one write call less, the same model: nothing stood between them).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace mals {

// positions of the set records and of the remove records, each ascending
struct LiveClasses {
  std::vector<int64_t> set_pos, rem_pos;
};

// a record whose value is NaN is a remove (the parser's mark of an empty third token), anything else a set
inline void live_classify(int64_t n, const float* value, LiveClasses& c) {
  c.set_pos.clear();
  c.rem_pos.clear();
  for (int64_t t = 0; t < n; ++t) (std::isnan(value[t]) ? c.rem_pos : c.set_pos).push_back(t);
}

// MALS_INGEST_OPT_LIVE_TAGS: the records carry their kind (0 a preference, 1 a tag in the user column -- setItemTag --, 2 a tag
// in the item column -- setUserTag).  A tag record whose value is NaN is neither a set nor a remove: ingest ignores it
// altogether (:281-293), so it stands in neither list and cuts no run.  Any other tag record is a set like a preference's
// (the same update on its two rows) and rides in the set runs; set_kind has the kind of every set record, by entry of set_pos.
struct LiveTagCounts {
  int64_t item_tag_sets = 0, user_tag_sets = 0, removes_ignored = 0;
};

inline void live_classify_kinds(int64_t n, const float* value, const uint8_t* kind, LiveClasses& c, std::vector<uint8_t>& set_kind,
                                LiveTagCounts& tags) {
  c.set_pos.clear();
  c.rem_pos.clear();
  set_kind.clear();
  tags = LiveTagCounts();
  for (int64_t t = 0; t < n; ++t) {
    const bool is_tag = kind[t] != 0;
    if (std::isnan(value[t])) {
      if (is_tag) ++tags.removes_ignored;
      else c.rem_pos.push_back(t);
      continue;
    }
    c.set_pos.push_back(t);
    set_kind.push_back(kind[t]);
    tags.item_tag_sets += kind[t] == 1;
    tags.user_tag_sets += kind[t] == 2;
  }
}

// the kinds of one set run of live_cut's plan, for the write driver: nullptr when the run holds preferences only (the
// driver's untagged path)
inline const uint8_t* live_run_kinds(const std::vector<uint8_t>& set_kind, int64_t begin, int64_t end) {
  for (int64_t j = begin; j < end; ++j)
    if (set_kind[(size_t)j] != 0) return set_kind.data() + begin;
  return nullptr;
}

// a set run: [begin, end) of the set records (indices into set_pos); a remove run: [begin, end) of the removes PASSED ON
// (indices into rem_keep)
struct LiveRun {
  bool is_set;
  int64_t begin, end;
};

struct LivePlan {
  std::vector<LiveRun> runs;       // in stream order; neighbours differ in kind
  std::vector<int64_t> rem_keep;   // the removes passed on, as indices into rem_pos, ascending
  int64_t dropped = 0;             // removes whose user or item has no row
};

// rem_urow / rem_irow: the rows of the remove records (one per entry of rem_pos), -1 = the id has no row
inline void live_cut(const LiveClasses& c, const int64_t* rem_urow, const int64_t* rem_irow, LivePlan& p) {
  p.runs.clear();
  p.rem_keep.clear();
  p.dropped = 0;
  size_t a = 0, b = 0;   // next set, next remove
  const size_t ns = c.set_pos.size(), nr = c.rem_pos.size();
  while (a < ns || b < nr) {
    const bool is_set = b == nr || (a < ns && c.set_pos[a] < c.rem_pos[b]);
    int64_t at;
    if (is_set) {
      at = (int64_t)a++;
    } else {
      const size_t j = b++;
      if (rem_urow[j] < 0 || rem_irow[j] < 0) {
        ++p.dropped;
        continue;
      }
      at = (int64_t)p.rem_keep.size();
      p.rem_keep.push_back((int64_t)j);
    }
    if (!p.runs.empty() && p.runs.back().is_set == is_set) p.runs.back().end = at + 1;
    else p.runs.push_back({is_set, at, at + 1});
  }
}

}  // namespace mals
