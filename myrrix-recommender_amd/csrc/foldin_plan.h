// foldin_plan.h -- the host logic of the online write path (foldin_host.h, popular_host.h) that needs no device: the level
// plan of a batch, the known-item overlay, the status word of foldin_update_kernel.  Host code only, no HIP include and no
// handle; tests/cpp/test_foldin_plan.cpp restates every function here naively.
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <utility>
#include <vector>

namespace mals {

// ---- the level plan -------------------------------------------------------------------------------------------------------
// An update's level: 1 + the larger level of the last earlier update of the same X row and of the same Y row (0: none).  The
// updates of one level touch distinct rows and run side by side; the levels run in order.
struct FoldinPlan {
  std::vector<int64_t> off, order;   // updates of level l (1 .. n_levels): order[off[l] .. off[l + 1]), ascending
  uint32_t n_levels = 0;
};

// per batch: row -> last level, an open-addressing table sized by the batch (cache-resident, nothing per model row); kept
// between batches so that the vectors are reused.  -1 is the empty key: the rows of a checked batch are >= 0.
struct FoldinPlanScratch {
  std::vector<int64_t> lk[2];
  std::vector<uint32_t> lv[2];
};

// row -> level of the last update of the batch that touched it (linear probing)
inline uint32_t& foldin_slot(std::vector<int64_t>& keys, std::vector<uint32_t>& vals, int64_t row) {
  const size_t mask = keys.size() - 1;
  size_t i = (size_t)(((uint64_t)row * 0x9E3779B97F4A7C15ull) >> 20) & mask;
  while (keys[i] != row && keys[i] != -1) i = (i + 1) & mask;
  if (keys[i] == -1) {
    keys[i] = row;
    vals[i] = 0;
  }
  return vals[i];
}

inline void foldin_set_plan(FoldinPlanScratch& sc, int64_t n, const int64_t* urow, const int64_t* irow, FoldinPlan& p) {
  size_t cap = 16;
  while (cap < 2 * (size_t)n) cap <<= 1;
  for (int s = 0; s < 2; ++s) {
    sc.lk[s].assign(cap, -1);
    sc.lv[s].resize(cap);
  }
  std::vector<uint32_t> level((size_t)n);
  uint32_t n_levels = 0;
  for (int64_t t = 0; t < n; ++t) {
    uint32_t& lu = foldin_slot(sc.lk[0], sc.lv[0], urow[t]);
    uint32_t& li = foldin_slot(sc.lk[1], sc.lv[1], irow[t]);
    const uint32_t l = std::max(lu, li) + 1;
    level[(size_t)t] = lu = li = l;
    n_levels = std::max(n_levels, l);
  }
  p.off.assign((size_t)n_levels + 2, 0);
  for (int64_t t = 0; t < n; ++t) ++p.off[level[(size_t)t] + 1];
  for (uint32_t l = 1; l <= n_levels + 1; ++l) p.off[l] += p.off[l - 1];
  std::vector<int64_t> pos(p.off);
  p.order.resize((size_t)n);
  for (int64_t t = 0; t < n; ++t) p.order[(size_t)pos[level[(size_t)t]]++] = t;
  p.n_levels = n_levels;
}

// ---- the status word of one update (foldin_update_kernel) -------------------------------------------------------------------
struct FoldinStatus {
  int code, why, big;   // MALS_OK or the failure; which check failed (foldin_why_text); fold-ins past BIG_FOLDIN_THRESHOLD
};
inline FoldinStatus foldin_status_decode(int32_t w) { return {w & 0xff, (w >> 8) & 0xff, (w >> 16) & 3}; }

inline const char* foldin_why_text(int why) {
  static const char* const text[] = {"", "estimate is not finite (foldInWeight: checkState)", "item fold-in delta is not finite (checkState, item loop)",
                                     "user fold-in delta is not finite (checkState, user loop)",
                                     "X^T X solver set without a Y^T Y solver: the reference's item branch reads norm(null)"};
  return why >= 0 && why < 5 ? text[why] : "";
}

// ---- the known-item overlay -------------------------------------------------------------------------------------------------
// knownItemIDs after the writes of this generation, beside the base CSR (the installed known items or the rows of R, never
// written): per local user row a chain of added items in one pool (O(1) per write, duplicates dropped when read), and --
// after the user's first removal -- the whole set, sorted (the base row and the chain no longer count).
class KnownOverlay {
 public:
  using Sets = std::unordered_map<int64_t, std::vector<int32_t>>;
  enum Removal { NOT_KNOWN, REMOVED, EMPTIED };

  bool any() const { return !pool_.empty() || !replaced_.empty(); }

  // a new generation: the memory goes too
  void clear() {
    std::vector<uint32_t>().swap(head_);
    std::vector<std::pair<int32_t, uint32_t>>().swap(pool_);
    replaced_.clear();
  }

  // knownItemIDs.get(row).add(item)
  void add(int64_t row, int32_t item) {
    if (!replaced_.empty()) {
      auto it = replaced_.find(row);
      if (it != replaced_.end()) {
        std::vector<int32_t>& v = it->second;
        auto p = std::lower_bound(v.begin(), v.end(), item);
        if (p == v.end() || *p != item) v.insert(p, item);
        return;
      }
    }
    if (row >= (int64_t)head_.size()) head_.resize((size_t)row + 1, UINT32_MAX);
    pool_.push_back({item, head_[(size_t)row]});
    head_[(size_t)row] = (uint32_t)(pool_.size() - 1);
  }

  // what a reader needs of a row beyond its base row: the items (appended to out, possibly repeated) and whether the base
  // row is dropped -- a whole set, or a row the base CSR (base_rows rows) does not have
  bool view(int64_t row, int64_t base_rows, std::vector<int64_t>& out) const {
    if (!replaced_.empty()) {
      auto it = replaced_.find(row);
      if (it != replaced_.end()) {
        out.insert(out.end(), it->second.begin(), it->second.end());
        return true;
      }
    }
    if (row >= 0 && row < (int64_t)head_.size())
      for (uint32_t e = head_[(size_t)row]; e != UINT32_MAX; e = pool_[e].second) out.push_back(pool_[e].first);
    return row >= base_rows;
  }

  bool has_set(int64_t row) const { return replaced_.count(row) != 0; }

  // the row's whole set (sorted, distinct; swapped in), in place of its base row and its chain
  void install(int64_t row, std::vector<int32_t>& set) {
    if (row >= 0 && row < (int64_t)head_.size()) head_[(size_t)row] = UINT32_MAX;
    replaced_[row].swap(set);
  }
  // whole sets for rows that have none (a loaded generation's kept users), without an allocation
  void install_all(Sets& sets) { replaced_.swap(sets); }

  // of a row with a whole set (install): an unknown row, or an item it does not know, is ignored
  Removal remove(int64_t row, int32_t item) {
    auto it = replaced_.find(row);
    if (it == replaced_.end()) return NOT_KNOWN;
    std::vector<int32_t>& v = it->second;
    auto p = std::lower_bound(v.begin(), v.end(), item);
    if (p == v.end() || *p != item) return NOT_KNOWN;
    v.erase(p);
    return v.empty() ? EMPTIED : REMOVED;
  }

  // the rows whose set is not their base row (an added chain or a whole set): sorted, distinct
  std::vector<int64_t> override_rows() const {
    std::vector<int64_t> rows;
    for (size_t r = 0; r < head_.size(); ++r)
      if (head_[r] != UINT32_MAX) rows.push_back((int64_t)r);
    for (const auto& kv : replaced_) rows.push_back(kv.first);
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    return rows;
  }

 private:
  std::vector<uint32_t> head_;                          // row -> newest pool entry, UINT32_MAX = none
  std::vector<std::pair<int32_t, uint32_t>> pool_;      // (item, next entry)
  Sets replaced_;
};

}  // namespace mals
