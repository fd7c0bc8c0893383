// foldin_host.h -- host side of the online write path (mals_set_preferences, mals_remove_preferences,
// mals_grow_factor_rows, the fold-in reads; include/myrrix_als.h; kernels in foldin_kernels.h).  Included by
// mals_serving.hip inside its anonymous namespace, after topn_host.h: every call here runs as an exclusive ticket of the
// serving front (topn_front_submit), so the passes formed before it have finished and the passes formed after it wait
// for its work on the handle's stream (ev_begin), and the state below is only ever touched by the front's leader.
#pragma once

// Errors of the calls below never go to h->err from inside a ticket (other request threads write it under the front's
// mutex): a run keeps its message in `msg`, and the public call publishes it with topn_fail once the ticket is done.
#define FCHK(msg, call)                                                                                   \
  do {                                                                                                    \
    hipError_t _e = (call);                                                                               \
    if (_e != hipSuccess) {                                                                               \
      (msg) = std::string(#call) + ": " + hipGetErrorString(_e);                                          \
      return _e == hipErrorOutOfMemory ? MALS_OOM : MALS_HIP_ERROR;                                       \
    }                                                                                                     \
  } while (0)

struct FoldinSide {
  DeviceBuffer<double> a, tau;  // the solver of M^T M (side X: X^T X) as PivotedQR::solve reads it
  DeviceBuffer<int32_t> ipiv;
  bool present = false;
};

struct FoldinState {
  FoldinSide solver[2];
  double rate = 1.0;                   // FOLDIN_LEARN_RATE
  double big_total = 0.0;              // smallest t with sqrt(t) > BIG_FOLDIN_THRESHOLD
  // knownItemIDs after the writes of this generation, beside the base CSR (the installed known items or the rows of R,
  // never written): per local user row a chain of added items in one pool (O(1) per write, duplicates dropped when read),
  // and -- after the user's first removal -- the whole set, sorted (the base row and the chain no longer count)
  std::vector<uint32_t> head;                          // local row -> newest pool entry, UINT32_MAX = none
  std::vector<std::pair<int32_t, uint32_t>> pool;      // (item, next entry)
  std::unordered_map<int64_t, std::vector<int32_t>> replaced;
  // per batch: row -> last level, an open-addressing table sized by the batch (cache-resident, nothing per model row)
  std::vector<int64_t> lk[2];
  std::vector<uint32_t> lv[2];
  DeviceBuffer<int64_t> d_rows;        // [2][n] user rows | item rows, level order
  DeviceBuffer<float> d_val;
  DeviceBuffer<int32_t> d_status;
  DeviceBuffer<double> d_fold;         // userFoldIn of every update of the batch
  PinnedBuffer<uint8_t> h_stage;
  hipEvent_t ev[2] = {nullptr, nullptr};
};

FoldinState* foldin_state(mals_handle h) {
  if (!h->serving->fo) {
    FoldinState* fs = new FoldinState();
    double t = 1e8;
    while (!(std::sqrt(t) > 1e4)) t = std::nextafter(t, std::numeric_limits<double>::infinity());
    fs->big_total = t;
    h->serving->fo = fs;
  }
  return h->serving->fo;
}

void foldin_free(mals_handle h) {
  FoldinState* fs = h->serving->fo;
  if (fs)
    for (hipEvent_t e : fs->ev)
      if (e) (void)hipEventDestroy(e);
  delete fs;
  h->serving->fo = nullptr;
}

// a new generation (mals_set_known_items, mals_set_matrix of side X, mals_set_factor_rows / mals_bind_factors of X)
void foldin_drop_overlay(mals_handle h) {
  h->grown_users_end.store(-1, std::memory_order_release);
  FoldinState* fs = h->serving->fo;
  if (!fs) return;
  std::vector<uint32_t>().swap(fs->head);
  std::vector<std::pair<int32_t, uint32_t>>().swap(fs->pool);
  fs->replaced.clear();
}

// rows of the base known-item CSR (users past them -- grown rows -- have an empty base set)
int64_t foldin_base_rows(mals_handle h) {
  const SideState& x = h->side[MALS_SIDE_X];
  return h->known_ptr ? h->known_rows : (x.has_matrix ? x.n_local : 0);
}

// one past the last global user row whose known items this handle holds: the local shard, and on a handle outside a
// group the rows mals_grow_factor_rows added (an atomic: read by request threads outside the front)
int64_t foldin_user_rows_end(mals_handle h) {
  const SideState& x = h->side[MALS_SIDE_X];
  const int64_t grown = h->grown_users_end.load(std::memory_order_acquire);
  return std::max(x.row_offset + x.n_local, grown);
}

bool foldin_has_overlay(mals_handle h) {
  const FoldinState* fs = h->serving->fo;
  return (fs && (!fs->pool.empty() || !fs->replaced.empty())) || h->grown_users_end.load(std::memory_order_acquire) >= 0 ||
         foldin_base_rows(h) < h->side[MALS_SIDE_X].n_local;
}

// what a recommend pass needs of a user's known items beyond its base row: the items to exclude (appended to out,
// possibly repeated) and whether the base row is dropped (a replaced set, or a grown row the base CSR does not have)
bool foldin_known_view(mals_handle h, int64_t local_row, std::vector<int64_t>& out) {
  bool drop = local_row >= foldin_base_rows(h);
  const FoldinState* fs = h->serving->fo;
  if (!fs) return drop;
  if (!fs->replaced.empty()) {
    auto it = fs->replaced.find(local_row);
    if (it != fs->replaced.end()) {
      out.insert(out.end(), it->second.begin(), it->second.end());
      return true;
    }
  }
  if (local_row < (int64_t)fs->head.size())
    for (uint32_t e = fs->head[(size_t)local_row]; e != UINT32_MAX; e = fs->pool[e].second) out.push_back(fs->pool[e].first);
  return drop;
}

void foldin_overlay_add(FoldinState& fs, int64_t local_row, int32_t item) {
  if (!fs.replaced.empty()) {
    auto it = fs.replaced.find(local_row);
    if (it != fs.replaced.end()) {
      std::vector<int32_t>& v = it->second;
      auto p = std::lower_bound(v.begin(), v.end(), item);
      if (p == v.end() || *p != item) v.insert(p, item);
      return;
    }
  }
  if (local_row >= (int64_t)fs.head.size()) fs.head.resize((size_t)local_row + 1, UINT32_MAX);
  fs.pool.push_back({item, fs.head[(size_t)local_row]});
  fs.head[(size_t)local_row] = (uint32_t)(fs.pool.size() - 1);
}

// the base rows of several local users from the device, with two synchronisations in all: outs[j] sorted, distinct
int foldin_fetch_bases(mals_handle h, const std::vector<int64_t>& rows, std::vector<std::vector<int32_t>>& outs, std::string& msg) {
  outs.assign(rows.size(), {});
  const SideState& x = h->side[MALS_SIDE_X];
  const int64_t* ptr = h->known_ptr ? h->known_ptr : x.row_ptr;
  const int32_t* idx = h->known_ptr ? h->known_idx : x.col;
  const int64_t base = foldin_base_rows(h);
  std::vector<int64_t> be(2 * rows.size(), 0);
  bool any = false;
  for (size_t j = 0; j < rows.size(); ++j)
    if (rows[j] >= 0 && rows[j] < base) {
      FCHK(msg, hipMemcpyAsync(&be[2 * j], ptr + rows[j], 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
      any = true;
    }
  if (!any) return MALS_OK;
  FCHK(msg, hipStreamSynchronize(h->stream));
  for (size_t j = 0; j < rows.size(); ++j) {
    outs[j].resize((size_t)(be[2 * j + 1] - be[2 * j]));
    if (!outs[j].empty())
      FCHK(msg, hipMemcpyAsync(outs[j].data(), idx + be[2 * j], sizeof(int32_t) * outs[j].size(), hipMemcpyDeviceToHost, h->stream));
  }
  FCHK(msg, hipStreamSynchronize(h->stream));
  for (std::vector<int32_t>& o : outs) {
    std::sort(o.begin(), o.end());
    o.erase(std::unique(o.begin(), o.end()), o.end());
  }
  return MALS_OK;
}

// the whole current sets of several local users (base row + additions, or the replaced set), sorted, distinct
int foldin_known_full(mals_handle h, const std::vector<int64_t>& rows, std::vector<std::vector<int32_t>>& outs, std::string& msg) {
  std::vector<std::vector<int64_t>> extra(rows.size());
  std::vector<int64_t> fetch(rows.size(), -1);
  for (size_t j = 0; j < rows.size(); ++j)
    if (!foldin_known_view(h, rows[j], extra[j])) fetch[j] = rows[j];
  if (int rc = foldin_fetch_bases(h, fetch, outs, msg)) return rc;
  for (size_t j = 0; j < rows.size(); ++j) {
    std::vector<int32_t>& o = outs[j];
    o.insert(o.end(), extra[j].begin(), extra[j].end());
    std::sort(o.begin(), o.end());
    o.erase(std::unique(o.begin(), o.end()), o.end());
  }
  return MALS_OK;
}

// a call that runs alone on the handle, in the front's queue order; a failure's message is published under the mutex
int foldin_exclusive(mals_handle h, const std::function<int()>& fn, const std::string& msg, const char* call) {
  TopnRequest rq;
  rq.kind = TOPN_KIND_CALL;
  rq.call = &fn;
  rq.how_many = 1;
  const int rc = topn_front_submit(h, rq, false);
  if (rc == MALS_OK) return rc;
  std::lock_guard<std::mutex> lk(topn_front(h)->mu);   // (as topn_fail: request threads write h->err under this mutex)
  h->err = std::string(call) + ": " + (msg.empty() ? std::string("failed") : msg);
  return rc;
}

// fn with the fronts of ALL the handles held at once (the members of a group): a ticket of hs[0] whose call is a ticket of
// hs[1], and so on; fn runs innermost, on whichever thread leads the last front.  Nothing else nests tickets and the order
// is always hs[0] first, so two such calls cannot wait for each other.  A thread that waits in a handle's front may be made
// its leader and then runs other callers' passes there: it is on that handle's device for as long as it is inside.
int foldin_exclusive_all(mals_handle* hs, int n, int i, const std::function<int()>& fn) {
  if (i == n) return fn();
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipSetDevice(hs[i]->cfg.device) != hipSuccess) return MALS_HIP_ERROR;
  const std::function<int()> inner = [&]() -> int { return foldin_exclusive_all(hs, n, i + 1, fn); };
  TopnRequest rq;
  rq.kind = TOPN_KIND_CALL;
  rq.call = &inner;
  rq.how_many = 1;
  const int rc = topn_front_submit(hs[i], rq, false);
  (void)hipSetDevice(dev);
  return rc;
}

int foldin_lds_limit(std::string& msg) {
  static std::once_flag once;
  static hipError_t e = hipSuccess;
  std::call_once(once, [] {
    const int lds = 128 * FOLDIN_LANES * (int)(sizeof(double) + sizeof(float));
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&foldin_update_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(&foldin_anonymous_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(&foldin_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  });
  FCHK(msg, e);
  return MALS_OK;
}

FoldinSolverView foldin_view(const FoldinSide& s) { return {s.a.get(), s.tau.get(), s.ipiv.get()}; }

// row -> level of the last update of the batch that touched it (open addressing, linear probing)
uint32_t& foldin_slot(std::vector<int64_t>& keys, std::vector<uint32_t>& vals, int64_t row) {
  const size_t mask = keys.size() - 1;
  size_t i = (size_t)(((uint64_t)row * 0x9E3779B97F4A7C15ull) >> 20) & mask;
  while (keys[i] != row && keys[i] != -1) i = (i + 1) & mask;
  if (keys[i] == -1) {
    keys[i] = row;
    vals[i] = 0;
  }
  return vals[i];
}

// ---- mals_set_preferences -------------------------------------------------------------------------------------------
// A batch runs in three steps, so that a group can have every member's kernels enqueued before it waits for any of them
// (mals_group_set_preferences): the level plan (the same for every replica the batch goes to), the enqueue half (uploads,
// the level kernels and the status copy on the handle's stream, no wait) and the collect half (the wait and the host-side
// bookkeeping).  One handle runs the three back to back.
struct FoldinPlan {
  std::vector<int64_t> off, order;   // updates of level l: order[off[l] .. off[l + 1])
  uint32_t n_levels = 0;
};

void foldin_set_plan(FoldinState& fs, int64_t n, const int64_t* urow, const int64_t* irow, FoldinPlan& p) {
  // levels: 1 + the larger level of the last update of the same X row and of the same Y row
  size_t cap = 16;
  while (cap < 2 * (size_t)n) cap <<= 1;
  for (int s = 0; s < 2; ++s) {
    fs.lk[s].assign(cap, -1);
    fs.lv[s].resize(cap);
  }
  std::vector<uint32_t> level((size_t)n);
  uint32_t n_levels = 0;
  for (int64_t t = 0; t < n; ++t) {
    uint32_t& lu = foldin_slot(fs.lk[0], fs.lv[0], urow[t]);
    uint32_t& li = foldin_slot(fs.lk[1], fs.lv[1], irow[t]);
    const uint32_t l = std::max(lu, li) + 1;
    level[(size_t)t] = lu = li = l;
    n_levels = std::max(n_levels, l);
  }
  std::vector<int64_t>& off = p.off;
  off.assign((size_t)n_levels + 2, 0);
  for (int64_t t = 0; t < n; ++t) ++off[level[(size_t)t] + 1];
  for (uint32_t l = 1; l <= n_levels + 1; ++l) off[l] += off[l - 1];
  std::vector<int64_t> pos(off.begin(), off.end());
  p.order.resize((size_t)n);
  for (int64_t t = 0; t < n; ++t) p.order[(size_t)pos[level[(size_t)t]]++] = t;
  p.n_levels = n_levels;
}

int foldin_set_enqueue(mals_handle h, int64_t n, const int64_t* urow, const int64_t* irow, const float* value, const FoldinPlan& p,
                       std::string& msg) {
  FoldinState& fs = *foldin_state(h);
  SideState& x = h->side[MALS_SIDE_X];
  SideState& y = h->side[MALS_SIDE_Y];
  const int k = h->cfg.features;
  if (int rc = foldin_lds_limit(msg)) return rc;
  const std::vector<int64_t>& off = p.off;
  const std::vector<int64_t>& order = p.order;
  const uint32_t n_levels = p.n_levels;
  // level order on the device: user rows | item rows | values, one copy
  const size_t bytes = sizeof(int64_t) * 2 * (size_t)n + sizeof(float) * (size_t)n;
  FCHK(msg, fs.h_stage.reserve(std::max(bytes, sizeof(int32_t) * (size_t)n), h->stream));
  FCHK(msg, fs.d_rows.reserve(2 * (size_t)n, h->stream));
  FCHK(msg, fs.d_val.reserve((size_t)n, h->stream));
  FCHK(msg, fs.d_status.reserve((size_t)n, h->stream));
  FCHK(msg, fs.d_fold.reserve((size_t)n * k, h->stream));
  for (hipEvent_t& e : fs.ev)
    if (!e) FCHK(msg, hipEventCreate(&e));
  int64_t* hu = reinterpret_cast<int64_t*>(fs.h_stage.get());
  int64_t* hi = hu + n;
  float* hv = reinterpret_cast<float*>(hi + n);
  for (int64_t j = 0; j < n; ++j) {
    const int64_t t = order[(size_t)j];
    hu[j] = urow[t];
    hi[j] = irow[t];
    hv[j] = value[t];
  }
  FCHK(msg, hipMemcpyAsync(fs.d_rows.get(), hu, sizeof(int64_t) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  FCHK(msg, hipMemcpyAsync(fs.d_val.get(), hv, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  const FoldinSide& SX = fs.solver[MALS_SIDE_X];
  const FoldinSide& SY = fs.solver[MALS_SIDE_Y];
  const size_t lds = (size_t)k * FOLDIN_LANES * sizeof(double);
  FCHK(msg, hipEventRecord(fs.ev[0], h->stream));
  for (uint32_t l = 1; l <= n_levels; ++l) {
    const int64_t u0 = off[l], u1 = off[l + 1];
    hipLaunchKernelGGL(foldin_update_kernel, dim3((unsigned)((u1 - u0 + FOLDIN_LANES - 1) / FOLDIN_LANES)), dim3(FOLDIN_LANES), lds, h->stream, x.F,
                       y.F, k, fs.d_rows.get(), fs.d_rows.get() + n, fs.d_val.get(), u0, u1, foldin_view(SX), foldin_view(SY), SX.present ? 1 : 0,
                       SY.present ? 1 : 0, fs.rate, fs.big_total, fs.d_fold.get(), fs.d_status.get());
  }
  FCHK(msg, hipGetLastError());
  FCHK(msg, hipEventRecord(fs.ev[1], h->stream));
  int32_t* hs = reinterpret_cast<int32_t*>(fs.h_stage.get());
  FCHK(msg, hipMemcpyAsync(hs, fs.d_status.get(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  return MALS_OK;
}

// the known items of the applied updates are recorded for the users in [own_lo, own_hi) only: on a group the owner of a
// user keeps its overlay (a single handle owns every user foldin_check_pairs let through)
int foldin_set_collect(mals_handle h, int64_t n, const int64_t* urow, const int64_t* irow, const FoldinPlan& p, int64_t own_lo, int64_t own_hi,
                       int32_t* status_out, std::string& msg) {
  FoldinState& fs = *foldin_state(h);
  SideState& x = h->side[MALS_SIDE_X];
  const std::vector<int64_t>& order = p.order;
  const uint32_t n_levels = p.n_levels;
  const int32_t* hs = reinterpret_cast<const int32_t*>(fs.h_stage.get());
  FCHK(msg, hipStreamSynchronize(h->stream));
  float dev_ms = 0.f;
  FCHK(msg, hipEventElapsedTime(&dev_ms, fs.ev[0], fs.ev[1]));
  // every write is a new model: the next half-iteration re-pads and recomputes its Gramian (the generation's solvers stay)
  for (int s = 0; s < 2; ++s) {
    h->side[s].G_valid = false;
    ++h->side[s].F_epoch;
  }
  int first = MALS_OK, first_why = 0;
  int64_t first_t = -1, applied = 0, failed = 0, big = 0;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t t = order[(size_t)j];
    const int32_t w = hs[j];
    const int code = w & 0xff;
    big += (w >> 16) & 3;
    if (status_out) status_out[t] = code;
    if (code != MALS_OK) {
      ++failed;
      if (first_t < 0 || t < first_t) {
        first_t = t;
        first = code;
        first_why = (w >> 8) & 0xff;
      }
      continue;
    }
    ++applied;
    if (urow[t] >= own_lo && urow[t] < own_hi)
      foldin_overlay_add(fs, urow[t] - x.row_offset, (int32_t)irow[t]);   // knownItemIDs.get(userID).add(itemID) (:813-836)
  }
  if (applied) popular_touch(h, false);   // known items were added: what mals_most_popular_items counted is stale
  std::atomic<int64_t>* c = h->foldin_counters;
  c[0] += applied;
  c[1] += failed;
  c[2] += big;
  c[3] += n_levels;
  c[4] += (int64_t)((double)dev_ms * 1e6);
  c[5].store((int64_t)((double)dev_ms * 1e6));
  if (first != MALS_OK) {
    static const char* why[] = {"", "estimate is not finite (foldInWeight: checkState)", "item fold-in delta is not finite (checkState, item loop)",
                                "user fold-in delta is not finite (checkState, user loop)",
                                "X^T X solver set without a Y^T Y solver: the reference's item branch reads norm(null)"};
    msg = "update " + std::to_string(first_t) + ": " + why[first_why < 5 ? first_why : 0];
  }
  return first;
}

int foldin_set_run(mals_handle h, int64_t n, const int64_t* urow, const int64_t* irow, const float* value, int32_t* status_out,
                   std::string& msg) {
  FoldinPlan p;
  foldin_set_plan(*foldin_state(h), n, urow, irow, p);
  if (int rc = foldin_set_enqueue(h, n, urow, irow, value, p, msg)) return rc;
  return foldin_set_collect(h, n, urow, irow, p, std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max(), status_out, msg);
}

// ---- mals_remove_preferences ----------------------------------------------------------------------------------------
// Three steps as well (mals_group_remove_preferences): the decision, which is the known items' holder's alone -- the pairs
// whose user lies in [own_lo, own_hi) against this handle's sets; (position in the batch, user) of every user a pair
// empties is appended to `emptied` -- then zeroing those rows of X (enqueue) and the wait (collect), which every replica
// runs with the same list.
int foldin_remove_decide(mals_handle h, int64_t n, const int64_t* urow, const int64_t* irow, int64_t own_lo, int64_t own_hi,
                         std::vector<std::pair<int64_t, int64_t>>& emptied, std::string& msg) {
  FoldinState& fs = *foldin_state(h);
  SideState& x = h->side[MALS_SIDE_X];
  auto mine = [&](int64_t t) { return urow[t] >= own_lo && urow[t] < own_hi; };
  // every user of the batch without a replaced set gets one first: its base row and additions, fetched together
  std::vector<int64_t> need;
  for (int64_t t = 0; t < n; ++t) {
    if (!mine(t)) continue;
    const int64_t lr = urow[t] - x.row_offset;
    if (!fs.replaced.count(lr)) need.push_back(lr);
  }
  std::sort(need.begin(), need.end());
  need.erase(std::unique(need.begin(), need.end()), need.end());
  std::vector<std::vector<int32_t>> full;
  if (int rc = foldin_known_full(h, need, full, msg)) return rc;
  popular_touch(h, false);   // (conservative: a batch that removes nothing recounts too)
  for (size_t j = 0; j < need.size(); ++j) {
    if (need[j] < (int64_t)fs.head.size()) fs.head[(size_t)need[j]] = UINT32_MAX;
    fs.replaced[need[j]].swap(full[j]);   // (an empty set: a user without known items, whose removals are ignored)
  }
  for (int64_t t = 0; t < n; ++t) {
    if (!mine(t)) continue;
    std::vector<int32_t>& v = fs.replaced[urow[t] - x.row_offset];
    auto p = std::lower_bound(v.begin(), v.end(), (int32_t)irow[t]);
    if (p == v.end() || *p != (int32_t)irow[t]) continue;  // an unknown user, or an item it does not know: ignored (:1024-1033)
    v.erase(p);
    if (v.empty()) emptied.push_back({t, urow[t]});  // the user goes (:1040-1058)
  }
  return MALS_OK;
}

// `removed` (host) and `d` (its device copy) stay the caller's until foldin_remove_collect has returned
int foldin_remove_enqueue(mals_handle h, const std::vector<int64_t>& removed, DeviceBuffer<int64_t>& d, std::string& msg) {
  if (removed.empty()) return MALS_OK;
  SideState& x = h->side[MALS_SIDE_X];
  FCHK(msg, d.alloc(removed.size()));
  FCHK(msg, hipMemcpyAsync(d.get(), removed.data(), sizeof(int64_t) * removed.size(), hipMemcpyHostToDevice, h->stream));
  const int64_t nk = (int64_t)removed.size() * h->cfg.features;
  hipLaunchKernelGGL(foldin_zero_rows_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, h->stream, x.F, h->cfg.features, d.get(),
                     (int64_t)removed.size());
  FCHK(msg, hipGetLastError());
  return MALS_OK;
}

int foldin_remove_collect(mals_handle h, bool any_removed, std::string& msg) {
  if (any_removed) FCHK(msg, hipStreamSynchronize(h->stream));
  for (int s = 0; s < 2; ++s) {
    h->side[s].G_valid = false;
    ++h->side[s].F_epoch;
  }
  return MALS_OK;
}

int foldin_remove_run(mals_handle h, int64_t n, const int64_t* urow, const int64_t* irow, int64_t* removed_out, int64_t* n_removed_out,
                      std::string& msg) {
  std::vector<std::pair<int64_t, int64_t>> emptied;
  if (int rc = foldin_remove_decide(h, n, urow, irow, std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max(), emptied, msg))
    return rc;
  std::vector<int64_t> removed;
  for (const auto& e : emptied) removed.push_back(e.second);
  DeviceBuffer<int64_t> d;
  if (int rc = foldin_remove_enqueue(h, removed, d, msg)) return rc;
  if (int rc = foldin_remove_collect(h, !removed.empty(), msg)) return rc;
  if (removed_out) std::copy(removed.begin(), removed.end(), removed_out);
  if (n_removed_out) *n_removed_out = (int64_t)removed.size();
  return MALS_OK;
}

// ---- mals_grow_factor_rows ------------------------------------------------------------------------------------------
// Two steps (mals_group_grow_factor_rows enqueues every member's copies before it waits for any): the new blocks and the
// copies into them on the handle's stream, then the wait and the swap.
struct FoldinGrow {
  DeviceBuffer<float> rows;      // the larger replica, when the capacity did not do
  DeviceBuffer<uint32_t> bits;   // the longer userTagIDs mask (side Y)
  bool grows = false;
};

int foldin_grow_enqueue(mals_handle h, int side, int64_t n_rows, FoldinGrow& gw, std::string& msg) {
  SideState& s = h->side[side];
  const int k = h->cfg.features;
  if (s.F != s.F_own.get()) {
    msg = "the replica is the caller's (mals_bind_factors)";
    return MALS_INVALID_ARG;
  }
  if (n_rows < s.n_total) {
    msg = "a replica only grows";
    return MALS_INVALID_ARG;
  }
  if (n_rows == s.n_total) return MALS_OK;
  gw.grows = true;
  const size_t need = (size_t)n_rows * k, have = (size_t)s.n_total * k;
  float* rows = s.F;
  if (s.F_own.capacity() < need) {  // capacity doubling: a stream of new users does not copy the replica each time
    FCHK(msg, gw.rows.alloc(std::max(need, 2 * s.F_own.capacity())));
    FCHK(msg, hipMemcpyAsync(gw.rows.get(), s.F, sizeof(float) * have, hipMemcpyDeviceToDevice, h->stream));
    rows = gw.rows.get();
  }
  FCHK(msg, hipMemsetAsync(rows + have, 0, sizeof(float) * (need - have), h->stream));
  if (side == MALS_SIDE_Y && h->tag_bits.get()) {  // userTagIDs: the new items are no tags
    const size_t old_words = ((size_t)((h->tag_bits_items + 31) / 32) + 1) & ~(size_t)1;
    const size_t words = ((size_t)((n_rows + 31) / 32) + 1) & ~(size_t)1;
    const size_t tail = sizeof(unsigned long long) / sizeof(uint32_t);
    FCHK(msg, gw.bits.alloc(words + tail));
    FCHK(msg, hipMemsetAsync(gw.bits.get(), 0, sizeof(uint32_t) * (words + tail), h->stream));
    FCHK(msg, hipMemcpyAsync(gw.bits.get(), h->tag_bits.get(), sizeof(uint32_t) * old_words, hipMemcpyDeviceToDevice, h->stream));
    FCHK(msg, hipMemcpyAsync(gw.bits.get() + words, h->tag_bits.get() + old_words, sizeof(uint32_t) * tail, hipMemcpyDeviceToDevice, h->stream));
  }
  return MALS_OK;
}

// owns_grown_users (side X): the new users' known items are this handle's
int foldin_grow_finish(mals_handle h, int side, int64_t n_rows, FoldinGrow& gw, bool owns_grown_users, std::string& msg) {
  if (!gw.grows) return MALS_OK;
  SideState& s = h->side[side];
  FCHK(msg, hipStreamSynchronize(h->stream));
  if (gw.rows) {
    s.F_own = std::move(gw.rows);
    s.F = s.F_own.get();
  }
  if (gw.bits) {
    h->tag_bits = std::move(gw.bits);
    h->tag_bits_items = n_rows;
  }
  s.n_total = n_rows;
  s.G_valid = false;
  ++s.F_epoch;
  if (side == MALS_SIDE_X && owns_grown_users) h->grown_users_end.store(n_rows, std::memory_order_release);
  popular_touch(h, false);
  return MALS_OK;
}

int foldin_grow_run(mals_handle h, int side, int64_t n_rows, std::string& msg) {
  // grown users are this handle's when its users already reached the end of the old replica (a single handle)
  const bool owns = foldin_user_rows_end(h) >= h->side[side].n_total;
  FoldinGrow gw;
  if (int rc = foldin_grow_enqueue(h, side, n_rows, gw, msg)) return rc;
  return foldin_grow_finish(h, side, n_rows, gw, owns, msg);
}

// ---- mals_anonymous_features / mals_estimate_for_anonymous ----------------------------------------------------------
int foldin_anonymous_run(mals_handle h, int32_t nq, const int64_t* item_ptr, const int64_t* item_row, const float* values, float* out,
                         int32_t* found_out, const int64_t* to_row, float* dot_out, std::string& msg) {
  FoldinState& fs = *foldin_state(h);
  const int k = h->cfg.features;
  if (int rc = foldin_lds_limit(msg)) return rc;
  const int64_t n_items = item_ptr[nq];
  const int n_blocks = (nq + FOLDIN_LANES - 1) / FOLDIN_LANES;
  std::vector<int32_t> max_len((size_t)n_blocks, 0);
  for (int q = 0; q < nq; ++q)
    max_len[(size_t)(q / FOLDIN_LANES)] = std::max<int32_t>(max_len[(size_t)(q / FOLDIN_LANES)], (int32_t)(item_ptr[q + 1] - item_ptr[q]));
  DeviceBuffer<int64_t> d_i;   // item_ptr | item_row | to_row
  DeviceBuffer<float> d_f;     // values | out | dots
  DeviceBuffer<int32_t> d_n;   // max_len | found
  FCHK(msg, d_i.alloc((size_t)(nq + 1) + (size_t)n_items + (size_t)nq));
  FCHK(msg, d_f.alloc((size_t)n_items + (size_t)nq * k + (size_t)nq));
  FCHK(msg, d_n.alloc((size_t)n_blocks + (size_t)nq));
  int64_t* dp = d_i.get();
  int64_t* dr = dp + nq + 1;
  int64_t* dt = dr + n_items;
  float* dv = d_f.get();
  float* dout = dv + n_items;
  float* ddot = dout + (size_t)nq * k;
  FCHK(msg, hipMemcpyAsync(dp, item_ptr, sizeof(int64_t) * (size_t)(nq + 1), hipMemcpyHostToDevice, h->stream));
  if (n_items) FCHK(msg, hipMemcpyAsync(dr, item_row, sizeof(int64_t) * (size_t)n_items, hipMemcpyHostToDevice, h->stream));
  if (to_row) FCHK(msg, hipMemcpyAsync(dt, to_row, sizeof(int64_t) * (size_t)nq, hipMemcpyHostToDevice, h->stream));
  if (values && n_items) FCHK(msg, hipMemcpyAsync(dv, values, sizeof(float) * (size_t)n_items, hipMemcpyHostToDevice, h->stream));
  FCHK(msg, hipMemcpyAsync(d_n.get(), max_len.data(), sizeof(int32_t) * (size_t)n_blocks, hipMemcpyHostToDevice, h->stream));
  const size_t lds = (size_t)k * FOLDIN_LANES * (sizeof(double) + sizeof(float));
  hipLaunchKernelGGL(foldin_anonymous_kernel, dim3((unsigned)n_blocks), dim3(FOLDIN_LANES), lds, h->stream, h->side[MALS_SIDE_Y].F, k, dp, dr,
                     values ? dv : nullptr, nq, d_n.get(), foldin_view(fs.solver[MALS_SIDE_Y]), fs.rate, dout, d_n.get() + n_blocks,
                     to_row ? dt : nullptr, ddot);
  FCHK(msg, hipGetLastError());
  FCHK(msg, hipMemcpyAsync(out, dout, sizeof(float) * (size_t)nq * k, hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipMemcpyAsync(found_out, d_n.get() + n_blocks, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, h->stream));
  if (to_row) FCHK(msg, hipMemcpyAsync(dot_out, ddot, sizeof(float) * (size_t)nq, hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipStreamSynchronize(h->stream));
  return MALS_OK;
}
