// foldin_host.h -- host side of the online write path (mals_set_preferences, mals_set_user_tags, mals_set_item_tags,
// mals_remove_preferences, mals_grow_factor_rows, the fold-in reads; include/myrrix_als.h; kernels in foldin_kernels.h; the logic that needs no
// device in foldin_plan.h).  Included by mals_serving.hip inside its anonymous namespace, after topn_host.h: every call
// here runs as an exclusive ticket of the serving front (topn_front_submit), so the passes formed before it have finished
// and the passes formed after it wait for its work on the handle's stream (ev_begin), and the state below is only ever
// touched by the front's leader.
//
// ONE DRIVER PER WRITE.  A write is the same steps on a handle and on the members of a group (every member applies the same
// batch to its own replicas with the same deterministic kernels; only a user's owner keeps its known items), so each has one
// driver over (hs, n_members) -- foldin_set_members, foldin_remove_members, foldin_grow_members, popular_members
// (popular_host.h) -- that runs INSIDE the ticket its caller holds: foldin_exclusive for a handle, which passes (&h, 1),
// foldin_exclusive_all for a group.  What the two say differently is `via_group` (which users a batch may name, the hints of
// the texts) and the owners; both mark the batch's rows recent on hs[0] (a group's record lives on its first member).
//
// THE MEMBER LOOP (member_loop), which they and malsi_group_factor_digest share: an enqueue step per member, then a finish step
// per member, so that every member's device work is on its way before the first wait.  Its rules:
//   1. member m's device is current for both of its steps and for the release of its slot (the per-member temporaries);
//   2. the first failure's code and message are the call's, and no step runs after it (no finish after a failed enqueue);
//   3. after a failure nothing of the call still runs when it returns: the members touched so far are waited for (all of them
//      once the finish phase has begun), before any slot is released.
// Set relies on 2 and 3 (a member that answers otherwise than member 0 fails the call), remove and grow on all three (their
// slots are device buffers the enqueued work reads), the digest on 3 (the enqueued copy writes the caller's array), popular
// on 1 and 2, and on 3 for the partial array of its sum.
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
  KnownOverlay known;                  // knownItemIDs after the writes of this generation, by local user row (foldin_plan.h)
  FoldinPlanScratch plan_scratch;      // the level plan's table, reused from batch to batch
  DeviceBuffer<int64_t> d_rows;        // [2][n] user rows | item rows, level order
  DeviceBuffer<float> d_val;
  DeviceBuffer<int32_t> d_status;
  DeviceBuffer<double> d_fold;         // userFoldIn of every update of the batch
  DeviceBuffer<uint8_t> d_kind;        // per update, level order: FOLDIN_KIND_* (a batch with tag updates only)
  bool tag_marked = false;             // the batch in flight ran foldin_tag_mark_kernel
  PinnedBuffer<uint8_t> h_stage;
  EventPair ev;                        // around a batch's update kernels (timing enabled: mals_foldin_stats reads the time)
};

void popular_add_tag_users(mals_handle h, std::vector<int64_t>& local_rows);   // popular_host.h

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
  delete h->serving->fo;
  h->serving->fo = nullptr;
}

// a new generation (mals_set_known_items, mals_set_matrix of side X, mals_set_factor_rows / mals_bind_factors of X)
void foldin_drop_overlay(mals_handle h) {
  h->grown_users_end.store(-1, std::memory_order_release);
  if (FoldinState* fs = h->serving->fo) fs->known.clear();
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
  return (fs && fs->known.any()) || h->grown_users_end.load(std::memory_order_acquire) >= 0 ||
         foldin_base_rows(h) < h->side[MALS_SIDE_X].n_local;
}

// what a recommend pass needs of a user's known items beyond its base row: the items to exclude (appended to out,
// possibly repeated) and whether the base row is dropped (a replaced set, or a grown row the base CSR does not have)
bool foldin_known_view(mals_handle h, int64_t local_row, std::vector<int64_t>& out) {
  const FoldinState* fs = h->serving->fo;
  return fs ? fs->known.view(local_row, foldin_base_rows(h), out) : local_row >= foldin_base_rows(h);
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

// ---- the tickets ------------------------------------------------------------------------------------------------------------
// via_group: the call comes from the member's group (a mals_group_* twin), which routes the known items to their owner
int foldin_refuse(mals_handle h, const char* call, bool via_group = false) {
  if (h->group_member && !via_group)
    return topn_fail(h, MALS_INVALID_ARG, (std::string(call) + ": not for a member of a group (writes and fold-in reads go through the group: mals_group_set_preferences ...)").c_str());
  if (hipSetDevice(h->cfg.device) != hipSuccess) return topn_fail(h, MALS_HIP_ERROR, "hipSetDevice failed");
  return MALS_OK;
}

// body(msg) runs alone on the handle, in the front's queue order; a failure's message is published under the mutex
template <class Body>
int foldin_exclusive(mals_handle h, const char* call, Body&& body) {
  std::string msg;
  const std::function<int()> fn = [&]() -> int { return body(msg); };
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

// ---- the member loop (the rules: at the head of this file) --------------------------------------------------------------------
// One slot of temporaries per member, the caller's; member 0's is inline, so that a single handle allocates nothing.
template <class T>
struct MemberSlots {
  explicit MemberSlots(int n_members) : more((size_t)std::max(0, n_members - 1)) {}
  T& operator[](int m) { return m == 0 ? first : more[(size_t)m - 1]; }
  void release(int m) { (*this)[m] = T(); }
  T first;
  std::vector<T> more;
};
struct NoSlots { void release(int) {} };

// enqueue(m, msg) for every member, then finish(m, msg) for every member: both -> MALS_OK or the call's failure
template <class Slots, class Enqueue, class Finish>
int member_loop(mals_handle* hs, int n_members, Slots& slots, std::string& msg, Enqueue&& enqueue, Finish&& finish) {
  // member m's device current.  hipSetDevice is not free even where it changes nothing, so it is called only when the
  // device does change: never for a handle, nor for members that share a device
  int dev = -1;
  FCHK(msg, hipGetDevice(&dev));
  auto on_device = [&](int m) -> hipError_t {
    if (hs[m]->cfg.device == dev) return hipSuccess;
    const hipError_t e = hipSetDevice(hs[m]->cfg.device);
    dev = e == hipSuccess ? hs[m]->cfg.device : -1;
    return e;
  };
  auto step = [&](int m, auto& fn) -> int {
    FCHK(msg, on_device(m));
    return fn(m, msg);
  };
  int rc = MALS_OK, touched = 0;
  while (rc == MALS_OK && touched < n_members) rc = step(touched++, enqueue);
  if constexpr (!std::is_null_pointer_v<std::decay_t<Finish>>)   // (member_each has no second walk)
    for (int m = 0; m < n_members && rc == MALS_OK; ++m) rc = step(m, finish);
  for (int m = 0; rc != MALS_OK && m < touched; ++m)   // nothing of the call may still run when it returns
    if (on_device(m) == hipSuccess) (void)hipStreamSynchronize(hs[m]->stream);
  for (int m = 0; !std::is_same_v<Slots, NoSlots> && m < n_members; ++m)
    if (on_device(m) == hipSuccess) slots.release(m);
  return rc;
}

// one step per member that leaves nothing enqueued (host work, or device work it waits for itself)
template <class Slots, class Step>
int member_each(mals_handle* hs, int n_members, Slots& slots, std::string& msg, Step&& step) {
  return member_loop(hs, n_members, slots, msg, step, nullptr);
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

// every write is a new model: the next half-iteration re-pads and recomputes its Gramian (the generation's solvers stay)
void foldin_new_model(mals_handle h) {
  for (int s = 0; s < 2; ++s) {
    h->side[s].G_valid = false;
    ++h->side[s].F_epoch;
  }
}

// ---- mals_set_foldin_solver / mals_set_foldin_learn_rate --------------------------------------------------------------------
// inside a ticket: the solver's factors onto the handle's device (ipiv: the inverse of its pivot permutation)
int foldin_solver_install(mals_handle h, int side, mals_solver s, const std::vector<int32_t>& ipiv, std::string& msg) {
  const int k = h->cfg.features;
  FoldinSide& fs = foldin_state(h)->solver[side];
  fs.present = false;
  if (!s) return MALS_OK;
  if (!fs.a.get()) {
    FCHK(msg, fs.a.alloc((size_t)k * k));
    FCHK(msg, fs.tau.alloc((size_t)k));
    FCHK(msg, fs.ipiv.alloc((size_t)k));
  }
  FCHK(msg, hipMemcpyAsync(fs.a.get(), s->qr.factors(), sizeof(double) * (size_t)k * k, hipMemcpyHostToDevice, h->stream));
  FCHK(msg, hipMemcpyAsync(fs.tau.get(), s->qr.taus(), sizeof(double) * (size_t)k, hipMemcpyHostToDevice, h->stream));
  FCHK(msg, hipMemcpyAsync(fs.ipiv.get(), ipiv.data(), sizeof(int32_t) * (size_t)k, hipMemcpyHostToDevice, h->stream));
  FCHK(msg, hipStreamSynchronize(h->stream));
  fs.present = true;
  return MALS_OK;
}

std::vector<int32_t> foldin_solver_ipiv(mals_solver s, int k) {
  std::vector<int32_t> ipiv((size_t)k);
  if (s)
    for (int j = 0; j < k; ++j) ipiv[(size_t)s->qr.pivots()[j]] = j;
  return ipiv;
}

int foldin_solver_members(mals_handle* hs, int n_members, int side, mals_solver s, std::string& msg) {
  const std::vector<int32_t> ipiv = foldin_solver_ipiv(s, hs[0]->cfg.features);
  NoSlots none;
  return member_each(hs, n_members, none, msg, [&](int m, std::string& why) { return foldin_solver_install(hs[m], side, s, ipiv, why); });
}

int foldin_rate_members(mals_handle* hs, int n_members, double rate) {
  for (int m = 0; m < n_members; ++m) foldin_state(hs[m])->rate = rate;
  return MALS_OK;
}

// the pairs against the replicas as they stand inside the ticket (a concurrent grow is ordered before or after it).
// local_users: a batch names the users whose known items this handle holds, [row_offset, min(foldin_user_rows_end, n_total));
// else any user of the replica
int foldin_check_pairs(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* item_row, bool allow_unknown, bool local_users,
                       std::string& msg) {
  const SideState& x = h->side[MALS_SIDE_X];
  const SideState& y = h->side[MALS_SIDE_Y];
  if (!x.F || !y.F) {
    msg = "factor replicas not available";
    return MALS_INVALID_ARG;
  }
  const int64_t u_lo = local_users ? x.row_offset : 0, u_hi = local_users ? std::min(foldin_user_rows_end(h), x.n_total) : x.n_total;
  for (int64_t t = 0; t < n; ++t) {
    const bool u_ok = (user_row[t] >= u_lo && user_row[t] < u_hi) || (allow_unknown && user_row[t] == -1);
    const bool i_ok = (item_row[t] >= 0 && item_row[t] < y.n_total) || (allow_unknown && item_row[t] == -1);
    if (!u_ok || !i_ok) {
      msg = "pair " + std::to_string(t) + ": row outside the factor replicas (or the user's known items are not on this handle)";
      return MALS_INVALID_ARG;
    }
  }
  return MALS_OK;
}

// a write's batch before any work: a handle's call names its own users, a group's any user (each member is asked all the
// same).  Both mark the rows recent (doAppend, DelegateGenerationManager.java:179-186): a group keeps that record once, in
// global rows, on its first member (mals_group_load_generation reads it there)
int foldin_write_ready(mals_handle* hs, int n_members, bool via_group, int64_t n, const int64_t* user_row, const int64_t* item_row, std::string& msg) {
  for (int m = 0; m < n_members; ++m)
    if (int rc = foldin_check_pairs(hs[m], n, user_row, item_row, false, !via_group, msg)) return rc;
  generation_mark_pairs(hs[0], n, user_row, item_row);
  return MALS_OK;
}

// ---- mals_set_preferences / mals_set_user_tags / mals_set_item_tags ---------------------------------------------------------
// userTagIDs.add of a batch, on the handle's stream behind its level kernels (d_rows holds the level-ordered rows).  A handle
// without a mask gets one, zeroed, for the rows of Y as they stand (a grow of the same call has lengthened an existing one:
// foldin_grow_enqueue); it is published as foldin_grow_finish publishes a longer one -- plain stores inside the ticket, which
// the passes formed after it read.  The mask's counter word carries n_tag_items to the kernel and back.
// the stage of a batch of n: user rows | item rows | values (the status words come back over them) | kinds | the mask's counter
size_t foldin_stage_kind_at(int64_t n) { return sizeof(int64_t) * 2 * (size_t)n + sizeof(float) * (size_t)n; }
size_t foldin_stage_count_at(int64_t n) { return (foldin_stage_kind_at(n) + (size_t)n + 7) & ~(size_t)7; }

int foldin_tag_mark_enqueue(mals_handle h, int64_t n, const uint8_t* kind, const FoldinPlan& p, std::string& msg) {
  FoldinState& fs = *foldin_state(h);
  const int64_t n_items = h->side[MALS_SIDE_Y].n_total;
  const size_t words = ((size_t)((n_items + 31) / 32) + 1) & ~(size_t)1;   // (the layout of mals_set_tag_items)
  const size_t tail = sizeof(unsigned long long) / sizeof(uint32_t);
  if (h->tag_bits.get() && h->tag_bits_items != n_items) {
    msg = "the tag items were set for another item count";
    return MALS_INVALID_ARG;
  }
  if (!h->tag_bits.get()) {
    DeviceBuffer<uint32_t> bits;
    FCHK(msg, bits.alloc(words + tail));
    FCHK(msg, hipMemsetAsync(bits.get(), 0, sizeof(uint32_t) * (words + tail), h->stream));
    h->tag_bits = std::move(bits);
    h->tag_bits_items = n_items;
    h->n_tag_items = 0;
  }
  FCHK(msg, fs.d_kind.reserve((size_t)n, h->stream));
  uint8_t* hk = fs.h_stage.get() + foldin_stage_kind_at(n);   // (foldin_set_enqueue reserved the stage for them)
  unsigned long long* hn = reinterpret_cast<unsigned long long*>(fs.h_stage.get() + foldin_stage_count_at(n));
  for (int64_t j = 0; j < n; ++j) hk[j] = kind[p.order[(size_t)j]];
  unsigned long long* d_n = reinterpret_cast<unsigned long long*>(h->tag_bits.get() + words);
  *hn = (unsigned long long)h->n_tag_items;
  FCHK(msg, hipMemcpyAsync(fs.d_kind.get(), hk, (size_t)n, hipMemcpyHostToDevice, h->stream));
  FCHK(msg, hipMemcpyAsync(d_n, hn, sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(foldin_tag_mark_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const int64_t*)(fs.d_rows.get() + n),
                     (const uint8_t*)fs.d_kind.get(), n, n_items, h->tag_bits.get(), d_n);
  FCHK(msg, hipGetLastError());
  FCHK(msg, hipMemcpyAsync(hn, d_n, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  fs.tag_marked = true;
  return MALS_OK;
}

// The level plan (foldin_plan.h, the same for every replica the batch goes to), then per member the enqueue half (uploads, the
// level kernels and the status copy on the handle's stream, no wait) and the collect half (the wait and the host-side
// bookkeeping).
// kind (FOLDIN_KIND_* per update, or nullptr: all preferences): a tag update is the same kernel on (row of X, row of Y, value);
// behind the levels the Y rows of the setUserTag updates go into the userTagIDs mask, whatever became of their updates
int foldin_set_enqueue(mals_handle h, int64_t n, const int64_t* urow, const int64_t* irow, const float* value, const uint8_t* kind,
                       const FoldinPlan& p, std::string& msg) {
  FoldinState& fs = *foldin_state(h);
  SideState& x = h->side[MALS_SIDE_X];
  SideState& y = h->side[MALS_SIDE_Y];
  const int k = h->cfg.features;
  if (int rc = foldin_lds_limit(msg)) return rc;
  // level order on the device: user rows | item rows | values, one copy
  const size_t bytes = foldin_stage_count_at(n) + sizeof(unsigned long long);
  FCHK(msg, fs.h_stage.reserve(bytes, h->stream));
  FCHK(msg, fs.d_rows.reserve(2 * (size_t)n, h->stream));
  FCHK(msg, fs.d_val.reserve((size_t)n, h->stream));
  FCHK(msg, fs.d_status.reserve((size_t)n, h->stream));
  FCHK(msg, fs.d_fold.reserve((size_t)n * k, h->stream));
  FCHK(msg, fs.ev.ensure());
  int64_t* hu = reinterpret_cast<int64_t*>(fs.h_stage.get());
  int64_t* hi = hu + n;
  float* hv = reinterpret_cast<float*>(hi + n);
  for (int64_t j = 0; j < n; ++j) {
    const int64_t t = p.order[(size_t)j];
    hu[j] = urow[t];
    hi[j] = irow[t];
    hv[j] = value[t];
  }
  FCHK(msg, hipMemcpyAsync(fs.d_rows.get(), hu, sizeof(int64_t) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  FCHK(msg, hipMemcpyAsync(fs.d_val.get(), hv, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  const FoldinSide& SX = fs.solver[MALS_SIDE_X];
  const FoldinSide& SY = fs.solver[MALS_SIDE_Y];
  const size_t lds = (size_t)k * FOLDIN_LANES * sizeof(double);
  FCHK(msg, hipEventRecord(fs.ev.begin, h->stream));
  for (uint32_t l = 1; l <= p.n_levels; ++l) {
    const int64_t u0 = p.off[l], u1 = p.off[l + 1];
    hipLaunchKernelGGL(foldin_update_kernel, dim3((unsigned)((u1 - u0 + FOLDIN_LANES - 1) / FOLDIN_LANES)), dim3(FOLDIN_LANES), lds, h->stream, x.F,
                       y.F, k, fs.d_rows.get(), fs.d_rows.get() + n, fs.d_val.get(), u0, u1, foldin_view(SX), foldin_view(SY), SX.present ? 1 : 0,
                       SY.present ? 1 : 0, fs.rate, fs.big_total, fs.d_fold.get(), fs.d_status.get());
  }
  FCHK(msg, hipGetLastError());
  FCHK(msg, hipEventRecord(fs.ev.end, h->stream));
  int32_t* hs = reinterpret_cast<int32_t*>(fs.h_stage.get());
  FCHK(msg, hipMemcpyAsync(hs, fs.d_status.get(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  fs.tag_marked = false;
  bool any_user_tag = false;
  for (int64_t t = 0; kind && t < n && !any_user_tag; ++t) any_user_tag = kind[t] == FOLDIN_KIND_USER_TAG;
  if (any_user_tag) return foldin_tag_mark_enqueue(h, n, kind, p, msg);
  return MALS_OK;
}

// the known items of the applied updates are recorded for the users in [own_lo, own_hi) only: on a group the owner of a
// user keeps its overlay (a single handle owns every user foldin_check_pairs let through)
// A tag update (kind 1 or 2) adds no known item (setUserTag / setItemTag never touch knownItemIDs); the tag's mark is made
// whatever its update's status: the Y rows are in the mask by now (foldin_tag_mark_kernel), the X rows of the setItemTag
// updates join the tag users of their owner here (itemTagIDs.add, :1139)
int foldin_set_collect(mals_handle h, int64_t n, const int64_t* urow, const int64_t* irow, const uint8_t* kind, const FoldinPlan& p, int64_t own_lo,
                       int64_t own_hi, int32_t* status_out, std::string& msg) {
  FoldinState& fs = *foldin_state(h);
  SideState& x = h->side[MALS_SIDE_X];
  const int32_t* hs = reinterpret_cast<const int32_t*>(fs.h_stage.get());
  FCHK(msg, hipStreamSynchronize(h->stream));
  float dev_ms = 0.f;
  FCHK(msg, hipEventElapsedTime(&dev_ms, fs.ev.begin, fs.ev.end));
  foldin_new_model(h);
  if (fs.tag_marked) {
    h->n_tag_items = (int64_t)*reinterpret_cast<const unsigned long long*>(fs.h_stage.get() + foldin_stage_count_at(n));
    fs.tag_marked = false;
  }
  if (kind) {
    std::vector<int64_t> tag_users;
    for (int64_t t = 0; t < n; ++t)
      if (kind[t] == FOLDIN_KIND_ITEM_TAG && urow[t] >= own_lo && urow[t] < own_hi) tag_users.push_back(urow[t] - x.row_offset);
    if (!tag_users.empty()) popular_add_tag_users(h, tag_users);
  }
  int first = MALS_OK, first_why = 0;
  int64_t first_t = -1, applied = 0, failed = 0, big = 0;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t t = p.order[(size_t)j];
    const FoldinStatus st = foldin_status_decode(hs[j]);
    big += st.big;
    if (status_out) status_out[t] = st.code;
    if (st.code != MALS_OK) {
      ++failed;
      if (first_t < 0 || t < first_t) {
        first_t = t;
        first = st.code;
        first_why = st.why;
      }
      continue;
    }
    ++applied;
    if (kind && kind[t] != FOLDIN_KIND_PREF) continue;
    if (urow[t] >= own_lo && urow[t] < own_hi) fs.known.add(urow[t] - x.row_offset, (int32_t)irow[t]);   // knownItemIDs.get(userID).add(itemID) (:813-836)
  }
  if (applied) popular_touch(h, false);   // known items were added: what mals_most_popular_items counted is stale
  std::atomic<int64_t>* c = h->foldin_counters;
  c[0] += applied;
  c[1] += failed;
  c[2] += big;
  c[3] += p.n_levels;
  c[4] += (int64_t)((double)dev_ms * 1e6);
  c[5].store((int64_t)((double)dev_ms * 1e6));
  if (first != MALS_OK) msg = "update " + std::to_string(first_t) + ": " + foldin_why_text(first_why);
  return first;
}

// own (n_members + 1): member m records the known items of the users own[m] <= u < own[m + 1]
int foldin_set_members(mals_handle* hs, int n_members, const int64_t* own, bool via_group, int64_t n, const int64_t* urow, const int64_t* irow,
                       const float* value, const uint8_t* kind, int32_t* status_out, std::string& msg) {
  if (int rc = foldin_write_ready(hs, n_members, via_group, n, urow, irow, msg)) return rc;
  FoldinPlan plan;
  foldin_set_plan(foldin_state(hs[0])->plan_scratch, n, urow, irow, plan);
  // The statuses are every replica's own (the same arithmetic on the same bits); the caller gets member 0's, failed updates
  // among them, and a member that answers otherwise is a failure of its own
  int first = MALS_OK;
  std::string first_msg;
  NoSlots none;
  const int rc = member_loop(
      hs, n_members, none, msg, [&](int m, std::string& why) { return foldin_set_enqueue(hs[m], n, urow, irow, value, kind, plan, why); },
      [&](int m, std::string& why) -> int {
        std::string mine;
        const int r = foldin_set_collect(hs[m], n, urow, irow, kind, plan, own[m], own[m + 1], m == 0 ? status_out : nullptr, mine);
        if (m == 0) {
          first = r;
          first_msg.swap(mine);
          return MALS_OK;
        }
        if (r == first) return MALS_OK;
        why = "member " + std::to_string(m) + " answered " + std::to_string(r) + " where member 0 answered " + std::to_string(first) + ": " + mine;
        return r == MALS_OK ? MALS_HIP_ERROR : r;
      });
  if (rc != MALS_OK) return rc;
  msg.swap(first_msg);
  return first;
}

// ---- mals_remove_preferences ----------------------------------------------------------------------------------------
// The decision first, which is the known items' holder's alone -- the pairs whose user lies in [own_lo, own_hi) against this
// handle's sets; (position in the batch, user) of every user a pair empties is appended to `emptied` -- then zeroing those
// rows of X (enqueue) and the wait (collect), which every replica runs with the same list.
int foldin_remove_decide(mals_handle h, int64_t n, const int64_t* urow, const int64_t* irow, int64_t own_lo, int64_t own_hi,
                         std::vector<std::pair<int64_t, int64_t>>& emptied, std::string& msg) {
  KnownOverlay& known = foldin_state(h)->known;
  SideState& x = h->side[MALS_SIDE_X];
  auto mine = [&](int64_t t) { return urow[t] >= own_lo && urow[t] < own_hi; };
  // every user of the batch without a whole set gets one first: its base row and additions, fetched together
  std::vector<int64_t> need;
  for (int64_t t = 0; t < n; ++t)
    if (mine(t) && !known.has_set(urow[t] - x.row_offset)) need.push_back(urow[t] - x.row_offset);
  std::sort(need.begin(), need.end());
  need.erase(std::unique(need.begin(), need.end()), need.end());
  std::vector<std::vector<int32_t>> full;
  if (int rc = foldin_known_full(h, need, full, msg)) return rc;
  popular_touch(h, false);   // (conservative: a batch that removes nothing recounts too)
  for (size_t j = 0; j < need.size(); ++j) known.install(need[j], full[j]);   // (an empty set: a user without known items, whose removals are ignored)
  for (int64_t t = 0; t < n; ++t)
    // an item the user does not know: ignored (:1024-1033); its last one: the user goes (:1040-1058)
    if (mine(t) && known.remove(urow[t] - x.row_offset, (int32_t)irow[t]) == KnownOverlay::EMPTIED) emptied.push_back({t, urow[t]});
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
  foldin_new_model(h);
  return MALS_OK;
}

int foldin_remove_members(mals_handle* hs, int n_members, const int64_t* own, bool via_group, int64_t n, const int64_t* urow, const int64_t* irow,
                          int64_t* removed_out, int64_t* n_removed_out, std::string& msg) {
  for (int m = 0; m < n_members; ++m)
    if (!hs[m]->side[MALS_SIDE_X].has_matrix && !hs[m]->known_ptr) {
      msg = std::string("the user-side matrix (or ") + (via_group ? "the installed known items" : "mals_set_known_items") + ") holds the known items";
      return MALS_INVALID_ARG;
    }
  if (int rc = foldin_write_ready(hs, n_members, via_group, n, urow, irow, msg)) return rc;
  // the owners decide (small reads of their own known items, each waited for), in batch order within each owner; a user has
  // one owner.  Every decision is made before any row is zeroed
  std::vector<std::pair<int64_t, int64_t>> emptied;
  NoSlots none;
  if (int rc = member_each(hs, n_members, none, msg, [&](int m, std::string& why) {
        return foldin_remove_decide(hs[m], n, urow, irow, own[m], own[m + 1], emptied, why);
      }))
    return rc;
  std::sort(emptied.begin(), emptied.end());
  std::vector<int64_t> removed;
  for (const auto& e : emptied) removed.push_back(e.second);
  // every replica zeroes the same rows
  MemberSlots<DeviceBuffer<int64_t>> d(n_members);
  if (int rc = member_loop(
          hs, n_members, d, msg, [&](int m, std::string& why) { return foldin_remove_enqueue(hs[m], removed, d[m], why); },
          [&](int m, std::string& why) { return foldin_remove_collect(hs[m], !removed.empty(), why); }))
    return rc;
  if (removed_out) std::copy(removed.begin(), removed.end(), removed_out);
  if (n_removed_out) *n_removed_out = (int64_t)removed.size();
  return MALS_OK;
}

// ---- mals_grow_factor_rows ------------------------------------------------------------------------------------------
// Per member the new blocks and the copies into them on the handle's stream (enqueue), then the wait and the swap (finish).
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

// grown_owner: the member that owns the users past the installed matrix, or -1
int foldin_grow_members(mals_handle* hs, int n_members, int side, int64_t n_rows, int grown_owner, bool via_group, std::string& msg) {
  for (int m = 0; m < n_members; ++m)
    if (!hs[m]->side[side].F) {
      msg = std::string("the replica is not declared (") + (via_group ? "mals_group_set_factor_rows" : "mals_set_factor_rows") + ")";
      return MALS_INVALID_ARG;
    }
  MemberSlots<FoldinGrow> gw(n_members);   // (what a failure left behind goes with its device current)
  return member_loop(
      hs, n_members, gw, msg, [&](int m, std::string& why) { return foldin_grow_enqueue(hs[m], side, n_rows, gw[m], why); },
      [&](int m, std::string& why) { return foldin_grow_finish(hs[m], side, n_rows, gw[m], m == grown_owner, why); });
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
