// popular_host.h -- host side of mals_most_popular_items / mals_set_tag_users (include/myrrix_als.h; kernels in
// popular_kernels.h).  Included by mals_serving.hip inside its anonymous namespace, after foldin_host.h: the read runs as an
// exclusive ticket of the serving front (foldin_exclusive), so the state below is only ever touched by the front's leader --
// except that mals_set_tag_users replaces the tag users under the rule of mals_set_tag_items (not while calls are in flight);
// a write's setItemTag updates add to them inside their ticket (popular_add_tag_users).  One driver
// (popular_members) serves a handle and the members of a group, over the member loop of foldin_host.h.
//
// THE COUNT CACHE.  The per-item count array stays on the device.  The handle carries a counter (pop_epoch) that every
// call which may change a counted user's set bumps (popular_touch: a new generation's known items or user-side matrix, a
// new X replica, every applied write batch, the tag users); a call recounts when the counter, or the item count, is not
// the one its array was counted at.  Rescorers and the tag ITEMS act after the count (popular_key_kernel).
#pragma once

struct PopularState {
  std::vector<int64_t> tag_users;          // itemTagIDs as local user rows: ascending, unique
  DeviceBuffer<uint32_t> count;            // [n_items]: this handle's users
  uint64_t counted_epoch = 0;              // the pop_epoch `count` was counted at (0: never), set once the recount is waited for
  uint64_t enqueued_epoch = 0;             // ... and the one of a recount on its way (popular_count_enqueue -> _finish)
  int64_t counted_items = -1;
  uint64_t ascending_epoch = 0;            // the pop_base_epoch base_ascending was decided at (0: never)
  bool base_ascending = false;             // every row of the base CSR is strictly ascending
  // per recount: the skip bitset over the base rows, the override CSR, the pair counter and the ascending flag
  std::vector<uint32_t> h_skip;             // (host images: they outlive the asynchronous copies made from them)
  std::vector<int64_t> h_optr;
  std::vector<int32_t> h_oidx;
  DeviceBuffer<uint32_t> d_skip;
  DeviceBuffer<int64_t> d_optr;
  DeviceBuffer<int32_t> d_oidx;
  DeviceBuffer<unsigned long long> d_pairs;   // {pairs, flag}
  // per call: the keys, the selection state, the histogram and the survivors
  DeviceBuffer<unsigned long long> d_keys, d_out;
  DeviceBuffer<PopularSelect> d_sel;
  DeviceBuffer<unsigned> d_hist;
  DeviceBuffer<uint32_t> d_sum;            // a group's summed counts (on the member that selects)
};

PopularState* popular_state(mals_handle h) {
  if (!h->serving->pop) h->serving->pop = new PopularState();
  return h->serving->pop;
}

void popular_free(mals_handle h) {
  delete h->serving->pop;
  h->serving->pop = nullptr;
}

// a new generation: the cache goes (with the overlay, malsi_clear_known_items); new_rows: the local user rows are new ones, the
// tag users named the old
void popular_new_generation(mals_handle h, bool new_rows) {
  popular_touch(h, true);
  PopularState* ps = h->serving->pop;
  if (!ps) return;
  ps->count.reset();
  ps->counted_epoch = 0;
  if (new_rows) std::vector<int64_t>().swap(ps->tag_users);
}

// itemTagIDs (ServerRecommender.java:626, :638): global user rows (host); every member keeps the rows it owns (those outside
// a handle's users are ignored)
int popular_set_tag_users(mals_handle* hs, int n_members, int64_t n, const int64_t* user_idx) {
  for (int m = 0; m < n_members; ++m) {
    mals_handle h = hs[m];
    const int64_t lo = h->side[MALS_SIDE_X].row_offset, hi = foldin_user_rows_end(h);
    std::vector<int64_t> v;
    for (int64_t j = 0; j < n; ++j)
      if (user_idx[j] >= lo && user_idx[j] < hi) v.push_back(user_idx[j] - lo);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    popular_state(h)->tag_users.swap(v);
    popular_touch(h, false);
  }
  return MALS_OK;
}

// itemTagIDs.add of a write batch (foldin_set_collect, inside its ticket): local user rows of this handle, in any order, repeats
// allowed, merged into the ascending set; what was counted is stale only if the set grew
void popular_add_tag_users(mals_handle h, std::vector<int64_t>& local_rows) {
  std::vector<int64_t>& have = popular_state(h)->tag_users;
  std::sort(local_rows.begin(), local_rows.end());
  local_rows.erase(std::unique(local_rows.begin(), local_rows.end()), local_rows.end());
  std::vector<int64_t> merged;
  merged.reserve(have.size() + local_rows.size());
  std::set_union(have.begin(), have.end(), local_rows.begin(), local_rows.end(), std::back_inserter(merged));
  if (merged.size() == have.size()) return;
  have.swap(merged);
  popular_touch(h, false);
}

unsigned popular_grid(mals_handle h, int64_t n_units, int per_block) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((int64_t)h->n_cu * 8, (n_units + per_block - 1) / per_block));
}

// whether a call on this handle has anything to count (the reference: knownItemIDs == null -> UnsupportedOperationException, :622)
bool popular_has_known(mals_handle h) { return h->side[MALS_SIDE_X].has_matrix || h->known_ptr || foldin_has_overlay(h); }

// count[] of this handle's users for n_items items, enqueued on the handle's stream unless the cache holds it; *recounted
// says which.  The host work of a recount (the override CSR) is done here; the stats of a recount are read back by
// popular_count_finish, after the wait.
int popular_count_enqueue(mals_handle h, int64_t n_items, bool* recounted, int64_t* n_override, std::string& msg) {
  PopularState& ps = *popular_state(h);
  const uint64_t epoch = h->pop_epoch.load(std::memory_order_acquire);
  *recounted = false;
  if (ps.count && ps.counted_epoch == epoch && ps.counted_items == n_items) return MALS_OK;
  const SideState& x = h->side[MALS_SIDE_X];
  if (h->known_ptr && h->known_rows != x.n_local) {
    msg = "the installed known items do not match the local user rows";
    return MALS_INVALID_ARG;
  }
  const int64_t n_base = foldin_base_rows(h);
  const int64_t* bptr = h->known_ptr ? h->known_ptr : x.row_ptr;
  const int32_t* bidx = h->known_ptr ? h->known_idx : x.col;
  // users whose current set is not their base row: an added chain or a replaced set (grown users have nothing else)
  const FoldinState* fs = h->serving->fo;
  const std::vector<int64_t> orows = fs ? fs->known.override_rows() : std::vector<int64_t>();
  // the skip bits of the base pass: tag users and the users of the override CSR; the override CSR leaves the tag users out
  const size_t words = (size_t)((n_base + 31) / 32);
  std::vector<uint32_t>& skip = ps.h_skip;
  skip.clear();
  auto mark = [&](int64_t r) {
    if (r < n_base) {
      if (skip.empty()) skip.assign(words, 0u);
      skip[(size_t)(r >> 5)] |= 1u << (r & 31);
    }
  };
  for (int64_t r : ps.tag_users) mark(r);
  std::vector<int64_t> counted;
  for (int64_t r : orows) {
    mark(r);
    if (!std::binary_search(ps.tag_users.begin(), ps.tag_users.end(), r)) counted.push_back(r);
  }
  std::vector<std::vector<int32_t>> sets;
  if (!counted.empty())
    if (int rc = foldin_known_full(h, counted, sets, msg)) return rc;   // sorted, distinct
  std::vector<int64_t>& optr = ps.h_optr;
  optr.assign(counted.size() + 1, 0);
  for (size_t j = 0; j < counted.size(); ++j) optr[j + 1] = optr[j] + (int64_t)sets[j].size();
  std::vector<int32_t>& oidx = ps.h_oidx;
  oidx.resize((size_t)optr.back());
  for (size_t j = 0; j < counted.size(); ++j) std::copy(sets[j].begin(), sets[j].end(), oidx.begin() + optr[j]);
  *n_override = (int64_t)counted.size();

  ps.counted_epoch = 0;
  if (ps.count.capacity() != (size_t)n_items) {
    FCHK(msg, hipStreamSynchronize(h->stream));
    FCHK(msg, ps.count.alloc((size_t)n_items));
  }
  if (!ps.d_pairs) FCHK(msg, ps.d_pairs.alloc(2));
  FCHK(msg, hipMemsetAsync(ps.count.get(), 0, sizeof(uint32_t) * (size_t)n_items, h->stream));
  FCHK(msg, hipMemsetAsync(ps.d_pairs.get(), 0, 2 * sizeof(unsigned long long), h->stream));
  if (n_base > 0) {
    // once per installed base: are all its rows strictly ascending?
    const uint64_t base_epoch = h->pop_base_epoch.load(std::memory_order_acquire);
    if (ps.ascending_epoch != base_epoch) {
      int* d_flag = reinterpret_cast<int*>(ps.d_pairs.get() + 1);
      int flag = 0;
      hipLaunchKernelGGL(popular_ascending_kernel, dim3(popular_grid(h, n_base, 4)), dim3(256), 0, h->stream, bptr, bidx, n_base, d_flag);
      FCHK(msg, hipGetLastError());
      FCHK(msg, hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
      FCHK(msg, hipStreamSynchronize(h->stream));
      ps.base_ascending = flag == 0;
      ps.ascending_epoch = base_epoch;
    }
    const uint32_t* d_skip = nullptr;
    if (!skip.empty()) {
      FCHK(msg, ps.d_skip.reserve(words, h->stream));
      FCHK(msg, hipMemcpyAsync(ps.d_skip.get(), skip.data(), sizeof(uint32_t) * words, hipMemcpyHostToDevice, h->stream));
      d_skip = ps.d_skip.get();
    }
    const unsigned grid = popular_grid(h, n_base, 4);
    if (ps.base_ascending)
      hipLaunchKernelGGL(popular_count_kernel<true>, dim3(grid), dim3(256), 0, h->stream, bptr, bidx, n_base, d_skip, n_items, ps.count.get(),
                         ps.d_pairs.get());
    else
      hipLaunchKernelGGL(popular_count_kernel<false>, dim3(grid), dim3(256), 0, h->stream, bptr, bidx, n_base, d_skip, n_items, ps.count.get(),
                         ps.d_pairs.get());
    FCHK(msg, hipGetLastError());
  }
  if (!oidx.empty()) {
    FCHK(msg, ps.d_optr.reserve(optr.size(), h->stream));
    FCHK(msg, ps.d_oidx.reserve(oidx.size(), h->stream));
    FCHK(msg, hipMemcpyAsync(ps.d_optr.get(), optr.data(), sizeof(int64_t) * optr.size(), hipMemcpyHostToDevice, h->stream));
    FCHK(msg, hipMemcpyAsync(ps.d_oidx.get(), oidx.data(), sizeof(int32_t) * oidx.size(), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(popular_count_kernel<true>, dim3(popular_grid(h, (int64_t)counted.size(), 4)), dim3(256), 0, h->stream, ps.d_optr.get(),
                       ps.d_oidx.get(), (int64_t)counted.size(), (const uint32_t*)nullptr, n_items, ps.count.get(), ps.d_pairs.get());
    FCHK(msg, hipGetLastError());
  }
  *recounted = true;
  ps.counted_items = n_items;
  ps.enqueued_epoch = epoch;   // (counted_epoch stays 0 until popular_count_finish: a recount nobody waited for does not count)
  return MALS_OK;
}

// after popular_count_enqueue said `recounted`: the wait and the pair count of the recount
int popular_count_finish(mals_handle h, int64_t* pairs, std::string& msg) {
  PopularState& ps = *popular_state(h);
  unsigned long long p = 0;
  hipError_t e = hipMemcpyAsync(&p, ps.d_pairs.get(), sizeof(p), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  FCHK(msg, e);
  ps.counted_epoch = ps.enqueued_epoch;
  *pairs = (int64_t)p;
  return MALS_OK;
}

// count[] -> the how_many best, on the handle's stream; out arrays: one block of how_many entries, padded with -1 / -inf
int popular_select_run(mals_handle h, const uint32_t* count, int64_t n_items, const mals_rescorer_s* r, int32_t how_many, int64_t* item_idx_out,
                       float* score_out, int32_t* n_out, std::string& msg) {
  PopularState& ps = *popular_state(h);
  FCHK(msg, ps.d_keys.reserve((size_t)n_items, h->stream));
  FCHK(msg, ps.d_out.reserve(4096, h->stream));
  if (!ps.d_sel) FCHK(msg, ps.d_sel.alloc(1));
  if (!ps.d_hist) FCHK(msg, ps.d_hist.alloc(256));
  const uint32_t* tags = h->tag_bits.get();
  const unsigned item_blocks = (unsigned)((n_items + 255) / 256);
  std::shared_ptr<const RescorerState> keep;
  TopnRescore rs;
  if (r) {
    rescorer_bind(r, keep, rs);
    hipLaunchKernelGGL(popular_key_kernel<true>, dim3(item_blocks), dim3(256), 0, h->stream, count, n_items, tags, rs, ps.d_keys.get());
  } else {
    hipLaunchKernelGGL(popular_key_kernel<false>, dim3(item_blocks), dim3(256), 0, h->stream, count, n_items, tags, rs, ps.d_keys.get());
  }
  hipLaunchKernelGGL(popular_select_init_kernel, dim3(1), dim3(256), 0, h->stream, ps.d_sel.get(), ps.d_hist.get(), (int)how_many);
  const unsigned grid = popular_grid(h, n_items, 256 * 8);
  for (int pass = 0; pass < 8; ++pass) {
    hipLaunchKernelGGL(popular_hist_kernel, dim3(grid), dim3(256), 0, h->stream, ps.d_keys.get(), n_items, pass, ps.d_sel.get(), ps.d_hist.get());
    hipLaunchKernelGGL(popular_pick_kernel, dim3(1), dim3(256), 0, h->stream, ps.d_sel.get(), ps.d_hist.get(), pass);
  }
  hipLaunchKernelGGL(popular_collect_kernel, dim3(grid), dim3(256), 0, h->stream, ps.d_keys.get(), n_items, ps.d_sel.get(), (int)how_many,
                     ps.d_out.get());
  FCHK(msg, hipGetLastError());
  // only the result block crosses: the selection state and the survivors
  PopularSelect sel;
  std::vector<unsigned long long> got((size_t)how_many);
  FCHK(msg, hipMemcpyAsync(&sel, ps.d_sel.get(), sizeof(sel), hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipMemcpyAsync(got.data(), ps.d_out.get(), sizeof(unsigned long long) * (size_t)how_many, hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipStreamSynchronize(h->stream));
  const int n = (int)std::min<uint32_t>(sel.taken, (uint32_t)how_many);
  std::sort(got.begin(), got.begin() + n, std::greater<unsigned long long>());   // best first, equal values in ascending index
  for (int j = 0; j < how_many; ++j) {
    item_idx_out[j] = j < n ? (int64_t)(0xffffffffu - (uint32_t)(got[(size_t)j] & 0xffffffffull)) : -1;
    score_out[j] = j < n ? key_score((uint32_t)(got[(size_t)j] >> 32)) : -std::numeric_limits<float>::infinity();
  }
  if (n_out) *n_out = n;
  return MALS_OK;
}

// what a call checks inside its ticket, over the members (a handle: one).  The texts are each caller's
int popular_ready(mals_handle* hs, int n_members, bool via_group, int64_t* n_items, std::string& msg) {
  bool any_known = false;
  for (int m = 0; m < n_members; ++m) {
    const SideState& y = hs[m]->side[MALS_SIDE_Y];
    if (!y.F || y.n_total <= 0 || (m > 0 && y.n_total != *n_items)) {
      msg = via_group ? "the item factor rows are not declared alike on every member"
                      : "the item factor rows are not declared (they say how many items there are)";
      return MALS_INVALID_ARG;
    }
    *n_items = y.n_total;
    any_known = any_known || popular_has_known(hs[m]);
  }
  if (!any_known) {
    msg = via_group ? "no known items: neither a user-side matrix, nor installed known items, nor writes"
                    : "no known items: neither a user-side matrix, nor mals_set_known_items, nor writes (the reference throws UnsupportedOperationException)";
    return MALS_INVALID_ARG;
  }
  if (hs[0]->tag_bits.get() && hs[0]->tag_bits_items != *n_items) {
    msg = via_group ? "the tag items were set for another item count" : "the tag items were set for another item count: call mals_set_tag_items again";
    return MALS_INVALID_ARG;
  }
  return MALS_OK;
}

void popular_note(mals_handle h, bool recounted, int64_t n_override, int64_t pairs) {
  std::atomic<int64_t>* c = h->popular_counters;
  ++c[0];
  if (recounted) {
    ++c[1];
    c[2].store(n_override);
    c[3].store(pairs);
  }
}

// Every member counts the users it owns, side by side; member 0 saturates, strikes the tag items and selects (r: a handle's
// rescorer, a group has none).  One member selects from its own array; of several, the partial arrays are added on member 0
// first (peer copies into d_sum) -- after the sum, as one handle would.
int popular_members(mals_handle* hs, int n_members, bool via_group, const mals_rescorer_s* r, int32_t how_many, int64_t* item_idx_out,
                    float* score_out, int32_t* n_out, std::string& msg) {
  int64_t n_items = 0;
  if (int rc = popular_ready(hs, n_members, via_group, &n_items, msg)) return rc;
  struct Recount { bool recounted = false; int64_t n_override = 0; };
  MemberSlots<Recount> rec(n_members);
  if (int rc = member_loop(
          hs, n_members, rec, msg,
          [&](int m, std::string& why) { return popular_count_enqueue(hs[m], n_items, &rec[m].recounted, &rec[m].n_override, why); },
          [&](int m, std::string& why) -> int {
            int64_t pairs = 0;
            if (rec[m].recounted)
              if (int rc = popular_count_finish(hs[m], &pairs, why)) return rc;
            popular_note(hs[m], rec[m].recounted, rec[m].n_override, pairs);
            return MALS_OK;
          }))
    return rc;
  // The sum and the selection are member 0's alone.  They go through the member loop all the same, over that one member:
  // it makes member 0's device current and, on a failure, waits for its stream before `part` goes (rules 1 and 3)
  MemberSlots<DeviceBuffer<uint32_t>> part(1);
  return member_each(hs, 1, part, msg, [&](int, std::string& why) -> int {
    mals_handle h0 = hs[0];
    PopularState& p0 = *popular_state(h0);
    const uint32_t* count = p0.count.get();
    if (n_members > 1) {
      const size_t bytes = sizeof(uint32_t) * (size_t)n_items;
      FCHK(why, p0.d_sum.reserve((size_t)n_items, h0->stream));
      FCHK(why, hipMemcpyAsync(p0.d_sum.get(), p0.count.get(), bytes, hipMemcpyDeviceToDevice, h0->stream));
      FCHK(why, part[0].alloc((size_t)n_items));
      for (int m = 1; m < n_members; ++m) {
        FCHK(why, hipMemcpyPeerAsync(part[0].get(), h0->cfg.device, popular_state(hs[m])->count.get(), hs[m]->cfg.device, bytes, h0->stream));
        hipLaunchKernelGGL(popular_add_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, h0->stream, p0.d_sum.get(), part[0].get(), n_items);
        FCHK(why, hipGetLastError());
      }
      count = p0.d_sum.get();
    }
    return popular_select_run(h0, count, n_items, r, how_many, item_idx_out, score_out, n_out, why);
  });
}
