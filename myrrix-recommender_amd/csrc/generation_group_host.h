// generation_group_host.h -- host side of mals_group_load_generation (include/myrrix_als.h; kernels in generation_kernels.h and
// generation_group_kernels.h; the ownership plan in generation_group_plan.h).  Included by mals_serving.hip inside its anonymous
// namespace, after generation_host.h.  The call runs with the serving fronts of ALL members held (foldin_exclusive_all).
//
// ONE MODEL, W MEMBERS.  Every member runs the load's JOIN / KEEP / SCAN / MAP / GATHER (generation_side_begin / _mid / _end) on
// its own replicas and its own stream -- the replicated state machine of the write path: the kernels are deterministic, nothing
// is exchanged, and every member's step is enqueued before any is waited for.  What is NOT replicated is the known items: they
// stay with a user's owner, and the owners change (the plan).  Per old owner the PLAIN kept users' sets are built on the device
// (COUNT, SCAN, FILL); what crosses to the host per member is the counts (the plan's sizes), their total and the dropped
// count.  The kept users WITH an overlay view (additions, a replaced set, a grown row: the few that were written) go the single
// handle's way (generation_kept_sets) and are installed on their new owner as whole sets beside an empty base row.  Every new
// owner's base CSR is then assembled on its own stream from its slice of the new model's CSR and the runs of the old owners'
// kept CSRs the plan sends it (peer copies, row pointers rebased by geng_rebase_kernel).
//
// ALL OR NOTHING: every member builds aside (GenPrepared); generation_swap_prepare for all, then generation_swap for all.  A
// failure before that leaves every member as it was, and nothing of the call in flight (generation_group_run waits).
#pragma once

// what an old owner builds of its kept users
struct GenGroupKept {
  int64_t k0 = 0, n = 0;                       // its run of the kept list
  std::vector<int64_t> rows;                   // per kept user: the local base row of a plain one, -1 of an overlay one
  std::vector<int64_t> overlay_at, overlay_rows;   // the overlay users: position in the run, local row
  DeviceBuffer<int64_t> d_rows, ptr;           // ptr: n + 1, over the plain users' mapped entries
  DeviceBuffer<unsigned long long> counts, tile_sums, dropped;
  DeviceBuffer<int32_t> idx;
  std::vector<int64_t> h_ptr;                  // the host's copy of ptr (the running sum of the counts)
  unsigned long long h_dropped = 0;
};

struct GenGroupMember {
  GenPrepared p;
  GenEvents ev[2];   // per side
  GenGroupKept kept;
};

unsigned generation_group_wave_grid(mals_handle h, int64_t n_users) {   // one user per wave, four waves per block
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((int64_t)h->n_cu * 8, (n_users + 3) / 4));
}

// COUNT and SCAN of old owner h's run of the kept list, and the copies of the counts and the dropped count to the host:
// enqueued, not waited for.  sizes: the run's slice of the plan's sizes (the counts land there, 64 bits each)
int generation_group_count(mals_handle h, const GenSide& gy, const int64_t* kept_rows, GenGroupKept& kk, int64_t* sizes, std::string& msg) {
  if (kk.n == 0) return MALS_OK;
  const SideState& x = h->side[MALS_SIDE_X];
  const int64_t n_base = foldin_base_rows(h);
  const FoldinState* fs = h->serving->fo;
  kk.rows.assign((size_t)kk.n, -1);
  std::vector<int64_t> scratch;
  for (int64_t i = 0; i < kk.n; ++i) {
    const int64_t local = kept_rows[kk.k0 + i] - x.row_offset;
    scratch.clear();
    const bool drop = fs ? fs->known.view(local, n_base, scratch) : local >= n_base;
    if (!drop && scratch.empty() && local >= 0 && local < n_base) {
      kk.rows[(size_t)i] = local;
    } else {
      kk.overlay_at.push_back(i);
      kk.overlay_rows.push_back(local);
    }
  }
  const int64_t* bptr = h->known_ptr ? h->known_ptr : x.row_ptr;
  const int32_t* bidx = h->known_ptr ? h->known_idx : x.col;
  const int64_t n_tiles = (kk.n + GENG_SCAN_TILE - 1) / GENG_SCAN_TILE;
  FCHK(msg, kk.d_rows.alloc((size_t)kk.n));
  FCHK(msg, kk.counts.alloc((size_t)kk.n));
  FCHK(msg, kk.tile_sums.alloc((size_t)n_tiles));
  FCHK(msg, kk.ptr.alloc((size_t)kk.n + 1));
  FCHK(msg, kk.dropped.alloc(1));
  FCHK(msg, hipMemcpyAsync(kk.d_rows.get(), kk.rows.data(), sizeof(int64_t) * (size_t)kk.n, hipMemcpyHostToDevice, h->stream));
  FCHK(msg, hipMemsetAsync(kk.dropped.get(), 0, sizeof(unsigned long long), h->stream));
  hipLaunchKernelGGL(geng_count_kernel, dim3(generation_group_wave_grid(h, kk.n)), dim3(256), 0, h->stream, bptr, bidx, (const int64_t*)kk.d_rows.get(), kk.n,
                     (const int64_t*)gy.map.get(), gy.n_cur, kk.counts.get(), kk.dropped.get());
  hipLaunchKernelGGL(geng_scan_reduce_kernel, dim3((unsigned)n_tiles), dim3(256), 0, h->stream, (const unsigned long long*)kk.counts.get(), kk.n,
                     kk.tile_sums.get());
  hipLaunchKernelGGL(geng_scan_sums_kernel, dim3(1), dim3(256), 0, h->stream, kk.tile_sums.get(), n_tiles);
  hipLaunchKernelGGL(geng_scan_apply_kernel, dim3((unsigned)n_tiles), dim3(256), 0, h->stream, (const unsigned long long*)kk.counts.get(), kk.n,
                     (const unsigned long long*)kk.tile_sums.get(), kk.ptr.get());
  FCHK(msg, hipGetLastError());
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "a count is copied into the plan's sizes");
  FCHK(msg, hipMemcpyAsync(sizes, kk.counts.get(), sizeof(int64_t) * (size_t)kk.n, hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipMemcpyAsync(&kk.h_dropped, kk.dropped.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  return MALS_OK;
}

// after the wait: the host's running sum of the counts, then FILL (enqueued)
int generation_group_fill(mals_handle h, const GenSide& gy, GenGroupKept& kk, const int64_t* sizes, std::string& msg) {
  if (kk.n == 0) return MALS_OK;
  const SideState& x = h->side[MALS_SIDE_X];
  kk.h_ptr.assign((size_t)kk.n + 1, 0);
  for (int64_t i = 0; i < kk.n; ++i) kk.h_ptr[(size_t)i + 1] = kk.h_ptr[(size_t)i] + sizes[i];
  const int64_t total = kk.h_ptr.back();
  FCHK(msg, kk.idx.alloc((size_t)std::max<int64_t>(total, 1)));
  if (total > 0) {
    const int64_t* bptr = h->known_ptr ? h->known_ptr : x.row_ptr;
    const int32_t* bidx = h->known_ptr ? h->known_idx : x.col;
    hipLaunchKernelGGL(geng_fill_kernel, dim3(generation_group_wave_grid(h, kk.n)), dim3(256), 0, h->stream, bptr, bidx, (const int64_t*)kk.d_rows.get(), kk.n,
                       (const int64_t*)gy.map.get(), gy.n_cur, (const int64_t*)kk.ptr.get(), kk.idx.get());
    FCHK(msg, hipGetLastError());
  }
  return MALS_OK;
}

// bytes of member `from`'s block to member `to`'s, on `to`'s stream: a peer copy between devices
hipError_t generation_group_copy(void* dst, mals_handle to, const void* src, mals_handle from, size_t bytes) {
  if (to->cfg.device == from->cfg.device) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, to->stream);
  return hipMemcpyPeerAsync(dst, to->cfg.device, src, from->cfg.device, bytes, to->stream);
}

// new owner j's base CSR over the merged users [b0, b1): its slice of the new model's CSR, then the runs of the old owners' kept
// CSRs, row pointers rebased to 0 -- enqueued on j's stream (every old owner's stream has been waited for)
int generation_group_assemble(mals_handle* hs, int n_members, int j, const mals_generation_load& L, const std::vector<int64_t>& new_ptr,
                              const GenGroupPlan& plan, std::vector<std::unique_ptr<GenGroupMember>>& M, std::string& msg) {
  mals_handle h = hs[j];
  GenPrepared& p = M[(size_t)j]->p;
  const int64_t n_new = (int64_t)new_ptr.size() - 1;
  const int64_t b0 = plan.bounds[(size_t)j], b1 = plan.bounds[(size_t)j + 1];
  const int64_t r0 = std::min(b0, n_new), r1 = std::min(b1, n_new);
  int64_t entries = new_ptr[(size_t)r1] - new_ptr[(size_t)r0], rows = r1 - r0;
  for (int m = 0; m < n_members; ++m) {
    const int64_t* run = plan.run(n_members, m, j);
    if (run[1] <= run[0]) continue;
    const GenGroupKept& kk = M[(size_t)m]->kept;
    if (run[0] < 0 || run[1] > kk.n || (int64_t)kk.h_ptr.size() != kk.n + 1) {
      msg = "the ownership plan names users member " + std::to_string(m) + " does not keep";
      return MALS_HIP_ERROR;
    }
    entries += kk.h_ptr[(size_t)run[1]] - kk.h_ptr[(size_t)run[0]];
    rows += run[1] - run[0];
  }
  if (rows != b1 - b0) {   // (before anything is written: the copies below fill exactly b1 - b0 rows)
    msg = "the ownership plan does not cover member " + std::to_string(j) + "'s users";
    return MALS_HIP_ERROR;
  }
  p.member = true;
  p.own_lo = b0;
  p.own_hi = b1;
  FCHK(msg, p.known_ptr.alloc((size_t)(b1 - b0) + 1));
  FCHK(msg, p.known_idx.alloc((size_t)std::max<int64_t>(entries, 1)));
  FCHK(msg, hipMemsetAsync(p.known_ptr.get(), 0, sizeof(int64_t), h->stream));
  int64_t row_at = 0, entry_at = 0;
  const unsigned grid_cap = (unsigned)h->n_cu * 8;
  auto rebase = [&](int64_t n_ptrs, int64_t first) {
    hipLaunchKernelGGL(geng_rebase_kernel, dim3(std::max(1u, std::min(grid_cap, (unsigned)((n_ptrs + 255) / 256)))), dim3(256), 0, h->stream,
                       p.known_ptr.get() + row_at, n_ptrs, first, entry_at);
  };
  if (r1 > r0) {   // the new model's slice (its row pointers are on the host: the plan read them)
    const int64_t e0 = new_ptr[(size_t)r0], n_e = new_ptr[(size_t)r1] - e0;
    FCHK(msg, hipMemcpyAsync(p.known_ptr.get(), new_ptr.data() + r0, sizeof(int64_t) * (size_t)(r1 - r0 + 1), hipMemcpyHostToDevice, h->stream));
    rebase(r1 - r0 + 1, e0);
    if (n_e > 0)
      FCHK(msg, hipMemcpyAsync(p.known_idx.get(), L.new_known_idx + e0, sizeof(int32_t) * (size_t)n_e,
                               L.new_mem_kind == MALS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->stream));
    row_at = r1 - r0;
    entry_at = n_e;
  }
  for (int m = 0; m < n_members; ++m) {
    const int64_t* run = plan.run(n_members, m, j);
    const int64_t n_rows = run[1] - run[0];
    if (n_rows <= 0) continue;
    const GenGroupKept& kk = M[(size_t)m]->kept;
    const int64_t e0 = kk.h_ptr[(size_t)run[0]], n_e = kk.h_ptr[(size_t)run[1]] - e0;
    // (the run's first pointer lands on the pointer that ends the rows before it: after the rebase both say entry_at)
    FCHK(msg, generation_group_copy(p.known_ptr.get() + row_at, h, kk.ptr.get() + run[0], hs[m], sizeof(int64_t) * (size_t)(n_rows + 1)));
    rebase(n_rows + 1, e0);
    if (n_e > 0)
      FCHK(msg, generation_group_copy(p.known_idx.get() + entry_at, h, kk.idx.get() + e0, hs[m], sizeof(int32_t) * (size_t)n_e));
    row_at += n_rows;
    entry_at += n_e;
  }
  FCHK(msg, hipGetLastError());
  if (row_at != b1 - b0 || entry_at != entries) {
    msg = "the ownership plan does not cover member " + std::to_string(j) + "'s users";
    return MALS_HIP_ERROR;
  }
  return MALS_OK;
}

// loads[m]: the call's arguments as member m reads them (device arrays on ITS device).  old_bounds: the group's bounds[X]
// (n_members + 1) or NULL; bounds_x_out / bounds_y_out: n_members + 1 each, written on success only.
int generation_group_body(mals_handle* hs, int n, const mals_generation_load* loads, mals_generation_result* R, const int64_t* old_bounds,
                          int64_t* bounds_x_out, int64_t* bounds_y_out, std::vector<std::unique_ptr<GenGroupMember>>& M, std::string& msg) {
  const auto t0 = std::chrono::steady_clock::now();
  const int k = hs[0]->cfg.features;
  bool holds_known = false;
  for (int m = 0; m < n; ++m) {
    if (int rc = generation_load_check(hs[m], loads[m], true, msg)) return rc;
    holds_known = holds_known || generation_holds_known(hs[m]);
  }
  const mals_generation_load& L0 = loads[0];
  if (holds_known && !L0.new_known_ptr) {
    msg = "the group holds known items: the new model's are needed (new_known_ptr)";
    return MALS_INVALID_ARG;
  }
  const GenerationState& gs0 = *generation_state(hs[0]);   // the group's recent rows
  NoSlots none;
  // THE SIDES, every member's steps enqueued before the wait
  if (int rc = member_loop(
          hs, n, none, msg,
          [&](int m, std::string& why) -> int {
            for (int sd = 0; sd < 2; ++sd)
              if (int rc = generation_side_begin(hs[m], sd, loads[m], gs0.recent[sd], M[(size_t)m]->ev[sd], M[(size_t)m]->p.side[sd], why)) return rc;
            return MALS_OK;
          },
          [&](int m, std::string& why) -> int {
            FCHK(why, hipStreamSynchronize(hs[m]->stream));
            for (int sd = 0; sd < 2; ++sd)
              if (int rc = generation_side_mid(hs[m], sd, loads[m], M[(size_t)m]->ev[sd], M[(size_t)m]->p.side[sd], why)) return rc;
            return MALS_OK;
          }))
    return rc;
  if (int rc = member_each(hs, n, none, msg, [&](int m, std::string& why) -> int {
        FCHK(why, hipStreamSynchronize(hs[m]->stream));
        for (int sd = 0; sd < 2; ++sd) generation_side_end(M[(size_t)m]->p.side[sd]);
        for (int sd = 0; sd < 2; ++sd)
          if (M[(size_t)m]->p.side[sd].n_kept != M[0]->p.side[sd].n_kept || M[(size_t)m]->p.side[sd].n_hit != M[0]->p.side[sd].n_hit) {
            why = "member " + std::to_string(m) + " joined otherwise than member 0 (the replicas differ)";
            return MALS_HIP_ERROR;
          }
        return MALS_OK;
      }))
    return rc;
  const GenSide& gx0 = M[0]->p.side[MALS_SIDE_X];
  const GenSide& gy0 = M[0]->p.side[MALS_SIDE_Y];
  const int64_t n_new = gx0.n_new, n_kept = gx0.n_kept, n_items = gy0.n_new + gy0.n_kept;
  const std::vector<int64_t>& kept_rows = gx0.h_kept_rows;
  const auto t1 = std::chrono::steady_clock::now();

  // KNOWN ITEMS
  const bool install = L0.new_known_ptr != nullptr;
  std::vector<int64_t> new_ptr, sizes((size_t)n_kept, 0);
  int64_t known_dropped = 0;
  GenGroupPlan plan;
  std::vector<int64_t> kept_start((size_t)n + 1, 0);
  generation_group_kept_start(n, n_kept, kept_rows.data(), old_bounds, kept_start.data());
  if (install) {
    new_ptr.assign((size_t)n_new + 1, 0);
    if (n_new > 0) {
      if (L0.new_mem_kind == MALS_MEM_HOST) {
        std::copy(L0.new_known_ptr, L0.new_known_ptr + n_new + 1, new_ptr.begin());
      } else {
        FCHK(msg, hipSetDevice(hs[0]->cfg.device));
        FCHK(msg, hipMemcpy(new_ptr.data(), L0.new_known_ptr, sizeof(int64_t) * (size_t)(n_new + 1), hipMemcpyDeviceToHost));
      }
    }
    bool ok = new_ptr[0] >= 0;
    for (int64_t r = 0; r < n_new && ok; ++r) ok = new_ptr[(size_t)r + 1] >= new_ptr[(size_t)r];
    if (!ok || (new_ptr.back() > new_ptr[0] && !L0.new_known_idx)) {
      msg = "bad known-item arrays of the new model";
      return MALS_INVALID_ARG;
    }
    if (n_kept > 0 && holds_known) {
      // every old owner: COUNT and SCAN enqueued, then (after its wait) FILL enqueued and the overlay users' sets on the host
      std::vector<std::vector<std::vector<int32_t>>> overlay_sets((size_t)n);
      if (int rc = member_loop(
              hs, n, none, msg,
              [&](int m, std::string& why) -> int {
                GenGroupKept& kk = M[(size_t)m]->kept;
                kk.k0 = kept_start[(size_t)m];
                kk.n = kept_start[(size_t)m + 1] - kk.k0;
                return generation_group_count(hs[m], M[(size_t)m]->p.side[MALS_SIDE_Y], kept_rows.data(), kk, sizes.data() + kk.k0, why);
              },
              [&](int m, std::string& why) -> int {
                GenGroupKept& kk = M[(size_t)m]->kept;
                FCHK(why, hipStreamSynchronize(hs[m]->stream));
                if (int rc = generation_group_fill(hs[m], M[(size_t)m]->p.side[MALS_SIDE_Y], kk, sizes.data() + kk.k0, why)) return rc;
                known_dropped += (int64_t)kk.h_dropped;
                if (!kk.overlay_rows.empty()) {
                  if (int rc = generation_kept_sets(hs[m], M[(size_t)m]->p.side[MALS_SIDE_Y], kk.overlay_rows, overlay_sets[(size_t)m], &known_dropped, why))
                    return rc;
                  for (size_t o = 0; o < kk.overlay_at.size(); ++o)
                    sizes[(size_t)(kk.k0 + kk.overlay_at[o])] = (int64_t)overlay_sets[(size_t)m][o].size();
                }
                return MALS_OK;
              }))
        return rc;
      if (int rc = member_each(hs, n, none, msg, [&](int m, std::string& why) -> int {
            FCHK(why, hipStreamSynchronize(hs[m]->stream));
            return MALS_OK;
          }))
        return rc;
      if (!generation_group_plan(n, k, n_new, new_ptr.data(), n_kept, sizes.data(), kept_rows.data(), old_bounds, plan)) {
        msg = "the ownership plan failed";
        return MALS_INVALID_ARG;
      }
      // the overlay users' sets to their new owners
      for (int m = 0; m < n; ++m) {
        const GenGroupKept& kk = M[(size_t)m]->kept;
        for (size_t o = 0; o < kk.overlay_at.size(); ++o) {
          std::vector<int32_t>& set = overlay_sets[(size_t)m][o];
          if (set.empty()) continue;
          const int64_t u = n_new + kk.k0 + kk.overlay_at[o];
          const int j = owner_of(plan.bounds, u);
          M[(size_t)j]->p.kept_sets[u - plan.bounds[(size_t)j]] = std::move(set);
        }
      }
    } else {
      for (int m = 0; m < n; ++m) {   // nothing kept, or nothing known before: empty kept CSRs
        GenGroupKept& kk = M[(size_t)m]->kept;
        kk.k0 = kept_start[(size_t)m];
        kk.n = kept_start[(size_t)m + 1] - kk.k0;
        kk.h_ptr.assign((size_t)kk.n + 1, 0);
      }
      if (int rc = member_each(hs, n, none, msg, [&](int m, std::string& why) -> int {
            GenGroupKept& kk = M[(size_t)m]->kept;
            if (kk.n == 0) return MALS_OK;
            FCHK(why, kk.ptr.alloc((size_t)kk.n + 1));
            FCHK(why, kk.idx.alloc(1));
            FCHK(why, hipMemsetAsync(kk.ptr.get(), 0, sizeof(int64_t) * ((size_t)kk.n + 1), hs[m]->stream));
            FCHK(why, hipStreamSynchronize(hs[m]->stream));
            return MALS_OK;
          }))
        return rc;
      if (!generation_group_plan(n, k, n_new, new_ptr.data(), n_kept, sizes.data(), kept_rows.data(), old_bounds, plan)) {
        msg = "the ownership plan failed";
        return MALS_INVALID_ARG;
      }
    }
    if (int rc = member_loop(
            hs, n, none, msg,
            [&](int j, std::string& why) -> int {
              M[(size_t)j]->p.install_known = true;
              return generation_group_assemble(hs, n, j, loads[j], new_ptr, plan, M, why);
            },
            [&](int j, std::string& why) -> int {
              FCHK(why, hipStreamSynchronize(hs[j]->stream));
              return MALS_OK;
            }))
      return rc;
  } else {
    // no known items before and none brought: the plan cuts by rows alone
    if (!generation_group_plan(n, k, n_new, nullptr, n_kept, sizes.data(), kept_rows.data(), old_bounds, plan)) {
      msg = "the ownership plan failed";
      return MALS_INVALID_ARG;
    }
  }
  const auto t2 = std::chrono::steady_clock::now();

  // TAG SETS: the tag users once (global merged rows, split by the new owners as mals_group_set_tag_users does), the tag items
  // on every member; ids without a row are counted once, by member 0
  int64_t without_row = 0;
  {
    std::vector<int64_t> live, tag_users;
    for (int m = 0; m < n; ++m)
      if (hs[m]->serving->pop)
        for (int64_t r : popular_state(hs[m])->tag_users) live.push_back(r + hs[m]->side[MALS_SIDE_X].row_offset);
    std::sort(live.begin(), live.end());
    FCHK(msg, hipSetDevice(hs[0]->cfg.device));
    if (int rc = generation_tag_users(hs[0], gx0, L0, gs0.recent[MALS_SIDE_X], live, tag_users, &without_row, msg)) return rc;
    if (install)
      for (int64_t u : tag_users) {
        const int j = owner_of(plan.bounds, u);
        M[(size_t)j]->p.tag_users.push_back(u - plan.bounds[(size_t)j]);
      }
    if (int rc = member_each(hs, n, none, msg, [&](int m, std::string& why) -> int {
          int64_t ignored = 0;
          return generation_tag_items(hs[m], M[(size_t)m]->p.side[MALS_SIDE_Y], loads[m], gs0.recent[MALS_SIDE_Y], M[(size_t)m]->p,
                                      m == 0 ? &without_row : &ignored, why);
        }))
      return rc;
  }
  const auto t3 = std::chrono::steady_clock::now();
  if (R) {
    generation_result_sides(R, M[0]->p, M[0]->ev[0], M[0]->ev[1]);
    for (int m = 1; m < n; ++m) {   // the device times: the slowest member's
      mals_generation_result r;
      r.struct_size = R->struct_size;
      generation_result_sides(&r, M[(size_t)m]->p, M[(size_t)m]->ev[0], M[(size_t)m]->ev[1]);
      for (int sd = 0; sd < 2; ++sd) {
        R->join_ms[sd] = std::max(R->join_ms[sd], r.join_ms[sd]);
        R->scan_ms[sd] = std::max(R->scan_ms[sd], r.scan_ms[sd]);
        R->gather_ms[sd] = std::max(R->gather_ms[sd], r.gather_ms[sd]);
      }
    }
    R->n_known_dropped = known_dropped;
    R->n_tag_ids_without_row = without_row;
    R->sides_ms = generation_wall_ms(t0, t1);
    R->known_ms = generation_wall_ms(t1, t2);
    R->tags_ms = generation_wall_ms(t2, t3);
  }
  // every member is ready: nothing below fails
  for (int m = 0; m < n; ++m)
    if (int rc = generation_swap_prepare(hs[m], msg)) return rc;
  if (int rc = member_each(hs, n, none, msg, [&](int m, std::string&) -> int {
        generation_swap(hs[m], M[(size_t)m]->p);
        return MALS_OK;
      }))
    return rc;
  std::copy(plan.bounds.begin(), plan.bounds.end(), bounds_x_out);
  {
    const std::vector<int64_t> zeros((size_t)n_items + 1, 0);
    (void)plan_shards(zeros.data(), n_items, n, -1.0, k, bounds_y_out);
  }
  if (R) R->total_ms = generation_wall_ms(t0, std::chrono::steady_clock::now());
  return MALS_OK;
}

int generation_group_run(mals_handle* hs, int n, const mals_generation_load* loads, mals_generation_result* R, const int64_t* old_bounds,
                         int64_t* bounds_x_out, int64_t* bounds_y_out, std::string& msg) {
  std::vector<std::unique_ptr<GenGroupMember>> M;
  for (int m = 0; m < n; ++m) M.emplace_back(new GenGroupMember());
  int dev = 0;
  (void)hipGetDevice(&dev);
  const int rc = generation_group_body(hs, n, loads, R, old_bounds, bounds_x_out, bounds_y_out, M, msg);
  // nothing of the call in flight when it returns, and every member's temporaries go with its device current
  for (int m = 0; m < n; ++m) {
    if (hipSetDevice(hs[m]->cfg.device) != hipSuccess) continue;
    if (rc != MALS_OK) (void)hipStreamSynchronize(hs[m]->stream);
  }
  for (int m = 0; m < n; ++m) {
    (void)hipSetDevice(hs[m]->cfg.device);
    M[(size_t)m].reset();
  }
  (void)hipSetDevice(dev);
  return rc;
}
