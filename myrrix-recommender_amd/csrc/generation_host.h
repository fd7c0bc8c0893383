// generation_host.h -- host side of mals_load_generation, mals_mark_recent / mals_get_recent and the mals_generation_*
// calls (include/myrrix_als.h; kernels in generation_kernels.h).  Included by mals_serving.hip inside its anonymous namespace,
// after popular_host.h: the load runs as ONE exclusive ticket of the serving front (foldin_exclusive), so the passes formed
// before it read the old generation, the passes formed after it the new one, and the state below is only ever touched by
// the front's leader.
//
// ALL OR NOTHING.  generation_load_run builds everything aside -- the merged replicas, ids and maps, the copy of the new
// known items, the kept users' sets, the tag masks -- and only generation_swap, which cannot fail, touches the handle.
#pragma once

struct GenerationState {
  // recentlyActiveUsers / recentlyActiveItems (DelegateGenerationManager.java:179-186) as one bit per row, written inside
  // the tickets of the writes; grown on demand (nothing per model row until a row is written)
  std::vector<uint32_t> recent[2];
  // of the last load: the merged ids in row order, and live row -> merged row (-1: pruned)
  DeviceBuffer<int64_t> d_ids[2], d_map[2];
  int64_t n_ids[2] = {0, 0}, n_map[2] = {0, 0};
  bool loaded = false;
};

GenerationState* generation_state(mals_handle h) {
  if (!h->serving->gen) h->serving->gen = new GenerationState();
  return h->serving->gen;
}

void generation_free(mals_handle h) {
  delete h->serving->gen;
  h->serving->gen = nullptr;
}

// the rows of a side were replaced by rows that are not theirs (mals_set_factor_rows, mals_bind_factors): what was written
// to the old ones says nothing about the new
void generation_drop_recent(mals_handle h, int side) {
  if (h->serving->gen) std::vector<uint32_t>().swap(h->serving->gen->recent[side]);
}

// inside a ticket: doAppend's recentlyActiveUsers.add(userID) / recentlyActiveItems.add(itemID)
void generation_mark(mals_handle h, int side, int64_t row) {
  if (row < 0) return;
  std::vector<uint32_t>& b = generation_state(h)->recent[side];
  const size_t w = (size_t)(row >> 5);
  if (w >= b.size()) b.resize(std::max(w + 1, 2 * b.size()), 0u);
  b[w] |= 1u << (row & 31);
}

void generation_mark_pairs(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* item_row) {
  for (int64_t t = 0; t < n; ++t) {
    generation_mark(h, MALS_SIDE_X, user_row[t]);
    generation_mark(h, MALS_SIDE_Y, item_row[t]);
  }
}

bool generation_is_recent(const std::vector<uint32_t>& b, int64_t row) {
  const size_t w = (size_t)(row >> 5);
  return w < b.size() && ((b[w] >> (row & 31)) & 1u) != 0u;
}

// ---- the join on the host: the specification of the device's (mals_generation_join_host) -----------------------------
// the same table, hash and slot rule, filled one id after another
struct GenHostTable {
  std::vector<uint64_t> key;
  std::vector<int64_t> val;   // 0 = empty, j + 1
  uint64_t mask = 0;
  // false: ids[j] is already there
  bool insert(const int64_t* ids, int64_t j) {
    uint64_t s = gen_hash(ids[j]) & mask;
    while (val[(size_t)s] != 0) {
      if ((int64_t)key[(size_t)s] == ids[j]) return false;
      s = (s + 1) & mask;
    }
    key[(size_t)s] = (uint64_t)ids[j];
    val[(size_t)s] = j + 1;
    return true;
  }
  int64_t find(int64_t id) const {
    uint64_t s = gen_hash(id) & mask;
    while (val[(size_t)s] != 0) {
      if ((int64_t)key[(size_t)s] == id) return val[(size_t)s] - 1;
      s = (s + 1) & mask;
    }
    return -1;
  }
  bool build(const int64_t* ids, int64_t n) {
    const uint64_t slots = gen_table_slots(n);
    key.assign((size_t)slots, 0);
    val.assign((size_t)slots, 0);
    mask = slots - 1;
    for (int64_t j = 0; j < n; ++j)
      if (!insert(ids, j)) return false;
    return true;
  }
};

int generation_join_host(const int64_t* cur_ids, int64_t n_cur, const int64_t* new_ids, int64_t n_new, const int64_t* recent_rows, int64_t n_recent,
                         int32_t flags, int64_t* map_out, int64_t* counts_out) {
  if (n_cur < 0 || n_new < 0 || n_recent < 0 || (n_cur > 0 && (!cur_ids || !map_out)) || (n_new > 0 && !new_ids) || (n_recent > 0 && !recent_rows))
    return MALS_INVALID_ARG;
  GenHostTable tn, tc;
  if (!tn.build(new_ids, n_new) || !tc.build(cur_ids, n_cur)) return MALS_INVALID_ARG;   // a duplicate id
  std::vector<uint8_t> rec((size_t)n_cur, (flags & MALS_GENERATION_KEEP_NOT_UPDATED) ? 1 : 0);
  for (int64_t t = 0; t < n_recent; ++t) {
    if (recent_rows[t] < 0 || recent_rows[t] >= n_cur) return MALS_INVALID_ARG;
    rec[(size_t)recent_rows[t]] = 1;
  }
  int64_t updated = 0, kept = 0;
  for (int64_t r = 0; r < n_cur; ++r) {
    const int64_t j = tn.find(cur_ids[r]);
    if (j >= 0) {
      map_out[r] = j;
      ++updated;
    } else if (rec[(size_t)r]) {
      map_out[r] = n_new + kept++;
    } else {
      map_out[r] = -1;
    }
  }
  if (counts_out) {
    counts_out[0] = n_new + kept;
    counts_out[1] = updated;
    counts_out[2] = kept;
    counts_out[3] = n_cur - updated - kept;
  }
  return MALS_OK;
}

// ---- the load ---------------------------------------------------------------------------------------------------------
struct GenEvents {   // HIP events of one call
  std::vector<Event> ev;
  hipError_t record(hipStream_t st) {
    Event e;
    hipError_t rc = e.ensure();
    if (rc != hipSuccess) return rc;
    ev.push_back(std::move(e));
    return hipEventRecord(ev.back(), st);
  }
  double ms(size_t a, size_t b) const {
    float t = 0.f;
    return hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? (double)t : 0.0;
  }
};

// what one side's join, scan and gather leave aside
struct GenSide {
  DeviceBuffer<int64_t> up_cur, up_new;         // uploads of host id arrays
  const int64_t* d_cur = nullptr;
  const int64_t* d_new = nullptr;
  DeviceBuffer<unsigned long long> table;       // of the new ids (kept for the tag ids)
  uint64_t mask = 0;
  DeviceBuffer<int64_t> map, ids, kept_rows;
  DeviceBuffer<float> rows;                     // the merged replica
  int64_t n_cur = 0, n_new = 0, n_hit = 0, n_kept = 0;
  std::vector<int64_t> h_kept_rows, h_kept_ids;
  std::unordered_map<int64_t, int64_t> kept_row_of_id;   // id -> merged row, of the kept rows
  std::vector<uint32_t> recent_img;             // host image of the recent bits (outlives the asynchronous copy made from it)
  size_t e0 = 0;                                // first of this side's six events
  // between generation_side_begin and generation_side_end: the live ids' table, {duplicate row of new, of cur, hits, kept
  // rows} on the device and where its copy lands, the keep flags and their tile sums, the recent bits
  DeviceBuffer<unsigned long long> cur_table, flags;
  unsigned long long got[4] = {~0ull, ~0ull, 0ull, 0ull};
  DeviceBuffer<unsigned> keep, tile_sums;
  DeviceBuffer<uint32_t> d_recent;
  int64_t n_tiles = 0;
};

unsigned generation_grid(mals_handle h, int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((int64_t)h->n_cu * 8, (n + 255) / 256)); }

// One side in three steps, so that a group enqueues every member's step before it waits for any (generation_group_host.h); a
// handle runs them back to back (generation_side).  BEGIN: the uploads, JOIN, KEEP and the scan's sums, and the copy of the
// four counters to g.got -- nothing waited for.  `recent`: the recent bits of the side (a group keeps them on its first member).
int generation_side_begin(mals_handle h, int side, const mals_generation_load& L, const std::vector<uint32_t>& recent, GenEvents& ev, GenSide& g,
                          std::string& msg) {
  const bool keep_all = (L.flags & MALS_GENERATION_KEEP_NOT_UPDATED) != 0;
  g.n_cur = L.n_cur[side];
  g.n_new = L.n_new[side];
  // the ids on the device
  g.d_cur = L.cur_ids[side];
  if (L.cur_mem_kind == MALS_MEM_HOST && g.n_cur > 0) {
    FCHK(msg, g.up_cur.alloc((size_t)g.n_cur));
    FCHK(msg, hipMemcpyAsync(g.up_cur.get(), L.cur_ids[side], sizeof(int64_t) * (size_t)g.n_cur, hipMemcpyHostToDevice, h->stream));
    g.d_cur = g.up_cur.get();
  }
  g.d_new = L.new_ids[side];
  if (L.new_mem_kind == MALS_MEM_HOST && g.n_new > 0) {
    FCHK(msg, g.up_new.alloc((size_t)g.n_new));
    FCHK(msg, hipMemcpyAsync(g.up_new.get(), L.new_ids[side], sizeof(int64_t) * (size_t)g.n_new, hipMemcpyHostToDevice, h->stream));
    g.d_new = g.up_new.get();
  }
  // JOIN: the table of the new ids, the live ids' own table (it only finds their duplicates), the probe
  const uint64_t slots = gen_table_slots(g.n_new), cur_slots = gen_table_slots(g.n_cur);
  g.mask = slots - 1;
  DeviceBuffer<unsigned long long>& cur_table = g.cur_table;
  DeviceBuffer<unsigned long long>& flags = g.flags;
  DeviceBuffer<unsigned>& keep = g.keep;
  DeviceBuffer<unsigned>& tile_sums = g.tile_sums;
  DeviceBuffer<uint32_t>& d_recent = g.d_recent;
  const int64_t n_tiles = g.n_tiles = (g.n_cur + GEN_SCAN_TILE - 1) / GEN_SCAN_TILE;
  FCHK(msg, g.table.alloc((size_t)(2 * slots)));
  FCHK(msg, flags.alloc(4));
  FCHK(msg, g.map.alloc((size_t)std::max<int64_t>(g.n_cur, 1)));
  FCHK(msg, keep.alloc((size_t)std::max<int64_t>(g.n_cur, 1)));
  FCHK(msg, tile_sums.alloc((size_t)std::max<int64_t>(n_tiles, 1)));
  static const unsigned long long init[4] = {~0ull, ~0ull, 0ull, 0ull};
  FCHK(msg, hipMemcpyAsync(flags.get(), init, sizeof(init), hipMemcpyHostToDevice, h->stream));
  std::vector<uint32_t>& recent_img = g.recent_img;
  const size_t rwords = (size_t)((g.n_cur + 31) / 32);
  if (!keep_all && g.n_cur > 0 && !recent.empty()) {
    recent_img.assign(rwords, 0u);
    std::copy(recent.begin(), recent.begin() + std::min(rwords, recent.size()), recent_img.begin());
    FCHK(msg, d_recent.alloc(rwords));
    FCHK(msg, hipMemcpyAsync(d_recent.get(), recent_img.data(), sizeof(uint32_t) * rwords, hipMemcpyHostToDevice, h->stream));
  }
  g.e0 = ev.ev.size();
  FCHK(msg, ev.record(h->stream));   // e0: join begins
  FCHK(msg, hipMemsetAsync(g.table.get(), 0, sizeof(unsigned long long) * (size_t)(2 * slots), h->stream));
  if (g.n_new > 0) {
    hipLaunchKernelGGL(gen_insert_kernel, dim3(generation_grid(h, g.n_new)), dim3(256), 0, h->stream, g.d_new, g.n_new, g.table.get(), g.mask, flags.get());
    hipLaunchKernelGGL(gen_fill_keys_kernel, dim3(generation_grid(h, (int64_t)slots)), dim3(256), 0, h->stream, g.d_new, g.table.get(), slots);
  }
  if (g.n_cur > 0) {
    FCHK(msg, cur_table.alloc((size_t)(2 * cur_slots)));
    FCHK(msg, hipMemsetAsync(cur_table.get(), 0, sizeof(unsigned long long) * (size_t)(2 * cur_slots), h->stream));
    hipLaunchKernelGGL(gen_insert_kernel, dim3(generation_grid(h, g.n_cur)), dim3(256), 0, h->stream, g.d_cur, g.n_cur, cur_table.get(), cur_slots - 1,
                       flags.get() + 1);
    hipLaunchKernelGGL(gen_probe_kernel, dim3(generation_grid(h, g.n_cur)), dim3(256), 0, h->stream, g.d_cur, g.n_cur, g.table.get(), g.mask,
                       (const uint32_t*)d_recent.get(), keep_all ? 1 : 0, g.map.get(), keep.get(), flags.get() + 2);
  }
  FCHK(msg, hipGetLastError());
  FCHK(msg, ev.record(h->stream));   // e0 + 1: join ends, scan begins
  if (g.n_cur > 0) {
    hipLaunchKernelGGL(gen_scan_reduce_kernel, dim3((unsigned)n_tiles), dim3(256), 0, h->stream, keep.get(), g.n_cur, tile_sums.get());
    hipLaunchKernelGGL(gen_scan_sums_kernel, dim3(1), dim3(256), 0, h->stream, tile_sums.get(), n_tiles, flags.get() + 3);
    FCHK(msg, hipGetLastError());
  }
  FCHK(msg, ev.record(h->stream));   // e0 + 2: the scan's sums are enqueued
  // the kept rows size everything behind the scan: one wait per side (the wait and the allocations are in no phase's time)
  FCHK(msg, hipMemcpyAsync(g.got, flags.get(), sizeof(g.got), hipMemcpyDeviceToHost, h->stream));
  return MALS_OK;
}

// MID, once the stream has been waited for: the duplicates' verdict, then MAP and GATHER and the copy of the kept rows and
// their ids to the host -- nothing waited for
int generation_side_mid(mals_handle h, int side, const mals_generation_load& L, GenEvents& ev, GenSide& g, std::string& msg) {
  SideState& s = h->side[side];
  const int k = h->cfg.features;
  const unsigned long long* got = g.got;
  const int64_t n_tiles = g.n_tiles;
  DeviceBuffer<unsigned>& keep = g.keep;
  DeviceBuffer<unsigned>& tile_sums = g.tile_sums;
  g.cur_table.reset();
  if (got[0] != ~0ull || got[1] != ~0ull) {
    const bool in_new = got[0] != ~0ull;
    msg = std::string("side ") + (side == MALS_SIDE_X ? "X" : "Y") + ": " + (in_new ? "new_ids" : "cur_ids") + " holds an id twice (row " +
          std::to_string((long long)(in_new ? got[0] : got[1])) + " repeats an earlier one)";
    return MALS_INVALID_ARG;
  }
  g.n_hit = (int64_t)got[2];
  g.n_kept = (int64_t)got[3];
  const int64_t n_merged = g.n_new + g.n_kept;
  if (n_merged <= 0) {
    msg = std::string("side ") + (side == MALS_SIDE_X ? "X" : "Y") + ": the merged model has no rows";
    return MALS_INVALID_ARG;
  }
  FCHK(msg, g.ids.alloc((size_t)n_merged));
  FCHK(msg, g.kept_rows.alloc((size_t)std::max<int64_t>(g.n_kept, 1)));
  // growth capacity: a replica the library owns grows in place until it is full (mals_grow_factor_rows)
  const int64_t cap_rows = n_merged + std::max<int64_t>(n_merged / 16, 1024);
  FCHK(msg, g.rows.alloc((size_t)cap_rows * (size_t)k));
  FCHK(msg, ev.record(h->stream));   // e0 + 3: the map begins
  if (g.n_cur > 0) {
    hipLaunchKernelGGL(gen_map_kernel, dim3((unsigned)n_tiles), dim3(256), 0, h->stream, keep.get(), g.n_cur, tile_sums.get(), g.d_cur, g.n_new,
                       g.map.get(), g.kept_rows.get(), g.ids.get() + g.n_new);
    FCHK(msg, hipGetLastError());
  }
  if (g.n_new > 0)
    FCHK(msg, hipMemcpyAsync(g.ids.get(), g.d_new, sizeof(int64_t) * (size_t)g.n_new, hipMemcpyDeviceToDevice, h->stream));
  FCHK(msg, ev.record(h->stream));   // e0 + 4: the map ends, gather begins
  // GATHER: the new rows into the head, the kept live rows into the tail
  if (g.n_new > 0) {
    const int64_t n = g.n_new * k;
    if (L.new_mem_kind == MALS_MEM_HOST) {
      FCHK(msg, hipMemcpyAsync(g.rows.get(), L.new_rows[side], sizeof(float) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    } else if ((reinterpret_cast<uintptr_t>(L.new_rows[side]) & 15) == 0) {   // (g.rows is a hipMalloc block: aligned)
      hipLaunchKernelGGL(gen_copy_rows_kernel<true>, dim3(generation_grid(h, n / 4 + 1)), dim3(256), 0, h->stream, L.new_rows[side], g.rows.get(), n);
    } else {
      hipLaunchKernelGGL(gen_copy_rows_kernel<false>, dim3(generation_grid(h, n)), dim3(256), 0, h->stream, L.new_rows[side], g.rows.get(), n);
    }
  }
  if (g.n_kept > 0)
    hipLaunchKernelGGL(gen_gather_rows_kernel, dim3(generation_grid(h, g.n_kept * k)), dim3(256), 0, h->stream, (const float*)s.F,
                       (const int64_t*)g.kept_rows.get(), g.n_kept, k, g.rows.get() + (size_t)g.n_new * k);
  FCHK(msg, hipGetLastError());
  FCHK(msg, ev.record(h->stream));   // e0 + 5: gather ends
  // the kept rows and their ids on the host: the known items and the tag ids need them (bounded by the writes between loads)
  g.h_kept_rows.resize((size_t)g.n_kept);
  g.h_kept_ids.resize((size_t)g.n_kept);
  if (g.n_kept > 0) {
    FCHK(msg, hipMemcpyAsync(g.h_kept_rows.data(), g.kept_rows.get(), sizeof(int64_t) * (size_t)g.n_kept, hipMemcpyDeviceToHost, h->stream));
    FCHK(msg, hipMemcpyAsync(g.h_kept_ids.data(), g.ids.get() + g.n_new, sizeof(int64_t) * (size_t)g.n_kept, hipMemcpyDeviceToHost, h->stream));
  }
  return MALS_OK;
}

// END, once the stream has been waited for again: the join's temporaries go, the kept ids are indexed
void generation_side_end(GenSide& g) {
  g.flags.reset();
  g.keep.reset();
  g.tile_sums.reset();
  g.d_recent.reset();
  for (int64_t i = 0; i < g.n_kept; ++i) g.kept_row_of_id[g.h_kept_ids[(size_t)i]] = g.n_new + i;
}

int generation_side(mals_handle h, int side, const mals_generation_load& L, GenEvents& ev, GenSide& g, std::string& msg) {
  if (int rc = generation_side_begin(h, side, L, generation_state(h)->recent[side], ev, g, msg)) return rc;
  FCHK(msg, hipStreamSynchronize(h->stream));
  if (int rc = generation_side_mid(h, side, L, ev, g, msg)) return rc;
  FCHK(msg, hipStreamSynchronize(h->stream));
  generation_side_end(g);
  return MALS_OK;
}

// out[i] = map[rows[i]] through the device (rows, out: host)
int generation_map_rows(mals_handle h, const GenSide& g, const std::vector<int64_t>& rows, std::vector<int64_t>& out, std::string& msg) {
  out.assign(rows.size(), -1);
  if (rows.empty()) return MALS_OK;
  DeviceBuffer<int64_t> d;   // rows | out
  FCHK(msg, d.alloc(2 * rows.size()));
  FCHK(msg, hipMemcpyAsync(d.get(), rows.data(), sizeof(int64_t) * rows.size(), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(gen_gather_i64_kernel, dim3(generation_grid(h, (int64_t)rows.size())), dim3(256), 0, h->stream, (const int64_t*)g.map.get(), g.n_cur,
                     (const int64_t*)d.get(), (int64_t)rows.size(), d.get() + rows.size());
  FCHK(msg, hipGetLastError());
  FCHK(msg, hipMemcpyAsync(out.data(), d.get() + rows.size(), sizeof(int64_t) * rows.size(), hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipStreamSynchronize(h->stream));
  return MALS_OK;
}

// the merged rows of n tag ids (the new model's arrays: host or device): the new table on the device, the kept rows on the
// host; ids without a merged row are counted
int generation_tag_rows(mals_handle h, const GenSide& g, const int64_t* ids, int64_t n, int mem_kind, std::vector<int64_t>& rows_out, int64_t* without_row,
                        std::string& msg) {
  rows_out.clear();
  if (n <= 0) return MALS_OK;
  DeviceBuffer<int64_t> d_in, d_out;
  std::vector<int64_t> h_ids((size_t)n), found((size_t)n);
  const int64_t* src = ids;
  if (mem_kind == MALS_MEM_HOST) {
    FCHK(msg, d_in.alloc((size_t)n));
    FCHK(msg, hipMemcpyAsync(d_in.get(), ids, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    src = d_in.get();
    std::copy(ids, ids + n, h_ids.begin());
  } else {
    FCHK(msg, hipMemcpyAsync(h_ids.data(), ids, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  }
  FCHK(msg, d_out.alloc((size_t)n));
  hipLaunchKernelGGL(gen_lookup_kernel, dim3(generation_grid(h, n)), dim3(256), 0, h->stream, src, n, (const unsigned long long*)g.table.get(), g.mask,
                     d_out.get());
  FCHK(msg, hipGetLastError());
  FCHK(msg, hipMemcpyAsync(found.data(), d_out.get(), sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipStreamSynchronize(h->stream));
  for (int64_t i = 0; i < n; ++i) {
    int64_t r = found[(size_t)i];
    if (r < 0) {
      auto it = g.kept_row_of_id.find(h_ids[(size_t)i]);
      if (it != g.kept_row_of_id.end()) r = it->second;
    }
    if (r < 0) ++*without_row;
    else rows_out.push_back(r);
  }
  return MALS_OK;
}

// The single handle's way to a kept user's set, and a group's for the few users with an overlay view: the whole current sets of
// the local user rows `rows` (foldin_known_full: base row + additions, or the replaced set), every item re-indexed through the
// item map gy.map, sorted.  Items without a merged row are dropped and counted (the reference keeps the bare id: only
// mostPopularItems could see it).
int generation_kept_sets(mals_handle h, const GenSide& gy, const std::vector<int64_t>& rows, std::vector<std::vector<int32_t>>& out, int64_t* dropped,
                         std::string& msg) {
  std::vector<std::vector<int32_t>> sets;
  if (int rc = foldin_known_full(h, rows, sets, msg)) return rc;   // base row + overlay, sorted, distinct
  std::vector<int64_t> flat, mapped;
  for (const auto& v : sets) flat.insert(flat.end(), v.begin(), v.end());
  if (int rc = generation_map_rows(h, gy, flat, mapped, msg)) return rc;
  out.assign(sets.size(), {});
  size_t at = 0;
  for (size_t i = 0; i < sets.size(); ++i) {
    for (size_t j = 0; j < sets[i].size(); ++j, ++at) {
      if (mapped[at] >= 0) out[i].push_back((int32_t)mapped[at]);
      else ++*dropped;
    }
    std::sort(out[i].begin(), out[i].end());
  }
  return MALS_OK;
}

// everything generation_swap installs
struct GenPrepared {
  GenSide side[2];
  bool install_known = false;
  DeviceBuffer<int64_t> known_ptr;
  DeviceBuffer<int32_t> known_idx;
  std::unordered_map<int64_t, std::vector<int32_t>> kept_sets;       // merged user row -> its known items as merged item rows
                                                                     // (KnownOverlay::Sets, foldin_plan.h: swapped in whole)
  std::vector<int64_t> tag_users;                                    // merged user rows: ascending, unique
  DeviceBuffer<uint32_t> tag_bits;
  int64_t n_tag_items = 0;
  std::vector<uint32_t> tag_recent_img;   // host image of the recent item bits (outlives the asynchronous copy made from it)
  // a member of a group (generation_group_host.h): it owns the merged users own_lo <= u < own_hi; known_ptr / known_idx are
  // its base CSR over exactly those users (new rows and kept rows alike), kept_sets and tag_users are keyed by u - own_lo
  bool member = false;
  int64_t own_lo = 0, own_hi = 0;
};

// Everything that can fail comes before the swap: the states the swap writes exist, the list of the requests the swap hands
// back has its room.  MALS_OOM, nothing changed.
int generation_swap_prepare(mals_handle h, std::string& msg) {
  try {
    (void)generation_state(h);
    (void)foldin_state(h);
    (void)popular_state(h);
    topn_generation_swap_reserve(h);
  } catch (const std::bad_alloc&) {
    msg = "out of host memory";
    return MALS_OOM;
  }
  return MALS_OK;
}

// After generation_swap_prepare.  Between topn_generation_swap_begin and the moment topn_generation_swap_end has made the
// sequence number even again nothing allocates: buffers and containers are moved or swapped whole, scalars assigned,
// memory released.  (What is left after that moment is topn_front_complete's wake list for 16 or more waiting callers.)
void generation_swap(mals_handle h, GenPrepared& p) {
  GenerationState& gs = *generation_state(h);
  topn_generation_swap_begin(h);   // the readers' argument checks wait, or are repeated (topn_generation_guard)
  for (int sd = 0; sd < 2; ++sd) {
    SideState& s = h->side[sd];
    GenSide& g = p.side[sd];
    free_matrix(s);   // the rows of R named live rows
    s.F_own = std::move(g.rows);
    s.F = s.F_own.get();
    s.n_total = g.n_new + g.n_kept;
    s.row_offset = 0;
    s.n_local = 0;
    s.nnz = 0;
    s.G_valid = false;
    ++s.F_epoch;
    gs.d_ids[sd] = std::move(g.ids);
    gs.d_map[sd] = std::move(g.map);
    gs.n_ids[sd] = s.n_total;
    gs.n_map[sd] = g.n_cur;
    ids_drop(h, sd);   // the rows are renumbered: the caller installs the merged ids (mals_generation_get_ids -> mals_ids_set)
    std::vector<uint32_t>().swap(gs.recent[sd]);   // recentlyActiveUsers.clear() / recentlyActiveItems.clear() (:97-98)
  }
  gs.loaded = true;
  malsi_clear_known_items(h);   // the live base and overlay (the kept users' sets were read from them before)
  popular_new_generation(h, true);
  SideState& x = h->side[MALS_SIDE_X];
  if (p.install_known) {
    h->known_ptr_copy = std::move(p.known_ptr);
    h->known_idx_copy = std::move(p.known_idx);
    h->known_ptr = h->known_ptr_copy.get();
    h->known_idx = h->known_idx_copy.get();
    h->known_rows = p.member ? p.own_hi - p.own_lo : p.side[MALS_SIDE_X].n_new;
    x.n_local = h->known_rows;
    if (p.member) {
      // the slice of the merged users this member owns; its kept users with an overlay view have an empty base row and a whole set
      x.row_offset = p.own_lo;
      if (!p.kept_sets.empty()) foldin_state(h)->known.install_all(p.kept_sets);
    } else if (p.side[MALS_SIDE_X].n_kept > 0) {
      // the kept users: rows past the base CSR with a whole set of their own, as grown users are after a removal
      foldin_state(h)->known.install_all(p.kept_sets);   // (malsi_clear_known_items left it empty)
      h->grown_users_end.store(x.n_total, std::memory_order_release);
    }
  }
  if (!p.tag_users.empty()) popular_state(h)->tag_users.swap(p.tag_users);
  h->tag_bits = std::move(p.tag_bits);
  h->tag_bits_items = h->tag_bits.get() ? h->side[MALS_SIDE_Y].n_total : 0;
  h->n_tag_items = p.n_tag_items;
  h->lsh.clear();   // the signatures were a snapshot of the live Y: the caller builds the filter again (mals_lsh_build)
  popular_touch(h, true);
  topn_generation_swap_end(h);
}

// what a handle's known items are made of before a load
bool generation_holds_known(mals_handle h) { return h->side[MALS_SIDE_X].has_matrix || h->known_ptr || foldin_has_overlay(h); }

// the checks that need no device work.  via_group: a member of a group holds a shard (row_offset != 0 is its normal state) and
// the group decides whether the new model's known items are needed (any member may hold some)
int generation_load_check(mals_handle h, const mals_generation_load& L, bool via_group, std::string& msg) {
  const int k = h->cfg.features;
  SideState& x = h->side[MALS_SIDE_X];
  if (L.features != k) {
    msg = "the new model has " + std::to_string(L.features) + " features, the handle " + std::to_string(k);
    return MALS_INVALID_ARG;
  }
  for (int sd = 0; sd < 2; ++sd) {
    const SideState& s = h->side[sd];
    if (L.n_cur[sd] != (s.F ? s.n_total : 0)) {
      msg = "cur_ids: one id per live row of the replica (" + std::to_string((long long)(s.F ? s.n_total : 0)) + " rows, " +
            std::to_string((long long)L.n_cur[sd]) + " ids)";
      return MALS_INVALID_ARG;
    }
    if (s.row_offset != 0 && !via_group) {
      msg = "the handle holds a shard of a larger model (row_offset != 0)";
      return MALS_INVALID_ARG;
    }
  }
  if (!via_group && generation_holds_known(h) && !L.new_known_ptr) {
    msg = "the handle holds known items: the new model's are needed (new_known_ptr)";
    return MALS_INVALID_ARG;
  }
  if (h->known_ptr && h->known_rows != x.n_local) {
    msg = "the installed known items do not match the local user rows";
    return MALS_INVALID_ARG;
  }
  return MALS_OK;
}

// TAG SETS: updated ids, plus the live tags that are recent (updateTagIDs :108-115, removeNotUpdated :88-95).
// itemTagIDs: user-side ids -> the tag users of mals_most_popular_items as merged user rows (ascending, unique).  live: the
// live tag users as GLOBAL live rows; recent_x: the recent bits of side X
int generation_tag_users(mals_handle h, const GenSide& gx, const mals_generation_load& L, const std::vector<uint32_t>& recent_x,
                         const std::vector<int64_t>& live_all, std::vector<int64_t>& tag_users, int64_t* without_row, std::string& msg) {
  const bool keep_all = (L.flags & MALS_GENERATION_KEEP_NOT_UPDATED) != 0;
  std::vector<int64_t> live, live_mapped;
  for (int64_t r : live_all)
    if (keep_all || generation_is_recent(recent_x, r)) live.push_back(r);
  if (int rc = generation_map_rows(h, gx, live, live_mapped, msg)) return rc;
  if (int rc = generation_tag_rows(h, gx, L.item_tag_ids, L.n_item_tag_ids, L.new_mem_kind, tag_users, without_row, msg)) return rc;
  for (int64_t m : live_mapped)
    if (m >= 0) tag_users.push_back(m);
  std::sort(tag_users.begin(), tag_users.end());
  tag_users.erase(std::unique(tag_users.begin(), tag_users.end()), tag_users.end());
  return MALS_OK;
}

// userTagIDs: item-side ids -> one bit per merged item (p.tag_bits, p.n_tag_items); recent_y: the recent bits of side Y
int generation_tag_items(mals_handle h, const GenSide& gy, const mals_generation_load& L, const std::vector<uint32_t>& recent_y, GenPrepared& p,
                         int64_t* without_row, std::string& msg) {
  const bool keep_all = (L.flags & MALS_GENERATION_KEEP_NOT_UPDATED) != 0;
  std::vector<int64_t> tag_items;
  if (int rc = generation_tag_rows(h, gy, L.user_tag_ids, L.n_user_tag_ids, L.new_mem_kind, tag_items, without_row, msg)) return rc;
  if (h->tag_bits.get() || !tag_items.empty()) {
    const int64_t n_items = gy.n_new + gy.n_kept;
    const size_t words = ((size_t)((n_items + 31) / 32) + 1) & ~(size_t)1;   // (the layout of mals_set_tag_items)
    const size_t tail = sizeof(unsigned long long) / sizeof(uint32_t);
    FCHK(msg, p.tag_bits.alloc(words + tail));
    unsigned long long* d_n = reinterpret_cast<unsigned long long*>(p.tag_bits.get() + words);
    FCHK(msg, hipMemsetAsync(p.tag_bits.get(), 0, sizeof(uint32_t) * (words + tail), h->stream));
    DeviceBuffer<uint32_t> d_recent;
    DeviceBuffer<int64_t> d_rows;
    std::vector<uint32_t>& recent_img = p.tag_recent_img;
    if (h->tag_bits.get() && h->tag_bits_items == gy.n_cur && gy.n_cur > 0) {
      const size_t rwords = (size_t)((gy.n_cur + 31) / 32);
      const std::vector<uint32_t>& recent = recent_y;
      if (!keep_all && !recent.empty()) {
        recent_img.assign(rwords, 0u);
        std::copy(recent.begin(), recent.begin() + std::min(rwords, recent.size()), recent_img.begin());
        FCHK(msg, d_recent.alloc(rwords));
        FCHK(msg, hipMemcpyAsync(d_recent.get(), recent_img.data(), sizeof(uint32_t) * rwords, hipMemcpyHostToDevice, h->stream));
      }
      if (keep_all || d_recent.get())
        hipLaunchKernelGGL(gen_tag_remap_kernel, dim3(generation_grid(h, gy.n_cur)), dim3(256), 0, h->stream, (const uint32_t*)h->tag_bits.get(), gy.n_cur,
                           (const uint32_t*)d_recent.get(), keep_all ? 1 : 0, (const int64_t*)gy.map.get(), n_items, p.tag_bits.get(), d_n);
    }
    if (!tag_items.empty()) {
      FCHK(msg, d_rows.alloc(tag_items.size()));
      FCHK(msg, hipMemcpyAsync(d_rows.get(), tag_items.data(), sizeof(int64_t) * tag_items.size(), hipMemcpyHostToDevice, h->stream));
      hipLaunchKernelGGL(topn_tag_bits_kernel, dim3((unsigned)((tag_items.size() + 255) / 256)), dim3(256), 0, h->stream, (const int64_t*)d_rows.get(),
                         (int64_t)tag_items.size(), n_items, p.tag_bits.get(), d_n);
    }
    FCHK(msg, hipGetLastError());
    unsigned long long n_set = 0;
    FCHK(msg, hipMemcpyAsync(&n_set, d_n, sizeof(n_set), hipMemcpyDeviceToHost, h->stream));
    FCHK(msg, hipStreamSynchronize(h->stream));
    p.n_tag_items = (int64_t)n_set;
    if (n_set == 0) p.tag_bits.reset();   // (as mals_set_tag_items: nothing to strike)
  }
  return MALS_OK;
}

double generation_wall_ms(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

// the counts and the device times of one handle's two sides (ev: the events of side sd; a handle's two sides share one list)
void generation_result_sides(mals_generation_result* R, const GenPrepared& p, const GenEvents& ev_x, const GenEvents& ev_y) {
  const int32_t size = R->struct_size;
  std::memset(R, 0, sizeof(*R));
  R->struct_size = size;
  for (int sd = 0; sd < 2; ++sd) {
    const GenSide& g = p.side[sd];
    const GenEvents& ev = sd == MALS_SIDE_X ? ev_x : ev_y;
    R->n_merged[sd] = g.n_new + g.n_kept;
    R->n_updated[sd] = g.n_hit;
    R->n_kept[sd] = g.n_kept;
    R->n_pruned[sd] = g.n_cur - g.n_hit - g.n_kept;
    R->join_ms[sd] = ev.ms(g.e0, g.e0 + 1);
    R->scan_ms[sd] = ev.ms(g.e0 + 1, g.e0 + 2) + ev.ms(g.e0 + 3, g.e0 + 4);
    R->gather_ms[sd] = ev.ms(g.e0 + 4, g.e0 + 5);
  }
}

// PREPARE (everything aside), then generation_swap_prepare, then generation_swap: a handle runs the three here; a group runs
// the same three for every member (generation_group_host.h) and swaps only when every member is ready.
int generation_load_body(mals_handle h, const mals_generation_load& L, mals_generation_result* R, GenPrepared& p, std::string& msg) {
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = generation_load_check(h, L, false, msg)) return rc;
  const bool holds_known = generation_holds_known(h);
  GenEvents ev;
  for (int sd = 0; sd < 2; ++sd)
    if (int rc = generation_side(h, sd, L, ev, p.side[sd], msg)) return rc;
  GenSide& gx = p.side[MALS_SIDE_X];
  GenSide& gy = p.side[MALS_SIDE_Y];
  const auto t1 = std::chrono::steady_clock::now();

  // KNOWN ITEMS: the new base (a copy: the handle owns its generation), and the kept users' effective live sets
  int64_t known_dropped = 0;
  if (L.new_known_ptr) {
    p.install_known = true;
    int64_t nnz = 0;
    FCHK(msg, p.known_ptr.alloc((size_t)(gx.n_new + 1)));
    const hipMemcpyKind kind = L.new_mem_kind == MALS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (gx.n_new > 0) {
      if (L.new_mem_kind == MALS_MEM_HOST) nnz = L.new_known_ptr[gx.n_new];
      else FCHK(msg, hipMemcpy(&nnz, L.new_known_ptr + gx.n_new, sizeof(int64_t), hipMemcpyDeviceToHost));
      FCHK(msg, hipMemcpyAsync(p.known_ptr.get(), L.new_known_ptr, sizeof(int64_t) * (size_t)(gx.n_new + 1), kind, h->stream));
    } else {
      FCHK(msg, hipMemsetAsync(p.known_ptr.get(), 0, sizeof(int64_t), h->stream));
    }
    if (nnz < 0 || (nnz > 0 && !L.new_known_idx)) {
      msg = "bad known-item arrays of the new model";
      return MALS_INVALID_ARG;
    }
    FCHK(msg, p.known_idx.alloc((size_t)std::max<int64_t>(nnz, 1)));
    if (nnz > 0) FCHK(msg, hipMemcpyAsync(p.known_idx.get(), L.new_known_idx, sizeof(int32_t) * (size_t)nnz, kind, h->stream));
    if (gx.n_kept > 0 && holds_known) {
      std::vector<std::vector<int32_t>> sets;
      if (int rc = generation_kept_sets(h, gy, gx.h_kept_rows, sets, &known_dropped, msg)) return rc;
      for (size_t i = 0; i < sets.size(); ++i)
        if (!sets[i].empty()) p.kept_sets[gx.n_new + (int64_t)i] = std::move(sets[i]);
    }
    FCHK(msg, hipStreamSynchronize(h->stream));
  }
  const auto t2 = std::chrono::steady_clock::now();

  int64_t without_row = 0;
  {
    const GenerationState& gs = *generation_state(h);
    static const std::vector<int64_t> none;
    if (int rc = generation_tag_users(h, gx, L, gs.recent[MALS_SIDE_X], h->serving->pop ? popular_state(h)->tag_users : none, p.tag_users, &without_row, msg))
      return rc;
    if (int rc = generation_tag_items(h, gy, L, gs.recent[MALS_SIDE_Y], p, &without_row, msg)) return rc;
  }
  FCHK(msg, hipStreamSynchronize(h->stream));
  const auto t3 = std::chrono::steady_clock::now();
  if (R) {
    generation_result_sides(R, p, ev, ev);
    R->n_known_dropped = known_dropped;
    R->n_tag_ids_without_row = without_row;
    R->sides_ms = generation_wall_ms(t0, t1);
    R->known_ms = generation_wall_ms(t1, t2);
    R->tags_ms = generation_wall_ms(t2, t3);
  }
  if (int rc = generation_swap_prepare(h, msg)) return rc;
  generation_swap(h, p);
  if (R) R->total_ms = generation_wall_ms(t0, std::chrono::steady_clock::now());
  return MALS_OK;
}

int generation_load_run(mals_handle h, const mals_generation_load& L, mals_generation_result* R, std::string& msg) {
  GenPrepared p;   // (a failure: nothing of it may still be in flight when it goes)
  const int rc = generation_load_body(h, L, R, p, msg);
  if (rc != MALS_OK) (void)hipStreamSynchronize(h->stream);
  return rc;
}

// the ids / the map of the last load, to the host
int generation_get(mals_handle h, int side, bool ids, int64_t* out, std::string& msg) {
  GenerationState* gs = h->serving->gen;
  if (!gs || !gs->loaded) {
    msg = "no generation was loaded into this handle (mals_load_generation)";
    return MALS_INVALID_ARG;
  }
  const int64_t n = ids ? gs->n_ids[side] : gs->n_map[side];
  const int64_t* src = ids ? gs->d_ids[side].get() : gs->d_map[side].get();
  if (n > 0) {
    FCHK(msg, hipMemcpyAsync(out, src, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    FCHK(msg, hipStreamSynchronize(h->stream));
  }
  return MALS_OK;
}
