// ingest_big_host.h -- mals_ingest_finish for more records than ONE sort pipeline holds (host code of ingest_api.hip).
// Expects before it: ingest_host.h (the ingest object, Scratch, finish_range, finish_tags) and ingest_big_kernels.h.
//
// The one-shot pipeline sorts all records at once: 32-bit positions, 52 bytes of workspace per record -- 2^31
// records at most, and 5e9 records (C5: InputFilesReader.readInputFiles, IFR:64-211, is the one entry point of every
// configuration) would need 260 GB beside 120 GB of records.  Here the same result is assembled from pieces that each fit:
//
//   1. the records are cut into P <= 250 ranges of USER id (splitters from a sorted sample of 65536 user ids, exact sizes
//      counted, P raised until every range fits `part_cap` records); a byte per record says which range it belongs to;
//   2. range by range, in ascending id order: the range's records are compacted (stable: stream order kept) into a
//      partition buffer and go through the unchanged stages of the one-shot pipeline (finish_range) -- composite stable sort
//      by (user id, item id), per-pair replay (MU:64-125, FBIFM:129-138), removeSmall (IFR:200-211).  Users of different
//      ranges are different users, so the range's user table, row pointers and surviving entries are final up to their
//      offsets, which are the running totals.  Items are shared between ranges: a range keeps its own ascending item table,
//      its liveness flags and writes the entries' columns as LOCAL item ranks;
//   3. the ranges' item tables are merged into one ascending table (binary-search merges, no sort), liveness is OR-ed
//      through the rank maps, the dense item index is the scan of it, and every range's columns are renumbered in place;
//   4. R^T: entries per item counted with atomics (an item's count is bounded by the users: no overflow), offsets by a
//      64-bit scan, then item range by item range (<= part_cap entries each): the entries whose item lies in the range are
//      compacted in user order, their row found by a search between the tile's first and last row, sorted stably on the
//      item half of (item << 32 | user) and written behind the item range's offset.
// Positions inside a partition stay 32-bit; everything that counts across partitions is 64-bit.  The result -- ids, both
// CSRs, values, knownItemIDs, tag sets -- is bit-identical to the one-shot pipeline's (tests/test_gpu_ingest_big.py runs
// the oracle suites through this path with a partition capacity of a few hundred records).
#pragma once

namespace {

struct BigPart {  // what a user range leaves behind until the items are known
  int64_t n_records = 0, n_users = 0, nnz = 0, n_known = 0;
  int64_t u_base = 0, nnz_base = 0, known_base = 0;
  int64_t n_items_local = 0;
  DeviceBuffer<int64_t> item_ids;     // the range's ascending item table
  DeviceBuffer<unsigned> item_alive;  // ... and which of them own an entry here
  DeviceBuffer<int64_t> user_ids;     // live users, ascending
  DeviceBuffer<int64_t> ptr_local;    // [n_users + 1] offsets into the range's entries
  DeviceBuffer<int64_t> known_ptr_local;
};

struct BigState {
  int64_t part_cap = 0;                   // records a user range (entries an item range) holds at most
  int64_t n_sample = 0;                   // user ids the splitters are picked from
  IdWidth width = {false, false};
  std::vector<unsigned long long> hist;   // records per user range
  std::vector<BigPart> parts;
  int64_t n_users = 0, n_items = 0, nnz = 0, n_known = 0;   // the totals, as the phases settle them
  DeviceBuffer<uint8_t> part;
  DeviceBuffer<int64_t> pu, pi;
  DeviceBuffer<float> pv;
  DeviceBuffer<int64_t> d_split;
  DeviceBuffer<int64_t> item_glob;   // merged ascending item table
  int64_t n_item_glob = 0;
  DeviceBuffer<unsigned> alive_glob, new_i, cnt;
  DeviceBuffer<unsigned long long> sums64;
  DeviceBuffer<int32_t> tile_row;
  int64_t sort_cap() const { return std::max<int64_t>(part_cap, n_sample); }   // what the arena's sort buffers hold
};

Grid big_tiles(int64_t n) { return {(unsigned)std::max<int64_t>(1, (n + BIG_TILE - 1) / BIG_TILE)}; }

// a = a U b for ascending tables (b's duplicates of a dropped); a is reallocated
int big_merge_tables(mals_ingest g, Scratch& s, DeviceBuffer<int64_t>& a, int64_t& na, const int64_t* b, int64_t nb) {
  if (nb == 0) return MALS_OK;
  if (na == 0) {
    ICHK(g, a.alloc((size_t)nb));
    ICHK(g, hipMemcpyAsync(a.get(), b, sizeof(int64_t) * (size_t)nb, hipMemcpyDeviceToDevice, g->stream));
    na = nb;
    return MALS_OK;
  }
  ITRY(launch(g, nb, big_fresh_kernel, b, nb, a.get(), na, s.head));
  unsigned n_fresh = 0;
  ITRY(scan_u32(g, s, s.head, s.scan, nb, &n_fresh));
  if (n_fresh == 0) return MALS_OK;
  DeviceBuffer<int64_t> fresh, merged;
  ICHK(g, fresh.alloc(n_fresh));
  if (merged.alloc((size_t)(na + n_fresh)) != hipSuccess) return fail(g, MALS_OOM, "item table merge: out of device memory");
  int rc = launch(g, nb, big_compact_fresh_kernel, b, nb, s.head, s.scan, fresh.get());
  if (!rc) rc = launch(g, na, big_merge_place_kernel, a.get(), na, fresh.get(), (int64_t)n_fresh, merged.get());
  if (!rc) rc = launch(g, n_fresh, big_merge_place_kernel, fresh.get(), (int64_t)n_fresh, a.get(), na, merged.get());
  const hipError_t e2 = hipStreamSynchronize(g->stream);   // (also after a failed launch: the tables below are in use until then)
  fresh.reset();
  a = std::move(merged);
  na += n_fresh;
  ITRY(rc);
  ICHK(g, e2);
  g->bytes_moved += 24.0 * (double)nb + 16.0 * (double)na;
  return MALS_OK;
}

// splitters for `n_parts` ranges from the sorted sample (host): strictly ascending, at most n_parts - 1
std::vector<int64_t> big_pick_splitters(const std::vector<int64_t>& sample, int n_parts) {
  std::vector<int64_t> sp;
  const size_t S = sample.size();
  for (int j = 1; j < n_parts; ++j) {
    const int64_t c = sample[std::min(S - 1, (size_t)((unsigned long long)j * S / (unsigned)n_parts))];
    if (sp.empty() || c > sp.back()) sp.push_back(c);
  }
  return sp;
}

// The buffers of the whole finish, before the pipeline starts.  part_cap = 0: as many records per range as the device's
// free memory holds (fewer ranges = fewer sweeps over the records).
int big_reserve(mals_ingest g, Scratch& s, BigState& B, int64_t part_cap) {
  const int64_t n = g->n;
  const auto t_ws = std::chrono::steady_clock::now();
  // results that are filled range by range: R by user with room for every record (entries <= records), knownItemIDs likewise
  ICHK(g, B.part.alloc((size_t)n + 8));
  ICHK(g, B.d_split.alloc(256));
  ICHK(g, g->col[0].alloc((size_t)n));
  ICHK(g, g->val[0].alloc((size_t)n));
  if (g->want_known) ICHK(g, g->known_idx.alloc((size_t)n));
  // ... and R by item likewise, now: a 20 GB allocation in the middle of the pipeline is a second of host time on some boxes
  ICHK(g, g->col[1].alloc((size_t)n));
  ICHK(g, g->val[1].alloc((size_t)n));
  if (part_cap <= 0) {
    // A range costs 76 bytes per record (24 in the partition buffer, 52 of sort workspace).  Of what is free now -- plus the
    // arena an earlier finish left, which is reused -- 70 % go to it: the id tables, the ranges' item tables and the row
    // bounds of R^T (8-16 bytes per user / item) come out of the rest.
    size_t free_b = 0, total_b = 0;
    ICHK(g, hipMemGetInfo(&free_b, &total_b));
    size_t arena = 0;
    for (int b = 0; b < mals_ingest_s::N_WS; ++b) arena += g->ws[b].capacity();
    const double budget = 0.7 * ((double)free_b + (double)arena);
    part_cap = (int64_t)std::min<double>((double)MALS_INGEST_ONE_SHOT_MAX, std::max<double>((double)MALS_INGEST_MIN_PART, budget / 76.0));
    // (no point in a range larger than the whole input spread over two ranges)
    part_cap = std::min<int64_t>(part_cap, std::max<int64_t>(MALS_INGEST_MIN_PART, n / 2 + n / 8));
  }
  B.part_cap = part_cap;
  B.n_sample = std::min<int64_t>(n, 65536);
  // the workspace of one partition; the scans over all records run on tiles of 2048 (one count per tile) and the dense item
  // index is a scan over at most 2^31 items: both inside the same tile-sum buffer
  ITRY(setup_workspace(g, s, B.sort_cap(), std::max<int64_t>((n + BIG_TILE - 1) / BIG_TILE, (int64_t)1 << 31)));
  ICHK(g, B.pu.alloc((size_t)part_cap));
  ICHK(g, B.pi.alloc((size_t)part_cap));
  ICHK(g, B.pv.alloc((size_t)part_cap));
  g->last_workspace_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_ws).count();
  return MALS_OK;
}

// ---- 0. ranges of user id: B.part says which range a record belongs to, B.hist how many records each holds --------------
int big_plan_user_ranges(mals_ingest g, Scratch& s, BigState& B) {
  const int64_t n = g->n, n_sample = B.n_sample, part_cap = B.part_cap;
  ITRY(launch(g, n_sample, big_sample_kernel, g->d_user.get(), n, n_sample, s.keys[0], s.pay[0]));
  int rs = 0;
  ITRY((radix_sort<uint64_t, unsigned>(g, s, s.keys, s.pay, n_sample, &rs)));
  std::vector<int64_t> sample((size_t)n_sample);
  {
    std::vector<uint64_t> sk((size_t)n_sample);
    ICHK(g, hipMemcpy(sk.data(), s.keys[rs], sizeof(uint64_t) * (size_t)n_sample, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < sk.size(); ++i) sample[i] = key_to_id(sk[i]);
  }
  int n_parts = (int)std::min<int64_t>(250, std::max<int64_t>(2, (n + (part_cap * 3) / 4 - 1) / ((part_cap * 3) / 4)));
  B.hist.assign(256, 0);
  std::vector<int64_t> splitters;
  for (int attempt = 0;; ++attempt) {
    splitters = big_pick_splitters(sample, n_parts);
    ICHK(g, hipMemcpyAsync(B.d_split.get(), splitters.data(), sizeof(int64_t) * splitters.size(), hipMemcpyHostToDevice, g->stream));
    ITRY(launch_grid(g, {blocks_for(n, 256, 1 << 16)}, big_assign_part_kernel, g->d_user.get(), n, B.d_split.get(), (int)splitters.size(), B.part.get()));
    ICHK(g, hipMemsetAsync(s.digit_tot, 0, 256 * sizeof(unsigned long long), g->stream));
    ITRY(launch_grid(g, {blocks_for(n, 256, 1 << 14)}, big_part_histogram_kernel, B.part.get(), n, s.digit_tot));
    ICHK(g, hipMemcpyAsync(B.hist.data(), s.digit_tot, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost, g->stream));
    ICHK(g, hipStreamSynchronize(g->stream));
    g->bytes_moved += 10.0 * (double)n;
    unsigned long long worst = 0;
    for (unsigned long long c : B.hist) worst = std::max(worst, c);
    if ((int64_t)worst <= part_cap) break;
    if (n_parts >= 250 || attempt >= 8)
      return fail(g, MALS_INVALID_ARG, "ingest: the records of one user-id range do not fit a partition (" + std::to_string(worst) + " records, capacity " +
                                           std::to_string(part_cap) + "): one user id owns too many lines, or MALS_INGEST_OPT_PARTITION_RECORDS is too small");
    n_parts = std::min(250, n_parts + std::max(1, n_parts / 2));
  }
  g->last_partitions = (int)splitters.size() + 1;
  B.parts.resize((size_t)g->last_partitions);
  return MALS_OK;
}

// ---- 1. range by range: R's rows of the range's users behind those of the ranges before it, columns as local item ranks ---
int big_finish_user_ranges(mals_ingest g, Scratch& s, BigState& B) {
  const int64_t n = g->n;
  const Grid n_tiles = big_tiles(n);
  for (size_t p = 0; p < B.parts.size(); ++p) {
    BigPart& bp = B.parts[p];
    bp.u_base = B.n_users;   // the running totals: the range's users, entries and known items land behind them
    bp.nnz_base = B.nnz;
    bp.known_base = B.n_known;
    const int64_t np = (int64_t)B.hist[p];
    bp.n_records = np;
    if (np == 0) continue;
    ITRY(launch_grid(g, n_tiles, big_count_part_kernel, B.part.get(), n, (uint8_t)p, s.head));
    unsigned counted = 0;
    ITRY(scan_u32(g, s, s.head, s.head, (int64_t)n_tiles.blocks, &counted));
    if ((int64_t)counted != np) return fail(g, MALS_HIP_ERROR, "ingest: partition size mismatch");
    ITRY(launch_grid(g, n_tiles, big_compact_part_kernel, B.part.get(), n, (uint8_t)p, s.head, g->d_user.get(), g->d_item.get(), g->d_value.get(), B.pu.get(),
                     B.pi.get(), B.pv.get()));
    g->bytes_moved += 2.0 * (double)n + 48.0 * (double)np;
    RangeTmp tp;   // the range's temporaries (freed at the end of the iteration)
    RangeCounts c;
    ITRY(finish_range(g, s, tp, Records{B.pu.get(), B.pi.get(), B.pv.get(), np}, B.width,
                      RangeOut{false, bp.user_ids, bp.ptr_local, bp.known_ptr_local, bp.nnz_base, bp.known_base}, c));
    bp.n_users = c.n_users;
    bp.nnz = c.nnz;
    bp.n_known = c.n_known;
    bp.n_items_local = c.n_i_all;
    bp.item_ids = std::move(tp.iid_all);     // kept: the range's item table and its liveness
    bp.item_alive = std::move(tp.alive_i);
    // the merged item table grows by what this range saw for the first time
    ITRY(big_merge_tables(g, s, B.item_glob, B.n_item_glob, bp.item_ids.get(), bp.n_items_local));
    ICHK(g, hipStreamSynchronize(g->stream));   // tp's allocations go away
    B.n_users += c.n_users;
    B.nnz += c.nnz;
    B.n_known += c.n_known;
    if (B.n_users > (int64_t)0x7fffff00 || B.n_item_glob > (int64_t)0x7fffff00)
      return fail(g, MALS_INVALID_ARG, "ingest: more than 2^31 distinct users or items (dense indices are 32-bit)");
  }
  B.pu.reset(); B.pi.reset(); B.pv.reset(); B.part.reset();
  return MALS_OK;
}

// ---- 2. items: liveness through the rank maps, dense index, renumbering; the ranges' user tables and offsets into place ---
int big_settle_items(mals_ingest g, Scratch& s, BigState& B) {
  const int64_t n_glob = B.n_item_glob, n_users = B.n_users;
  ICHK(g, B.alive_glob.alloc(std::max<size_t>((size_t)n_glob, 1)));
  ICHK(g, B.new_i.alloc(std::max<size_t>((size_t)n_glob, 1)));
  ICHK(g, hipMemsetAsync(B.alive_glob.get(), 0, sizeof(unsigned) * std::max<size_t>((size_t)n_glob, 1), g->stream));
  // (the maps live in the keys arena: a range's item table is no longer than the range)
  int64_t* map = reinterpret_cast<int64_t*>(s.keys[0]);
  int32_t* final_map = reinterpret_cast<int32_t*>(s.keys[1]);
  for (BigPart& bp : B.parts) {
    if (bp.n_items_local == 0) continue;
    ITRY(launch(g, bp.n_items_local, index_of_ids_kernel, bp.item_ids.get(), bp.n_items_local, B.item_glob.get(), n_glob, map));
    ITRY(launch(g, bp.n_items_local, big_mark_alive_kernel, bp.item_alive.get(), map, bp.n_items_local, B.alive_glob.get()));
  }
  unsigned n_items_u = 0;
  ITRY(scan_u32(g, s, B.alive_glob.get(), B.new_i.get(), n_glob, &n_items_u));
  const int64_t n_items = B.n_items = n_items_u;
  g->n_users = n_users;
  g->n_items = n_items;
  g->nnz = B.nnz;
  g->n_known = B.n_known;
  ICHK(g, g->ids[0].alloc(std::max<size_t>((size_t)n_users, 1)));
  ICHK(g, g->ids[1].alloc(std::max<size_t>((size_t)n_items, 1)));
  ICHK(g, g->ptr[0].alloc((size_t)n_users + 1));
  ICHK(g, g->ptr[1].alloc((size_t)n_items + 1));
  if (g->want_known) ICHK(g, g->known_ptr.alloc((size_t)n_users + 1));
  ITRY(launch(g, n_glob, compact_ids_kernel, B.item_glob.get(), B.alive_glob.get(), B.new_i.get(), n_glob, g->ids[1].get()));
  ICHK(g, hipMemsetAsync(g->ptr[0].get(), 0, sizeof(int64_t), g->stream));   // (no range, no user: the one offset there is)
  if (g->want_known) ICHK(g, hipMemsetAsync(g->known_ptr.get(), 0, sizeof(int64_t), g->stream));
  for (BigPart& bp : B.parts) {
    if (bp.n_records == 0) continue;
    ITRY(launch(g, bp.n_items_local, index_of_ids_kernel, bp.item_ids.get(), bp.n_items_local, B.item_glob.get(), n_glob, map));
    ITRY(launch(g, bp.n_items_local, big_final_map_kernel, map, bp.n_items_local, B.new_i.get(), final_map));
    if (bp.nnz) ITRY(launch(g, bp.nnz, big_remap_kernel, g->col[0].get() + bp.nnz_base, bp.nnz, final_map));
    if (g->want_known && bp.n_known) ITRY(launch(g, bp.n_known, big_remap_kernel, g->known_idx.get() + bp.known_base, bp.n_known, final_map));
    if (bp.n_users) ICHK(g, hipMemcpyAsync(g->ids[0].get() + bp.u_base, bp.user_ids.get(), sizeof(int64_t) * (size_t)bp.n_users, hipMemcpyDeviceToDevice, g->stream));
    ITRY(launch(g, bp.n_users + 1, big_add_base_kernel, bp.ptr_local.get(), bp.n_users + 1, bp.nnz_base, g->ptr[0].get() + bp.u_base));
    if (g->want_known)
      ITRY(launch(g, bp.n_users + 1, big_add_base_kernel, bp.known_ptr_local.get(), bp.n_users + 1, bp.known_base, g->known_ptr.get() + bp.u_base));
    g->bytes_moved += 8.0 * (double)bp.nnz + 24.0 * (double)bp.n_users;
  }
  ICHK(g, hipStreamSynchronize(g->stream));
  B.parts.clear();
  B.alive_glob.reset(); B.new_i.reset(); B.item_glob.reset();
  return MALS_OK;
}

// item ranges from a sample of the entries (every 61st), cut at 0.7 of a partition; *todo: the ranges still to do, the first
// on top.  Leaves R^T's offsets zeroed and B.tile_row filled.
int big_plan_item_ranges(mals_ingest g, BigState& B, std::vector<std::pair<int64_t, int64_t>>* todo) {
  const int64_t n_items = B.n_items, nnz = B.nnz;
  ICHK(g, B.cnt.alloc((size_t)n_items + 8));
  const int64_t tiles64 = (n_items + SC_TILE - 1) / SC_TILE + 1;
  ICHK(g, B.sums64.alloc((size_t)tiles64 + 1));
  ICHK(g, hipMemsetAsync(B.cnt.get(), 0, sizeof(unsigned) * ((size_t)n_items + 8), g->stream));
  const int64_t stride = nnz > ((int64_t)1 << 24) ? 61 : 1;
  if (nnz) ITRY(launch_grid(g, {blocks_for((nnz + stride - 1) / stride, 256, 1 << 16)}, big_item_sample_kernel, g->col[0].get(), nnz, stride, B.cnt.get()));
  const unsigned t64 = (unsigned)std::max<int64_t>(1, (n_items + SC_TILE - 1) / SC_TILE);
  ITRY(launch_grid(g, {t64}, big_scan64_reduce_kernel, B.cnt.get(), n_items, B.sums64.get()));
  ITRY(launch_grid(g, {1, 64}, big_scan64_sums_kernel, B.sums64.get(), (int64_t)t64, B.sums64.get() + t64));
  ITRY(launch_grid(g, {t64}, big_scan64_apply_kernel, B.cnt.get(), n_items, B.sums64.get(), B.sums64.get() + t64, g->ptr[1].get()));
  g->bytes_moved += 4.0 * (double)nnz / (double)stride + 16.0 * (double)n_items;
  std::vector<int64_t> cp((size_t)n_items + 1);   // estimated offsets, in sampled entries
  ICHK(g, hipMemcpyAsync(cp.data(), g->ptr[1].get(), sizeof(int64_t) * cp.size(), hipMemcpyDeviceToHost, g->stream));
  ICHK(g, hipStreamSynchronize(g->stream));
  const int64_t budget = std::max<int64_t>(1, (int64_t)(0.7 * (double)B.part_cap / (double)stride));
  std::vector<std::pair<int64_t, int64_t>> ranges;
  for (int64_t a = 0; a < n_items;) {
    int64_t b = std::upper_bound(cp.begin() + a + 1, cp.end(), cp[(size_t)a] + budget) - cp.begin() - 1;
    b = std::min(std::max(b, a + 1), n_items);
    ranges.emplace_back(a, b);
    a = b;
  }
  todo->assign(ranges.rbegin(), ranges.rend());
  const Grid e_tiles = big_tiles(nnz);
  ICHK(g, B.tile_row.alloc((size_t)e_tiles.blocks + 1));
  ITRY(launch(g, (int64_t)e_tiles.blocks + 1, big_tile_rows_kernel, g->ptr[0].get(), std::max<int64_t>(B.n_users, 1), nnz, (int64_t)e_tiles.blocks, B.tile_row.get()));
  ICHK(g, hipMemsetAsync(g->ptr[1].get(), 0, sizeof(int64_t) * ((size_t)n_items + 1), g->stream));
  return MALS_OK;
}

// ---- 3. R^T, item range by item range; a range that turns out larger than a partition is halved -----------------------------
// (Not transpose_by_item: the range's entries are selected out of R and land behind the ranges before it -- the write
// kernel takes the offset, the pointers of the range get a base added -- where the one-shot transpose gathers into whole
// arrays; the sort on the item half is all the two have in common.)
int big_transpose(mals_ingest g, Scratch& s, BigState& B) {
  const int64_t nnz = B.nnz, part_cap = B.part_cap;
  std::vector<std::pair<int64_t, int64_t>> todo;
  ITRY(big_plan_item_ranges(g, B, &todo));
  const Grid e_tiles = big_tiles(nnz);
  int64_t done_entries = 0;   // R^T's offsets so far: every range starts where the one before it ended
  while (!todo.empty()) {
    const int64_t a = todo.back().first, b = todo.back().second;
    todo.pop_back();
    int64_t nq = 0;
    if (nnz > 0) {
      ITRY(launch_grid(g, e_tiles, big_count_items_kernel, g->col[0].get(), nnz, (int32_t)a, (int32_t)b, s.head));
      unsigned counted = 0;
      ITRY(scan_u32(g, s, s.head, s.head, (int64_t)e_tiles.blocks, &counted));
      nq = counted;
      g->bytes_moved += 4.0 * (double)nnz;
    }
    if (nq > part_cap) {   // the sample underestimated it: two halves (a single item that does not fit is refused)
      if (b - a < 2) return fail(g, MALS_INVALID_ARG, "ingest: the entries of one item do not fit a partition (" + std::to_string(nq) + ")");
      const int64_t mid = a + (b - a) / 2;
      todo.emplace_back(mid, b);
      todo.emplace_back(a, mid);
      continue;
    }
    ++g->last_item_ranges;
    if (nq > 0) {
      ITRY(launch_grid(g, e_tiles, big_select_items_kernel, g->col[0].get(), g->val[0].get(), nnz, g->ptr[0].get(), B.tile_row.get(), (int32_t)a, (int32_t)b, s.head,
                       s.keys[0], s.pay[0]));
      int r2 = 0;
      ITRY((radix_sort<uint64_t, unsigned>(g, s, s.keys, s.pay, nq, &r2, 4, ((uint64_t)(b - a - 1) << 32) | 0xffffffffull)));
      ITRY(launch(g, nq, big_transpose_write_kernel, s.keys[r2], s.pay[r2], nq, s.coo_row, g->col[1].get() + done_entries, g->val[1].get() + done_entries));
      g->bytes_moved += 4.0 * (double)nnz + 40.0 * (double)nq;
    }
    // offsets of the range's items: local from the sorted item column, then shifted behind the ranges before it
    ITRY(launch(g, nq + 1, row_ptr_from_sorted_kernel, s.coo_row, nq, b - a, g->ptr[1].get() + a));
    ITRY(launch(g, b - a + 1, big_add_base_inplace_kernel, g->ptr[1].get() + a, b - a + 1, done_entries));
    done_entries += nq;
  }
  if (done_entries != nnz) return fail(g, MALS_HIP_ERROR, "ingest: the item ranges do not add up to the entries");
  return MALS_OK;
}

// the pipeline proper starts at e0, once the buffers exist
int finish_big(mals_ingest g, hipEvent_t e0, int64_t part_cap) {
  Scratch s;
  BigState B;
  ITRY(big_reserve(g, s, B, part_cap));
  ICHK(g, hipEventRecord(e0, g->stream));
  ITRY(probe_id_width(g, s, &B.width));
  ITRY(big_plan_user_ranges(g, s, B));
  ITRY(big_finish_user_ranges(g, s, B));
  ITRY(big_settle_items(g, s, B));
  ITRY(big_transpose(g, s, B));
  // ---- 4. tag id sets, userTagIDs as rows of R^T ----------------------------------------------------------------------------
  ITRY(finish_tags(g, s, B.sort_cap()));
  ICHK(g, hipStreamSynchronize(g->stream));
  return MALS_OK;
}

}  // namespace
