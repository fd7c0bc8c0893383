// ids_host.h -- host side of the id directory (mals_ids_*) and of mals_ingest_apply (include/myrrix_als.h; kernels in
// ids_kernels.h and generation_kernels.h; the logic that needs no device in ingest_live_plan.h).  Included by mals_serving.hip
// inside its anonymous namespace, after popular_host.h and before generation_host.h: every call here runs as an exclusive
// ticket of the serving front (foldin_exclusive), so a lookup sees every resolve queued before it, and the state below is
// only ever touched by the front's leader.
//
// A side's directory COVERS the side when it holds one id per row of the replica.  Only mals_ids_resolve grows the two
// together; whatever else changes the rows leaves a directory that no longer covers them (mals_grow_factor_rows) or drops
// it (ids_drop: mals_load_generation, mals_set_factor_rows, mals_bind_factors), and every call is refused until
// mals_ids_set installs the ids of the rows as they are.
#pragma once

struct IdsSide {
  bool present = false;
  int64_t n = 0;                            // rows that have an id
  DeviceBuffer<int64_t> row_id;             // row -> id, with room to grow (capacity doubling)
  DeviceBuffer<unsigned long long> table;   // id -> row: slots x {key, value = row + 1}
  uint64_t slots = 0;
};

struct IdsState {
  IdsSide side[2];
  // the temporaries of a resolve, grow-only
  DeviceBuffer<unsigned long long> batch, total;
  DeviceBuffer<uint64_t> slot;
  DeviceBuffer<unsigned> first, tile_sums;
  // mals_ingest_apply_times, of the last apply: {gather + resolve + lookup (HIP events on the handle's stream: the host's waits
  // between the kernels are inside), classify + cut + batches built (host clock), the write drivers (host clock), the whole
  // ticket (host clock)} in ms
  EventPair ev;
  double apply_ms[4] = {0.0, 0.0, 0.0, 0.0};
  // mals_ingest_apply_tag_stats, of the last apply: {setItemTag records, setUserTag records, tag removes ignored, rows newly
  // marked (bits of the userTagIDs mask + tag users)}
  int64_t tag_stats[4] = {0, 0, 0, 0};
};

IdsState* ids_state(mals_handle h) {
  if (!h->serving->ids) h->serving->ids = new IdsState();
  return h->serving->ids;
}

void ids_free(mals_handle h) {
  delete h->serving->ids;
  h->serving->ids = nullptr;
}

// the rows of the side were renumbered or replaced: their ids are the caller's to install again
void ids_drop(mals_handle h, int side) {
  if (h->serving->ids) h->serving->ids->side[side] = IdsSide();
}

const char* ids_side_name(int side) { return side == MALS_SIDE_X ? "side X" : "side Y"; }

int64_t ids_replica_rows(mals_handle h, int side) { return h->side[side].F ? h->side[side].n_total : 0; }

unsigned ids_grid(mals_handle h, int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((int64_t)h->n_cu * 8, (n + 255) / 256)); }

// the directory covers the replica, or the message says which rows have no id
int ids_ready(mals_handle h, int side, std::string& msg) {
  const IdsState* st = h->serving->ids;
  const int64_t rows = ids_replica_rows(h, side);
  const int64_t have = st && st->side[side].present ? st->side[side].n : 0;
  if (have > 0 && have == rows) return MALS_OK;
  if (have < rows)
    msg = std::string(ids_side_name(side)) + ": rows [" + std::to_string((long long)have) + ", " + std::to_string((long long)rows) +
          ") have no id (the directory is installed by mals_ids_set and grows with mals_ids_resolve alone)";
  else if (rows == 0)
    msg = std::string(ids_side_name(side)) + ": the replica has no rows, so no row has an id (mals_set_factor_rows, then mals_ids_set)";
  else
    msg = std::string(ids_side_name(side)) + ": the directory names " + std::to_string((long long)have) + " rows, the replica has " +
          std::to_string((long long)rows) + " (mals_ids_set)";
  return MALS_INVALID_ARG;
}

// ---- mals_ids_set -----------------------------------------------------------------------------------------------------------
// Built aside and moved in when it is whole.  The table is the batch table of a resolve over an empty directory: row j
// joins the slot of ids[j], the slot keeps its smallest row, and a row that is not its slot's first repeats an earlier one.
int ids_set_run(mals_handle h, int side, int64_t n, const int64_t* ids, int mem_kind, std::string& msg) {
  const int64_t rows = ids_replica_rows(h, side);
  if (n != rows) {
    msg = std::string(ids_side_name(side)) + ": one id per row of the replica (" + std::to_string((long long)rows) + " rows, " +
          std::to_string((long long)n) + " ids)";
    return MALS_INVALID_ARG;
  }
  if (n == 0) {
    ids_drop(h, side);
    return MALS_OK;
  }
  IdsSide ns;
  DeviceBuffer<uint64_t> slot;
  DeviceBuffer<unsigned> first;
  DeviceBuffer<unsigned long long> dup;
  DeviceBuffer<int64_t> rows_tmp;
  ns.slots = gen_table_slots(n);
  FCHK(msg, ns.row_id.alloc((size_t)(n + std::max<int64_t>(n / 16, 1024))));
  FCHK(msg, ns.table.alloc((size_t)(2 * ns.slots)));
  FCHK(msg, slot.alloc((size_t)n));
  FCHK(msg, first.alloc((size_t)n));
  FCHK(msg, rows_tmp.alloc((size_t)n));
  FCHK(msg, dup.alloc(1));
  FCHK(msg, hipMemcpyAsync(ns.row_id.get(), ids, sizeof(int64_t) * (size_t)n, mem_kind == MALS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                           h->stream));
  FCHK(msg, hipMemsetAsync(ns.table.get(), 0, sizeof(unsigned long long) * (size_t)(2 * ns.slots), h->stream));
  FCHK(msg, hipMemsetAsync(dup.get(), 0xff, sizeof(unsigned long long), h->stream));
  const unsigned grid = ids_grid(h, n);
  hipLaunchKernelGGL(ids_probe_kernel, dim3(grid), dim3(256), 0, h->stream, (const int64_t*)ns.row_id.get(), n, (const unsigned long long*)nullptr,
                     (uint64_t)0, ns.table.get(), ns.slots - 1, rows_tmp.get(), slot.get());
  hipLaunchKernelGGL(ids_first_kernel, dim3(grid), dim3(256), 0, h->stream, (const unsigned long long*)ns.table.get(), (const uint64_t*)slot.get(), n,
                     first.get());
  hipLaunchKernelGGL(ids_min_repeat_kernel, dim3(grid), dim3(256), 0, h->stream, (const unsigned*)first.get(), n, dup.get());
  hipLaunchKernelGGL(gen_fill_keys_kernel, dim3(ids_grid(h, (int64_t)ns.slots)), dim3(256), 0, h->stream, (const int64_t*)ns.row_id.get(), ns.table.get(),
                     ns.slots);
  FCHK(msg, hipGetLastError());
  unsigned long long got = ~0ull;
  FCHK(msg, hipMemcpyAsync(&got, dup.get(), sizeof(got), hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipStreamSynchronize(h->stream));
  if (got != ~0ull) {
    msg = std::string(ids_side_name(side)) + ": the ids hold an id twice (row " + std::to_string((long long)got) + " repeats an earlier one)";
    return MALS_INVALID_ARG;
  }
  ns.present = true;
  ns.n = n;
  ids_state(h)->side[side] = std::move(ns);
  return MALS_OK;
}

// ---- lookup and resolve on device arrays (mals_ingest_apply hands its records' ids over as they lie) --------------------------
// nothing waited for
int ids_lookup_dev(mals_handle h, int side, int64_t n, const int64_t* d_ids, int64_t* d_rows, std::string& msg) {
  if (int rc = ids_ready(h, side, msg)) return rc;
  if (n == 0) return MALS_OK;
  const IdsSide& sd = ids_state(h)->side[side];
  hipLaunchKernelGGL(gen_lookup_kernel, dim3(ids_grid(h, n)), dim3(256), 0, h->stream, d_ids, n, (const unsigned long long*)sd.table.get(), sd.slots - 1,
                     d_rows);
  FCHK(msg, hipGetLastError());
  return MALS_OK;
}

// the new rows are in the directory and in the replica, and d_rows is written, when it returns.  A failure before the
// replica has grown changes nothing.
int ids_resolve_dev(mals_handle h, int side, int64_t n, const int64_t* d_ids, int64_t* d_rows, int64_t* n_new_out, std::string& msg) {
  *n_new_out = 0;
  if (int rc = ids_ready(h, side, msg)) return rc;
  if (n == 0) return MALS_OK;
  IdsState& st = *ids_state(h);
  IdsSide& sd = st.side[side];
  const uint64_t bslots = gen_table_slots(n);
  const int64_t n_tiles = (n + GEN_SCAN_TILE - 1) / GEN_SCAN_TILE;
  FCHK(msg, st.batch.reserve((size_t)(2 * bslots), h->stream));
  FCHK(msg, st.slot.reserve((size_t)n, h->stream));
  FCHK(msg, st.first.reserve((size_t)n, h->stream));
  FCHK(msg, st.tile_sums.reserve((size_t)n_tiles, h->stream));
  FCHK(msg, st.total.reserve(1, h->stream));
  const unsigned grid = ids_grid(h, n);
  FCHK(msg, hipMemsetAsync(st.batch.get(), 0, sizeof(unsigned long long) * (size_t)(2 * bslots), h->stream));
  hipLaunchKernelGGL(ids_probe_kernel, dim3(grid), dim3(256), 0, h->stream, d_ids, n, (const unsigned long long*)sd.table.get(), sd.slots - 1,
                     st.batch.get(), bslots - 1, d_rows, st.slot.get());
  hipLaunchKernelGGL(ids_first_kernel, dim3(grid), dim3(256), 0, h->stream, (const unsigned long long*)st.batch.get(), (const uint64_t*)st.slot.get(), n,
                     st.first.get());
  hipLaunchKernelGGL(gen_scan_reduce_kernel, dim3((unsigned)n_tiles), dim3(256), 0, h->stream, (const unsigned*)st.first.get(), n, st.tile_sums.get());
  hipLaunchKernelGGL(gen_scan_sums_kernel, dim3(1), dim3(256), 0, h->stream, st.tile_sums.get(), n_tiles, st.total.get());
  FCHK(msg, hipGetLastError());
  unsigned long long total = 0;
  FCHK(msg, hipMemcpyAsync(&total, st.total.get(), sizeof(total), hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipStreamSynchronize(h->stream));   // the new rows size everything behind the scan
  const int64_t n_new = (int64_t)total;
  if (n_new == 0) return MALS_OK;   // (no miss: every row is written)
  const int64_t new_n = sd.n + n_new;
  // what the larger directory needs, aside: a failure here leaves the handle as it was
  DeviceBuffer<int64_t> row_id;
  DeviceBuffer<unsigned long long> table;
  const uint64_t new_slots = ids_grown_slots(sd.slots, new_n);
  if (sd.row_id.capacity() < (size_t)new_n) {
    FCHK(msg, row_id.alloc(std::max((size_t)new_n, 2 * sd.row_id.capacity())));
    FCHK(msg, hipMemcpyAsync(row_id.get(), sd.row_id.get(), sizeof(int64_t) * (size_t)sd.n, hipMemcpyDeviceToDevice, h->stream));
  }
  if (new_slots != sd.slots) {
    FCHK(msg, table.alloc((size_t)(2 * new_slots)));
    FCHK(msg, hipMemsetAsync(table.get(), 0, sizeof(unsigned long long) * (size_t)(2 * new_slots), h->stream));
  }
  // the replica: the existing grow path (userTagIDs, known items of grown users, capacity doubling)
  const int grown_owner = foldin_user_rows_end(h) >= h->side[side].n_total ? 0 : -1;
  if (int rc = foldin_grow_members(&h, 1, side, new_n, grown_owner, false, msg)) {
    (void)hipStreamSynchronize(h->stream);   // (the copy into row_id may still run)
    return rc;
  }
  int64_t* rid = row_id ? row_id.get() : sd.row_id.get();
  unsigned long long* tab = table ? table.get() : sd.table.get();
  hipLaunchKernelGGL(ids_assign_kernel, dim3((unsigned)n_tiles), dim3(256), 0, h->stream, (const unsigned*)st.first.get(), n,
                     (const unsigned*)st.tile_sums.get(), d_ids, sd.n, d_rows, rid);
  hipLaunchKernelGGL(ids_follow_kernel, dim3(grid), dim3(256), 0, h->stream, (const unsigned long long*)st.batch.get(), (const uint64_t*)st.slot.get(),
                     (const unsigned*)st.first.get(), n, d_rows);
  const int64_t from = table ? 0 : sd.n;   // a larger table takes every row, the old one the new rows
  hipLaunchKernelGGL(ids_insert_rows_kernel, dim3(ids_grid(h, new_n - from)), dim3(256), 0, h->stream, (const int64_t*)rid, from, new_n, tab,
                     new_slots - 1);
  FCHK(msg, hipGetLastError());
  FCHK(msg, hipStreamSynchronize(h->stream));
  if (row_id) sd.row_id = std::move(row_id);
  if (table) sd.table = std::move(table);
  sd.slots = new_slots;
  sd.n = new_n;
  *n_new_out = n_new;
  return MALS_OK;
}

// ---- mals_ids_lookup / mals_ids_resolve / mals_ids_get: host arrays ------------------------------------------------------------
int ids_rows_of_run(mals_handle h, int side, int64_t n, const int64_t* ids, int64_t* rows_out, int64_t* n_new_out, bool add, std::string& msg) {
  if (n_new_out) *n_new_out = 0;
  if (int rc = ids_ready(h, side, msg)) return rc;
  if (n == 0) return MALS_OK;
  DeviceBuffer<int64_t> d;   // ids | rows
  FCHK(msg, d.alloc(2 * (size_t)n));
  FCHK(msg, hipMemcpyAsync(d.get(), ids, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  int64_t n_new = 0;
  const int rc = add ? ids_resolve_dev(h, side, n, d.get(), d.get() + n, &n_new, msg) : ids_lookup_dev(h, side, n, d.get(), d.get() + n, msg);
  if (rc != MALS_OK) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  FCHK(msg, hipMemcpyAsync(rows_out, d.get() + n, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipStreamSynchronize(h->stream));
  if (n_new_out) *n_new_out = n_new;
  return MALS_OK;
}

int ids_get_run(mals_handle h, int side, int64_t row_begin, int64_t n, int64_t* ids_out, std::string& msg) {
  if (int rc = ids_ready(h, side, msg)) return rc;
  const IdsSide& sd = ids_state(h)->side[side];
  if (row_begin < 0 || n < 0 || row_begin > sd.n || n > sd.n - row_begin) {
    msg = "rows outside the directory";
    return MALS_INVALID_ARG;
  }
  if (n == 0) return MALS_OK;
  FCHK(msg, hipMemcpyAsync(ids_out, sd.row_id.get() + row_begin, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipStreamSynchronize(h->stream));
  return MALS_OK;
}

// ---- mals_ingest_apply ------------------------------------------------------------------------------------------------------
// ServerRecommender.ingest (ServerRecommender.java:268-298) over the records of an ingest, inside ONE ticket: classify (host,
// from the values), resolve the sets' ids and look the removes' ids up (device), the rows to the host once, the cut into
// runs (ingest_live_plan.h), and every run through the write path's own drivers.  *changed: the handle may differ from what
// it was (from the first resolve on); before that a failure is a refusal of the whole call.
const int64_t IDS_OWN_ALL[2] = {std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max()};

// d_kind (MALS_INGEST_OPT_LIVE_TAGS; else nullptr): the records' kinds -- tag sets ride in the set runs, tag removes are ignored
int ids_apply_run(mals_handle h, int64_t n, const int64_t* d_user, const int64_t* d_item, const float* d_value, const uint8_t* d_kind,
                  int64_t* stats_out8,
                  int64_t* removed_ids_out, int64_t removed_cap, int64_t* n_removed_out, bool* changed, std::string& msg) {
  *changed = false;
  int64_t stats[8] = {n, 0, 0, 0, 0, 0, 0, 0}, n_removed = 0;
  auto publish = [&] {
    if (stats_out8) std::copy(stats, stats + 8, stats_out8);
    if (n_removed_out) *n_removed_out = n_removed;
  };
  publish();
  for (int sd = 0; sd < 2; ++sd)
    if (int rc = ids_ready(h, sd, msg)) return rc;
  if (n == 0) return MALS_OK;
  using Clock = std::chrono::steady_clock;
  auto ms_since = [](Clock::time_point a) { return std::chrono::duration<double, std::milli>(Clock::now() - a).count(); };
  IdsState& st = *ids_state(h);
  std::fill(st.tag_stats, st.tag_stats + 4, (int64_t)0);
  const Clock::time_point t_begin = Clock::now();
  double plan_ms = 0.0;
  FCHK(msg, st.ev.ensure());
  std::vector<float> val((size_t)n);
  std::vector<uint8_t> kinds(d_kind ? (size_t)n : 0), set_kind;
  FCHK(msg, hipMemcpyAsync(val.data(), d_value, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  if (d_kind) FCHK(msg, hipMemcpyAsync(kinds.data(), d_kind, (size_t)n, hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipStreamSynchronize(h->stream));
  LiveClasses cls;
  LiveTagCounts tags;
  if (d_kind) live_classify_kinds(n, val.data(), kinds.data(), cls, set_kind, tags);
  else live_classify(n, val.data(), cls);
  const int64_t ns = (int64_t)cls.set_pos.size(), nr = (int64_t)cls.rem_pos.size(), n_used = ns + nr;
  auto marked_rows = [&] { return h->n_tag_items + (h->serving->pop ? (int64_t)popular_state(h)->tag_users.size() : 0); };
  const int64_t marked_before = marked_rows();
  if (nr > removed_cap || (nr > 0 && !removed_ids_out)) {
    msg = "removed_cap (" + std::to_string((long long)removed_cap) + ") is smaller than the remove records (" + std::to_string((long long)nr) + ")";
    return MALS_INVALID_ARG;
  }
  if (nr > 0 && !h->side[MALS_SIDE_X].has_matrix && !h->known_ptr) {
    msg = "the stream removes preferences: the user-side matrix (or mals_set_known_items) holds the known items";
    return MALS_INVALID_ARG;
  }
  // the ids of the sets and of the removes, gathered as they lie: [set users | set items | remove users | remove items]
  std::vector<int64_t> pos;
  pos.reserve((size_t)n);
  pos.insert(pos.end(), cls.set_pos.begin(), cls.set_pos.end());
  pos.insert(pos.end(), cls.rem_pos.begin(), cls.rem_pos.end());
  plan_ms += ms_since(t_begin);
  DeviceBuffer<int64_t> d_pos, d_ids, d_rows;
  FCHK(msg, hipEventRecord(st.ev.begin, h->stream));
  FCHK(msg, d_pos.alloc((size_t)n));
  FCHK(msg, d_ids.alloc(2 * (size_t)n));
  FCHK(msg, d_rows.alloc(2 * (size_t)n));
  if (n_used) FCHK(msg, hipMemcpyAsync(d_pos.get(), pos.data(), sizeof(int64_t) * (size_t)n_used, hipMemcpyHostToDevice, h->stream));   // (ignored tag removes: n_used < n)
  int64_t* ids_su = d_ids.get();
  int64_t* ids_si = ids_su + ns;
  int64_t* ids_ru = ids_si + ns;
  int64_t* ids_ri = ids_ru + nr;
  auto gather = [&](const int64_t* src, const int64_t* idx, int64_t cnt, int64_t* out) {
    if (cnt > 0)
      hipLaunchKernelGGL(gen_gather_i64_kernel, dim3(ids_grid(h, cnt)), dim3(256), 0, h->stream, src, n, idx, cnt, out);
  };
  gather(d_user, d_pos.get(), ns, ids_su);
  gather(d_item, d_pos.get(), ns, ids_si);
  gather(d_user, d_pos.get() + ns, nr, ids_ru);
  gather(d_item, d_pos.get() + ns, nr, ids_ri);
  FCHK(msg, hipGetLastError());
  struct Waited {   // nothing of this call still runs when its buffers go
    hipStream_t s;
    ~Waited() { (void)hipStreamSynchronize(s); }
  } waited{h->stream};
  *changed = true;
  int64_t* rows_su = d_rows.get();
  if (int rc = ids_resolve_dev(h, MALS_SIDE_X, ns, ids_su, rows_su, &stats[5], msg)) return rc;
  if (int rc = ids_resolve_dev(h, MALS_SIDE_Y, ns, ids_si, rows_su + ns, &stats[6], msg)) return rc;
  if (int rc = ids_lookup_dev(h, MALS_SIDE_X, nr, ids_ru, rows_su + 2 * ns, msg)) return rc;
  if (int rc = ids_lookup_dev(h, MALS_SIDE_Y, nr, ids_ri, rows_su + 2 * ns + nr, msg)) return rc;
  // the rows to the host, once: the level plan and the known items are host work
  std::vector<int64_t> rows(2 * (size_t)n), rem_uid((size_t)nr);
  if (n_used) FCHK(msg, hipMemcpyAsync(rows.data(), d_rows.get(), sizeof(int64_t) * 2 * (size_t)n_used, hipMemcpyDeviceToHost, h->stream));
  if (nr > 0) FCHK(msg, hipMemcpyAsync(rem_uid.data(), ids_ru, sizeof(int64_t) * (size_t)nr, hipMemcpyDeviceToHost, h->stream));
  FCHK(msg, hipEventRecord(st.ev.end, h->stream));
  FCHK(msg, hipStreamSynchronize(h->stream));
  float resolve_ms = 0.f;
  FCHK(msg, hipEventElapsedTime(&resolve_ms, st.ev.begin, st.ev.end));
  const Clock::time_point t_plan = Clock::now();
  const int64_t* set_u = rows.data();
  const int64_t* set_i = set_u + ns;
  const int64_t* rem_u = set_i + ns;
  const int64_t* rem_i = rem_u + nr;
  LivePlan plan;
  live_cut(cls, rem_u, rem_i, plan);
  const int64_t nk = (int64_t)plan.rem_keep.size();
  std::vector<float> set_v((size_t)ns);
  for (int64_t j = 0; j < ns; ++j) set_v[(size_t)j] = val[(size_t)cls.set_pos[(size_t)j]];
  std::vector<int64_t> keep_u((size_t)nk), keep_i((size_t)nk), keep_uid((size_t)nk), removed_rows((size_t)nk);
  for (int64_t j = 0; j < nk; ++j) {
    const size_t r = (size_t)plan.rem_keep[(size_t)j];
    keep_u[(size_t)j] = rem_u[r];
    keep_i[(size_t)j] = rem_i[r];
    keep_uid[(size_t)j] = rem_uid[r];
  }
  std::vector<int32_t> status((size_t)ns, 0);
  stats[1] = ns;
  stats[2] = nk;
  stats[3] = plan.dropped;
  int first = MALS_OK;
  std::string first_msg;
  plan_ms += ms_since(t_plan);
  const Clock::time_point t_writes = Clock::now();
  auto times = [&] {
    st.apply_ms[0] = resolve_ms;
    st.apply_ms[1] = plan_ms;
    st.apply_ms[2] = ms_since(t_writes);
    st.apply_ms[3] = ms_since(t_begin);
    st.tag_stats[0] = tags.item_tag_sets;
    st.tag_stats[1] = tags.user_tag_sets;
    st.tag_stats[2] = tags.removes_ignored;
    st.tag_stats[3] = marked_rows() - marked_before;
  };
  for (const LiveRun& run : plan.runs) {
    const int64_t b = run.begin, len = run.end - run.begin;
    std::string why;
    ++stats[7];
    if (run.is_set) {
      const uint8_t* run_kind = d_kind ? live_run_kinds(set_kind, run.begin, run.end) : nullptr;
      const int rc = foldin_set_members(&h, 1, IDS_OWN_ALL, false, len, set_u + b, set_i + b, set_v.data() + b, run_kind, status.data() + b, why);
      int64_t failed = 0;
      for (int64_t j = 0; j < len; ++j) failed += status[(size_t)(b + j)] != MALS_OK ? 1 : 0;
      stats[4] += failed;
      if (rc != MALS_OK && failed == 0) {   // not an update's failure: the call's
        msg = why;
        publish();
        return rc;
      }
      if (rc != MALS_OK && first == MALS_OK) {   // the first failed update in stream order; the others go on
        first = rc;
        first_msg = "set record " + std::to_string((long long)cls.set_pos[(size_t)b]) + " ff.: " + why;
      }
    } else {
      int64_t got = 0;
      if (int rc = foldin_remove_members(&h, 1, IDS_OWN_ALL, false, len, keep_u.data() + b, keep_i.data() + b, removed_rows.data(), &got, why)) {
        msg = why;
        publish();
        return rc;
      }
      // the emptied users by id: a row of this run's records
      std::unordered_map<int64_t, int64_t> id_of_row;
      for (int64_t j = 0; got > 0 && j < len; ++j) id_of_row[keep_u[(size_t)(b + j)]] = keep_uid[(size_t)(b + j)];
      for (int64_t e = 0; e < got; ++e) removed_ids_out[n_removed++] = id_of_row[removed_rows[(size_t)e]];
    }
  }
  publish();
  times();
  msg = first_msg;
  return first;
}
