// ingest_host.h -- what every finisher of the ingest -> CSR path shares (host code of ingest_api.hip, included first): the
// ingest object, the status and launch helpers, the arena of one sort pipeline, the sort and the scan, and the steps that
// the one-shot finish (ingest_api.hip), the partitioned finish (ingest_big_host.h) and the group finish
// (ingest_group_host.h) all run: the id-width probe, the core of a range of records, the transpose by item, the tag sets.
// Expects before it: ingest_kernels.h, ingest_big_kernels.h, hip_buffer.h, include/myrrix_als.h and `using namespace mals`.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

constexpr int64_t MALS_INGEST_MAX_RECORDS = (int64_t)1 << 36;       // (the record arrays alone are 1.6 TB there)
constexpr int64_t MALS_INGEST_ONE_SHOT_MAX = (int64_t)0x7fffff00;   // what one sort pipeline holds (32-bit positions)
constexpr int64_t MALS_SPLIT_MAX_SHARES = 256;                      // the split kernel's byte-wide destination (split_kernels.h)
constexpr int64_t MALS_INGEST_MIN_PART = (int64_t)1 << 26;          // smallest user range the automatic choice makes (ingest_big_host.h)

struct mals_ingest_s {
  int device = 0;
  float zero_threshold = 1.0e-4f;
  hipStream_t stream = nullptr;
  std::string err;
  // appended records (device), capacity-doubling
  int64_t n = 0;
  DeviceBuffer<int64_t> d_user, d_item;
  DeviceBuffer<float> d_value;
  DeviceBuffer<uint8_t> d_kind;   // MALS_INGEST_OPT_LIVE_TAGS only: 0 a preference, 1 setItemTag, 2 setUserTag (compact_records_kernel)
  // results
  bool finished = false;
  int64_t n_users = 0, n_items = 0, nnz = 0;
  DeviceBuffer<int64_t> ids[2];  // dense index -> id, ascending
  DeviceBuffer<int64_t> ptr[2];  // CSR row pointers (side X: by user, side Y: by item)
  DeviceBuffer<int32_t> col[2];
  DeviceBuffer<float> val[2];
  // sort/scan workspace, kept between finishes, one allocation per buffer.  On some boxes a fresh
  // allocation of tens of GB takes 1-1.5 s and returns memory in which this pipeline runs ~2x slower
  // (driver memory placement, not under the library's control); workspace_ms reports the former.
  static constexpr int N_WS = 12;
  DeviceBuffer<uint8_t> ws[N_WS];
  double last_workspace_ms = 0.0;  // host time spent (re)allocating the workspace in the last finish
  double last_finish_ms = 0.0;
  double bytes_moved = 0.0;  // algorithmic bytes of the last finish (reads + writes of every pass)
  int radix_passes = 0;
  // ---- text -> records (ingest_text_host.h) ----
  size_t text_block_bytes = (size_t)256 << 20;
  DeviceBuffer<uint8_t> d_text;   // [carried tail][new bytes][padding]
  DeviceBuffer<uint8_t> d_carry;  // the unterminated tail of the previous block
  size_t carry_len = 0;
  bool carry_ends_cr = false;
  PinnedBuffer<uint8_t> h_pinned;  // staging buffer of mals_ingest_read_file
  DeviceBuffer<unsigned> t_block_counts, t_tile_sums;
  DeviceBuffer<unsigned> t_starts, t_flag, t_defer;  // per-line arrays of one block (t_starts' capacity: lines they hold)
  DeviceBuffer<uint8_t> t_status;
  DeviceBuffer<int64_t> t_user, t_item;
  DeviceBuffer<uint32_t> t_value;
  DeviceBuffer<uint8_t> t_counters;  // mals::TextCounters + two tag cursors
  DeviceBuffer<int64_t> d_tags[2];   // [0]: itemTagIDs (tags seen in the user column), [1]: userTagIDs; with repeats
  size_t n_tags_raw[2] = {0, 0};
  int64_t lines = 0, bad_lines = 0, header_lines = 0, skipped_lines = 0, slow_lines = 0, text_bytes = 0;
  bool live_tags = false;      // MALS_INGEST_OPT_LIVE_TAGS: tag lines are writes of mals_ingest_apply (the records carry their kind)
  bool tab_delimiter = false;  // MALS_INGEST_OPT_TAB_DELIMITER: tabs are read as commas (ServerRecommender.ingest's splitter)
  bool abort_armed = false;    // badLines > 100: the next line throws (IFR:96-98)
  bool text_failed = false;
  int text_fail_code = 0;
  std::string text_fail_msg;
  double parse_ms = 0.0, stage_ms = 0.0;
  EventPair t_ev;   // around the staging of a text block
  // results of the last finish that come from the text path's extras
  DeviceBuffer<int64_t> tag_ids[2];  // ascending, unique
  int64_t n_tag_ids[2] = {0, 0};
  bool want_known = false;
  int64_t n_known = 0;
  DeviceBuffer<int64_t> known_ptr;  // knownItemIDs as a CSR over the dense user / item indices
  DeviceBuffer<int32_t> known_idx;
  DeviceBuffer<int64_t> tag_item_idx;  // dense item index of every userTagID (ascending ids), -1: the tag owns no row of R^T
  int64_t part_cap = 0;       // MALS_INGEST_OPT_PARTITION_RECORDS (0: default) -- ingest_big_host.h
  int32_t last_partitions = 0, last_item_ranges = 0;
  // ---- one share of a stream ingested by a group (MALS_INGEST_OPT_SHARE, ingest_group_host.h) ----
  int32_t share = 0;
  std::vector<int64_t> bad_pos;   // line number (1-based, in this share) of each of the first 101 bad lines
  int64_t fatal_line = 0;         // line (1-based, in this share) of a lone-quote token, 0: none
  bool sharded = false;           // the results are this member's slices (mals_group_ingest_finish)
  int64_t shard_records = 0;     // records this member finished in the group finish (its records are released afterwards)
  bool spent = false;             // its records went into a group finish (which then failed, or left slices): no append / finish
  int64_t work_at_replicas = -1;  // work bytes held when the group declared its factor replicas (-1: not in a group finish)
  int64_t slice_begin[2] = {0, 0}, slice_rows[2] = {0, 0}, slice_nnz[2] = {0, 0};
  double split_ms = 0.0, split_bytes = 0.0;   // the split kernels of the last group finish

  // The two resets stand under the fields they reset: a buffer added above belongs into one of them (and into
  // mals_ingest_memory, ingest_group_host.h).
  // the results of the last finish
  void free_results() {
    for (int sd = 0; sd < 2; ++sd) {
      ids[sd].reset(); ptr[sd].reset(); col[sd].reset(); val[sd].reset(); tag_ids[sd].reset();
      n_tag_ids[sd] = 0;
    }
    known_ptr.reset(); known_idx.reset(); tag_item_idx.reset();
    finished = sharded = false;
    n_users = n_items = nnz = n_known = 0;
  }
  // records, workspace and text buffers: what a group finish releases before the factor replicas are declared
  void release_work() {
    d_user.reset(); d_item.reset(); d_value.reset(); d_kind.reset();
    for (int b = 0; b < N_WS; ++b) ws[b].reset();
    d_text.reset(); d_carry.reset();
    t_block_counts.reset(); t_tile_sums.reset(); t_starts.reset(); t_flag.reset(); t_defer.reset();
    t_status.reset(); t_user.reset(); t_item.reset(); t_value.reset(); t_counters.reset();
    d_tags[0].reset(); d_tags[1].reset();
    n_tags_raw[0] = n_tags_raw[1] = 0;
    n = 0;
    carry_len = 0;
  }
};

namespace {

int fail(mals_ingest g, int code, const std::string& msg) {
  if (g) g->err = msg;
  return code;
}

#define ICHK(g, call)                                                                  \
  do {                                                                                 \
    hipError_t _e = (call);                                                            \
    if (_e != hipSuccess) {                                                            \
      const int _code = (_e == hipErrorOutOfMemory) ? MALS_OOM : MALS_HIP_ERROR;       \
      return fail(g, _code, std::string(#call) + ": " + hipGetErrorString(_e));        \
    }                                                                                  \
  } while (0)

// a step that returns a library status: leave with it unless it is MALS_OK
#define ITRY(step) do { if (int _rc = (step)) return _rc; } while (0)

unsigned blocks_for(int64_t n, int per_block = 256, int64_t cap = 1 << 20) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, cap));
}

// One kernel on the ingest's stream, its launch checked; the status is what ICHK gives.  launch: the default grid for n
// elements, blocks_for(n) workgroups of 256.  launch_grid: the sites that count tiles or cap the grid themselves.
struct Grid { unsigned blocks, threads = 256; };
template <typename... KArgs, typename... Args>
int launch_grid(mals_ingest g, Grid grid, void (*kernel)(KArgs...), Args&&... args) {
  hipLaunchKernelGGL(kernel, dim3(grid.blocks), dim3(grid.threads), 0, g->stream, static_cast<KArgs>(args)...);
  ICHK(g, hipGetLastError());
  return MALS_OK;
}
template <typename... KArgs, typename... Args>
int launch(mals_ingest g, int64_t n, void (*kernel)(KArgs...), Args&&... args) {
  return launch_grid(g, Grid{blocks_for(n)}, kernel, std::forward<Args>(args)...);
}

// The arena of one sort pipeline (the ingest object's workspace), carved into the views the sorts, the scans and the stages
// of a finish use.  The text path fills in tile_sums and total alone, for its scans.
struct Scratch {
  uint64_t* keys[2] = {nullptr, nullptr};
  unsigned* pay[2] = {nullptr, nullptr};
  uint64_t* pay64[2] = {nullptr, nullptr};
  unsigned* counts = nullptr;     // 256 * n_blocks
  unsigned* tile_sums = nullptr;  // scan tiles
  unsigned long long* digit_tot = nullptr;  // [8][256]
  unsigned* total = nullptr;      // grand total of a scan
  unsigned *head = nullptr, *scan = nullptr, *ri = nullptr;  // per position: run heads, their scan, item ranks
  // dead after the composite sort: the 64-bit payload buffers carry the replay outputs
  unsigned *keep = nullptr, *present = nullptr;
  float* pair_val = nullptr;
  int32_t* coo_row = nullptr;
};

// device temporaries of one range of records, sized by its number of distinct ids; they live as long as the caller keeps them
struct RangeTmp {
  DeviceBuffer<unsigned> alive_u, alive_i, new_u, new_i;
  DeviceBuffer<int64_t> uid_all, iid_all;
};

// the records a sort pipeline works on: all of the ingest's, or one user range of them (ingest_big_host.h)
struct Records {
  const int64_t* user;
  const int64_t* item;
  const float* value;
  int64_t n;
};

// exclusive scan of `n` uint32 (in != out allowed to alias); optional grand total copied to *host_total
int scan_u32(mals_ingest g, Scratch& s, const unsigned* in, unsigned* out, int64_t n, unsigned* host_total) {
  if (n <= 0) {
    if (host_total) *host_total = 0;
    return MALS_OK;
  }
  const int64_t tiles = (n + SC_TILE - 1) / SC_TILE;
  ITRY(launch_grid(g, {(unsigned)tiles}, scan_reduce_kernel, in, n, s.tile_sums));
  ITRY(launch_grid(g, {1}, scan_sums_kernel, s.tile_sums, tiles, s.total));
  ITRY(launch_grid(g, {(unsigned)tiles}, scan_apply_kernel, in, n, out, s.tile_sums));
  g->bytes_moved += 12.0 * (double)n;
  if (host_total) {
    ICHK(g, hipMemcpyAsync(host_total, s.total, sizeof(unsigned), hipMemcpyDeviceToHost, g->stream));
    ICHK(g, hipStreamSynchronize(g->stream));
  }
  return MALS_OK;
}

// Stable LSD radix sort of (keys[0], pay[0]) by the key digits >= first_digit; *result = index of the
// buffer pair holding the sorted data.  Digits on which all keys agree are skipped.  K = uint32_t when the caller knows
// that every key fits (ids below 2^32): 12 bytes less per record and pass, and a third workgroup per CU (LDS).
// key_bound (optional): a value no key exceeds, when the caller knows one (dense ranks): the digits above it are skipped
// without the pass over the keys that counts them.
template <typename K, typename P>
int radix_sort(mals_ingest g, Scratch& s, K* const (&keys)[2], P* const (&pay)[2], int64_t n, int* result, int first_digit = 0,
               uint64_t key_bound = 0) {
  constexpr int ND = (int)sizeof(K);
  *result = 0;
  if (n <= 1) return MALS_OK;
  std::vector<unsigned long long> tot(8 * 256, 0ull);
  if (key_bound != 0) {
    for (int d = 0; d < ND; ++d)
      if ((key_bound >> (8 * d)) == 0) tot[(size_t)d * 256] = (unsigned long long)n;  // every key has a zero there
  } else {
    ICHK(g, hipMemsetAsync(s.digit_tot, 0, 8 * 256 * sizeof(unsigned long long), g->stream));
    ITRY(launch_grid(g, {blocks_for(n, 256 * 16, 4096)}, rs_digit_totals_kernel<K>, keys[0], n, s.digit_tot));
    ICHK(g, hipMemcpyAsync(tot.data(), s.digit_tot, tot.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, g->stream));
    ICHK(g, hipStreamSynchronize(g->stream));
    g->bytes_moved += (double)sizeof(K) * (double)n;
  }
  const int64_t n_blocks = (n + RS_BLOCK_TILE - 1) / RS_BLOCK_TILE;
  const Grid grid = {(unsigned)n_blocks};
  int cur = 0;
  for (int d = first_digit; d < ND; ++d) {
    bool trivial = false;
    for (int b = 0; b < 256; ++b)
      if (tot[(size_t)d * 256 + b] == (unsigned long long)n) trivial = true;
    if (trivial) continue;
    ITRY(launch_grid(g, grid, rs_histogram_kernel<K>, keys[cur], n, 8 * d, n_blocks, s.counts));
    ITRY(scan_u32(g, s, s.counts, s.counts, 256 * n_blocks, nullptr));
    ITRY(launch_grid(g, grid, rs_scatter_kernel<K, P>, keys[cur], pay[cur], n, 8 * d, n_blocks, s.counts, keys[1 - cur], pay[1 - cur]));
    g->bytes_moved += ((double)sizeof(K) + 2.0 * ((double)sizeof(K) + sizeof(P))) * (double)n;  // histogram read; scatter read + write
    ++g->radix_passes;
    cur = 1 - cur;
  }
  *result = cur;
  return MALS_OK;
}

int64_t record_capacity(mals_ingest g) { return (int64_t)g->d_user.capacity(); }

// the record arrays (three, and the kinds of MALS_INGEST_OPT_LIVE_TAGS) moved to blocks of `cap` records, the first g->n kept.
// All new blocks exist before the old ones go: a failed allocation leaves the records as they were (and allocates nothing).
int grow_records(mals_ingest g, int64_t cap) {
  DeviceBuffer<int64_t> u, it;
  DeviceBuffer<float> v;
  DeviceBuffer<uint8_t> kd;
  ICHK(g, u.alloc((size_t)cap));
  ICHK(g, it.alloc((size_t)cap));
  ICHK(g, v.alloc((size_t)cap));
  if (g->live_tags) ICHK(g, kd.alloc((size_t)cap));
  if (g->n) {
    if (g->live_tags) ICHK(g, hipMemcpyAsync(kd.get(), g->d_kind.get(), (size_t)g->n, hipMemcpyDeviceToDevice, g->stream));
    ICHK(g, hipMemcpyAsync(u.get(), g->d_user.get(), sizeof(int64_t) * (size_t)g->n, hipMemcpyDeviceToDevice, g->stream));
    ICHK(g, hipMemcpyAsync(it.get(), g->d_item.get(), sizeof(int64_t) * (size_t)g->n, hipMemcpyDeviceToDevice, g->stream));
    ICHK(g, hipMemcpyAsync(v.get(), g->d_value.get(), sizeof(float) * (size_t)g->n, hipMemcpyDeviceToDevice, g->stream));
    ICHK(g, hipStreamSynchronize(g->stream));
  }
  g->d_user = std::move(u);
  g->d_item = std::move(it);
  g->d_value = std::move(v);
  g->d_kind = std::move(kd);
  return MALS_OK;
}

int alloc_results(mals_ingest g, unsigned n_users, unsigned n_items, unsigned nnz) {
  g->n_users = n_users;
  g->n_items = n_items;
  g->nnz = nnz;
  const size_t nnz1 = std::max<size_t>(nnz, 1);
  ICHK(g, g->ids[0].alloc(std::max<size_t>(n_users, 1)));
  ICHK(g, g->ids[1].alloc(std::max<size_t>(n_items, 1)));
  ICHK(g, g->ptr[0].alloc((size_t)n_users + 1));
  ICHK(g, g->ptr[1].alloc((size_t)n_items + 1));
  for (int sd = 0; sd < 2; ++sd) {
    ICHK(g, g->col[sd].alloc(nnz1));
    ICHK(g, g->val[sd].alloc(nnz1));
  }
  return MALS_OK;
}

// the arena of one sort pipeline over n records (52 bytes per record + digit counts), carved into the views the stages use;
// scan_extra: the longest scan the caller runs beside the pipeline's own
int setup_workspace(mals_ingest g, Scratch& s, int64_t n, int64_t scan_extra) {
  const int64_t n_blocks = (n + RS_BLOCK_TILE - 1) / RS_BLOCK_TILE;
  const int64_t scan_len = std::max<int64_t>(std::max<int64_t>(n, 256 * n_blocks), scan_extra);
  const int64_t tiles = (scan_len + SC_TILE - 1) / SC_TILE + 1;
  const size_t k8 = sizeof(uint64_t) * (size_t)n, k4 = sizeof(unsigned) * (size_t)n;
  const size_t want[mals_ingest_s::N_WS] = {k8, k8, k4, k4, k8, k8, k4, k4, k4, sizeof(unsigned) * (size_t)(256 * n_blocks),
                                            sizeof(unsigned) * (size_t)tiles, sizeof(unsigned long long) * 8 * 256 + 256};
  const auto t0 = std::chrono::steady_clock::now();
  for (int b = 0; b < mals_ingest_s::N_WS; ++b)
    if (want[b] > g->ws[b].capacity()) ICHK(g, g->ws[b].alloc(want[b]));
  g->last_workspace_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  s.keys[0] = (uint64_t*)g->ws[0].get();
  s.keys[1] = (uint64_t*)g->ws[1].get();
  s.pay[0] = (unsigned*)g->ws[2].get();
  s.pay[1] = (unsigned*)g->ws[3].get();
  s.pay64[0] = (uint64_t*)g->ws[4].get();
  s.pay64[1] = (uint64_t*)g->ws[5].get();
  s.head = (unsigned*)g->ws[6].get();
  s.scan = (unsigned*)g->ws[7].get();
  s.ri = (unsigned*)g->ws[8].get();
  s.counts = (unsigned*)g->ws[9].get();
  s.tile_sums = (unsigned*)g->ws[10].get();
  s.digit_tot = (unsigned long long*)g->ws[11].get();
  s.total = (unsigned*)((char*)g->ws[11].get() + sizeof(unsigned long long) * 8 * 256);
  s.keep = (unsigned*)s.pay64[0];
  s.pair_val = (float*)((char*)s.pay64[0] + k4);
  s.coo_row = (int32_t*)s.pay64[1];
  s.present = g->want_known ? (unsigned*)((char*)s.pay64[1] + k4) : nullptr;  // coo_row needs 4 bytes per entry at most
  return MALS_OK;
}

// 0. do the ids of all the ingest's records fit 32 bits?  Then the sorts run on 32-bit keys, and the user ids ride through
//    the first sort so that nothing has to be gathered by record index
struct IdWidth { bool user32, item32; };
int probe_id_width(mals_ingest g, Scratch& s, IdWidth* w) {
  const int64_t n = g->n;
  ICHK(g, hipMemsetAsync(s.digit_tot, 0, 2 * sizeof(unsigned long long), g->stream));
  ITRY(launch_grid(g, {blocks_for(n, 256, 8192)}, ids_high_bits_kernel, g->d_user.get(), n, s.digit_tot));
  ITRY(launch_grid(g, {blocks_for(n, 256, 8192)}, ids_high_bits_kernel, g->d_item.get(), n, s.digit_tot + 1));
  unsigned long long high[2] = {1, 1};
  ICHK(g, hipMemcpyAsync(high, s.digit_tot, sizeof(high), hipMemcpyDeviceToHost, g->stream));
  ICHK(g, hipStreamSynchronize(g->stream));
  const bool narrow = !std::getenv("MALS_INGEST_WIDE_KEYS");   // A/B and test switch
  *w = {high[0] == 0 && narrow, high[1] == 0 && narrow};
  g->bytes_moved += 16.0 * (double)n;
  return MALS_OK;
}

// 1. records sorted by item id (stable: stream order inside an item); dense item rank of every position
template <typename K>
int stage_items(mals_ingest g, Scratch& s, RangeTmp& t, const Records& rec, bool user32, int* ra_out, unsigned* n_i_all) {
  const int64_t n = rec.n;
  K* const kb[2] = {reinterpret_cast<K*>(s.keys[0]), reinterpret_cast<K*>(s.keys[1])};
  ITRY(launch(g, n, user32 ? item_stage_kernel<K, true> : item_stage_kernel<K, false>, rec.item, rec.user, rec.value, n, kb[0], s.pay64[0]));
  g->bytes_moved += (12.0 + (user32 ? 8.0 : 0.0) + sizeof(K) + 8.0) * (double)n;
  int ra = 0;
  ITRY((radix_sort<K, uint64_t>(g, s, kb, s.pay64, n, &ra)));
  ITRY(launch(g, n, heads_kernel<K>, kb[ra], n, s.head));
  ITRY(scan_u32(g, s, s.head, s.scan, n, n_i_all));
  ICHK(g, t.iid_all.alloc(*n_i_all));
  ITRY(launch(g, n, position_ranks_kernel<K>, kb[ra], s.head, s.scan, n, s.ri, t.iid_all.get()));
  g->bytes_moved += (sizeof(K) + 4.0 + sizeof(K) + 8.0 + 4.0) * (double)n;
  *ra_out = ra;
  return MALS_OK;
}

// 2. ... then by user id (stable again): the records are now ordered by (user, item, stream order) -- one sort of the
//    composite key in two stable stages, with the item rank and the value riding along; 3. pair keys
//    (user rank << 32 | item rank) and values in that order.  *r_out = the key buffer that holds the pair keys.
template <typename K>
int stage_users(mals_ingest g, Scratch& s, RangeTmp& t, const Records& rec, int ra, float* sorted_val, int* r_out, unsigned* n_u_all) {
  const int64_t n = rec.n;
  constexpr bool USER32 = sizeof(K) == 4;
  K* const kb[2] = {reinterpret_cast<K*>(s.keys[0]), reinterpret_cast<K*>(s.keys[1])};
  // (reads pay64[ra][i] and writes pay64[0][i]: the same thread, the same index -- safe when ra == 0)
  ITRY(launch(g, n, user_stage_kernel<K, USER32>, rec.user, s.pay64[ra], s.ri, n, kb[0], s.pay64[0]));
  g->bytes_moved += (8.0 + 4.0 + (USER32 ? 0.0 : 8.0) + sizeof(K) + 8.0) * (double)n;
  int rb = 0;
  ITRY((radix_sort<K, uint64_t>(g, s, kb, s.pay64, n, &rb)));
  ITRY(launch(g, n, heads_kernel<K>, kb[rb], n, s.head));
  ITRY(scan_u32(g, s, s.head, s.scan, n, n_u_all));
  ICHK(g, t.uid_all.alloc(*n_u_all));
  const int r = 1 - rb;  // the other key buffer is free now
  ITRY(launch(g, n, pair_from_sorted_kernel<K>, kb[rb], s.pay64[rb], s.head, s.scan, n, s.keys[r], sorted_val, t.uid_all.get()));
  g->bytes_moved += (sizeof(K) + 4.0 + sizeof(K) + 8.0 + 4.0 + 4.0 + 8.0 + 4.0) * (double)n;
  *r_out = r;
  return MALS_OK;
}

// Where the core of a range writes.  The one-shot finish (renumber_items) allocates the ingest's results once the counts
// are known and writes dense item indices at once; a user range of the partitioned finish writes behind the ranges before
// it, into results that exist already, and leaves the columns as range-local item ranks for the merge of the item tables.
struct RangeOut {
  bool renumber_items;
  DeviceBuffer<int64_t>&user_ids, &ptr, &known_ptr;   // live users ascending, offsets into the range's entries / known items
  int64_t entry_base, known_base;                     // the range's first entry in col[0] / val[0], in known_idx
};
struct RangeCounts {
  unsigned n_u_all = 0, n_i_all = 0;           // distinct ids among the records
  unsigned n_users = 0, n_items = 0, nnz = 0;  // ... that still own an entry (n_items: with renumber_items only), entries
  unsigned n_known = 0;
};

// The core of a range of records: 1.-3. the composite sort by key width, 4. the replay of every pair, 5. the ids that still
// own an entry, 6. the surviving entries as rows of R, 6b. knownItemIDs of the range.  t outlives the call: the caller takes
// the range's item table and its liveness from it (iid_all, alive_i) and decides when its buffers go.
int finish_range(mals_ingest g, Scratch& s, RangeTmp& t, const Records& rec, IdWidth w, const RangeOut& out, RangeCounts& c) {
  const int64_t n = rec.n;
  int ra = 0, r = 0;
  float* sorted_val = reinterpret_cast<float*>(s.pay[0]);
  ITRY(w.item32 ? stage_items<uint32_t>(g, s, t, rec, w.user32, &ra, &c.n_i_all) : stage_items<uint64_t>(g, s, t, rec, w.user32, &ra, &c.n_i_all));
  ITRY(w.user32 ? stage_users<uint32_t>(g, s, t, rec, ra, sorted_val, &r, &c.n_u_all) : stage_users<uint64_t>(g, s, t, rec, ra, sorted_val, &r, &c.n_u_all));
  // 4. replay every pair's records in order
  ICHK(g, t.alive_u.alloc(c.n_u_all));
  ICHK(g, t.alive_i.alloc(c.n_i_all));
  ICHK(g, t.new_u.alloc(c.n_u_all));
  if (out.renumber_items) ICHK(g, t.new_i.alloc(c.n_i_all));
  ICHK(g, hipMemsetAsync(t.alive_u.get(), 0, sizeof(unsigned) * (size_t)c.n_u_all, g->stream));
  ICHK(g, hipMemsetAsync(t.alive_i.get(), 0, sizeof(unsigned) * (size_t)c.n_i_all, g->stream));
  ITRY(launch(g, n, replay_pairs_kernel, s.keys[r], sorted_val, n, g->zero_threshold, s.keep, s.pair_val, t.alive_u.get(), t.alive_i.get(), s.present));
  g->bytes_moved += (8.0 + 4.0 + 8.0 + (s.present ? 4.0 : 0.0)) * (double)n;
  // 5. ids that still own an entry, renumbered densely (ascending id)
  ITRY(scan_u32(g, s, t.alive_u.get(), t.new_u.get(), c.n_u_all, &c.n_users));
  if (out.renumber_items) ITRY(scan_u32(g, s, t.alive_i.get(), t.new_i.get(), c.n_i_all, &c.n_items));
  // 6. surviving entries (|value| >= threshold): already sorted by (user, item)
  ITRY(scan_u32(g, s, s.keep, s.scan, n, &c.nnz));
  if (out.renumber_items) {
    ITRY(alloc_results(g, c.n_users, c.n_items, c.nnz));
  } else {
    ICHK(g, out.user_ids.alloc(std::max<size_t>(c.n_users, 1)));
    ICHK(g, out.ptr.alloc((size_t)c.n_users + 1));
  }
  int32_t* col = g->col[0].get() + out.entry_base;
  float* val = g->val[0].get() + out.entry_base;
  ITRY(launch(g, c.n_u_all, compact_ids_kernel, t.uid_all.get(), t.alive_u.get(), t.new_u.get(), (int64_t)c.n_u_all, out.user_ids.get()));
  if (out.renumber_items) {
    ITRY(launch(g, c.n_i_all, compact_ids_kernel, t.iid_all.get(), t.alive_i.get(), t.new_i.get(), (int64_t)c.n_i_all, g->ids[1].get()));
    ITRY(launch(g, n, compact_pairs_kernel, s.keys[r], s.keep, s.scan, s.pair_val, n, t.new_u.get(), t.new_i.get(), s.coo_row, col, val));
  } else {
    ITRY(launch(g, n, big_compact_pairs_kernel, s.keys[r], s.keep, s.scan, s.pair_val, n, t.new_u.get(), s.coo_row, col, val));
  }
  ITRY(launch(g, (int64_t)c.nnz + 1, row_ptr_from_sorted_kernel, s.coo_row, (int64_t)c.nnz, (int64_t)c.n_users, out.ptr.get()));
  g->bytes_moved += 16.0 * (double)n + 16.0 * (double)c.nnz + 8.0 * (double)c.n_users;
  // 6b. knownItemIDs (IFR:173-191): the pairs present at the end of the stream, pruned from R or not, as a CSR over
  //    the same dense indices (its users are exactly the rows of RbyRow, its items rows of RbyColumn)
  if (!g->want_known) return MALS_OK;
  ITRY(scan_u32(g, s, s.present, s.scan, n, &c.n_known));
  ICHK(g, out.known_ptr.alloc((size_t)c.n_users + 1));
  if (out.renumber_items) ICHK(g, g->known_idx.alloc(std::max<size_t>(c.n_known, 1)));
  int32_t* known_row = (int32_t*)s.ri;
  int32_t* known_idx = g->known_idx.get() + out.known_base;
  if (out.renumber_items)
    ITRY(launch(g, n, compact_known_kernel, s.keys[r], s.present, s.scan, n, t.new_u.get(), t.new_i.get(), known_row, known_idx));
  else
    ITRY(launch(g, n, big_compact_pairs_kernel, s.keys[r], s.present, s.scan, nullptr, n, t.new_u.get(), known_row, known_idx, nullptr));
  ITRY(launch(g, (int64_t)c.n_known + 1, row_ptr_from_sorted_kernel, known_row, (int64_t)c.n_known, (int64_t)c.n_users, out.known_ptr.get()));
  g->bytes_moved += (4.0 + 12.0 + 8.0) * (double)n + 12.0 * (double)c.n_known + 8.0 * (double)c.n_users;
  return MALS_OK;
}

// 7. The transposed matrix of m entries whose sort keys (row of R^T << 32 | its column) and value bits the caller has built
//    in (s.keys[0], s.pay[0]), in ascending column order: a STABLE sort on the row half of the key alone leaves the columns
//    ascending inside every row, so the four low digits are not sorted; the row half is a dense index below n_rows: no
//    counting pass.  Then the gather into col / val and the n_rows + 1 row pointers.
int transpose_by_item(mals_ingest g, Scratch& s, int64_t m, int64_t n_rows, int64_t* ptr, int32_t* col, float* val) {
  if (m > 0) {
    int r2 = 0;
    ITRY((radix_sort<uint64_t, unsigned>(g, s, s.keys, s.pay, m, &r2, 4, ((uint64_t)(n_rows > 0 ? n_rows - 1 : 0) << 32) | 0xffffffffull)));
    ITRY(launch(g, m, transpose_gather_kernel, s.keys[r2], s.pay[r2], m, s.coo_row, col, val));
  }
  return launch(g, m + 1, row_ptr_from_sorted_kernel, s.coo_row, m, n_rows, ptr);
}

// 8. tag id sets (IFR:159-165): sorted, unique; 9. userTagIDs as rows of R^T.  sort_cap: what the arena's sort buffers hold
int finish_tags(mals_ingest g, Scratch& s, int64_t sort_cap) {
  for (int which = 0; which < 2; ++which) {
    const int64_t nt = (int64_t)g->n_tags_raw[which];
    if (nt == 0) continue;  // nt <= n: every tag comes from a record
    if (nt > sort_cap) return fail(g, MALS_INVALID_ARG, "ingest: more tag lines than a partition holds records");
    ITRY(launch(g, nt, ids_to_keys_kernel, g->d_tags[which].get(), nt, s.keys[0], s.pay[0]));
    int rt = 0;
    ITRY((radix_sort<uint64_t, unsigned>(g, s, s.keys, s.pay, nt, &rt)));
    ITRY(launch(g, nt, heads_kernel<uint64_t>, s.keys[rt], nt, s.head));
    unsigned n_unique = 0;
    ITRY(scan_u32(g, s, s.head, s.scan, nt, &n_unique));
    ICHK(g, g->tag_ids[which].alloc(n_unique));
    g->n_tag_ids[which] = n_unique;
    ITRY(launch(g, nt, unique_ids_kernel, s.keys[rt], s.head, s.scan, nt, g->tag_ids[which].get()));
  }
  // 9. userTagIDs as rows of R^T: what top-N must never return (RecommendIterator.java:72)
  if (g->n_tag_ids[1] > 0) {
    ICHK(g, g->tag_item_idx.alloc((size_t)g->n_tag_ids[1]));
    ITRY(launch(g, g->n_tag_ids[1], index_of_ids_kernel, g->tag_ids[1].get(), g->n_tag_ids[1], g->ids[1].get(), g->n_items, g->tag_item_idx.get()));
  }
  return MALS_OK;
}

}  // namespace
