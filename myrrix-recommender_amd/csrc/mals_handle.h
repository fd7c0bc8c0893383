// mals_handle.h -- the handle of libmyrrix_als.so as its two host units see it: mals_api.hip (the solver: matrices, work
// lists, Gramian / rows / dual / LDS kernels) and mals_serving.hip (top-N, similarity, rescorers, candidate filter, online
// writes, popular items, generation load).  Host-side headers only: no kernel header comes in through here, so an edit of
// either side's kernels recompiles that side alone.  The types live in a named namespace: mals_handle_s is ONE type.
#pragma once
#include "../../include/myrrix_als.h"
#include "hip_buffer.h"
#include "host_solver.h"
#include "work_plan.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

struct ServingState;   // mals_serving.hip

namespace mals __attribute__((visibility("hidden"))) {

struct SideState {
  // factor replica
  int64_t n_total = 0;
  float* F = nullptr;           // F_own, or the caller's block (mals_bind_factors)
  DeviceBuffer<float> F_own;
  // local matrix shard
  int64_t row_offset = 0, n_local = 0, nnz = 0;
  int64_t* row_ptr = nullptr;   // the *_own blocks, or the caller's (mals_set_matrix from device memory)
  int32_t* col = nullptr;
  float* val = nullptr;
  DeviceBuffer<int64_t> row_ptr_own;
  DeviceBuffer<int32_t> col_own;
  DeviceBuffer<float> val_own;
  bool has_matrix = false;
  std::vector<int64_t> h_row_ptr;  // host copy (work-list construction, chunked upload)
  int64_t append_rows = 0, append_nnz = 0;
  bool appending = false;
  // work lists
  DeviceBuffer<WorkItem> itemsA;  // rows no longer than segment_nnz, longest first
  DeviceBuffer<WorkItem> itemsB;  // segments of the long rows, longest first; behind them the chunk's banded segments
                                  // (band_plan.h), band by band
  DeviceBuffer<RowC> rowsC;
  DeviceBuffer<float> scratch;
  DeviceBuffer<uint8_t> refine;   // per local row: marked for als_refine_kernel by the kernel that solved it
  int32_t col_min = 0, col_max = -1;  // range of the column indices (checked against the opposite replica)
  float max_abs_val = 0.f;  // bound on |value| used for the operand scale (>= local_max_abs_val)
  float local_max_abs_val = 0.f;  // largest |value| of the shard
  double mean_abs_val = 0.0;      // mean |value| used by the operand-range check (all shards if the caller synced it)
  double local_mean_abs_val = 0.0;  // mean |value| of the shard
  // the lists are stored chunk-major, each chunk sorted by length (work_plan.h: ChunkRange)
  int64_t n_dual_rows = 0;
  bool band_front = true;  // the banded segments run as one front (one segment per wave) instead of the strided grid
  int64_t chunk_rows_override = -1;  // mals_set_chunk_rows: per-side value of cfg.chunk_rows (-1 = use cfg)
  std::vector<ChunkRange> chunks;
  // Gramian of THIS side's factors (consumed when solving the other side)
  DeviceBuffer<double> G;
  DeviceBuffer<float> Gf;
  DeviceBuffer<uint8_t> partials;   // wave / slab partials of K1 (doubles, or floats for the split kernel)
  bool G_valid = false;
  uint64_t G_version = 0;  // bumped whenever G changes (cached operand scale of the split-precision gather)
  DeviceBuffer<unsigned> d_ymax;  // bit pattern of max |element| over the rows G was formed from, recorded by the Gramian kernels
  uint64_t ymax_version = 0;   // the G_version d_ymax belongs to (0 = none: G came from outside, gather_scale_kernel then
                               // bounds |y| by sqrt(max_f G_ff))
  uint64_t F_epoch = 0;    // bumped whenever the library itself writes the replica (uploads, solves, rebinding)
};

// the candidate filter of mals_recommend* (mals_lsh_build; kernels in lsh_kernels.h): LocationSensitiveHash.java as built
// for one generation -- the signatures are a snapshot of Y at build time (the reference buckets once per generation)
struct LshState {
  int H = 0;              // num_hashes; 0: no filter, every item a candidate
  int mb = 0;             // maxBitsDiffering (may be -1)
  int64_t n_signed = 0;   // rows of Y signed at build time; later rows (mals_grow_factor_rows) are new items: always candidates
  DeviceBuffer<uint64_t> d_sig;    // [n_signed]
  DeviceBuffer<uint64_t> d_mask;   // [features]: bit h = randomVectors[h][f]
  DeviceBuffer<double> d_mean;     // [features]
  // queries answered with the filter on, by the bf16 filter path / by the dense path (mals_lsh_info)
  std::atomic<int64_t> q_filter{0}, q_dense{0};
  void clear() {
    H = 0;
    mb = 0;
    n_signed = 0;
    d_sig.reset();
    d_mask.reset();
    d_mean.reset();
  }
};

struct HalfStamp {  // what a cache that is rebuilt once per half-iteration holds: the solved side, the OPPOSITE side's G_version
  int side = -1;
  uint64_t version = 0;
  bool operator==(const HalfStamp& o) const { return side == o.side && version == o.version; }
  bool operator!=(const HalfStamp& o) const { return !(*this == o); }
};

struct PendingEvent {
  EventPair ev;   // around the launch; created per timed launch (begin_timed), empty while timing is off
  int kind;  // 0 = rows, 1 = segments, 2 = finish, 3 = gramian, 4 = dual, 5 = rotate
  double bytes;
};

}  // namespace mals
using namespace mals;   // (both units are written in it)

struct mals_handle_s {
  mals_config cfg;
  int T = 0;
  bool split_f16 = false;  // cfg.gramian_mode resolved
  bool split3 = false;     // MALS_GRAMIAN_SPLIT3_F16: three f16 terms per operand (features 49..64)
  int dual_blocks = 0;     // cfg.solve_mode resolved: rows up to 16*dual_blocks entries go to the dual lists (0 = none)
  // dual path state (dual_kernels.h): rotated copy of the gathered factor matrix, Q / Q^T / eigenvalues
  DeviceBuffer<float> d_Mr;
  // gather table of the direct kernels when features % 16 != 0: zero-padded copy of the gathered factor matrix
  // (pad_rows_kernel), rebuilt once per half-iteration
  DeviceBuffer<float> d_Mp;
  // mixed-precision refinement of ill-conditioned rows (als_refine_kernel): estimate above which a row is re-solved
  // (MALS_REFINE_LIMIT / mals_set_refine_limit; 0 = off), rows refined so far (device counter)
  float refine_limit = 64.f;
  bool exact_ready = false;   // als_exact_kernel's dynamic LDS limit raised
  DeviceBuffer<int> d_gref_state;   // {a row was marked in this half-iteration, Gref is valid, arrival ticket}
  DeviceBuffer<double> d_Gref;      // the reference-rounded Gramian of the gathered side (gramian_ref_kernel), on demand
  DeviceBuffer<double> d_gref_part;
  DeviceBuffer<unsigned long long> d_refined;
  HalfStamp pad;              // what the copy holds, and the factor-upload count of the opposite side at the time of the copy
  uint64_t pad_epoch = 0;
  std::vector<uint8_t> pad_done;  // chunks solved from the current copy: solving one again starts a new half-iteration
  DeviceBuffer<char> d_eig;   // device image of eig_stage; the four pointers below are views into it
  double* d_Q = nullptr;      // [2][16T][16T]: Q (k x 16T, zero padded) and Q^T
  float* d_Qf = nullptr;      // the same in fp32
  bool rotate_f64 = false;    // this half-iteration's forward rotation runs on the fp64 matrix cores
  bool rotate_split = false;  // k % 8 == 0: rotations on the f16 matrix pipe with split operands
  int32_t* d_Bs = nullptr;    // [2][KC][T][2][64][4]: Q and Q^T as split-f16 B operands
  size_t Bs_stride = 0;
  float* d_lam = nullptr;     // [2][16T]: eigenvalues, 1/sqrt(L + lambda alpha)
  DeviceBuffer<unsigned> d_zbound;
  PinnedBuffer<double> h_G;   // k x k
  Event ev_G;
  // host half of the dual preparation: the eigendecomposition of G turned into what the device half uploads, in ONE
  // pinned block (asynchronous copies straight out of it, no stream synchronisation): Q | Q^T (doubles), the same in
  // fp32, eigenvalues | 1/sqrt(L + lambda alpha), and Q / Q^T as split-f16 B operands
  PinnedBuffer<char> eig_stage;
  bool eig_ok = false;        // the staged decomposition qualifies for the dual path
  double eig_gmax = 0.0;      // max_f G_ff of the decomposed Gramian
  bool dual_pending = false;  // a chunk's direct kernels are enqueued, its dual part waits for the eigendecomposition
  int dual_pending_side = -1, dual_pending_chunk = -1;
  double tl[4] = {0.0, 0.0, 0.0, 0.0};  // mals_get_timeline
  HalfStamp dual;             // what the rotated copy currently holds
  bool dual_ok = false;       // the half-iteration's systems qualify for the dual path
  // k = 128 with the split-precision gather: the rows / segments kernels that stage the gather through LDS (lds_kernels.h)
  // and the Gramian image in their feature order (all zeros under lossIgnoresUnspecified), rebuilt when the opposite
  // side's Gramian changes
  // Chunks of one half-iteration on alternating streams (mals_group.cpp): ev_ready = everything the half-iteration sets up
  // once, in its first chunk (operand scale, padded / permuted images, the rotated copy of the dual path), is enqueued
  // behind it -- a later chunk on the OTHER stream waits for it; ev_refine serialises the chunks' refinement blocks
  // (gramian_ref_kernel's arrival ticket assumes one launch at a time)
  Event ev_ready, ev_refine;
  bool refine_recorded = false;
  mals_iteration_fn iter_fn = nullptr;   // mals_set_iteration_callback
  void* iter_user = nullptr;
  bool lds_gather = false;
  DeviceBuffer<float> d_Gperm;
  HalfStamp gperm;
  DeviceBuffer<float> d_zscale;  // {S, 1/S^2} of the split-precision gather (gather_scale_kernel)
  HalfStamp zs;               // what d_zscale currently holds, with the value bound and mean it was computed from
  float zs_bound = -1.f;
  double zs_mean = -1.0;
  DeviceBuffer<unsigned> d_maxabs;
  DeviceBuffer<int> d_colrange;
  int n_cu = 256;
  SideState side[2];
  hipStream_t stream = nullptr;   // borrowed (mals_set_stream), or the null stream
  // The three independent parts of a chunk -- rows list, long rows (segments + finish), dual lists (rotation + dual
  // kernels) -- are enqueued on three streams between a fork and a join event: the small launches (a few hundred
  // workgroups: the long rows of C2, the dual classes, the rotations) fill the slots the rows kernel's tail leaves
  // instead of each paying its own ramp-up and tail.  Measured (round 3, same box, one stream vs three): C2 2.22 ->
  // 2.18 ms, C4 81.8 -> 80.6, C5 rank 168.8 -> 165.3, C3 14.8 -> 15.3 (worse: its long rows then fight the rows
  // kernel for the cache-resident table) -- 1-2 %, and every per-kernel HIP-event time (the roofline figures of
  // mals_stats) then includes the other streams' contention.  So: OFF unless MALS_OVERLAP=1.
  Stream aux[2];
  Event ev_fork, ev_join[2];
  bool overlap = false;
  bool forked[2] = {false, false};
  std::string err;
  DeviceBuffer<unsigned long long> d_bad;   // [4]: first non-PD row per side, then the smallest-pivot suspect per side
  PinnedBuffer<unsigned long long> h_bad;
  int32_t sing_side = -1;
  int64_t sing_row = -1;
  int32_t sing_rank = 0;
  std::atomic<int> cancelled{0};
  bool timing = false;
  mals_stats stats;
  std::vector<PendingEvent> pending;
  DeviceBuffer<unsigned long long> d_trace;  // MALS_DEBUG_TRACE
  ServingState* serving = nullptr;   // top-N workspace and front, write path, popular items, generation (mals_serving.hip)
  // userTagIDs as one bit per item (mals_set_tag_items): never recommended (RecommendIterator.java:72)
  DeviceBuffer<uint32_t> tag_bits;
  int64_t tag_bits_items = 0, n_tag_items = 0;
  // knownItemIDs (mals_set_known_items): what mals_recommend skips instead of the rows of R when present
  const int64_t* known_ptr = nullptr;   // the *_copy blocks, or the caller's (device memory)
  const int32_t* known_idx = nullptr;
  int64_t known_rows = 0;
  DeviceBuffer<int64_t> known_ptr_copy;   // copies of host arrays
  DeviceBuffer<int32_t> known_idx_copy;
  DeviceBuffer<double> d_sd;       // mals_sample_dots: estimates, indices
  DeviceBuffer<int64_t> d_sd_idx;
  DeviceBuffer<int64_t> d_idx;  // gather scratch
  DeviceBuffer<float> d_rows;
  LshState lsh;                 // the candidate filter of mals_recommend* (mals_lsh_build)
  bool group_member = false;    // a member of a mals_group (malsi_mark_group_member): the write path refuses it
  // mals_foldin_stats: applied, failed, large fold-ins, levels, device ns (all calls), device ns (last call) -- atomics,
  // read without a ticket
  std::atomic<int64_t> foldin_counters[6] = {};
  // one past the last user row mals_grow_factor_rows added to this handle's users (-1: none); read by request threads
  std::atomic<int64_t> grown_users_end{-1};
  // mals_most_popular_items (popular_host.h): the counter every call that may change a counted user's set bumps
  // (popular_touch), the same for the base CSR alone, and mals_most_popular_stats
  std::atomic<uint64_t> pop_epoch{1}, pop_base_epoch{1};
  std::atomic<int64_t> popular_counters[4] = {};
};

// mals_solver_* (mals_api.hip); the write path uploads its factors (mals_set_foldin_solver, mals_serving.hip)
struct mals_solver_s {
  mals::PivotedQR qr;
};

static inline int fail(mals_handle h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

#define HIPCHK(h, call)                                                                     \
  do {                                                                                      \
    hipError_t _e = (call);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      const int _code = (_e == hipErrorOutOfMemory) ? MALS_OOM : MALS_HIP_ERROR;            \
      return fail(h, _code, std::string(#call) + ": " + hipGetErrorString(_e));             \
    }                                                                                       \
  } while (0)

#define CHECK_SIDE(h, side)                                                  \
  do {                                                                       \
    if (!(h)) return MALS_INVALID_ARG;                                       \
    if ((side) != MALS_SIDE_X && (side) != MALS_SIDE_Y)                      \
      return fail(h, MALS_INVALID_ARG, "side must be MALS_SIDE_X or _Y");    \
  } while (0)

static inline int use_device(mals_handle h) {
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return MALS_OK;
}

// a side without its matrix shard and work lists (the matrix setters; mals_load_generation: the rows of R named live rows)
static inline void free_matrix(SideState& s) {
  s.row_ptr_own.reset();
  s.col_own.reset();
  s.val_own.reset();
  s.row_ptr = nullptr;
  s.col = nullptr;
  s.val = nullptr;
  s.has_matrix = false;
  s.itemsA.reset();
  s.itemsB.reset();
  s.rowsC.reset();
  s.scratch.reset();
  s.refine.reset();
  s.chunks.clear();
  s.h_row_ptr.clear();
  s.h_row_ptr.shrink_to_fit();
}

// popular_host.h: what mals_most_popular_items counted is stale (base: the base CSR itself is another one)
static inline void popular_touch(mals_handle h, bool base) {
  h->pop_epoch.fetch_add(1, std::memory_order_acq_rel);
  if (base) h->pop_base_epoch.fetch_add(1, std::memory_order_acq_rel);
}

// What mals_api.hip calls of mals_serving.hip (NOT part of the C-ABI, like mals_internal.h).  mals_create / mals_destroy:
// the serving state with its front (MALS_TOPN_FRONT_DEPTH, MALS_TOPN_FRONT_SPIN_US); the front goes before the handle's
// stream is synchronised, the rest -- workspace, write path, popular items, generation -- last, with the device current.
extern "C" {
__attribute__((visibility("hidden"))) void malsi_serving_create(mals_handle h);
__attribute__((visibility("hidden"))) void malsi_serving_stop_front(mals_handle h);
__attribute__((visibility("hidden"))) void malsi_serving_free(mals_handle h);
// the matrix and factor setters: a new generation's known items (overlay, installed known items and popular counts go),
// new user rows (popular_new_generation), new factor rows (generation_drop_recent; ids_drop: their ids are not the old rows')
__attribute__((visibility("hidden"))) void malsi_clear_known_items(mals_handle h);
__attribute__((visibility("hidden"))) void malsi_popular_new_generation(mals_handle h, bool new_rows);
__attribute__((visibility("hidden"))) void malsi_generation_drop_recent(mals_handle h, int side);
__attribute__((visibility("hidden"))) void malsi_ids_drop(mals_handle h, int side);
}
