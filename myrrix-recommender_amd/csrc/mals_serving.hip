// mals_serving.hip -- the serving side of libmyrrix_als.so: the calls of include/myrrix_als.h that read and write a live
// model on the handle's GPU -- mals_recommend* and the similarity calls through the serving front (topn_host.h), rescorers,
// the candidate filter, the online writes and fold-in reads with their group forms (foldin_host.h), mals_most_popular_items
// (popular_host.h), mals_load_generation (generation_host.h), mals_factor_digest.  The handle and what the solver's unit
// (mals_api.hip) calls of this one: mals_handle.h.  No solver kernel header is included here, and no serving kernel header
// there: an edit on one side does not recompile the other.
#include "../../include/myrrix_als.h"
#include "topn_kernels.h"
#include "foldin_kernels.h"
#include "popular_kernels.h"
#include "generation_kernels.h"
#include "ids_kernels.h"
#include "generation_group_kernels.h"
#define MALS_FACTOR_DIGEST_KERNEL
#include "factor_digest.h"
#include "mals_internal.h"
#include "mals_handle.h"
#include "foldin_plan.h"
#include "ingest_live_plan.h"
#include "generation_group_plan.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

using namespace mals;

namespace {
struct TopnWorkspace;
struct TopnFront;
struct FoldinState;
struct PopularState;
struct GenerationState;
struct IdsState;
}  // namespace

// What a handle holds of this unit (mals_handle_s::serving), made by mals_create and freed by mals_destroy.  The front lives
// as long as the handle serves; the others are made by the first call that needs them (a pass of topn_host.h, foldin_state,
// popular_state, generation_state).
struct ServingState {
  TopnWorkspace* tn_ws = nullptr;     // top-N workspace (topn_host.h), grow-only
  TopnFront* tn_front = nullptr;      // the serving front of mals_recommend*: queue, leader, passes in flight (topn_host.h)
  FoldinState* fo = nullptr;          // the online write path (foldin_host.h): device solvers, known-item overlay, levels
  PopularState* pop = nullptr;        // mals_most_popular_items (popular_host.h): the count cache and the tag users
  GenerationState* gen = nullptr;     // mals_load_generation (generation_host.h): the recent rows, the ids and maps of the last load
  IdsState* ids = nullptr;            // the id directory of mals_ids_* and mals_ingest_apply (ids_host.h): row -> id, id -> row per side
};

// ---- rescorers (mals_rescorer_*, include/myrrix_als.h; the kernels' side in topn_kernels.h, RESCORED MODE) ---------------
// What a pass reads is an immutable snapshot: mals_rescorer_set_* builds a new one (an exclusive ticket of the serving front,
// so every call sees the rescorer as it was when the call was queued) and passes in flight keep the one they were formed with.
struct RescorerState {
  // the caller's definition (host copies: the next set_* rebuilds from them)
  std::vector<int64_t> filt_idx;         // sorted, unique
  std::vector<double> scale, offset;     // per-item weights (either may be empty), rows [0, n_rows)
  int64_t n_rows = 0;
  double us = 1.0, uo = 0.0;             // the uniform weights of every other row (mals_rescorer_set_uniform)
  // on the device
  DeviceBuffer<uint32_t> d_filt;
  DeviceBuffer<double> d_scale, d_offset;
  DeviceBuffer<uint4> d_fdata;
  TopnRescore args;
  bool filter_ok = true;                 // every weight inside the filter's range (topn_kernels.h), else the dense path answers
  bool cos_filter_ok = true;             // ... inside the narrower range of RESCORED COSINE MODE (mals_most_similar_items_rescored)
};
struct mals_rescorer_s {
  mals_handle h = nullptr;
  std::shared_ptr<const RescorerState> st;
};

namespace {
bool rescorer_filter_ok(const mals_rescorer_s* r) { return r->st->filter_ok; }
bool rescorer_cos_filter_ok(const mals_rescorer_s* r) { return r->st->cos_filter_ok; }
void rescorer_bind(const mals_rescorer_s* r, std::shared_ptr<const RescorerState>& keep, TopnRescore& args) {
  keep = r->st;
  args = keep->args;
}
}  // namespace

namespace {
// foldin_host.h (included after topn_host.h, which reads the known-item overlay through these)
bool foldin_known_view(mals_handle h, int64_t local_row, std::vector<int64_t>& out);
bool foldin_has_overlay(mals_handle h);
int foldin_known_full(mals_handle h, const std::vector<int64_t>& rows, std::vector<std::vector<int32_t>>& outs, std::string& msg);
#include "topn_host.h"

// (a failed argument check of a recommend call: the message under the front's mutex -- other request threads may be
// inside the same handle)
int topn_fail(mals_handle h, int code, const char* msg) {
  std::lock_guard<std::mutex> lk(topn_front(h)->mu);
  h->err = msg;
  return code;
}

// generation_host.h (included after foldin_host.h, whose writes mark their rows recent through this)
void generation_mark_pairs(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* item_row);
#include "foldin_host.h"
#include "popular_host.h"
#include "ids_host.h"
#include "generation_host.h"
#include "generation_group_host.h"
}  // namespace

// ---- what mals_api.hip calls of this unit (mals_handle.h) ------------------------------------------------------------------
void malsi_serving_create(mals_handle h) {
  h->serving = new ServingState();
  h->serving->tn_front = new TopnFront();
  if (const char* e = std::getenv("MALS_TOPN_FRONT_DEPTH")) topn_front(h)->depth = std::max(1, std::min(TOPN_SLOTS, std::atoi(e)));
  if (const char* e = std::getenv("MALS_TOPN_FRONT_SPIN_US")) topn_front(h)->spin_us = std::max(0, std::atoi(e));
}

void malsi_serving_stop_front(mals_handle h) {
  delete topn_front(h);
  h->serving->tn_front = nullptr;
}

void malsi_serving_free(mals_handle h) {
  topn_free(h);
  foldin_free(h);
  popular_free(h);
  generation_free(h);
  ids_free(h);
  delete h->serving;
  h->serving = nullptr;
}

void malsi_clear_known_items(mals_handle h) {
  foldin_drop_overlay(h);   // a new generation's known items: the writes of the old one are gone with it
  popular_new_generation(h, false);   // ... and so is what mals_most_popular_items counted
  h->known_ptr_copy.reset();
  h->known_idx_copy.reset();
  h->known_ptr = nullptr;
  h->known_idx = nullptr;
  h->known_rows = 0;
}

void malsi_popular_new_generation(mals_handle h, bool new_rows) { popular_new_generation(h, new_rows); }
void malsi_generation_drop_recent(mals_handle h, int side) { generation_drop_recent(h, side); }
void malsi_ids_drop(mals_handle h, int side) { ids_drop(h, side); }

extern "C" {

// the last checks of a call that scores items: the tag items fit the catalogue, the calling thread is on the handle's device
static int topn_serving_ready(mals_handle h) {
  if (h->tag_bits.get() && h->tag_bits_items != h->side[MALS_SIDE_Y].n_total)
    return topn_fail(h, MALS_INVALID_ARG, "the tag items were set for another item count: call mals_set_tag_items again");
  if (hipSetDevice(h->cfg.device) != hipSuccess) return topn_fail(h, MALS_HIP_ERROR, "hipSetDevice failed");
  return MALS_OK;
}

static int topn_recommend_once(mals_handle h, mals_rescorer r, const int64_t* user_idx, int32_t n_queries, int32_t how_many,
                               int32_t consider_known_items, int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  if (!h) return MALS_INVALID_ARG;
  if (r && r->h != h) return topn_fail(h, MALS_INVALID_ARG, "the rescorer belongs to another handle");
  SideState& x = h->side[MALS_SIDE_X];
  SideState& y = h->side[MALS_SIDE_Y];
  if (!x.F || !y.F || y.n_total == 0) return topn_fail(h, MALS_INVALID_ARG, "factor replicas not available");
  if (n_queries < 0 || how_many <= 0 || how_many > 4096 || (n_queries > 0 && (!user_idx || !item_idx_out || !score_out)))
    return topn_fail(h, MALS_INVALID_ARG, "bad recommend arguments (how_many in 1..4096)");
  if (!consider_known_items && !x.has_matrix && !h->known_ptr)
    return topn_fail(h, MALS_INVALID_ARG, "the user-side matrix (or mals_set_known_items) is needed to skip known items");
  if (!consider_known_items && h->known_ptr && h->known_rows != x.n_local)
    return topn_fail(h, MALS_INVALID_ARG, "the installed known items do not match the local user rows");
  for (int q = 0; q < n_queries; ++q) {
    if (user_idx[q] < 0 || user_idx[q] >= x.n_total) return topn_fail(h, MALS_INVALID_ARG, "user index outside the factor replica");
    if (!consider_known_items && (user_idx[q] < x.row_offset || user_idx[q] >= foldin_user_rows_end(h)))
      return topn_fail(h, MALS_INVALID_ARG, "known items of this user are not on this handle (row outside the local shard)");
  }
  if (n_queries == 0) return MALS_OK;
  if (int rc = topn_serving_ready(h)) return rc;
  TopnRequest rq;
  rq.n_queries = n_queries;
  rq.how_many = how_many;
  rq.user_idx = user_idx;
  rq.skip_known = !consider_known_items;
  rq.item_idx_out = item_idx_out;
  rq.score_out = score_out;
  rq.n_out = n_out;
  rq.rescorer = r;
  return topn_front_submit(h, rq, n_queries < TOPN_FRONT_BULK && how_many <= TOPN_FILTER_MAX_N);
}
static int topn_recommend_impl(mals_handle h, mals_rescorer r, const int64_t* user_idx, int32_t n_queries, int32_t how_many,
                               int32_t consider_known_items, int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  return topn_generation_guard(h, [&]() -> int { return topn_recommend_once(h, r, user_idx, n_queries, how_many, consider_known_items, item_idx_out, score_out, n_out); });
}

int mals_recommend(mals_handle h, const int64_t* user_idx, int32_t n_queries, int32_t how_many, int32_t consider_known_items,
                   int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  return topn_recommend_impl(h, nullptr, user_idx, n_queries, how_many, consider_known_items, item_idx_out, score_out, n_out);
}

int mals_set_known_items(mals_handle h, int64_t n_rows, const int64_t* row_ptr, const int32_t* item_idx, int mem_kind) {
  if (!h) return MALS_INVALID_ARG;
  if (mem_kind != MALS_MEM_HOST && mem_kind != MALS_MEM_DEVICE) return fail(h, MALS_INVALID_ARG, "mem_kind must be MALS_MEM_HOST or MALS_MEM_DEVICE");
  if (int rc = use_device(h)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  malsi_clear_known_items(h);
  if (!row_ptr) return MALS_OK;  // back to the rows of R
  SideState& x = h->side[MALS_SIDE_X];
  if (n_rows != x.n_local) return fail(h, MALS_INVALID_ARG, "known items: one row per local user row of side X");
  if (mem_kind == MALS_MEM_DEVICE) {
    h->known_ptr = row_ptr;
    h->known_idx = item_idx;
  } else {
    const int64_t n = row_ptr[n_rows];
    if (n < 0 || (n > 0 && !item_idx)) return fail(h, MALS_INVALID_ARG, "bad known-item arrays");
    HIPCHK(h, h->known_ptr_copy.alloc((size_t)(n_rows + 1)));
    HIPCHK(h, h->known_idx_copy.alloc((size_t)std::max<int64_t>(n, 1)));
    HIPCHK(h, hipMemcpy(h->known_ptr_copy.get(), row_ptr, sizeof(int64_t) * (size_t)(n_rows + 1), hipMemcpyHostToDevice));
    if (n) HIPCHK(h, hipMemcpy(h->known_idx_copy.get(), item_idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    h->known_ptr = h->known_ptr_copy.get();
    h->known_idx = h->known_idx_copy.get();
  }
  h->known_rows = n_rows;
  return MALS_OK;
}

int mals_set_tag_items(mals_handle h, int64_t n, const int64_t* item_idx, int mem_kind) {
  if (!h) return MALS_INVALID_ARG;
  if (mem_kind != MALS_MEM_HOST && mem_kind != MALS_MEM_DEVICE) return fail(h, MALS_INVALID_ARG, "mem_kind must be MALS_MEM_HOST or MALS_MEM_DEVICE");
  if (n < 0 || (n > 0 && !item_idx)) return fail(h, MALS_INVALID_ARG, "bad tag item list");
  if (int rc = use_device(h)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->tag_bits.reset();
  h->tag_bits_items = h->n_tag_items = 0;
  if (n == 0) return MALS_OK;
  const int64_t n_items = h->side[MALS_SIDE_Y].n_total;
  if (n_items <= 0) return fail(h, MALS_INVALID_ARG, "tag items: the item factor replica comes first (mals_set_factor_rows)");
  const size_t words = ((size_t)((n_items + 31) / 32) + 1) & ~(size_t)1;   // even: the counter behind them is 8-byte aligned
  DeviceBuffer<uint32_t> bits;   // the words, then the counter
  HIPCHK(h, bits.alloc(words + sizeof(unsigned long long) / sizeof(uint32_t)));
  unsigned long long* d_n = reinterpret_cast<unsigned long long*>(bits.get() + words);
  HIPCHK(h, hipMemsetAsync(bits.get(), 0, sizeof(uint32_t) * words + sizeof(unsigned long long), h->stream));
  DeviceBuffer<int64_t> d_idx;
  const int64_t* src = item_idx;
  if (mem_kind == MALS_MEM_HOST) {
    HIPCHK(h, d_idx.alloc((size_t)n));
    HIPCHK(h, hipMemcpyAsync(d_idx.get(), item_idx, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    src = d_idx.get();
  }
  hipLaunchKernelGGL(topn_tag_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, src, n, n_items, bits.get(), d_n);
  unsigned long long n_set = 0;
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&n_set, d_n, sizeof(n_set), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  d_idx.reset();
  if (e != hipSuccess) return fail(h, MALS_HIP_ERROR, std::string("mals_set_tag_items: ") + hipGetErrorString(e));
  if (n_set == 0) return MALS_OK;  // none of them owns a row of Y: nothing to strike
  h->tag_bits = std::move(bits);
  h->tag_bits_items = n_items;
  h->n_tag_items = (int64_t)n_set;
  return MALS_OK;
}

int mals_get_tag_item_count(mals_handle h, int64_t* n_out) {
  if (!h || !n_out) return MALS_INVALID_ARG;
  *n_out = h->n_tag_items;
  return MALS_OK;
}

static int topn_to_many_once(mals_handle h, mals_rescorer r, const float* vectors, const int64_t* vector_ptr, int32_t n_queries, int32_t how_many,
                             const int64_t* exclude_ptr, const int64_t* exclude_idx, int64_t* item_idx_out, float* score_out,
                             int32_t* n_out) {
  if (!h) return MALS_INVALID_ARG;
  if (r && r->h != h) return topn_fail(h, MALS_INVALID_ARG, "the rescorer belongs to another handle");
  SideState& y = h->side[MALS_SIDE_Y];
  if (!y.F || y.n_total == 0) return topn_fail(h, MALS_INVALID_ARG, "item factor replica not available");
  if (n_queries < 0 || how_many <= 0 || how_many > 4096 || (n_queries > 0 && (!vectors || !item_idx_out || !score_out)))
    return topn_fail(h, MALS_INVALID_ARG, "bad recommend arguments (how_many in 1..4096)");
  if ((exclude_ptr == nullptr) != (exclude_idx == nullptr) && exclude_ptr && exclude_ptr[n_queries] > 0)
    return topn_fail(h, MALS_INVALID_ARG, "exclude_ptr and exclude_idx go together");
  if (vector_ptr) {
    if (vector_ptr[0] != 0) return topn_fail(h, MALS_INVALID_ARG, "vector_ptr[0] must be 0");
    for (int q = 0; q < n_queries; ++q) {
      const int64_t n = vector_ptr[q + 1] - vector_ptr[q];
      if (n < 1) return topn_fail(h, MALS_INVALID_ARG, "features must not be empty");  // RecommendIterator.java:52
      if (n > (1 << 20)) return topn_fail(h, MALS_INVALID_ARG, "too many vectors in one query");
    }
  }
  if (n_queries == 0) return MALS_OK;
  if (int rc = topn_serving_ready(h)) return rc;
  TopnRequest rq;
  rq.n_queries = n_queries;
  rq.how_many = how_many;
  rq.vectors = vectors;
  rq.vec_ptr = vector_ptr;
  rq.excl_ptr = exclude_ptr;
  rq.excl_idx = exclude_idx;
  rq.item_idx_out = item_idx_out;
  rq.score_out = score_out;
  rq.n_out = n_out;
  rq.rescorer = r;
  const int64_t n_vec = vector_ptr ? vector_ptr[n_queries] : (int64_t)n_queries;
  const int64_t n_ex = (exclude_ptr && exclude_idx) ? exclude_ptr[n_queries] - exclude_ptr[0] : 0;
  // a small call (an anonymous user, recommendToMany for a handful of users) is folded into a pass with the other callers'
  return topn_front_submit(h, rq, n_queries < TOPN_FRONT_BULK && how_many <= TOPN_FILTER_MAX_N && n_vec <= 4 * TOPN_FRONT_BULK && n_ex <= (1 << 16) &&
                                      (!exclude_ptr || exclude_ptr[0] == 0));
}
static int topn_to_many_impl(mals_handle h, mals_rescorer r, const float* vectors, const int64_t* vector_ptr, int32_t n_queries, int32_t how_many,
                             const int64_t* exclude_ptr, const int64_t* exclude_idx, int64_t* item_idx_out, float* score_out,
                             int32_t* n_out) {
  return topn_generation_guard(h, [&]() -> int { return topn_to_many_once(h, r, vectors, vector_ptr, n_queries, how_many, exclude_ptr, exclude_idx, item_idx_out, score_out, n_out); });
}

int mals_recommend_to_many(mals_handle h, const float* vectors, const int64_t* vector_ptr, int32_t n_queries, int32_t how_many,
                           const int64_t* exclude_ptr, const int64_t* exclude_idx, int64_t* item_idx_out, float* score_out,
                           int32_t* n_out) {
  return topn_to_many_impl(h, nullptr, vectors, vector_ptr, n_queries, how_many, exclude_ptr, exclude_idx, item_idx_out, score_out, n_out);
}

int mals_recommend_vectors(mals_handle h, const float* query_vectors, int32_t n_queries, int32_t how_many,
                           const int64_t* exclude_ptr, const int64_t* exclude_idx, int64_t* item_idx_out, float* score_out,
                           int32_t* n_out) {
  return mals_recommend_to_many(h, query_vectors, nullptr, n_queries, how_many, exclude_ptr, exclude_idx, item_idx_out, score_out, n_out);
}

// ---- item-to-item similarity (topn_kernels.h, cosine mode): through the same serving front as mals_recommend* ----------
static int topn_check_items(mals_handle h, const int64_t* idx, int64_t n) {
  const int64_t n_items = h->side[MALS_SIDE_Y].n_total;
  for (int64_t i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= n_items) return topn_fail(h, MALS_INVALID_ARG, "item index outside the item factor replica");
  return MALS_OK;
}

static int topn_most_similar_once(mals_handle h, mals_rescorer r, int32_t flags, const int64_t* item_idx, const int64_t* item_ptr, int32_t n_queries,
                                  int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  if (!h) return MALS_INVALID_ARG;
  if (r && r->h != h) return topn_fail(h, MALS_INVALID_ARG, "the rescorer belongs to another handle");
  if (flags & ~MALS_SIMILAR_FILTER_QUERY_ITEMS) return topn_fail(h, MALS_INVALID_ARG, "unknown mostSimilarItems flags");
  if (r && h->group_member) return topn_fail(h, MALS_INVALID_ARG, "rescorers are not available on the members of a group");
  SideState& y = h->side[MALS_SIDE_Y];
  if (!y.F || y.n_total == 0) return topn_fail(h, MALS_INVALID_ARG, "item factor replica not available");
  if (n_queries < 0 || how_many <= 0 || how_many > 4096 || (n_queries > 0 && (!item_idx || !item_idx_out || !score_out)))
    return topn_fail(h, MALS_INVALID_ARG, "bad mostSimilarItems arguments (how_many in 1..4096)");
  std::vector<int64_t> one_each;
  if (item_ptr) {
    if (n_queries > 0 && item_ptr[0] != 0) return topn_fail(h, MALS_INVALID_ARG, "item_ptr[0] must be 0");
    for (int q = 0; q < n_queries; ++q) {
      const int64_t n = item_ptr[q + 1] - item_ptr[q];
      if (n < 1) return topn_fail(h, MALS_INVALID_ARG, "every query needs at least one item");
      if (n > (1 << 20)) return topn_fail(h, MALS_INVALID_ARG, "too many items in one query");
    }
  } else {
    one_each.resize((size_t)n_queries + 1);
    for (int q = 0; q <= n_queries; ++q) one_each[(size_t)q] = q;
    item_ptr = one_each.data();
  }
  if (n_queries == 0) return MALS_OK;
  if (int rc = topn_check_items(h, item_idx, item_ptr[n_queries])) return rc;
  if (int rc = topn_serving_ready(h)) return rc;
  TopnRequest rq;
  rq.n_queries = n_queries;
  rq.how_many = how_many;
  rq.item_rows = item_idx;
  rq.vec_ptr = item_ptr;
  rq.excl_ptr = item_ptr;   // the query items are never returned (MostSimilarItemIterator.java:81-85)
  rq.excl_idx = item_idx;
  rq.cosine = true;
  rq.item_idx_out = item_idx_out;
  rq.score_out = score_out;
  rq.n_out = n_out;
  rq.rescorer = r;
  rq.flags = r ? flags : 0;   // (without a rescorer no pair is filtered: the plain call, whatever the flags)
  // a small call is folded into a pass with other callers' mostSimilarItems calls (of the same rescorer and flags)
  return topn_front_submit(h, rq, n_queries < TOPN_FRONT_BULK && how_many <= TOPN_FILTER_MAX_N && item_ptr[n_queries] <= 4 * TOPN_FRONT_BULK);
}
int mals_most_similar_items(mals_handle h, const int64_t* item_idx, const int64_t* item_ptr, int32_t n_queries, int32_t how_many,
                            int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  return topn_generation_guard(h, [&]() -> int { return topn_most_similar_once(h, nullptr, 0, item_idx, item_ptr, n_queries, how_many, item_idx_out, score_out, n_out); });
}
int mals_most_similar_items_rescored(mals_handle h, mals_rescorer r, int32_t flags, const int64_t* item_idx, const int64_t* item_ptr, int32_t n_queries,
                                     int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  return topn_generation_guard(h, [&]() -> int { return topn_most_similar_once(h, r, flags, item_idx, item_ptr, n_queries, how_many, item_idx_out, score_out, n_out); });
}
int mals_similar_stats(mals_handle h, int64_t* out4) {
  if (!h || !out4) return MALS_INVALID_ARG;
  for (int i = 0; i < 4; ++i) out4[i] = topn_front(h)->similar[i].load(std::memory_order_relaxed);
  return MALS_OK;
}

static int topn_similarity_to_once(mals_handle h, int64_t to_item, const int64_t* item_idx, int32_t n, float* out) {
  if (!h) return MALS_INVALID_ARG;
  SideState& y = h->side[MALS_SIDE_Y];
  if (!y.F || y.n_total == 0) return topn_fail(h, MALS_INVALID_ARG, "item factor replica not available");
  if (n < 0 || (n > 0 && (!item_idx || !out))) return topn_fail(h, MALS_INVALID_ARG, "bad similarityToItem arguments");
  if (to_item < 0 || to_item >= y.n_total) return topn_fail(h, MALS_INVALID_ARG, "item index outside the item factor replica");
  if (int rc = topn_check_items(h, item_idx, n)) return rc;
  if (n == 0) return MALS_OK;
  if (hipSetDevice(h->cfg.device) != hipSuccess) return topn_fail(h, MALS_HIP_ERROR, "hipSetDevice failed");
  TopnRequest rq;
  rq.kind = TOPN_KIND_SIMILARITY_TO;
  rq.n_queries = n;
  rq.how_many = 1;
  rq.item_rows = item_idx;
  rq.to_item = to_item;
  rq.sim_out = out;
  return topn_front_submit(h, rq, false);
}
int mals_similarity_to_item(mals_handle h, int64_t to_item, const int64_t* item_idx, int32_t n, float* out) {
  return topn_generation_guard(h, [&]() -> int { return topn_similarity_to_once(h, to_item, item_idx, n, out); });
}

static int topn_because_once(mals_handle h, const int64_t* user_idx, const int64_t* item_idx, int32_t n_queries, int32_t how_many,
                             int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  if (!h) return MALS_INVALID_ARG;
  SideState& x = h->side[MALS_SIDE_X];
  SideState& y = h->side[MALS_SIDE_Y];
  if (!y.F || y.n_total == 0) return topn_fail(h, MALS_INVALID_ARG, "item factor replica not available");
  if (n_queries < 0 || how_many <= 0 || how_many > 4096 || (n_queries > 0 && (!user_idx || !item_idx || !item_idx_out || !score_out)))
    return topn_fail(h, MALS_INVALID_ARG, "bad recommendedBecause arguments (how_many in 1..4096)");
  if (!x.has_matrix && !h->known_ptr)
    return topn_fail(h, MALS_INVALID_ARG, "the user-side matrix (or mals_set_known_items) is needed for the known items");
  if (h->known_ptr && h->known_rows != x.n_local)
    return topn_fail(h, MALS_INVALID_ARG, "the installed known items do not match the local user rows");
  for (int q = 0; q < n_queries; ++q) {
    if (user_idx[q] < 0 || user_idx[q] >= x.n_total) return topn_fail(h, MALS_INVALID_ARG, "user index outside the factor replica");
    if (user_idx[q] < x.row_offset || user_idx[q] >= foldin_user_rows_end(h))
      return topn_fail(h, MALS_INVALID_ARG, "known items of this user are not on this handle (row outside the local shard)");
  }
  if (n_queries == 0) return MALS_OK;
  if (int rc = topn_check_items(h, item_idx, n_queries)) return rc;
  if (int rc = topn_serving_ready(h)) return rc;
  TopnRequest rq;
  rq.kind = TOPN_KIND_BECAUSE;
  rq.n_queries = n_queries;
  rq.how_many = how_many;
  rq.item_rows = item_idx;
  rq.because_user = user_idx;
  rq.cosine = true;
  rq.item_idx_out = item_idx_out;
  rq.score_out = score_out;
  rq.n_out = n_out;
  return topn_front_submit(h, rq, false);
}
int mals_recommended_because(mals_handle h, const int64_t* user_idx, const int64_t* item_idx, int32_t n_queries, int32_t how_many,
                             int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  return topn_generation_guard(h, [&]() -> int { return topn_because_once(h, user_idx, item_idx, n_queries, how_many, item_idx_out, score_out, n_out); });
}

int mals_recommend_front_stats(mals_handle h, int64_t* out4) {
  if (!h || !out4) return MALS_INVALID_ARG;
  TopnFront* f = topn_front(h);
  std::lock_guard<std::mutex> lk(f->mu);
  out4[0] = (int64_t)f->calls;
  out4[1] = (int64_t)f->queries;
  out4[2] = (int64_t)f->passes;
  out4[3] = (int64_t)f->bulk_calls;
  return MALS_OK;
}

int mals_recommend_set_spin_us(mals_handle h, int32_t spin_us) {
  if (!h || spin_us < 0 || spin_us > 1000000) return MALS_INVALID_ARG;
  TopnFront* f = topn_front(h);
  std::lock_guard<std::mutex> lk(f->mu);
  f->spin_us = spin_us;
  return MALS_OK;
}

int mals_recommend_set_depth(mals_handle h, int32_t passes_in_flight) {
  if (!h || passes_in_flight < 1 || passes_in_flight > TOPN_SLOTS) return MALS_INVALID_ARG;
  TopnFront* f = topn_front(h);
  std::lock_guard<std::mutex> lk(f->mu);
  if (f->n_busy > 0 || f->leader) { h->err = "mals_recommend_set_depth: calls are in flight"; return MALS_INVALID_ARG; }
  f->depth = passes_in_flight;
  f->next_slot = f->oldest = 0;
  return MALS_OK;
}

// ---- the online write path (foldin_host.h, foldin_kernels.h) ---------------------------------------------------------
void malsi_mark_group_member(mals_handle h) {
  if (h) h->group_member = true;
}

int mals_set_foldin_solver(mals_handle h, int side, mals_solver s) {
  CHECK_SIDE(h, side);
  if (int rc = foldin_refuse(h, "mals_set_foldin_solver")) return rc;
  if (s && s->qr.dim() != h->cfg.features) return topn_fail(h, MALS_INVALID_ARG, "mals_set_foldin_solver: the solver's dimension is not the handle's features");
  return foldin_exclusive(h, "mals_set_foldin_solver", [&](std::string& msg) -> int { return foldin_solver_members(&h, 1, side, s, msg); });
}

int mals_set_foldin_learn_rate(mals_handle h, double rate) {
  if (!h) return MALS_INVALID_ARG;
  if (!std::isfinite(rate)) return topn_fail(h, MALS_INVALID_ARG, "the fold-in learning rate must be finite");
  if (int rc = foldin_refuse(h, "mals_set_foldin_learn_rate")) return rc;
  return foldin_exclusive(h, "mals_set_foldin_learn_rate", [&](std::string&) -> int { return foldin_rate_members(&h, 1, rate); });
}

int mals_foldin_stats(mals_handle h, int64_t* out6) {
  if (!h || !out6) return MALS_INVALID_ARG;
  for (int i = 0; i < 6; ++i) out6[i] = h->foldin_counters[i].load();
  return MALS_OK;
}

// a handle owns every user its pair check lets through (foldin_write_ready)
static const int64_t FOLDIN_OWN_ALL[2] = {std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max()};

// setPreference, setUserTag and setItemTag: one batch of one kind (FOLDIN_KIND_*), one exclusive ticket
static int foldin_set_impl(mals_handle h, const char* call, uint8_t kind, int64_t n, const int64_t* user_row, const int64_t* item_row, const float* value,
                           int32_t* status_out) {
  if (!h) return MALS_INVALID_ARG;
  if (int rc = foldin_refuse(h, call)) return rc;
  if (n < 0 || (n > 0 && (!user_row || !item_row || !value))) return topn_fail(h, MALS_INVALID_ARG, (std::string(call) + ": bad arguments").c_str());
  if (n > (int64_t)1 << 30) return topn_fail(h, MALS_INVALID_ARG, (std::string(call) + ": at most 2^30 updates per call").c_str());
  if (n == 0) return MALS_OK;
  const std::vector<uint8_t> kinds(kind == FOLDIN_KIND_PREF ? 0 : (size_t)n, kind);
  return foldin_exclusive(h, call, [&](std::string& msg) -> int {
    return foldin_set_members(&h, 1, FOLDIN_OWN_ALL, false, n, user_row, item_row, value, kinds.empty() ? nullptr : kinds.data(), status_out, msg);
  });
}

int mals_set_preferences(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* item_row, const float* value, int32_t* status_out) {
  return foldin_set_impl(h, "mals_set_preferences", FOLDIN_KIND_PREF, n, user_row, item_row, value, status_out);
}

int mals_set_user_tags(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* tag_item_row, const float* value, int32_t* status_out) {
  return foldin_set_impl(h, "mals_set_user_tags", FOLDIN_KIND_USER_TAG, n, user_row, tag_item_row, value, status_out);
}

int mals_set_item_tags(mals_handle h, int64_t n, const int64_t* tag_user_row, const int64_t* item_row, const float* value, int32_t* status_out) {
  return foldin_set_impl(h, "mals_set_item_tags", FOLDIN_KIND_ITEM_TAG, n, tag_user_row, item_row, value, status_out);
}

// the tag sets as they stand, read inside a ticket: side Y = the set bits of the userTagIDs mask, side X = the tag users
// (global rows), ascending.  *n_out is the set's size whatever cap is; rows_out takes the first min(cap, size)
int mals_get_tag_rows(mals_handle h, int side, int64_t* rows_out, int64_t cap, int64_t* n_out) {
  CHECK_SIDE(h, side);
  if (!n_out || cap < 0 || (cap > 0 && !rows_out)) return topn_fail(h, MALS_INVALID_ARG, "mals_get_tag_rows: bad arguments");
  *n_out = 0;
  if (int rc = foldin_refuse(h, "mals_get_tag_rows", true)) return rc;   // (a read of one handle's own sets: a group's member answers too)
  return foldin_exclusive(h, "mals_get_tag_rows", [&](std::string& msg) -> int {
    std::vector<int64_t> rows;
    if (side == MALS_SIDE_X) {
      if (h->serving->pop)
        for (int64_t r : popular_state(h)->tag_users) rows.push_back(r + h->side[MALS_SIDE_X].row_offset);
    } else if (h->tag_bits.get()) {
      std::vector<uint32_t> words((size_t)((h->tag_bits_items + 31) / 32));
      FCHK(msg, hipMemcpyAsync(words.data(), h->tag_bits.get(), sizeof(uint32_t) * words.size(), hipMemcpyDeviceToHost, h->stream));
      FCHK(msg, hipStreamSynchronize(h->stream));
      for (size_t w = 0; w < words.size(); ++w)
        for (uint32_t b = words[w]; b; b &= b - 1) {
          const int64_t r = (int64_t)w * 32 + __builtin_ctz(b);
          if (r < h->tag_bits_items) rows.push_back(r);
        }
    }
    *n_out = (int64_t)rows.size();
    std::copy(rows.begin(), rows.begin() + std::min<int64_t>(cap, (int64_t)rows.size()), rows_out);
    return MALS_OK;
  });
}

int mals_remove_preferences(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* item_row, int64_t* removed_users_out,
                            int64_t* n_removed_out) {
  if (!h) return MALS_INVALID_ARG;
  if (n_removed_out) *n_removed_out = 0;
  if (int rc = foldin_refuse(h, "mals_remove_preferences")) return rc;
  if (n < 0 || (n > 0 && (!user_row || !item_row))) return topn_fail(h, MALS_INVALID_ARG, "mals_remove_preferences: bad arguments");
  if (n == 0) return MALS_OK;
  return foldin_exclusive(h, "mals_remove_preferences", [&](std::string& msg) -> int {
    return foldin_remove_members(&h, 1, FOLDIN_OWN_ALL, false, n, user_row, item_row, removed_users_out, n_removed_out, msg);
  });
}

int mals_grow_factor_rows(mals_handle h, int side, int64_t n_rows_total) {
  CHECK_SIDE(h, side);
  if (int rc = foldin_refuse(h, "mals_grow_factor_rows")) return rc;
  return foldin_exclusive(h, "mals_grow_factor_rows", [&](std::string& msg) -> int {
    // grown users are this handle's when its users already reached the end of the old replica
    const int grown_owner = foldin_user_rows_end(h) >= h->side[side].n_total ? 0 : -1;
    return foldin_grow_members(&h, 1, side, n_rows_total, grown_owner, false, msg);
  });
}

static int foldin_estimate_impl(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* item_row, float* out, bool via_group) {
  if (!h) return MALS_INVALID_ARG;
  if (int rc = foldin_refuse(h, "mals_estimate_preferences", via_group)) return rc;
  if (n < 0 || (n > 0 && (!user_row || !item_row || !out))) return topn_fail(h, MALS_INVALID_ARG, "mals_estimate_preferences: bad arguments");
  if (n == 0) return MALS_OK;
  return foldin_exclusive(h, "mals_estimate_preferences", [&](std::string& msg) -> int {
    if (int rc = foldin_check_pairs(h, n, user_row, item_row, true, false, msg)) return rc;
    DeviceBuffer<int64_t> d_rows;
    DeviceBuffer<float> d_out;
    FCHK(msg, d_rows.alloc(2 * (size_t)n));
    FCHK(msg, d_out.alloc((size_t)n));
    FCHK(msg, hipMemcpyAsync(d_rows.get(), user_row, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    FCHK(msg, hipMemcpyAsync(d_rows.get() + n, item_row, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(foldin_estimate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->side[MALS_SIDE_X].F, h->side[MALS_SIDE_Y].F,
                       h->cfg.features, d_rows.get(), d_rows.get() + n, n, d_out.get());
    FCHK(msg, hipGetLastError());
    FCHK(msg, hipMemcpyAsync(out, d_out.get(), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    FCHK(msg, hipStreamSynchronize(h->stream));
    for (int64_t t = 0; t < n; ++t)   // Preconditions.checkState(isFinite(value), "Bad estimate") (:718)
      if (!std::isfinite(out[t])) {
        msg = "bad estimate (not finite) for pair " + std::to_string(t);
        return MALS_INVALID_ARG;
      }
    return MALS_OK;
  });
}

int mals_estimate_preferences(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* item_row, float* out) {
  return foldin_estimate_impl(h, n, user_row, item_row, out, false);
}

static int foldin_anonymous(mals_handle h, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row, const float* values, float* out,
                            int32_t* status_out, const int64_t* to_item, float* dot_out, const char* call, bool via_group = false) {
  if (!h) return MALS_INVALID_ARG;
  if (int rc = foldin_refuse(h, call, via_group)) return rc;
  if (n_queries < 0 || (n_queries > 0 && (!item_ptr || !out || (item_ptr[n_queries] > 0 && !item_row))) || (n_queries > 0 && item_ptr[0] != 0))
    return topn_fail(h, MALS_INVALID_ARG, (std::string(call) + ": bad arguments").c_str());
  for (int32_t q = 0; q < n_queries; ++q)
    if (item_ptr[q + 1] < item_ptr[q] || item_ptr[q + 1] - item_ptr[q] > (1 << 20))
      return topn_fail(h, MALS_INVALID_ARG, (std::string(call) + ": bad item_ptr").c_str());
  if (n_queries == 0) return MALS_OK;
  std::vector<int32_t> found((size_t)n_queries, 0);
  bool no_solver = false;
  const int rc = foldin_exclusive(h, call, [&](std::string& msg) -> int {
    const SideState& y = h->side[MALS_SIDE_Y];
    if (!y.F) {
      msg = "item factor replica not available";
      return MALS_INVALID_ARG;
    }
    for (int64_t j = 0; j < item_ptr[n_queries]; ++j)
      if (item_row[j] < -1 || item_row[j] >= y.n_total) {
        msg = "item row outside the item factor replica";
        return MALS_INVALID_ARG;
      }
    for (int32_t q = 0; to_item && q < n_queries; ++q)
      if (to_item[q] < 0 || to_item[q] >= y.n_total) {
        msg = "item row outside the item factor replica";
        return MALS_INVALID_ARG;
      }
    no_solver = !foldin_state(h)->solver[MALS_SIDE_Y].present;
    if (no_solver) return MALS_OK;
    return foldin_anonymous_run(h, n_queries, item_ptr, item_row, values, out, found.data(), to_item, dot_out, msg);
  });
  if (rc != MALS_OK) return rc;
  int first = MALS_OK;
  for (int32_t q = 0; q < n_queries; ++q) {
    // no Y^T Y solver: NotReadyException (:570-573); no item of the query has a row: NoSuchItemException (:603-605)
    const int st = (no_solver || !found[(size_t)q]) ? MALS_INVALID_ARG : MALS_OK;
    if (status_out) status_out[q] = st;
    if (st != MALS_OK && first == MALS_OK) first = st;
  }
  if (first != MALS_OK)
    return topn_fail(h, first, (std::string(call) + (no_solver ? ": no Y^T Y solver (mals_set_foldin_solver)" : ": a query has no item with a row")).c_str());
  return MALS_OK;
}

int mals_anonymous_features(mals_handle h, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row, const float* values, float* out,
                            int32_t* status_out) {
  return foldin_anonymous(h, n_queries, item_ptr, item_row, values, out, status_out, nullptr, nullptr, "mals_anonymous_features");
}

static int foldin_estimate_anonymous_impl(mals_handle h, int32_t n_queries, const int64_t* to_item, const int64_t* item_ptr, const int64_t* item_row,
                                          const float* values, float* out, int32_t* status_out, bool via_group) {
  if (!h) return MALS_INVALID_ARG;
  if (n_queries > 0 && (!to_item || !out)) return topn_fail(h, MALS_INVALID_ARG, "mals_estimate_for_anonymous: bad arguments");
  std::vector<float> feats((size_t)std::max(n_queries, 0) * h->cfg.features);
  return foldin_anonymous(h, n_queries, item_ptr, item_row, values, feats.data(), status_out, to_item, out, "mals_estimate_for_anonymous", via_group);
}

int mals_estimate_for_anonymous(mals_handle h, int32_t n_queries, const int64_t* to_item, const int64_t* item_ptr, const int64_t* item_row,
                                const float* values, float* out, int32_t* status_out) {
  return foldin_estimate_anonymous_impl(h, n_queries, to_item, item_ptr, item_row, values, out, status_out, false);
}

// two tickets: the vectors, then the top-N (like the reference, which holds no lock across the two, a write may land between)
static int topn_anonymous_impl(mals_handle h, mals_rescorer r, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row,
                               const float* values, int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out, int32_t* status_out,
                               bool via_group = false) {
  if (!h) return MALS_INVALID_ARG;
  if (r && r->h != h) return topn_fail(h, MALS_INVALID_ARG, "the rescorer belongs to another handle");
  if (n_queries > 0 && (how_many <= 0 || how_many > 4096 || !item_idx_out || !score_out))
    return topn_fail(h, MALS_INVALID_ARG, "mals_recommend_to_anonymous: bad arguments (how_many in 1..4096)");
  const int k = h->cfg.features;
  std::vector<float> feats((size_t)std::max(n_queries, 0) * k);
  std::vector<int32_t> st((size_t)std::max(n_queries, 0), MALS_OK);
  const int rc_f = foldin_anonymous(h, n_queries, item_ptr, item_row, values, feats.data(), st.data(), nullptr, nullptr, "mals_recommend_to_anonymous", via_group);
  if (rc_f != MALS_OK && rc_f != MALS_INVALID_ARG) return rc_f;
  if (n_queries <= 0) return rc_f;
  if (rc_f == MALS_INVALID_ARG && std::all_of(st.begin(), st.end(), [](int32_t v) { return v == MALS_OK; })) return rc_f;   // (an argument error)
  // the queries that have a vector, their items as exclusions (rows -1 are no items)
  std::vector<int32_t> qs;
  std::vector<float> vecs;
  std::vector<int64_t> eptr(1, 0), eidx;
  for (int32_t q = 0; q < n_queries; ++q) {
    if (status_out) status_out[q] = st[(size_t)q];
    for (int j = 0; j < how_many; ++j) {
      item_idx_out[(size_t)q * how_many + j] = -1;
      score_out[(size_t)q * how_many + j] = -std::numeric_limits<float>::infinity();
    }
    if (n_out) n_out[q] = 0;
    if (st[(size_t)q] != MALS_OK) continue;
    qs.push_back(q);
    vecs.insert(vecs.end(), feats.begin() + (size_t)q * k, feats.begin() + (size_t)(q + 1) * k);
    for (int64_t j = item_ptr[q]; j < item_ptr[q + 1]; ++j)
      if (item_row[j] >= 0) eidx.push_back(item_row[j]);
    eptr.push_back((int64_t)eidx.size());
  }
  if (!qs.empty()) {
    std::vector<int64_t> idx(qs.size() * (size_t)how_many);
    std::vector<float> sc(qs.size() * (size_t)how_many);
    std::vector<int32_t> cnt(qs.size());
    if (int rc = topn_to_many_impl(h, r, vecs.data(), nullptr, (int32_t)qs.size(), how_many, eptr.data(), eidx.data(), idx.data(), sc.data(), cnt.data()))
      return rc;
    for (size_t i = 0; i < qs.size(); ++i) {
      std::copy(idx.begin() + i * how_many, idx.begin() + (i + 1) * how_many, item_idx_out + (size_t)qs[i] * how_many);
      std::copy(sc.begin() + i * how_many, sc.begin() + (i + 1) * how_many, score_out + (size_t)qs[i] * how_many);
      if (n_out) n_out[qs[i]] = cnt[i];
    }
  }
  return rc_f;
}

int mals_recommend_to_anonymous(mals_handle h, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row, const float* values,
                                int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out, int32_t* status_out) {
  return topn_anonymous_impl(h, nullptr, n_queries, item_ptr, item_row, values, how_many, item_idx_out, score_out, n_out, status_out);
}

int mals_foldin_solve(mals_handle h, int side, const float* b, int32_t n_rhs, double* x_out) {
  CHECK_SIDE(h, side);
  if (int rc = foldin_refuse(h, "mals_foldin_solve")) return rc;
  if (n_rhs < 0 || (n_rhs > 0 && (!b || !x_out))) return topn_fail(h, MALS_INVALID_ARG, "mals_foldin_solve: bad arguments");
  if (n_rhs == 0) return MALS_OK;
  const int k = h->cfg.features;
  return foldin_exclusive(h, "mals_foldin_solve", [&](std::string& msg) -> int {
    FoldinState& fs = *foldin_state(h);
    if (!fs.solver[side].present) {
      msg = "no solver on that side (mals_set_foldin_solver)";
      return MALS_INVALID_ARG;
    }
    if (int rc = foldin_lds_limit(msg)) return rc;
    DeviceBuffer<float> d_b;
    DeviceBuffer<double> d_x;
    FCHK(msg, d_b.alloc((size_t)n_rhs * k));
    FCHK(msg, d_x.alloc((size_t)n_rhs * k));
    FCHK(msg, hipMemcpyAsync(d_b.get(), b, sizeof(float) * (size_t)n_rhs * k, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(foldin_solve_kernel, dim3((unsigned)((n_rhs + FOLDIN_LANES - 1) / FOLDIN_LANES)), dim3(FOLDIN_LANES),
                       (size_t)k * FOLDIN_LANES * sizeof(double), h->stream, foldin_view(fs.solver[side]), k, d_b.get(), n_rhs, d_x.get());
    FCHK(msg, hipGetLastError());
    FCHK(msg, hipMemcpyAsync(x_out, d_x.get(), sizeof(double) * (size_t)n_rhs * k, hipMemcpyDeviceToHost, h->stream));
    FCHK(msg, hipStreamSynchronize(h->stream));
    return MALS_OK;
  });
}

// ---- mostPopularItems (popular_host.h) ------------------------------------------------------------------------------------
int mals_set_tag_users(mals_handle h, int64_t n, const int64_t* user_idx, int mem_kind) {
  if (!h) return MALS_INVALID_ARG;
  if (mem_kind != MALS_MEM_HOST && mem_kind != MALS_MEM_DEVICE) return fail(h, MALS_INVALID_ARG, "mem_kind must be MALS_MEM_HOST or MALS_MEM_DEVICE");
  if (n < 0 || (n > 0 && !user_idx)) return fail(h, MALS_INVALID_ARG, "bad tag user list");
  std::vector<int64_t> host;
  if (mem_kind == MALS_MEM_DEVICE && n > 0) {
    if (int rc = use_device(h)) return rc;
    host.resize((size_t)n);
    HIPCHK(h, hipMemcpy(host.data(), user_idx, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
    user_idx = host.data();
  }
  return popular_set_tag_users(&h, 1, n, user_idx);
}

int mals_get_tag_user_count(mals_handle h, int64_t* n_out) {
  if (!h || !n_out) return MALS_INVALID_ARG;
  *n_out = h->serving->pop ? (int64_t)popular_state(h)->tag_users.size() : 0;
  return MALS_OK;
}

int mals_most_popular_items(mals_handle h, mals_rescorer r, int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  if (!h) return MALS_INVALID_ARG;
  if (r && r->h != h) return topn_fail(h, MALS_INVALID_ARG, "the rescorer belongs to another handle");
  if (int rc = foldin_refuse(h, "mals_most_popular_items")) return rc;
  if (how_many <= 0 || how_many > 4096 || !item_idx_out || !score_out)
    return topn_fail(h, MALS_INVALID_ARG, "mals_most_popular_items: bad arguments (how_many in 1..4096)");
  return foldin_exclusive(h, "mals_most_popular_items", [&](std::string& msg) -> int {
    return popular_members(&h, 1, false, r, how_many, item_idx_out, score_out, n_out, msg);
  });
}

int mals_most_popular_stats(mals_handle h, int64_t* out4) {
  if (!h || !out4) return MALS_INVALID_ARG;
  for (int i = 0; i < 4; ++i) out4[i] = h->popular_counters[i].load();
  return MALS_OK;
}

// ---- loading a new generation into a live handle (generation_host.h) ------------------------------------------------------
int mals_load_generation(mals_handle h, const mals_generation_load* load, mals_generation_result* result_out) {
  if (!h) return MALS_INVALID_ARG;
  if (int rc = foldin_refuse(h, "mals_load_generation")) return rc;
  if (!load || load->struct_size != (int32_t)sizeof(mals_generation_load) || (result_out && result_out->struct_size != (int32_t)sizeof(mals_generation_result)))
    return topn_fail(h, MALS_INVALID_ARG, "mals_load_generation: null argument or struct_size mismatch");
  const mals_generation_load& L = *load;
  bool ok = (L.cur_mem_kind == MALS_MEM_HOST || L.cur_mem_kind == MALS_MEM_DEVICE) && (L.new_mem_kind == MALS_MEM_HOST || L.new_mem_kind == MALS_MEM_DEVICE);
  for (int sd = 0; sd < 2 && ok; ++sd)
    ok = L.n_cur[sd] >= 0 && L.n_new[sd] >= 0 && (L.n_cur[sd] == 0 || L.cur_ids[sd]) && (L.n_new[sd] == 0 || (L.new_ids[sd] && L.new_rows[sd])) &&
         L.n_cur[sd] < ((int64_t)1 << 31) && L.n_new[sd] < ((int64_t)1 << 31);
  ok = ok && L.n_item_tag_ids >= 0 && L.n_user_tag_ids >= 0 && (L.n_item_tag_ids == 0 || L.item_tag_ids) && (L.n_user_tag_ids == 0 || L.user_tag_ids);
  if (!ok) return topn_fail(h, MALS_INVALID_ARG, "mals_load_generation: bad arguments (mem kinds, counts in [0, 2^31), null arrays)");
  return foldin_exclusive(h, "mals_load_generation", [&](std::string& msg) -> int {
    if (int rc = generation_load_run(h, L, result_out, msg)) return rc;
    if (L.flags & MALS_GENERATION_RECOMPUTE_SOLVERS) {   // Generation.recomputeState: the solvers of the merged X and Y
      int first = MALS_OK;
      mals_solver sv[2] = {nullptr, nullptr};
      for (int sd = 0; sd < 2 && first == MALS_OK; ++sd) first = mals_recompute_solver(h, sd, &sv[sd], nullptr);
      for (int sd = 0; sd < 2 && first == MALS_OK; ++sd) {
        std::string why;
        first = foldin_solver_install(h, sd, sv[sd], foldin_solver_ipiv(sv[sd], h->cfg.features), why);
      }
      for (mals_solver s : sv)
        if (s) (void)mals_solver_destroy(s);
      if (result_out) result_out->solver_status = first;
    }
    return MALS_OK;
  });
}

static int generation_get_impl(mals_handle h, int side, bool ids, int64_t* out, const char* call) {
  CHECK_SIDE(h, side);
  if (!out) return topn_fail(h, MALS_INVALID_ARG, "the output array must not be NULL");
  if (hipSetDevice(h->cfg.device) != hipSuccess) return topn_fail(h, MALS_HIP_ERROR, "hipSetDevice failed");
  return foldin_exclusive(h, call, [&](std::string& msg) -> int { return generation_get(h, side, ids, out, msg); });
}
int mals_generation_get_ids(mals_handle h, int side, int64_t* ids_out) { return generation_get_impl(h, side, true, ids_out, "mals_generation_get_ids"); }
int mals_generation_get_map(mals_handle h, int side, int64_t* map_out) { return generation_get_impl(h, side, false, map_out, "mals_generation_get_map"); }

int mals_mark_recent(mals_handle h, int side, int64_t n, const int64_t* rows) {
  CHECK_SIDE(h, side);
  if (n < 0 || (n > 0 && !rows)) return topn_fail(h, MALS_INVALID_ARG, "mals_mark_recent: bad arguments");
  return foldin_exclusive(h, "mals_mark_recent", [&](std::string& msg) -> int {
    const int64_t n_rows = h->side[side].F ? h->side[side].n_total : 0;
    for (int64_t t = 0; t < n; ++t)
      if (rows[t] < 0 || rows[t] >= n_rows) {
        msg = "row " + std::to_string(t) + " is outside the replica";
        return MALS_INVALID_ARG;
      }
    for (int64_t t = 0; t < n; ++t) generation_mark(h, side, rows[t]);
    return MALS_OK;
  });
}

int mals_get_recent(mals_handle h, int side, int64_t* rows_out, int64_t* n_out) {
  CHECK_SIDE(h, side);
  if (!n_out) return topn_fail(h, MALS_INVALID_ARG, "mals_get_recent: n_out must not be NULL");
  return foldin_exclusive(h, "mals_get_recent", [&](std::string& msg) -> int {
    const std::vector<uint32_t>& b = generation_state(h)->recent[side];
    const int64_t n_rows = h->side[side].F ? h->side[side].n_total : 0;   // (rows_out holds the replica's rows: never more)
    int64_t n = 0;
    for (size_t w = 0; w < b.size(); ++w)
      for (uint32_t bits = b[w]; bits; bits &= bits - 1) {
        const int64_t row = (int64_t)w * 32 + __builtin_ctz(bits);
        if (row >= n_rows) continue;
        if (rows_out) rows_out[n] = row;
        ++n;
      }
    *n_out = n;
    return MALS_OK;
  });
}

// ---- the id directory (ids_host.h, ids_kernels.h) ---------------------------------------------------------------------------
int mals_ids_set(mals_handle h, int side, int64_t n, const int64_t* ids, int mem_kind) {
  CHECK_SIDE(h, side);
  if (int rc = foldin_refuse(h, "mals_ids_set")) return rc;
  if (n < 0 || (n > 0 && !ids) || n > (int64_t)1 << 30 || (mem_kind != MALS_MEM_HOST && mem_kind != MALS_MEM_DEVICE))
    return topn_fail(h, MALS_INVALID_ARG, "mals_ids_set: bad arguments (n in [0, 2^30], ids, mem_kind)");
  return foldin_exclusive(h, "mals_ids_set", [&](std::string& msg) -> int { return ids_set_run(h, side, n, ids, mem_kind, msg); });
}

static int ids_rows_of(mals_handle h, int side, int64_t n, const int64_t* ids, int64_t* rows_out, int64_t* n_new_out, bool add, const char* call) {
  CHECK_SIDE(h, side);
  if (n_new_out) *n_new_out = 0;
  if (int rc = foldin_refuse(h, call)) return rc;
  if (n < 0 || (n > 0 && (!ids || !rows_out)) || n > (int64_t)1 << 30)
    return topn_fail(h, MALS_INVALID_ARG, (std::string(call) + ": bad arguments (n in [0, 2^30], ids, rows_out)").c_str());
  return foldin_exclusive(h, call, [&](std::string& msg) -> int { return ids_rows_of_run(h, side, n, ids, rows_out, n_new_out, add, msg); });
}

int mals_ids_lookup(mals_handle h, int side, int64_t n, const int64_t* ids, int64_t* rows_out) {
  return ids_rows_of(h, side, n, ids, rows_out, nullptr, false, "mals_ids_lookup");
}

int mals_ids_resolve(mals_handle h, int side, int64_t n, const int64_t* ids, int64_t* rows_out, int64_t* n_new_out) {
  return ids_rows_of(h, side, n, ids, rows_out, n_new_out, true, "mals_ids_resolve");
}

int mals_ids_get(mals_handle h, int side, int64_t row_begin, int64_t n, int64_t* ids_out) {
  CHECK_SIDE(h, side);
  if (int rc = foldin_refuse(h, "mals_ids_get")) return rc;
  if (n > 0 && !ids_out) return topn_fail(h, MALS_INVALID_ARG, "mals_ids_get: ids_out must not be NULL");
  return foldin_exclusive(h, "mals_ids_get", [&](std::string& msg) -> int { return ids_get_run(h, side, row_begin, n, ids_out, msg); });
}

int mals_ids_count(mals_handle h, int side, int64_t* n_out) {
  CHECK_SIDE(h, side);
  if (int rc = foldin_refuse(h, "mals_ids_count")) return rc;
  if (!n_out) return topn_fail(h, MALS_INVALID_ARG, "mals_ids_count: n_out must not be NULL");
  return foldin_exclusive(h, "mals_ids_count", [&](std::string& msg) -> int {
    if (int rc = ids_ready(h, side, msg)) return rc;
    *n_out = ids_state(h)->side[side].n;
    return MALS_OK;
  });
}

int mals_ingest_apply_times(mals_handle h, double* out4) {
  if (!h || !out4) return MALS_INVALID_ARG;
  return foldin_exclusive(h, "mals_ingest_apply_times", [&](std::string&) -> int {
    const IdsState* st = h->serving->ids;
    for (int i = 0; i < 4; ++i) out4[i] = st ? st->apply_ms[i] : 0.0;
    return MALS_OK;
  });
}

int mals_ingest_apply_tag_stats(mals_handle h, int64_t* out4) {
  if (!h || !out4) return MALS_INVALID_ARG;
  return foldin_exclusive(h, "mals_ingest_apply_tag_stats", [&](std::string&) -> int {
    const IdsState* st = h->serving->ids;
    for (int i = 0; i < 4; ++i) out4[i] = st ? st->tag_stats[i] : 0;
    return MALS_OK;
  });
}

uint64_t mals_generation_hash_host(int64_t id) { return gen_hash(id); }

int mals_generation_join_host(const int64_t* cur_ids, int64_t n_cur, const int64_t* new_ids, int64_t n_new, const int64_t* recent_rows,
                              int64_t n_recent, int32_t flags, int64_t* map_out, int64_t* counts_out) {
  return generation_join_host(cur_ids, n_cur, new_ids, n_new, recent_rows, n_recent, flags, map_out, counts_out);
}

}  // extern "C"

// ---- the write path on the members of a group (mals_group.cpp: the mals_group_* twins) ---------------------------------
// Each call below holds the fronts of ALL members (foldin_exclusive_all) while the write's one driver (foldin_host.h,
// popular_host.h) enqueues every member's device work and only then waits for each: the members work side by side, and a
// read of any member sees the model before the write or after it.  The caller (the group) orders the writes among themselves.
namespace {
// body(msg) with every member's front held; a failure's text goes to *err
template <class Body>
int group_call(mals_handle* hs, int n_members, std::string* err, Body&& body) {
  std::string msg;
  const std::function<int()> fn = [&]() -> int { return body(msg); };
  const int rc = foldin_exclusive_all(hs, n_members, 0, fn);
  if (rc != MALS_OK && err) *err = msg.empty() ? std::string("failed") : msg;
  return rc;
}
}  // namespace

int malsi_group_set_foldin_solver(mals_handle* hs, int n_members, int side, mals_solver s, std::string* err) {
  if (s && s->qr.dim() != hs[0]->cfg.features) {
    if (err) *err = "the solver's dimension is not the group's features";
    return MALS_INVALID_ARG;
  }
  return group_call(hs, n_members, err, [&](std::string& msg) { return foldin_solver_members(hs, n_members, side, s, msg); });
}

int malsi_group_set_foldin_learn_rate(mals_handle* hs, int n_members, double rate, std::string* err) {
  return group_call(hs, n_members, err, [&](std::string&) { return foldin_rate_members(hs, n_members, rate); });
}

int malsi_group_set_preferences(mals_handle* hs, int n_members, const int64_t* own, int64_t n, const int64_t* user_row, const int64_t* item_row,
                                const float* value, int kind, int32_t* status_out, std::string* err) {
  const std::vector<uint8_t> kinds(kind == FOLDIN_KIND_PREF ? 0 : (size_t)n, (uint8_t)kind);
  return group_call(hs, n_members, err, [&](std::string& msg) -> int {
    return foldin_set_members(hs, n_members, own, true, n, user_row, item_row, value, kinds.empty() ? nullptr : kinds.data(), status_out, msg);
  });
}

int malsi_group_remove_preferences(mals_handle* hs, int n_members, const int64_t* own, int64_t n, const int64_t* user_row, const int64_t* item_row,
                                   int64_t* removed_users_out, int64_t* n_removed_out, std::string* err) {
  return group_call(hs, n_members, err, [&](std::string& msg) -> int {
    return foldin_remove_members(hs, n_members, own, true, n, user_row, item_row, removed_users_out, n_removed_out, msg);
  });
}

// grown_owner: the member that owns the users past the installed matrix (the last rank), or -1
int malsi_group_grow_factor_rows(mals_handle* hs, int n_members, int side, int64_t n_rows_total, int grown_owner, std::string* err) {
  return group_call(hs, n_members, err, [&](std::string& msg) { return foldin_grow_members(hs, n_members, side, n_rows_total, grown_owner, true, msg); });
}

// the digest of rows [row_begin, row_begin + n_rows) of every handle's replica, all taken between the same two writes
int malsi_group_factor_digest(mals_handle* hs, int n_members, int side, int64_t row_begin, int64_t n_rows, uint64_t* out, std::string* err) {
  return group_call(hs, n_members, err, [&](std::string& msg) -> int {
    for (int m = 0; m < n_members; ++m) {
      const SideState& s = hs[m]->side[side];
      if (!s.F) {
        msg = "the replica is not declared";
        return MALS_INVALID_ARG;
      }
      if (row_begin < 0 || n_rows < 0 || row_begin > s.n_total || n_rows > s.n_total - row_begin) {
        msg = "rows outside the factor replica";
        return MALS_INVALID_ARG;
      }
      out[m] = 0;
    }
    if (n_rows == 0) return MALS_OK;
    const int k = hs[0]->cfg.features;
    const int64_t e0 = row_begin * k, e1 = (row_begin + n_rows) * k;
    // enough workgroups to keep every CU streaming (8 per CU of 256), never more than the float4s ask for
    const unsigned grid = (unsigned)std::min<int64_t>(2048, std::max<int64_t>(1, ((e1 - e0) / 4 + 255) / 256));
    MemberSlots<DeviceBuffer<unsigned long long>> cell(n_members);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the digest cell is 64 bits");
    return member_loop(
        hs, n_members, cell, msg,
        [&](int m, std::string& why) -> int {
          FCHK(why, cell[m].alloc(1));
          FCHK(why, hipMemsetAsync(cell[m].get(), 0, sizeof(unsigned long long), hs[m]->stream));
          hipLaunchKernelGGL(factor_digest_kernel, dim3(grid), dim3(256), 0, hs[m]->stream, hs[m]->side[side].F, e0, e1, cell[m].get());
          FCHK(why, hipGetLastError());
          FCHK(why, hipMemcpyAsync(out + m, cell[m].get(), sizeof(uint64_t), hipMemcpyDeviceToHost, hs[m]->stream));
          return MALS_OK;
        },
        [&](int m, std::string& why) -> int {
          FCHK(why, hipStreamSynchronize(hs[m]->stream));
          return MALS_OK;
        });
  });
}

int malsi_group_set_tag_users(mals_handle* hs, int n_members, int64_t n, const int64_t* user_idx, std::string* err) {
  return group_call(hs, n_members, err, [&](std::string&) { return popular_set_tag_users(hs, n_members, n, user_idx); });
}

int malsi_group_most_popular_items(mals_handle* hs, int n_members, int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out,
                                   std::string* err) {
  return group_call(hs, n_members, err, [&](std::string& msg) -> int {
    return popular_members(hs, n_members, true, nullptr, how_many, item_idx_out, score_out, n_out, msg);
  });
}

// mals_group_load_generation (generation_group_host.h): loads[m] = the arguments as member m reads them; old_bounds_x = the
// group's bounds[X] (n_members + 1) or NULL; on success bounds_x_out / bounds_y_out (n_members + 1 each) are the new ones
int malsi_group_load_generation(mals_handle* hs, int n_members, const mals_generation_load* loads, mals_generation_result* result_out,
                                const int64_t* old_bounds_x, int64_t* bounds_x_out, int64_t* bounds_y_out, std::string* err) {
  return group_call(hs, n_members, err, [&](std::string& msg) -> int {
    if (int rc = generation_group_run(hs, n_members, loads, result_out, old_bounds_x, bounds_x_out, bounds_y_out, msg)) return rc;
    if (loads[0].flags & MALS_GENERATION_RECOMPUTE_SOLVERS) {   // the merged replicas are the same everywhere: computed once, installed on all
      int first = MALS_OK;
      mals_solver sv[2] = {nullptr, nullptr};
      if (hipSetDevice(hs[0]->cfg.device) != hipSuccess) first = MALS_HIP_ERROR;
      for (int sd = 0; sd < 2 && first == MALS_OK; ++sd) first = mals_recompute_solver(hs[0], sd, &sv[sd], nullptr);
      for (int sd = 0; sd < 2 && first == MALS_OK; ++sd) {
        std::string why;
        first = foldin_solver_members(hs, n_members, sd, sv[sd], why);
      }
      for (mals_solver s : sv)
        if (s) (void)mals_solver_destroy(s);
      if (result_out) result_out->solver_status = first;
    }
    return MALS_OK;
  });
}

// the fold-in reads on ONE member (any: the replicas and the solvers are complete everywhere)
int malsi_member_estimate_preferences(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* item_row, float* out) {
  return foldin_estimate_impl(h, n, user_row, item_row, out, true);
}

int malsi_member_anonymous_features(mals_handle h, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row, const float* values, float* out,
                                    int32_t* status_out) {
  return foldin_anonymous(h, n_queries, item_ptr, item_row, values, out, status_out, nullptr, nullptr, "mals_anonymous_features", true);
}

int malsi_member_recommend_to_anonymous(mals_handle h, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row, const float* values,
                                        int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out, int32_t* status_out) {
  return topn_anonymous_impl(h, nullptr, n_queries, item_ptr, item_row, values, how_many, item_idx_out, score_out, n_out, status_out, true);
}

int malsi_member_estimate_for_anonymous(mals_handle h, int32_t n_queries, const int64_t* to_item, const int64_t* item_ptr, const int64_t* item_row,
                                        const float* values, float* out, int32_t* status_out) {
  return foldin_estimate_anonymous_impl(h, n_queries, to_item, item_ptr, item_row, values, out, status_out, true);
}

// ---- mals_ingest_apply (ingest_api.hip holds the records; ids_host.h applies them) --------------------------------------------
int malsi_ingest_apply(mals_handle h, int32_t ingest_device, int64_t n, const int64_t* d_user, const int64_t* d_item, const float* d_value,
                       const uint8_t* d_kind, int64_t* stats_out8, int64_t* removed_user_ids_out, int64_t removed_cap, int64_t* n_removed_out, int* changed_out) {
  *changed_out = 0;
  if (!h) return MALS_INVALID_ARG;
  if (int rc = foldin_refuse(h, "mals_ingest_apply")) return rc;
  if (ingest_device != h->cfg.device) return topn_fail(h, MALS_INVALID_ARG, "mals_ingest_apply: the ingest's records are on another device than the handle");
  if (removed_cap < 0) return topn_fail(h, MALS_INVALID_ARG, "mals_ingest_apply: removed_cap must not be negative");
  if (n > (int64_t)1 << 30) return topn_fail(h, MALS_INVALID_ARG, "mals_ingest_apply: at most 2^30 records per call");
  bool changed = false;
  const int rc = foldin_exclusive(h, "mals_ingest_apply", [&](std::string& msg) -> int {
    return ids_apply_run(h, n, d_user, d_item, d_value, d_kind, stats_out8, removed_user_ids_out, removed_cap, n_removed_out, &changed, msg);
  });
  *changed_out = changed ? 1 : 0;
  return rc;
}

extern "C" int mals_factor_digest(mals_handle h, int side, int64_t row_begin, int64_t n_rows, uint64_t* out) {
  CHECK_SIDE(h, side);
  if (!out) return topn_fail(h, MALS_INVALID_ARG, "mals_factor_digest: out is NULL");
  std::string msg;
  const int rc = malsi_group_factor_digest(&h, 1, side, row_begin, n_rows, out, &msg);
  if (rc != MALS_OK) return topn_fail(h, rc, ("mals_factor_digest: " + msg).c_str());
  return MALS_OK;
}


// ---- rescorers: RecommendIterator's IDRescorer in the form the device runs (topn_kernels.h, RESCORED MODE) ------------
namespace {
uint16_t rescorer_bf16(float v) {   // round to nearest even (finite v)
  uint32_t u;
  std::memcpy(&u, &v, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float rescorer_bf16_value(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// the filter's 16 bytes of one item (topn_kernels.h)
uint4 rescorer_fdata(double s, double o, bool filtered, bool wild = false) {
  if (filtered) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    uint32_t z;
    std::memcpy(&z, &nan, 4);
    return make_uint4(0u, (uint32_t)rescorer_bf16(-0x1p120f), z, 0u);
  }
  const double rs = 1.0 / s, os = o / s;
  const uint16_t rh = rescorer_bf16((float)rs), rl = rescorer_bf16((float)(rs - (double)rescorer_bf16_value(rh)));
  const uint16_t oh = rescorer_bf16((float)os), ol = rescorer_bf16((float)(os - (double)rescorer_bf16_value(oh)));
  const float sf = (float)s;
  uint32_t z;
  std::memcpy(&z, &sf, 4);
  return make_uint4((uint32_t)rh | ((uint32_t)rl << 16), (uint32_t)oh | ((uint32_t)ol << 16), z, wild ? TOPN_FDATA_WILD : 0u);
}
bool rescorer_in_range(double s, double o) {
  return s >= 1.0 / TOPN_RS_MAX_SCALE && s <= TOPN_RS_MAX_SCALE && std::fabs(o) <= TOPN_RS_MAX_OFFSET;
}
// the device side of a new definition (runs as an exclusive ticket: nothing else is on the handle's stream)
int rescorer_upload(mals_handle h, RescorerState& st) {
  const int64_t n_filt = st.filt_idx.empty() ? 0 : st.filt_idx.back() + 1;
  const int64_t n_f = std::max<int64_t>(n_filt, (st.scale.empty() && st.offset.empty()) ? 0 : st.n_rows);
  std::vector<uint32_t> bits((size_t)((n_filt + 31) / 32), 0u);
  for (int64_t i : st.filt_idx) bits[(size_t)(i >> 5)] |= 1u << (i & 31);
  st.filter_ok = rescorer_in_range(st.us, st.uo);
  st.cos_filter_ok = topn_cos_rs_in_range(st.us, st.uo);
  std::vector<uint4> fd((size_t)n_f);
  int64_t n_wild = 0;
  for (int64_t i = 0; i < n_f; ++i) {
    const bool arr = i < st.n_rows;
    const double s = arr && !st.scale.empty() ? st.scale[(size_t)i] : st.us, o = arr && !st.offset.empty() ? st.offset[(size_t)i] : st.uo;
    const bool f = i < n_filt && ((bits[(size_t)(i >> 5)] >> (i & 31)) & 1u);
    if (!f && !rescorer_in_range(s, o)) st.filter_ok = false;
    const bool wild = !f && !topn_cos_rs_in_range(s, o);   // rescored cosine mode: a candidate of every query, up to a few of them
    if (wild && ++n_wild > TOPN_COS_RS_MAX_WILD) st.cos_filter_ok = false;
    fd[(size_t)i] = rescorer_fdata(s, o, f, wild);
  }
  TopnRescore& a = st.args;
  a = TopnRescore();
  if (n_filt) {
    HIPCHK(h, st.d_filt.alloc(bits.size()));
    HIPCHK(h, hipMemcpyAsync(st.d_filt.get(), bits.data(), sizeof(uint32_t) * bits.size(), hipMemcpyHostToDevice, h->stream));
    a.filt = st.d_filt.get();
    a.filt_items = n_filt;
  }
  if (!st.scale.empty()) {
    HIPCHK(h, st.d_scale.alloc(st.scale.size()));
    HIPCHK(h, hipMemcpyAsync(st.d_scale.get(), st.scale.data(), sizeof(double) * st.scale.size(), hipMemcpyHostToDevice, h->stream));
    a.scale = st.d_scale.get();
  }
  if (!st.offset.empty()) {
    HIPCHK(h, st.d_offset.alloc(st.offset.size()));
    HIPCHK(h, hipMemcpyAsync(st.d_offset.get(), st.offset.data(), sizeof(double) * st.offset.size(), hipMemcpyHostToDevice, h->stream));
    a.offset = st.d_offset.get();
  }
  a.n_rows = (st.scale.empty() && st.offset.empty()) ? 0 : st.n_rows;
  a.us = st.us;
  a.uo = st.uo;
  if (n_f) {
    HIPCHK(h, st.d_fdata.alloc((size_t)n_f));
    HIPCHK(h, hipMemcpyAsync(st.d_fdata.get(), fd.data(), sizeof(uint4) * (size_t)n_f, hipMemcpyHostToDevice, h->stream));
    a.fdata = st.d_fdata.get();
    a.n_fdata = n_f;
  }
  a.fdef = rescorer_fdata(st.us, st.uo, false);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MALS_OK;
}
// a new definition = the current one changed by `edit`, swapped in as an exclusive ticket of the front
int rescorer_replace(mals_rescorer r, const char* call, const std::function<std::string(RescorerState&)>& edit) {
  mals_handle h = r->h;
  return foldin_exclusive(h, call, [&](std::string& msg) -> int {
    auto st = std::make_shared<RescorerState>();
    st->filt_idx = r->st->filt_idx;
    st->scale = r->st->scale;
    st->offset = r->st->offset;
    st->n_rows = r->st->n_rows;
    st->us = r->st->us;
    st->uo = r->st->uo;
    msg = edit(*st);
    if (!msg.empty()) return MALS_INVALID_ARG;
    if (int rc = use_device(h)) {
      msg = h->err;
      return rc;
    }
    if (int rc = rescorer_upload(h, *st)) {
      msg = h->err;
      return rc;
    }
    r->st = std::move(st);
    return MALS_OK;
  });
}
template <typename T>
bool rescorer_host_copy(mals_handle h, const T* p, int64_t n, int mem_kind, std::vector<T>& out) {
  out.resize((size_t)n);
  if (n == 0) return true;
  if (mem_kind == MALS_MEM_HOST) {
    std::memcpy(out.data(), p, sizeof(T) * (size_t)n);
    return true;
  }
  return hipMemcpy(out.data(), p, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess;
}
}  // namespace

int mals_rescorer_create(mals_handle h, mals_rescorer* out) {
  if (!h || !out) return MALS_INVALID_ARG;
  mals_rescorer r = new (std::nothrow) mals_rescorer_s();
  if (!r) return fail(h, MALS_OOM, "mals_rescorer_create: out of host memory");
  r->h = h;
  auto st = std::make_shared<RescorerState>();
  st->args.fdef = rescorer_fdata(1.0, 0.0, false);
  r->st = std::move(st);
  *out = r;
  return MALS_OK;
}

int mals_rescorer_destroy(mals_rescorer r) {
  delete r;   // (passes formed with it keep their snapshot)
  return MALS_OK;
}

int mals_rescorer_set_filter(mals_rescorer r, int64_t n, const int64_t* item_idx, int mem_kind) {
  if (!r) return MALS_INVALID_ARG;
  mals_handle h = r->h;
  if (mem_kind != MALS_MEM_HOST && mem_kind != MALS_MEM_DEVICE) return topn_fail(h, MALS_INVALID_ARG, "mals_rescorer_set_filter: bad mem_kind");
  if (n < 0 || (n > 0 && !item_idx)) return topn_fail(h, MALS_INVALID_ARG, "mals_rescorer_set_filter: bad item list");
  std::vector<int64_t> idx;
  if (n > 0 && (mem_kind == MALS_MEM_DEVICE && use_device(h) != MALS_OK)) return MALS_HIP_ERROR;
  if (!rescorer_host_copy(h, item_idx, n, mem_kind, idx)) return topn_fail(h, MALS_HIP_ERROR, "mals_rescorer_set_filter: copy failed");
  return rescorer_replace(r, "mals_rescorer_set_filter", [&](RescorerState& st) -> std::string {
    const int64_t n_items = h->side[MALS_SIDE_Y].n_total;
    for (int64_t i : idx)
      if (i < 0 || i >= n_items) return "item index outside the item factor replica";
    std::sort(idx.begin(), idx.end());
    idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
    st.filt_idx = std::move(idx);
    return std::string();
  });
}

int mals_rescorer_set_weights(mals_rescorer r, const double* scale, const double* offset, int64_t n_rows, int mem_kind) {
  if (!r) return MALS_INVALID_ARG;
  mals_handle h = r->h;
  if (mem_kind != MALS_MEM_HOST && mem_kind != MALS_MEM_DEVICE) return topn_fail(h, MALS_INVALID_ARG, "mals_rescorer_set_weights: bad mem_kind");
  if (n_rows < 0) return topn_fail(h, MALS_INVALID_ARG, "mals_rescorer_set_weights: n_rows < 0");
  std::vector<double> sc, of;
  if (n_rows > 0 && (scale || offset) && mem_kind == MALS_MEM_DEVICE && use_device(h) != MALS_OK) return MALS_HIP_ERROR;
  if ((scale && !rescorer_host_copy(h, scale, n_rows, mem_kind, sc)) || (offset && !rescorer_host_copy(h, offset, n_rows, mem_kind, of)))
    return topn_fail(h, MALS_HIP_ERROR, "mals_rescorer_set_weights: copy failed");
  for (double v : sc)
    if (!(v > 0.0 && v < std::numeric_limits<double>::infinity())) return topn_fail(h, MALS_INVALID_ARG, "mals_rescorer_set_weights: every scale must be finite and > 0");
  for (double v : of)
    if (!std::isfinite(v)) return topn_fail(h, MALS_INVALID_ARG, "mals_rescorer_set_weights: every offset must be finite");
  return rescorer_replace(r, "mals_rescorer_set_weights", [&](RescorerState& st) -> std::string {
    st.scale = std::move(sc);
    st.offset = std::move(of);
    st.n_rows = (st.scale.empty() && st.offset.empty()) ? 0 : n_rows;
    st.us = 1.0;
    st.uo = 0.0;
    return std::string();
  });
}

int mals_rescorer_set_uniform(mals_rescorer r, double scale, double offset) {
  if (!r) return MALS_INVALID_ARG;
  if (!(scale > 0.0 && scale < std::numeric_limits<double>::infinity()) || !std::isfinite(offset))
    return topn_fail(r->h, MALS_INVALID_ARG, "mals_rescorer_set_uniform: scale must be finite and > 0, offset finite");
  return rescorer_replace(r, "mals_rescorer_set_uniform", [&](RescorerState& st) -> std::string {
    st.scale.clear();
    st.offset.clear();
    st.n_rows = 0;
    st.us = scale;
    st.uo = offset;
    return std::string();
  });
}

int mals_recommend_rescored(mals_handle h, mals_rescorer r, const int64_t* user_idx, int32_t n_queries, int32_t how_many,
                            int32_t consider_known_items, int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  return topn_recommend_impl(h, r, user_idx, n_queries, how_many, consider_known_items, item_idx_out, score_out, n_out);
}

int mals_recommend_to_many_rescored(mals_handle h, mals_rescorer r, const float* vectors, const int64_t* vector_ptr, int32_t n_queries,
                                    int32_t how_many, const int64_t* exclude_ptr, const int64_t* exclude_idx, int64_t* item_idx_out,
                                    float* score_out, int32_t* n_out) {
  return topn_to_many_impl(h, r, vectors, vector_ptr, n_queries, how_many, exclude_ptr, exclude_idx, item_idx_out, score_out, n_out);
}

int mals_recommend_to_anonymous_rescored(mals_handle h, mals_rescorer r, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row,
                                         const float* values, int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out,
                                         int32_t* status_out) {
  return topn_anonymous_impl(h, r, n_queries, item_ptr, item_row, values, how_many, item_idx_out, score_out, n_out, status_out);
}

// ---- the candidate filter: LocationSensitiveHash on the device (lsh_kernels.h) --------------------------------------------
// LSH:98-108: accumulate C(H, b) / 2^H for b = 0, 1, ... while b < H and the sum is below the ratio; the last b minus 1.
// ArithmeticUtils.binomialCoefficientDouble is the exact binomial for n <= 66, rounded once to fp64.
int mals_lsh_max_bits_differing(double sample_ratio, int32_t num_hashes, int32_t* out) {
  if (!out || num_hashes < 1 || num_hashes > 64 || !(sample_ratio > 0.0 && sample_ratio <= 1.0)) return MALS_INVALID_ARG;
  double cumulative = 0.0;
  const double denominator = std::ldexp(1.0, num_hashes);
  int bits = -1;
  unsigned __int128 binom = 1;   // C(H, 0)
  while (bits < num_hashes && cumulative < sample_ratio) {
    ++bits;
    if (bits > 0) binom = binom * (unsigned __int128)(num_hashes - bits + 1) / (unsigned __int128)bits;
    cumulative += (double)(uint64_t)binom / denominator;   // (C(64, 32) < 2^61)
  }
  *out = bits - 1;
  return MALS_OK;
}

namespace {
// the device side of a build (an exclusive ticket: nothing else is on the handle's stream, no pass is in flight)
int lsh_build_run(mals_handle h, int H, int mb, const uint8_t* rv, const double* mean, std::string& msg) {
  SideState& y = h->side[MALS_SIDE_Y];
  const int k = h->cfg.features;
  if (!y.F || y.n_total <= 0) {
    msg = "the item factor replica comes first (mals_set_factor_rows)";
    return MALS_INVALID_ARG;
  }
  const int64_t n = y.n_total;
  std::vector<uint64_t> mask((size_t)k, 0ull);
  for (int hh = 0; hh < H; ++hh)
    for (int f = 0; f < k; ++f)
      if (rv[(size_t)hh * k + f]) mask[(size_t)f] |= 1ull << hh;
  LshState nl;
  FCHK(msg, nl.d_mask.alloc((size_t)k));
  FCHK(msg, nl.d_mean.alloc((size_t)k));
  FCHK(msg, nl.d_sig.alloc((size_t)n));
  FCHK(msg, hipMemcpyAsync(nl.d_mask.get(), mask.data(), sizeof(uint64_t) * (size_t)k, hipMemcpyHostToDevice, h->stream));
  DeviceBuffer<double> part;
  if (mean) {
    FCHK(msg, hipMemcpyAsync(nl.d_mean.get(), mean, sizeof(double) * (size_t)k, hipMemcpyHostToDevice, h->stream));
  } else {   // LSH:154-167, in a fixed order
    const int n_part = LSH_MEAN_BLOCKS * lsh_mean_slots(k);
    FCHK(msg, part.alloc((size_t)n_part * (size_t)k));
    hipLaunchKernelGGL(lsh_mean_partial_kernel, dim3(LSH_MEAN_BLOCKS), dim3(256), 0, h->stream, y.F, n, k, part.get());
    hipLaunchKernelGGL(lsh_mean_final_kernel, dim3(1), dim3(128), 0, h->stream, part.get(), n_part, k, n, nl.d_mean.get());
  }
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 63) / 64, (int64_t)h->n_cu * 4));
  const size_t lds = sizeof(float) * 64 * (size_t)(k + 1);
  const int nh = (H + 3) / 4;
  if (nh <= 5)
    hipLaunchKernelGGL(lsh_sign_rows_kernel<5>, dim3(grid), dim3(256), lds, h->stream, y.F, n, k, nl.d_mean.get(), nl.d_mask.get(), H, nl.d_sig.get());
  else if (nh <= 9)
    hipLaunchKernelGGL(lsh_sign_rows_kernel<9>, dim3(grid), dim3(256), lds, h->stream, y.F, n, k, nl.d_mean.get(), nl.d_mask.get(), H, nl.d_sig.get());
  else
    hipLaunchKernelGGL(lsh_sign_rows_kernel<16>, dim3(grid), dim3(256), lds, h->stream, y.F, n, k, nl.d_mean.get(), nl.d_mask.get(), H, nl.d_sig.get());
  FCHK(msg, hipGetLastError());
  FCHK(msg, hipStreamSynchronize(h->stream));   // (the host's mask and the caller's mean are read until here)
  LshState& l = h->lsh;
  std::lock_guard<std::mutex> lk(topn_front(h)->mu);   // (mals_lsh_info reads under it)
  l.d_sig = std::move(nl.d_sig);
  l.d_mask = std::move(nl.d_mask);
  l.d_mean = std::move(nl.d_mean);
  l.H = H;
  l.mb = mb;
  l.n_signed = n;
  return MALS_OK;
}
}  // namespace

int mals_lsh_build(mals_handle h, int32_t num_hashes, int32_t max_bits_differing, const uint8_t* random_vectors, const double* mean) {
  if (!h) return MALS_INVALID_ARG;
  if (int rc = foldin_refuse(h, "mals_lsh_build")) return rc;
  if (num_hashes < 1 || num_hashes > 64) return topn_fail(h, MALS_INVALID_ARG, "mals_lsh_build: num_hashes in 1..64 (LocationSensitiveHash.java:75)");
  if (max_bits_differing < -1 || max_bits_differing > num_hashes) return topn_fail(h, MALS_INVALID_ARG, "mals_lsh_build: max_bits_differing in -1..num_hashes");
  if (!random_vectors) return topn_fail(h, MALS_INVALID_ARG, "mals_lsh_build: random_vectors is NULL");
  return foldin_exclusive(h, "mals_lsh_build", [&](std::string& msg) -> int { return lsh_build_run(h, num_hashes, max_bits_differing, random_vectors, mean, msg); });
}

int mals_lsh_clear(mals_handle h) {
  if (!h) return MALS_INVALID_ARG;
  if (int rc = foldin_refuse(h, "mals_lsh_clear")) return rc;
  return foldin_exclusive(h, "mals_lsh_clear", [&](std::string& msg) -> int {
    FCHK(msg, hipStreamSynchronize(h->stream));
    std::lock_guard<std::mutex> lk(topn_front(h)->mu);
    h->lsh.clear();
    return MALS_OK;
  });
}

// a read of a few words under the front's mutex: no ticket, the serving front is not drained for a statistics query (and
// a member of a group answers too: it has no filter)
int mals_lsh_info(mals_handle h, int64_t* out6) {
  if (!h || !out6) return MALS_INVALID_ARG;
  std::lock_guard<std::mutex> lk(topn_front(h)->mu);
  const LshState& l = h->lsh;
  out6[0] = l.H;
  out6[1] = l.mb;
  out6[2] = l.n_signed;
  out6[3] = h->side[MALS_SIDE_Y].n_total;
  out6[4] = l.q_filter.load();
  out6[5] = l.q_dense.load();
  return MALS_OK;
}

int mals_lsh_get(mals_handle h, double* mean_out, int64_t row_begin, int64_t n_rows, uint64_t* signatures_out) {
  if (!h) return MALS_INVALID_ARG;
  if (int rc = foldin_refuse(h, "mals_lsh_get")) return rc;
  if (n_rows < 0 || row_begin < 0 || (n_rows > 0 && !signatures_out)) return topn_fail(h, MALS_INVALID_ARG, "mals_lsh_get: bad arguments");
  return foldin_exclusive(h, "mals_lsh_get", [&](std::string& msg) -> int {
    const LshState& l = h->lsh;
    if (l.H == 0) {
      msg = "no candidate filter is built (mals_lsh_build)";
      return MALS_INVALID_ARG;
    }
    if (row_begin + n_rows > l.n_signed) {
      msg = "rows outside the rows signed at build time";
      return MALS_INVALID_ARG;
    }
    if (mean_out) FCHK(msg, hipMemcpyAsync(mean_out, l.d_mean.get(), sizeof(double) * (size_t)h->cfg.features, hipMemcpyDeviceToHost, h->stream));
    if (n_rows > 0)
      FCHK(msg, hipMemcpyAsync(signatures_out, l.d_sig.get() + row_begin, sizeof(uint64_t) * (size_t)n_rows, hipMemcpyDeviceToHost, h->stream));
    FCHK(msg, hipStreamSynchronize(h->stream));
    return MALS_OK;
  });
}

int mals_lsh_signatures(mals_handle h, const float* vectors, int32_t n, uint64_t* out) {
  if (!h) return MALS_INVALID_ARG;
  if (int rc = foldin_refuse(h, "mals_lsh_signatures")) return rc;
  if (n < 0 || (n > 0 && (!vectors || !out))) return topn_fail(h, MALS_INVALID_ARG, "mals_lsh_signatures: bad arguments");
  return foldin_exclusive(h, "mals_lsh_signatures", [&](std::string& msg) -> int {
    const LshState& l = h->lsh;
    if (l.H == 0) {
      msg = "no candidate filter is built (mals_lsh_build)";
      return MALS_INVALID_ARG;
    }
    if (n == 0) return MALS_OK;
    const int k = h->cfg.features;
    DeviceBuffer<float> d_v;
    DeviceBuffer<uint64_t> d_s;
    FCHK(msg, d_v.alloc((size_t)n * (size_t)k));
    FCHK(msg, d_s.alloc((size_t)n));
    FCHK(msg, hipMemcpyAsync(d_v.get(), vectors, sizeof(float) * (size_t)n * (size_t)k, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(lsh_sign_vectors_kernel, dim3((unsigned)n), dim3(64), 0, h->stream, d_v.get(), nullptr, (int)n, k, l.d_mean.get(), l.d_mask.get(), l.H,
                       d_s.get(), nullptr, TopnLsh());
    FCHK(msg, hipGetLastError());
    FCHK(msg, hipMemcpyAsync(out, d_s.get(), sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    FCHK(msg, hipStreamSynchronize(h->stream));
    return MALS_OK;
  });
}
