// ingest_api.hip -- the ingest -> CSR path (mals_ingest_*, include/myrrix_als.h) as one translation unit: its kernel
// headers, then its host headers in dependency order, then the C entry points of the record path and the one-shot finish.
// Everything between "records appended" and "two CSR matrices + id tables in HBM" runs on the device; the host only
// sequences kernels and reads back a few counters.
#include "../../include/myrrix_als.h"
#include "mals_internal.h"
#include "hip_buffer.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <limits>
#include <new>

// kernels
#include "ingest_kernels.h"
#include "ingest_text_kernels.h"
#include "ingest_big_kernels.h"
#include "split_kernels.h"

using namespace mals;

// host: what all finishers share, the partitioned finish, text -> records (with its entry points), the group finish (with its)
#include "ingest_host.h"
#include "ingest_big_host.h"
#include "ingest_text_host.h"
#include "ingest_group_host.h"

namespace {

// e0: recorded where the pipeline proper starts (behind the workspace allocations)
int finish_impl(mals_ingest g, hipEvent_t e0) {
  const int64_t n = g->n;
  g->last_partitions = g->last_item_ranges = 0;
  if (n == 0) {
    ICHK(g, hipEventRecord(e0, g->stream));
    ITRY(alloc_results(g, 0, 0, 0));
    ICHK(g, hipMemsetAsync(g->ptr[0].get(), 0, sizeof(int64_t), g->stream));
    ICHK(g, hipMemsetAsync(g->ptr[1].get(), 0, sizeof(int64_t), g->stream));
    if (g->want_known) {
      ICHK(g, g->known_ptr.alloc(1));
      ICHK(g, g->known_idx.alloc(1));
      ICHK(g, hipMemsetAsync(g->known_ptr.get(), 0, sizeof(int64_t), g->stream));
    }
    return MALS_OK;
  }
  // more records than one sort pipeline holds (or than the caller wants it to hold): user range by user range
  if (n > MALS_INGEST_ONE_SHOT_MAX || (g->part_cap > 0 && n > g->part_cap))
    return finish_big(g, e0, g->part_cap);   // 0: ranges as large as the free memory holds
  Scratch s;
  ITRY(setup_workspace(g, s, n, 0));
  ICHK(g, hipEventRecord(e0, g->stream));
  IdWidth width;
  ITRY(probe_id_width(g, s, &width));
  RangeTmp t;
  RangeCounts c;
  ITRY(finish_range(g, s, t, Records{g->d_user.get(), g->d_item.get(), g->d_value.get(), n}, width,
                    RangeOut{true, g->ids[0], g->ptr[0], g->known_ptr, 0, 0}, c));
  g->n_known = c.n_known;
  // 7. the transposed matrix: the entries are sorted by (user, item)
  const int64_t nnz = c.nnz, n_items = c.n_items;
  if (nnz > 0) {
    ITRY(launch(g, nnz, transpose_keys_kernel, s.coo_row, g->col[0].get(), g->val[0].get(), nnz, s.keys[0], s.pay[0]));
    g->bytes_moved += 24.0 * (double)nnz + 24.0 * (double)nnz;   // the keys built; the gather
  }
  ITRY(transpose_by_item(g, s, nnz, n_items, g->ptr[1].get(), g->col[1].get(), g->val[1].get()));
  g->bytes_moved += 4.0 * (double)nnz + 8.0 * (double)n_items;
  ITRY(finish_tags(g, s, n));
  ICHK(g, hipStreamSynchronize(g->stream));
  return MALS_OK;
}

}  // namespace

extern "C" {

int mals_ingest_create(int32_t device, float zero_threshold, mals_ingest* out) {
  if (!out) return MALS_INVALID_ARG;
  *out = nullptr;
  if (!(zero_threshold >= 0.f)) return MALS_INVALID_ARG;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return MALS_HIP_ERROR;
  mals_ingest g = new (std::nothrow) mals_ingest_s();
  if (!g) return MALS_OOM;
  g->device = device;
  g->zero_threshold = zero_threshold;
  *out = g;
  return MALS_OK;
}

int mals_ingest_destroy(mals_ingest g) {
  if (!g) return MALS_INVALID_ARG;
  (void)hipSetDevice(g->device);
  (void)hipStreamSynchronize(g->stream);
  delete g;   // (its buffers and events go on its device)
  return MALS_OK;
}

const char* mals_ingest_last_error(mals_ingest g) { return g ? g->err.c_str() : "null ingest handle"; }

int mals_ingest_append(mals_ingest g, int64_t n, const int64_t* user_ids, const int64_t* item_ids, const float* values,
                       int mem_kind) {
  if (!g) return MALS_INVALID_ARG;
  if (n < 0 || (n > 0 && (!user_ids || !item_ids || !values))) return fail(g, MALS_INVALID_ARG, "bad record arrays");
  if (mem_kind != MALS_MEM_HOST && mem_kind != MALS_MEM_DEVICE) return fail(g, MALS_INVALID_ARG, "mem_kind must be MALS_MEM_HOST or MALS_MEM_DEVICE");
  if (g->spent) return fail(g, MALS_INVALID_ARG, "the ingest's records went into mals_group_ingest_finish: create a new ingest");
  if (g->n + n >= MALS_INGEST_MAX_RECORDS) return fail(g, MALS_INVALID_ARG, "at most 2^36 records per ingest");
  if (n == 0) return MALS_OK;
  ICHK(g, hipSetDevice(g->device));
  if (g->finished) g->free_results();
  const int64_t cap = record_capacity(g);
  if (g->n + n > cap) ITRY(grow_records(g, std::max<int64_t>(g->n + n, cap * 2)));
  const hipMemcpyKind kind = mem_kind == MALS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  ICHK(g, hipMemcpyAsync(g->d_user.get() + g->n, user_ids, sizeof(int64_t) * (size_t)n, kind, g->stream));
  ICHK(g, hipMemcpyAsync(g->d_item.get() + g->n, item_ids, sizeof(int64_t) * (size_t)n, kind, g->stream));
  ICHK(g, hipMemcpyAsync(g->d_value.get() + g->n, values, sizeof(float) * (size_t)n, kind, g->stream));
  if (g->live_tags) ICHK(g, hipMemsetAsync(g->d_kind.get() + g->n, 0, (size_t)n, g->stream));   // records are preferences
  ICHK(g, hipStreamSynchronize(g->stream));
  g->n += n;
  return MALS_OK;
}

int mals_ingest_finish(mals_ingest g) {
  if (!g) return MALS_INVALID_ARG;
  if (g->spent) return fail(g, MALS_INVALID_ARG, "the ingest's records went into mals_group_ingest_finish: create a new ingest");
  if (g->text_failed) return fail(g, g->text_fail_code, g->text_fail_msg);
  if (g->carry_len) return fail(g, MALS_INVALID_ARG, "text pending: the last mals_ingest_append_text of a file must say end_of_file");
  ICHK(g, hipSetDevice(g->device));
  g->free_results();
  g->bytes_moved = 0.0;
  g->radix_passes = 0;
  EventPair ev;
  ICHK(g, ev.ensure());
  g->last_workspace_ms = 0.0;
  const int rc = finish_impl(g, ev.begin);
  if (rc != MALS_OK) {
    g->free_results();
    return rc;
  }
  ICHK(g, hipEventRecord(ev.end, g->stream));
  ICHK(g, hipEventSynchronize(ev.end));
  float ms = 0.f;
  ICHK(g, hipEventElapsedTime(&ms, ev.begin, ev.end));
  g->last_finish_ms = ms;
  g->finished = true;
  return MALS_OK;
}

int mals_ingest_counts(mals_ingest g, int64_t* n_records, int64_t* n_users, int64_t* n_items, int64_t* nnz) {
  if (!g) return MALS_INVALID_ARG;
  if (n_records) *n_records = g->sharded ? g->shard_records : g->n;
  if (!g->finished && (n_users || n_items || nnz)) return fail(g, MALS_INVALID_ARG, "mals_ingest_finish has not run");
  if (n_users) *n_users = g->n_users;
  if (n_items) *n_items = g->n_items;
  if (nnz) *nnz = g->nnz;
  return MALS_OK;
}

int mals_ingest_get_ids(mals_ingest g, int side, int64_t* host_ids_out) {
  if (!g || !host_ids_out) return MALS_INVALID_ARG;
  if (side != MALS_SIDE_X && side != MALS_SIDE_Y) return fail(g, MALS_INVALID_ARG, "side must be MALS_SIDE_X or _Y");
  if (!g->finished) return fail(g, MALS_INVALID_ARG, "mals_ingest_finish has not run");
  ICHK(g, hipSetDevice(g->device));
  const int64_t cnt = side == MALS_SIDE_X ? g->n_users : g->n_items;
  if (cnt) ICHK(g, hipMemcpy(host_ids_out, g->ids[side].get(), sizeof(int64_t) * (size_t)cnt, hipMemcpyDeviceToHost));
  return MALS_OK;
}

int mals_ingest_get_csr(mals_ingest g, int side, int64_t* host_row_ptr, int32_t* host_col_idx, float* host_val) {
  if (!g) return MALS_INVALID_ARG;
  if (side != MALS_SIDE_X && side != MALS_SIDE_Y) return fail(g, MALS_INVALID_ARG, "side must be MALS_SIDE_X or _Y");
  if (!g->finished) return fail(g, MALS_INVALID_ARG, "mals_ingest_finish has not run");
  ICHK(g, hipSetDevice(g->device));
  const int64_t rows = g->sharded ? g->slice_rows[side] : side == MALS_SIDE_X ? g->n_users : g->n_items;
  const int64_t nnz = g->sharded ? g->slice_nnz[side] : g->nnz;
  if (host_row_ptr) ICHK(g, hipMemcpy(host_row_ptr, g->ptr[side].get(), sizeof(int64_t) * (size_t)(rows + 1), hipMemcpyDeviceToHost));
  if (host_col_idx && nnz) ICHK(g, hipMemcpy(host_col_idx, g->col[side].get(), sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost));
  if (host_val && nnz) ICHK(g, hipMemcpy(host_val, g->val[side].get(), sizeof(float) * (size_t)nnz, hipMemcpyDeviceToHost));
  return MALS_OK;
}

int mals_ingest_device_csr(mals_ingest g, int side, const int64_t** row_ptr, const int32_t** col_idx, const float** val) {
  if (!g) return MALS_INVALID_ARG;
  if (side != MALS_SIDE_X && side != MALS_SIDE_Y) return fail(g, MALS_INVALID_ARG, "side must be MALS_SIDE_X or _Y");
  if (!g->finished) return fail(g, MALS_INVALID_ARG, "mals_ingest_finish has not run");
  if (row_ptr) *row_ptr = g->ptr[side].get();
  if (col_idx) *col_idx = g->col[side].get();
  if (val) *val = g->val[side].get();
  return MALS_OK;
}

int mals_ingest_install(mals_ingest g, mals_handle h) {
  if (!g || !h) return MALS_INVALID_ARG;
  if (!g->finished) return fail(g, MALS_INVALID_ARG, "mals_ingest_finish has not run");
  if (g->sharded || g->spent) return fail(g, MALS_INVALID_ARG, "the ingest holds one member's slices (mals_group_ingest_finish)");
  if (int rc = mals_set_matrix(h, MALS_SIDE_X, 0, g->n_users, g->nnz, g->ptr[0].get(), g->col[0].get(), g->val[0].get(), MALS_MEM_DEVICE))
    return fail(g, rc, mals_last_error(h));
  if (int rc = mals_set_matrix(h, MALS_SIDE_Y, 0, g->n_items, g->nnz, g->ptr[1].get(), g->col[1].get(), g->val[1].get(), MALS_MEM_DEVICE))
    return fail(g, rc, mals_last_error(h));
  // knownItemIDs, if they were asked for: what mals_recommend skips (ServerRecommender.java:394-425), entries that
  // removeSmall pruned from R included
  // (mals_set_matrix(side X) has dropped whatever known items an earlier install left on the handle)
  if (g->known_ptr)
    if (int rc = mals_set_known_items(h, g->n_users, g->known_ptr.get(), g->known_idx.get(), MALS_MEM_DEVICE)) return fail(g, rc, mals_last_error(h));
  // userTagIDs: rows of Y top-N never returns (RecommendIterator.java:72).  Needs the item factor rows: declare them here if
  // the caller has not (a caller-bound or larger replica is left alone).
  void* fy = nullptr;
  int64_t fy_rows = 0;
  (void)mals_factor_device_ptr(h, MALS_SIDE_Y, &fy, &fy_rows);
  if (g->n_tag_ids[1] > 0 && (!fy || fy_rows < g->n_items))
    if (int rc = mals_set_factor_rows(h, MALS_SIDE_Y, g->n_items)) return fail(g, rc, mals_last_error(h));
  if (int rc = mals_set_tag_items(h, g->n_tag_ids[1], g->tag_item_idx.get(), MALS_MEM_DEVICE)) return fail(g, rc, mals_last_error(h));
  // itemTagIDs as rows of R: the "users" mals_most_popular_items does not count (ServerRecommender.java:631-638); -1 (a tag
  // that owns no row) is outside the handle's users and ignored there.  (mals_set_matrix(side X) has dropped an earlier set.)
  if (g->n_tag_ids[0] > 0) {
    ICHK(g, hipSetDevice(g->device));
    DeviceBuffer<int64_t> tag_user_idx;
    ICHK(g, tag_user_idx.alloc((size_t)g->n_tag_ids[0]));
    ITRY(launch(g, g->n_tag_ids[0], index_of_ids_kernel, g->tag_ids[0].get(), g->n_tag_ids[0], g->ids[0].get(), g->n_users, tag_user_idx.get()));
    ICHK(g, hipStreamSynchronize(g->stream));
    if (int rc = mals_set_tag_users(h, g->n_tag_ids[0], tag_user_idx.get(), MALS_MEM_DEVICE)) return fail(g, rc, mals_last_error(h));
  }
  return MALS_OK;
}

// ServerRecommender.ingest(Reader): the records appended since the ingest's creation or its last apply go into the live model
// of h (ids_host.h).  Refused whole -- nothing changed, the records stay -- unless the ingest could still be finished and
// has seen no tag (with MALS_INGEST_OPT_LIVE_TAGS its tag lines are writes like the others); afterwards the records are released and the stream's counters and carried partial line stay.
int mals_ingest_apply(mals_ingest g, mals_handle h, int64_t* stats_out8, int64_t* removed_user_ids_out, int64_t removed_cap, int64_t* n_removed_out) {
  if (!g || !h) return MALS_INVALID_ARG;
  if (n_removed_out) *n_removed_out = 0;
  if (stats_out8) std::memset(stats_out8, 0, 8 * sizeof(int64_t));
  if (g->spent || g->sharded) return fail(g, MALS_INVALID_ARG, "mals_ingest_apply: the ingest's records went into mals_group_ingest_finish");
  if (g->finished) return fail(g, MALS_INVALID_ARG, "mals_ingest_apply: the ingest is finished (its records became matrices: mals_ingest_install)");
  if (g->text_failed) return fail(g, MALS_INVALID_ARG, "mals_ingest_apply: the ingest's text has failed (" + g->text_fail_msg + "); nothing of it is applied");
  if (!g->live_tags && (g->n_tags_raw[0] || g->n_tags_raw[1]))
    return fail(g, MALS_INVALID_ARG, "mals_ingest_apply: the text holds tag lines (setUserTag / setItemTag), which the live write path does not serve");
  ICHK(g, hipSetDevice(g->device));
  ICHK(g, hipStreamSynchronize(g->stream));   // the records are whole before the handle's stream reads them
  int changed = 0;
  const int rc = malsi_ingest_apply(h, g->device, g->n, g->d_user.get(), g->d_item.get(), g->d_value.get(), g->live_tags ? g->d_kind.get() : nullptr,
                                    stats_out8, removed_user_ids_out, removed_cap, n_removed_out, &changed);
  if (rc != MALS_OK) g->err = std::string("mals_ingest_apply: ") + mals_last_error(h);
  if (rc == MALS_OK || changed) {   // applied (a failed update is reported, the others went on): released
    g->n = 0;
    if (g->live_tags) g->n_tags_raw[0] = g->n_tags_raw[1] = 0;   // (the tag lines were among them)
  }
  return rc;
}

// tagHasher.toLongID(tag): the parser's own hash (text_parse.h) of the token "<tag>"
int mals_tag_id_host(const void* utf8, int64_t n_bytes, int64_t* id_out) {
  if (!id_out || n_bytes < 0 || n_bytes > (int64_t)1 << 30 || (n_bytes > 0 && !utf8)) return MALS_INVALID_ARG;
  std::string token((size_t)n_bytes + 2, '"');
  if (n_bytes) std::memcpy(&token[1], utf8, (size_t)n_bytes);
  const text::PtrSrc src{reinterpret_cast<const uint8_t*>(token.data())};
  *id_out = text::tag_to_long(src, 0, (uint32_t)token.size());
  return MALS_OK;
}

int mals_ingest_device(mals_ingest g, int32_t* device_out) {
  if (!g || !device_out) return MALS_INVALID_ARG;
  *device_out = g->device;
  return MALS_OK;
}

int mals_ingest_get_tag_items(mals_ingest g, int64_t* host_idx_out) {
  if (!g || !host_idx_out) return MALS_INVALID_ARG;
  if (!g->finished) return fail(g, MALS_INVALID_ARG, "mals_ingest_finish has not run");
  ICHK(g, hipSetDevice(g->device));
  if (g->n_tag_ids[1]) ICHK(g, hipMemcpy(host_idx_out, g->tag_item_idx.get(), sizeof(int64_t) * (size_t)g->n_tag_ids[1], hipMemcpyDeviceToHost));
  return MALS_OK;
}

int mals_ingest_device_tag_items(mals_ingest g, const int64_t** device_idx_out, int64_t* n_out) {
  if (!g) return MALS_INVALID_ARG;
  if (!g->finished) return fail(g, MALS_INVALID_ARG, "mals_ingest_finish has not run");
  if (device_idx_out) *device_idx_out = g->tag_item_idx.get();
  if (n_out) *n_out = g->n_tag_ids[1];
  return MALS_OK;
}

int mals_ingest_partitions(mals_ingest g, int32_t* user_ranges, int32_t* item_ranges) {
  if (!g) return MALS_INVALID_ARG;
  if (user_ranges) *user_ranges = g->last_partitions;
  if (item_ranges) *item_ranges = g->last_item_ranges;
  return MALS_OK;
}

int mals_ingest_stats(mals_ingest g, double* finish_ms, double* workspace_ms, double* bytes_moved, int32_t* radix_passes) {
  if (!g) return MALS_INVALID_ARG;
  if (finish_ms) *finish_ms = g->last_finish_ms;
  if (workspace_ms) *workspace_ms = g->last_workspace_ms;
  if (bytes_moved) *bytes_moved = g->bytes_moved;
  if (radix_passes) *radix_passes = g->radix_passes;
  return MALS_OK;
}

}  // extern "C"
