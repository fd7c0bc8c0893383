// mals_internal.h -- entry points shared by the translation units of libmyrrix_als.so, NOT part of the C-ABI
// (include/myrrix_als.h).  mals_group.cpp drives several handles from one thread: it must be able to enqueue the
// direct kernels of EVERY member before any host work (the eigendecomposition of the dual path) starts, and to
// decompose the group's Gramian once instead of once per member.
#pragma once
#include "../../include/myrrix_als.h"

extern "C" {
// mals_solve_chunk in two calls: BEGIN enqueues everything of the chunk that does not need the eigendecomposition
// of the opposite Gramian; when malsi_dual_pending(h) is then 1, the caller runs malsi_dual_host (on one member:
// from = NULL computes it; on the others: from = that member copies it) and END enqueues the rest.
__attribute__((visibility("hidden"))) int malsi_solve_chunk_begin(mals_handle h, int side, int32_t chunk);
__attribute__((visibility("hidden"))) int malsi_solve_chunk_end(mals_handle h, int side, int32_t chunk);
__attribute__((visibility("hidden"))) int malsi_dual_pending(mals_handle h);
__attribute__((visibility("hidden"))) int malsi_dual_host(mals_handle h, int side, mals_handle from);
// mals_gramian_partial / mals_set_gramian with the exact bound on |y| of the split-precision gather: the partial Gramian
// kernels also record max |element| of their rows (device_max: malsi_ymax_slots() caller-zeroed device words, bit patterns
// of floats >= 0, spread over several addresses because same-address atomics serialise; the maximum is what counts);
// the group all-reduces the members' maxima and installs the result with the summed Gramian.
__attribute__((visibility("hidden"))) int malsi_gramian_partial(mals_handle h, int side, int64_t row_begin, int64_t n_rows, double* device_out,
                                                              unsigned* device_max);
__attribute__((visibility("hidden"))) int malsi_ymax_slots(void);
__attribute__((visibility("hidden"))) int malsi_set_gramian(mals_handle h, int side, const double* G, int mem_kind, const unsigned* device_max);
// the event behind which everything a half-iteration sets up once (in its first chunk) is enqueued: a later chunk solved on
// ANOTHER stream waits for it (mals_group.cpp alternates two compute streams between consecutive chunks)
__attribute__((visibility("hidden"))) void* malsi_ready_event(mals_handle h);
// the thread's "why did create fail" text (mals_create_error): set by whichever create call fails, cleared by one that succeeds
__attribute__((visibility("hidden"))) void malsi_set_create_error(const char* text);
// a handle that mals_group_create made for a member: the online write path (mals_set_preferences ...) refuses it
__attribute__((visibility("hidden"))) void malsi_mark_group_member(mals_handle h);
}

// The write path and the fold-in reads of a group (the mals_group_* twins of mals_set_preferences ...; mals_serving.hip).  hs =
// the handles of the local members; every call holds ALL their serving fronts while it enqueues each member's work and
// then waits for each.  own (n_members + 1): member m keeps the known items of the users own[m] <= u < own[m + 1].  A
// failure's text goes to *err.  The caller orders the writes among themselves (the group's write lock).
#include <string>
__attribute__((visibility("hidden"))) int malsi_group_set_foldin_solver(mals_handle* hs, int n_members, int side, mals_solver s, std::string* err);
__attribute__((visibility("hidden"))) int malsi_group_set_foldin_learn_rate(mals_handle* hs, int n_members, double rate, std::string* err);
__attribute__((visibility("hidden"))) int malsi_group_set_preferences(mals_handle* hs, int n_members, const int64_t* own, int64_t n,
                                                                    const int64_t* user_row, const int64_t* item_row, const float* value,
                                                                    int kind, int32_t* status_out, std::string* err);   // kind: 0 preferences, 1 setItemTag, 2 setUserTag
__attribute__((visibility("hidden"))) int malsi_group_remove_preferences(mals_handle* hs, int n_members, const int64_t* own, int64_t n,
                                                                       const int64_t* user_row, const int64_t* item_row, int64_t* removed_users_out,
                                                                       int64_t* n_removed_out, std::string* err);
__attribute__((visibility("hidden"))) int malsi_group_grow_factor_rows(mals_handle* hs, int n_members, int side, int64_t n_rows_total,
                                                                     int grown_owner, std::string* err);
__attribute__((visibility("hidden"))) int malsi_group_factor_digest(mals_handle* hs, int n_members, int side, int64_t row_begin, int64_t n_rows,
                                                                  uint64_t* out, std::string* err);
// mals_group_set_tag_users / mals_group_most_popular_items (popular_host.h): every member counts its own users, member 0 adds
// the partial arrays and selects
__attribute__((visibility("hidden"))) int malsi_group_set_tag_users(mals_handle* hs, int n_members, int64_t n, const int64_t* user_idx, std::string* err);
__attribute__((visibility("hidden"))) int malsi_group_most_popular_items(mals_handle* hs, int n_members, int32_t how_many, int64_t* item_idx_out,
                                                                       float* score_out, int32_t* n_out, std::string* err);
// mals_group_load_generation (generation_group_host.h): loads[m] = the call's arguments as member m reads them (device arrays on
// ITS device); old_bounds_x: the group's bounds[X] (n_members + 1) or NULL; the new bounds (n_members + 1 each) on success
__attribute__((visibility("hidden"))) int malsi_group_load_generation(mals_handle* hs, int n_members, const mals_generation_load* loads,
                                                                    mals_generation_result* result_out, const int64_t* old_bounds_x,
                                                                    int64_t* bounds_x_out, int64_t* bounds_y_out, std::string* err);
// the fold-in reads on one member's handle (any member answers: replicas and solvers are complete everywhere)
__attribute__((visibility("hidden"))) int malsi_member_estimate_preferences(mals_handle h, int64_t n, const int64_t* user_row,
                                                                          const int64_t* item_row, float* out);
__attribute__((visibility("hidden"))) int malsi_member_anonymous_features(mals_handle h, int32_t n_queries, const int64_t* item_ptr,
                                                                        const int64_t* item_row, const float* values, float* out, int32_t* status_out);
__attribute__((visibility("hidden"))) int malsi_member_recommend_to_anonymous(mals_handle h, int32_t n_queries, const int64_t* item_ptr,
                                                                            const int64_t* item_row, const float* values, int32_t how_many,
                                                                            int64_t* item_idx_out, float* score_out, int32_t* n_out,
                                                                            int32_t* status_out);
__attribute__((visibility("hidden"))) int malsi_member_estimate_for_anonymous(mals_handle h, int32_t n_queries, const int64_t* to_item,
                                                                            const int64_t* item_ptr, const int64_t* item_row, const float* values,
                                                                            float* out, int32_t* status_out);

// mals_ingest_apply: the ingest side (ingest_api.hip) checks its own state and hands the serving side (ids_host.h) the records
// as they lie on the device; *changed_out = 0: the call was refused whole and the handle is as it was.  The failure's text is
// the handle's (mals_last_error).
__attribute__((visibility("hidden"))) int malsi_ingest_apply(mals_handle h, int32_t ingest_device, int64_t n, const int64_t* d_user,
                                                           const int64_t* d_item, const float* d_value, const uint8_t* d_kind,
                                                           int64_t* stats_out8, int64_t* removed_user_ids_out, int64_t removed_cap, int64_t* n_removed_out,
                                                           int* changed_out);

// mals_group_ingest_finish (mals_group.cpp) hands the ingest side (ingest_group_host.h) the group's transport: collectives over
// every rank, called with one device buffer per LOCAL member (on that member's device), returning once they are complete.
struct malsi_group_ops {
  void* ctx;
  int32_t world, n_local, features;
  const int32_t* ranks;                                                          // rank of local member i
  int (*allreduce_i64)(void* ctx, int64_t* const* dev, int64_t n, int op_max);   // in place: sum (0) / max (1)
  // send / recv: byte buffers; send_off / recv_off: n_local rows of world + 1 byte offsets (row i: member i's run per peer rank)
  int (*exchange)(void* ctx, const uint8_t* const* send, const int64_t* send_off, uint8_t* const* recv, const int64_t* recv_off);
  // the worst of every rank's status (local_rc: one per local member), through buffers the group already holds (no allocation)
  int (*agree)(void* ctx, const int* local_rc);
  const char* (*last_error)(void* ctx);
};
// the ingest half of mals_group_ingest_finish: every rank returns the same status; on success bounds_x / bounds_y (world + 1)
// are the group's slices and every ingest holds its member's
// the ingest holds a member's slices (mals_group_ingest_finish) or gave its records to one that failed: install / finish refuse it
__attribute__((visibility("hidden"))) int malsi_ingest_spent(mals_ingest g);
// called by mals_group_ingest_finish right before it declares the factor replicas (mals_ingest_memory reports what it saw)
__attribute__((visibility("hidden"))) void malsi_ingest_note_replicas(mals_ingest g);
__attribute__((visibility("hidden"))) int malsi_ingest_shard_finish(mals_ingest* ingests, const malsi_group_ops* ops, int64_t* bounds_x,
                                                                  int64_t* bounds_y);

