// ids_kernels.h -- device side of the id directory a handle keeps per side (mals_ids_*, include/myrrix_als.h; host side in
// ids_host.h), gfx950, wave64.  The directory is row -> id (a dense array) and id -> row: the open-addressing table of
// generation_kernels.h -- 16-byte {key, value} slots, value 0 = empty, row + 1 otherwise, gen_hash, linear probing, at most
// half the slots taken, every 64-bit pattern a legal id.  The hash, the slot count, gen_insert_kernel / gen_fill_keys_kernel
// (mals_ids_set: a whole table with its duplicate check), gen_lookup_kernel (mals_ids_lookup) and the scan's reduce and sums
// come from that header; what is new here is RESOLVE, a lookup that gives an unknown id a row:
//   PROBE   rows[t] = the resident row of ids[t].  A miss goes into a table of the batch (zeroed, gen_table_slots(n) slots)
//           whose value word holds t + 1: it claims a slot by a 64-bit compare-and-swap from 0, and where it meets its own key
//           -- read through ids[value - 1], as gen_insert_kernel reads it: the key words of this table are never written --
//           it lowers the value with a 64-bit atomic min.  A slot's key never changes once claimed (a value is only ever
//           replaced by a position with the same id), slots are never freed, so every position of one id ends at the same
//           slot, whatever the order, and when the kernel is done that slot holds the SMALLEST position of the id + 1.
//   FIRST   first[t] = the slot of t holds t + 1: t is where its id first appears in the batch.
//   SCAN    exclusive scan of first (gen_scan_reduce_kernel, gen_scan_sums_kernel, and the apply fused into ASSIGN).
//   ASSIGN  a first occurrence gets row n_rows + its rank among the first occurrences -- the order of first appearance --
//           and its id is appended to row -> id;  FOLLOW: every other miss takes the row of the position its slot names.
//   INSERT  rows [a, b) of row -> id into the resident table (the new rows, or every row into a larger table).  The ids
//           are distinct and none is in the table, so a taken slot is always another id's: claim by compare-and-swap,
//           then write the key word, which nothing reads before the kernel is done.
// Nothing depends on the grid or on the order in which the hardware runs the positions: the result is that of a
// dictionary that reads the batch front to back (tests/cpp/test_ingest_live_plan.cpp runs the slot functions below on
// the CPU in every order of a batch's positions).
#pragma once
#include "generation_kernels.h"

namespace mals {

constexpr uint64_t IDS_NO_SLOT = ~(uint64_t)0;

// ---- the slot functions: host and device (on the host they run single-threaded, plain loads and stores) ---------------------
MALS_GEN_HD inline unsigned long long ids_cas_u64(unsigned long long* p, unsigned long long expect, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(p, expect, v);
#else
  const unsigned long long old = *p;
  if (old == expect) *p = v;
  return old;
#endif
}

MALS_GEN_HD inline void ids_min_u64(unsigned long long* p, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, v);
#else
  if (v < *p) *p = v;
#endif
}

// a complete table (every taken slot's key word written): the row of `id`, or -1
MALS_GEN_HD inline int64_t ids_find(const unsigned long long* table, uint64_t mask, int64_t id) {
  uint64_t s = gen_hash(id) & mask;
  for (;;) {
#if defined(__HIP_DEVICE_COMPILE__)
    const ulonglong2 kv = *reinterpret_cast<const ulonglong2*>(table + 2 * s);   // (one 16-byte load: a hipMalloc block)
    const unsigned long long key = kv.x, val = kv.y;
#else
    const unsigned long long key = table[2 * s], val = table[2 * s + 1];
#endif
    if (val == 0ull) return -1;
    if ((int64_t)key == id) return (int64_t)val - 1;
    s = (s + 1) & mask;
  }
}

// the batch's table: position t joins the slot of ids[t] (claiming it when the id has none) -> that slot.  Afterwards the
// slot's value word is 1 + the smallest position that joined it.
MALS_GEN_HD inline uint64_t ids_batch_claim(unsigned long long* batch, uint64_t mask, const int64_t* ids, int64_t t) {
  const int64_t id = ids[t];
  uint64_t s = gen_hash(id) & mask;
  for (;;) {
    const unsigned long long old = ids_cas_u64(&batch[2 * s + 1], 0ull, (unsigned long long)(t + 1));
    if (old == 0ull) return s;
    if (ids[old - 1] == id) {
      ids_min_u64(&batch[2 * s + 1], (unsigned long long)(t + 1));
      return s;
    }
    s = (s + 1) & mask;
  }
}

// once every position has joined: the position where the id of slot s first appears
MALS_GEN_HD inline int64_t ids_batch_first_pos(const unsigned long long* batch, uint64_t s) { return (int64_t)batch[2 * s + 1] - 1; }

// an id that is not in the table (nor is any id inserted beside it) gets `row`
MALS_GEN_HD inline void ids_insert_distinct(unsigned long long* table, uint64_t mask, int64_t id, int64_t row) {
  uint64_t s = gen_hash(id) & mask;
  while (ids_cas_u64(&table[2 * s + 1], 0ull, (unsigned long long)(row + 1)) != 0ull) s = (s + 1) & mask;
  table[2 * s] = (unsigned long long)id;
}

// slots of a table that holds n ids, reached from `slots` by doubling (the table is rebuilt before it would pass half full)
MALS_GEN_HD inline uint64_t ids_grown_slots(uint64_t slots, int64_t n) {
  uint64_t s = slots < 64 ? 64 : slots;
  while (s < 2 * (uint64_t)(n < 0 ? 0 : n)) s <<= 1;
  return s;
}

#if defined(__HIPCC__)

// PROBE.  table: the resident one (complete; NULL: an empty directory, every position a miss); batch: zeroed.  rows[t]: the
// resident row or -1; slot[t]: IDS_NO_SLOT for a hit
__global__ __launch_bounds__(256) void ids_probe_kernel(const int64_t* __restrict__ ids, int64_t n, const unsigned long long* __restrict__ table,
                                                        uint64_t mask, unsigned long long* batch, uint64_t batch_mask, int64_t* __restrict__ rows,
                                                        uint64_t* __restrict__ slot) {
  MALS_GEN_STRIDE(t, n) {
    const int64_t r = table ? ids_find(table, mask, ids[t]) : -1;
    rows[t] = r;
    slot[t] = r >= 0 ? IDS_NO_SLOT : ids_batch_claim(batch, batch_mask, ids, t);
  }
}

// FIRST
__global__ __launch_bounds__(256) void ids_first_kernel(const unsigned long long* __restrict__ batch, const uint64_t* __restrict__ slot, int64_t n,
                                                        unsigned* __restrict__ first) {
  MALS_GEN_STRIDE(t, n) first[t] = (slot[t] != IDS_NO_SLOT && ids_batch_first_pos(batch, slot[t]) == t) ? 1u : 0u;
}

// mals_ids_set: the smallest position that is not its id's first (repeat: set to all ones first), one atomic per wave
__global__ __launch_bounds__(256) void ids_min_repeat_kernel(const unsigned* __restrict__ first, int64_t n, unsigned long long* __restrict__ repeat) {
  unsigned long long mine = ~0ull;
  MALS_GEN_STRIDE(t, n)
    if (first[t] == 0u && (unsigned long long)t < mine) mine = (unsigned long long)t;
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_down(mine, d, 64);
    mine = o < mine ? o : mine;
  }
  if ((threadIdx.x & 63) == 0 && mine != ~0ull) atomicMin(repeat, mine);
}

// ASSIGN (the scan's apply, tile by tile as gen_map_kernel): row_id has room for n_rows + the first occurrences
__global__ __launch_bounds__(256) void ids_assign_kernel(const unsigned* __restrict__ first, int64_t n, const unsigned* __restrict__ tile_offsets,
                                                         const int64_t* __restrict__ ids, int64_t n_rows, int64_t* __restrict__ rows,
                                                         int64_t* __restrict__ row_id) {
  const int64_t b = (int64_t)blockIdx.x * GEN_SCAN_TILE + threadIdx.x * 8;
  unsigned v[8], s = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = b + i < n ? first[b + i] : 0u;
    s += v[i];
  }
  unsigned pre = tile_offsets[blockIdx.x] + gen_block_scan(s, nullptr);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (v[i]) {   // (v[i] != 0 only inside the array)
      rows[b + i] = n_rows + (int64_t)pre;
      row_id[n_rows + (int64_t)pre] = ids[b + i];
      ++pre;
    }
  }
}

// FOLLOW (after ASSIGN: it reads the rows of the first occurrences, which it never writes)
__global__ __launch_bounds__(256) void ids_follow_kernel(const unsigned long long* __restrict__ batch, const uint64_t* __restrict__ slot,
                                                         const unsigned* __restrict__ first, int64_t n, int64_t* rows) {
  MALS_GEN_STRIDE(t, n)
    if (slot[t] != IDS_NO_SLOT && first[t] == 0u) rows[t] = rows[ids_batch_first_pos(batch, slot[t])];
}

// INSERT
__global__ __launch_bounds__(256) void ids_insert_rows_kernel(const int64_t* __restrict__ row_id, int64_t row_begin, int64_t row_end,
                                                              unsigned long long* table, uint64_t mask) {
  MALS_GEN_STRIDE(i, row_end - row_begin) ids_insert_distinct(table, mask, row_id[row_begin + i], row_begin + i);
}

#endif   // __HIPCC__

}  // namespace mals
