// generation_kernels.h -- device side of mals_load_generation (include/myrrix_als.h; host side in generation_host.h),
// gfx950, wave64.  GenerationLoader.loadModel (GenerationLoader.java:49-106) restated for dense rows:
//   JOIN    the ids of a side's new rows go into an open-addressing table (linear probing); every live id probes it once.
//           SLOTS: gen_table_slots(n) = the smallest power of two >= max(64, 2 n), so at most half the slots are taken and
//           every probe chain ends at an empty slot.  A slot is 16 bytes {key, value}: value 0 = empty, j + 1 = row j of
//           the inserted array.  Every 64-bit pattern is a legal id, so the key word cannot say whether a slot is taken:
//           an insert claims a slot by a 64-bit compare-and-swap of the VALUE word from 0 to j + 1.  While inserts run the
//           key of a taken slot is read where it cannot be half-written -- ids[value - 1], the caller's array -- and the
//           key words are filled by a pass of their own afterwards (gen_fill_keys_kernel), so that a probe costs one
//           16-byte load per slot.  An insert that meets its own key reports a duplicate (the smallest row that did).
//   KEEP    keep[r] = the probe missed and (row r is recent or every row is kept): removeNotUpdated (:137-152).
//   SCAN    exclusive scan of keep over any number of 2048-row tiles (reduce, one block over the tile sums, apply).
//   MAP     live row -> merged row: j for a hit (updateMap is a put, :117-126), n_new + scan[r] for a kept row, else -1;
//           the kept rows in their live order as a list.
//   GATHER  the kept live rows into the tail of the new replica; the new rows into its head (a flat copy).
//   TAGS    userTagIDs of the live generation (one bit per live item) onto merged rows.
// Nothing here is floating-point arithmetic: rows are copied bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MALS_GEN_HD __host__ __device__
#else
#define MALS_GEN_HD
#endif

namespace mals {

constexpr uint64_t GEN_HASH_MUL_A = 0x9E3779B97F4A7C15ull;
constexpr uint64_t GEN_HASH_MUL_B = 0xD6E8FEB86659FD93ull;

// mals_generation_hash_host: the home slot of an id is gen_hash(id) & (slots - 1)
MALS_GEN_HD inline uint64_t gen_hash(int64_t id) {
  uint64_t z = (uint64_t)id * GEN_HASH_MUL_A;
  z ^= z >> 32;
  z *= GEN_HASH_MUL_B;
  z ^= z >> 32;
  return z;
}

MALS_GEN_HD inline uint64_t gen_table_slots(int64_t n) {
  uint64_t s = 64;
  while (s < 2 * (uint64_t)(n < 0 ? 0 : n)) s <<= 1;
  return s;
}

#if defined(__HIPCC__)

constexpr int GEN_SCAN_TILE = 2048;   // 256 threads x 8 rows

#define MALS_GEN_STRIDE(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// table: slots x {key, value}, zeroed by the caller.  dup: the smallest row whose insert met its own key (caller: set to
// LLONG_MAX's bit pattern first).
__global__ __launch_bounds__(256) void gen_insert_kernel(const int64_t* __restrict__ ids, int64_t n, unsigned long long* table, uint64_t mask,
                                                         unsigned long long* __restrict__ dup) {
  MALS_GEN_STRIDE(j, n) {
    const int64_t id = ids[j];
    uint64_t s = gen_hash(id) & mask;
    for (;;) {
      const unsigned long long old = atomicCAS(&table[2 * s + 1], 0ull, (unsigned long long)(j + 1));
      if (old == 0ull) break;
      if (ids[old - 1] == id) {   // (the other row's id from the caller's array: the slot's key word is not written yet)
        atomicMin(dup, (unsigned long long)j);
        break;
      }
      s = (s + 1) & mask;
    }
  }
}

__global__ __launch_bounds__(256) void gen_fill_keys_kernel(const int64_t* __restrict__ ids, unsigned long long* __restrict__ table, uint64_t slots) {
  MALS_GEN_STRIDE(s, (int64_t)slots) {
    const unsigned long long v = table[2 * s + 1];
    if (v != 0ull) table[2 * s] = (unsigned long long)ids[v - 1];
  }
}

// one probe chain: the row of the inserted array that holds `id`, or -1 (16-byte loads: the table is a hipMalloc block)
__device__ __forceinline__ int64_t gen_probe(const unsigned long long* __restrict__ table, uint64_t mask, int64_t id) {
  uint64_t s = gen_hash(id) & mask;
  for (;;) {
    const ulonglong2 kv = *reinterpret_cast<const ulonglong2*>(table + 2 * s);
    if (kv.y == 0ull) return -1;
    if ((int64_t)kv.x == id) return (int64_t)kv.y - 1;
    s = (s + 1) & mask;
  }
}

// the live ids against the table of the new ids: map[r] = the new row (hit) or -1; keep[r] as above.  recent: one bit per
// live row (nullable: none).  n_hit: the hits, one atomic per wave.
__global__ __launch_bounds__(256) void gen_probe_kernel(const int64_t* __restrict__ cur_ids, int64_t n_cur, const unsigned long long* __restrict__ table,
                                                        uint64_t mask, const uint32_t* __restrict__ recent, int keep_all, int64_t* __restrict__ map,
                                                        unsigned* __restrict__ keep, unsigned long long* __restrict__ n_hit) {
  unsigned long long mine = 0;
  MALS_GEN_STRIDE(r, n_cur) {
    const int64_t j = gen_probe(table, mask, cur_ids[r]);
    const bool rec = keep_all != 0 || (recent != nullptr && ((recent[r >> 5] >> (r & 31)) & 1u) != 0u);
    map[r] = j;
    keep[r] = (j < 0 && rec) ? 1u : 0u;
    mine += j >= 0 ? 1ull : 0ull;
  }
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_hit, mine);
}

// ids -> rows of the inserted array (-1: none): the updated tag ids against the new model's table
__global__ __launch_bounds__(256) void gen_lookup_kernel(const int64_t* __restrict__ ids, int64_t n, const unsigned long long* __restrict__ table,
                                                         uint64_t mask, int64_t* __restrict__ rows_out) {
  MALS_GEN_STRIDE(i, n) rows_out[i] = gen_probe(table, mask, ids[i]);
}

// ---- exclusive scan of the keep flags -------------------------------------------------------------------------------
__device__ __forceinline__ unsigned gen_block_scan(unsigned v, unsigned* total) {   // exclusive, 256 threads
  __shared__ unsigned ws[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) ws[w] = x;
  __syncthreads();
  unsigned pre = 0;
  for (int i = 0; i < w; ++i) pre += ws[i];
  if (total) *total = ws[0] + ws[1] + ws[2] + ws[3];
  __syncthreads();
  return pre + x - v;
}

__global__ __launch_bounds__(256) void gen_scan_reduce_kernel(const unsigned* __restrict__ keep, int64_t n, unsigned* __restrict__ tile_sums) {
  const int64_t b = (int64_t)blockIdx.x * GEN_SCAN_TILE + threadIdx.x * 8;
  unsigned s = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += b + i < n ? keep[b + i] : 0u;
  unsigned total;
  gen_block_scan(s, &total);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// one block: the tile sums in place (exclusive), carrying across rounds of 2048 tiles; *grand_total = the kept rows
__global__ __launch_bounds__(256) void gen_scan_sums_kernel(unsigned* __restrict__ sums, int64_t n_tiles, unsigned long long* __restrict__ grand_total) {
  unsigned carry = 0;
  for (int64_t b0 = 0; b0 < n_tiles; b0 += GEN_SCAN_TILE) {
    const int64_t b = b0 + threadIdx.x * 8;
    unsigned v[8], s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = b + i < n_tiles ? sums[b + i] : 0u;
      s += v[i];
    }
    unsigned total;
    unsigned pre = carry + gen_block_scan(s, &total);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (b + i < n_tiles) sums[b + i] = pre;
      pre += v[i];
    }
    carry += total;
  }
  if (threadIdx.x == 0) *grand_total = carry;
}

// MAP: the kept rows get n_new + their rank, and are listed (kept_rows[rank] = r, kept_ids[rank] = its id)
__global__ __launch_bounds__(256) void gen_map_kernel(const unsigned* __restrict__ keep, int64_t n, const unsigned* __restrict__ tile_offsets,
                                                      const int64_t* __restrict__ cur_ids, int64_t n_new, int64_t* __restrict__ map,
                                                      int64_t* __restrict__ kept_rows, int64_t* __restrict__ kept_ids) {
  const int64_t b = (int64_t)blockIdx.x * GEN_SCAN_TILE + threadIdx.x * 8;
  unsigned v[8], s = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = b + i < n ? keep[b + i] : 0u;
    s += v[i];
  }
  unsigned pre = tile_offsets[blockIdx.x] + gen_block_scan(s, nullptr);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (v[i]) {   // (v[i] != 0 only inside the array)
      map[b + i] = n_new + (int64_t)pre;
      kept_rows[pre] = b + i;
      kept_ids[pre] = cur_ids[b + i];
      ++pre;
    }
  }
}

// ---- the rows ---------------------------------------------------------------------------------------------------------
// GATHER: dst row n_new + i = src row kept_rows[i], k floats each (k = 1..128: rows are not 16-byte multiples in general,
// so this moves single floats; a wave covers 64 consecutive floats of the destination, which is contiguous, and of a
// source row)
__global__ __launch_bounds__(256) void gen_gather_rows_kernel(const float* __restrict__ src, const int64_t* __restrict__ kept_rows, int64_t n_kept,
                                                              int k, float* __restrict__ dst_tail) {
  MALS_GEN_STRIDE(e, n_kept * k) {
    const int64_t i = e / k;
    const int f = (int)(e - i * k);
    dst_tail[e] = src[kept_rows[i] * k + f];
  }
}

// the new rows into the head of the replica: a flat copy of n floats.  VEC: both addresses are 16-byte aligned (the caller
// checked the pointers), the body moves float4 and the last n % 4 floats go one by one.
template <bool VEC>
__global__ __launch_bounds__(256) void gen_copy_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n) {
  if constexpr (VEC) {
    const int64_t n4 = n / 4;
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
    MALS_GEN_STRIDE(i, n4) d4[i] = s4[i];
    if (blockIdx.x == 0 && 4 * n4 + (int64_t)threadIdx.x < n) dst[4 * n4 + threadIdx.x] = src[4 * n4 + threadIdx.x];
  } else {
    MALS_GEN_STRIDE(i, n) dst[i] = src[i];
  }
}

// merged ids behind the new ones / any small gather of int64: out[i] = table[idx[i]] (-1 for an index outside [0, n_table))
__global__ __launch_bounds__(256) void gen_gather_i64_kernel(const int64_t* __restrict__ table, int64_t n_table, const int64_t* __restrict__ idx, int64_t n,
                                                             int64_t* __restrict__ out) {
  MALS_GEN_STRIDE(i, n) {
    const int64_t r = idx[i];
    out[i] = (r >= 0 && r < n_table) ? table[r] : -1;
  }
}

// TAGS: a live tag item that is recent (or every row is kept) and has a merged row stays a tag there (removeNotUpdated of
// userTagIDs against recentlyActiveItems, :92-95).  new_bits: zeroed, one bit per merged item; n_set: bits newly set.
__global__ __launch_bounds__(256) void gen_tag_remap_kernel(const uint32_t* __restrict__ old_bits, int64_t n_old_items, const uint32_t* __restrict__ recent,
                                                            int keep_all, const int64_t* __restrict__ map, int64_t n_merged,
                                                            uint32_t* __restrict__ new_bits, unsigned long long* __restrict__ n_set) {
  MALS_GEN_STRIDE(r, n_old_items) {
    if (((old_bits[r >> 5] >> (r & 31)) & 1u) == 0u) continue;
    const bool rec = keep_all != 0 || (recent != nullptr && ((recent[r >> 5] >> (r & 31)) & 1u) != 0u);
    const int64_t m = map[r];
    if (!rec || m < 0 || m >= n_merged) continue;
    const uint32_t bit = 1u << (m & 31);
    if ((atomicOr(&new_bits[m >> 5], bit) & bit) == 0u) atomicAdd(n_set, 1ull);
  }
}

#endif   // __HIPCC__

}  // namespace mals
