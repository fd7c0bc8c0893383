// generation_group_kernels.h -- device side of the kept users' known items in mals_group_load_generation
// (include/myrrix_als.h; host side in generation_group_host.h), gfx950, wave64.  An old owner turns the base rows of its PLAIN
// kept users (current set = base row: no additions, no replaced set, not a grown row) into rows over MERGED item rows without
// a per-user trip to the host:
//   COUNT   ONE KEPT USER PER WAVE (a grid-stride loop of waves): the lanes read the base row 64 entries at a time, look every
//           item up in the live-item -> merged-item map (the member's own, already on the device) and count the entries with a
//           merged row.  The others are dropped; a wave adds its dropped entries with one atomic when it is done.  A user
//           with rows[i] < 0 (an overlay user: it goes the host's way) counts 0.
//   SCAN    exclusive scan of the counts in 64 bits over any number of 1024-user tiles (reduce, one block over the tile sums,
//           apply): ptr[0 .. n], ptr[n] = the total.
//   FILL    the same walk; the mapped entries of a 64-entry step are compacted with a wave ballot and the lanes' prefix in it,
//           so a row's entries keep their BASE-ROW ORDER and the result is deterministic.
//   REBASE  a run of row pointers copied from another CSR (the new model's slice, an old owner's kept CSR) becomes a run of
//           the new owner's: ptr[r] = ptr[r] - first + base.  The index pieces move with plain (peer) copies.
// ROW ORDER.  A kept row is NOT sorted: it is the base row's order with the pruned items left out, and the item map is not
// monotone.  No reader of a member's base CSR assumes ascending rows: the known-item strike of the top-N passes scatters
// (topn_mask_kernel, the filter path's drop of known buckets and topn_rescore's strike go entry by entry), recommendedBecause
// takes the row as an unordered candidate list and selects by (score, index) (topn_known_cand_kernel), the membership test of
// a removal sorts what it fetched (foldin_fetch_bases), and the popular count asks the base itself once per generation
// (popular_ascending_kernel) and runs its unordered variant when a row descends.  So rows of any length stay in base order.
// Nothing here is floating-point arithmetic.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace mals {

constexpr int GENG_SCAN_TILE = 1024;   // 256 threads x 4 users

__device__ __forceinline__ unsigned long long geng_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// item -> merged item, -1: no merged row (pruned, or outside the map)
__device__ __forceinline__ int64_t geng_map_item(const int64_t* __restrict__ item_map, int64_t n_map, int32_t item) {
  return item >= 0 && (int64_t)item < n_map ? item_map[item] : -1;
}

// COUNT.  rows[i]: the local base row of kept user i (inside [0, n_base): the host checked), or -1
__global__ __launch_bounds__(256) void geng_count_kernel(const int64_t* __restrict__ base_ptr, const int32_t* __restrict__ base_idx,
                                                         const int64_t* __restrict__ rows, int64_t n, const int64_t* __restrict__ item_map,
                                                         int64_t n_map, unsigned long long* __restrict__ counts,
                                                         unsigned long long* __restrict__ dropped) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  unsigned long long d = 0;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += n_waves) {
    const int64_t r = rows[i];
    unsigned long long c = 0;
    if (r >= 0) {
      const int64_t e = base_ptr[r + 1];
      for (int64_t p = base_ptr[r] + lane; p < e; p += 64) {
        if (geng_map_item(item_map, n_map, base_idx[p]) >= 0) ++c;
        else ++d;
      }
    }
    c = geng_wave_sum(c);
    if (lane == 0) counts[i] = c;
  }
  d = geng_wave_sum(d);
  if (lane == 0 && d != 0) atomicAdd(dropped, d);
}

// ---- SCAN (64 bits) ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long geng_block_scan(unsigned long long v, unsigned long long* total) {   // exclusive, 256 threads
  __shared__ unsigned long long ws[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) ws[w] = x;
  __syncthreads();
  unsigned long long pre = 0;
  for (int i = 0; i < w; ++i) pre += ws[i];
  if (total) *total = ws[0] + ws[1] + ws[2] + ws[3];
  __syncthreads();
  return pre + x - v;
}

__global__ __launch_bounds__(256) void geng_scan_reduce_kernel(const unsigned long long* __restrict__ counts, int64_t n,
                                                               unsigned long long* __restrict__ tile_sums) {
  const int64_t b = (int64_t)blockIdx.x * GENG_SCAN_TILE + threadIdx.x * 4;
  unsigned long long s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += b + i < n ? counts[b + i] : 0ull;
  unsigned long long total;
  geng_block_scan(s, &total);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// one block: the tile sums in place (exclusive), carrying across rounds of 1024 tiles
__global__ __launch_bounds__(256) void geng_scan_sums_kernel(unsigned long long* __restrict__ sums, int64_t n_tiles) {
  unsigned long long carry = 0;
  for (int64_t b0 = 0; b0 < n_tiles; b0 += GENG_SCAN_TILE) {
    const int64_t b = b0 + threadIdx.x * 4;
    unsigned long long v[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = b + i < n_tiles ? sums[b + i] : 0ull;
      s += v[i];
    }
    unsigned long long total;
    unsigned long long pre = carry + geng_block_scan(s, &total);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (b + i < n_tiles) sums[b + i] = pre;
      pre += v[i];
    }
    carry += total;
  }
}

// ptr[i] = the entries before user i; ptr[n] = all of them (ptr: n + 1)
__global__ __launch_bounds__(256) void geng_scan_apply_kernel(const unsigned long long* __restrict__ counts, int64_t n,
                                                              const unsigned long long* __restrict__ tile_offsets, int64_t* __restrict__ ptr) {
  const int64_t b = (int64_t)blockIdx.x * GENG_SCAN_TILE + threadIdx.x * 4;
  unsigned long long v[4], s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = b + i < n ? counts[b + i] : 0ull;
    s += v[i];
  }
  unsigned long long pre = tile_offsets[blockIdx.x] + geng_block_scan(s, nullptr);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (b + i < n) ptr[b + i] = (int64_t)pre;
    pre += v[i];
    if (b + i == n - 1) ptr[n] = (int64_t)pre;
  }
}

// FILL.  ptr: what SCAN made of COUNT's counts over the same rows and the same map, so a row's writes stay inside
// [ptr[i], ptr[i + 1]) (and inside idx_out's ptr[n] entries)
__global__ __launch_bounds__(256) void geng_fill_kernel(const int64_t* __restrict__ base_ptr, const int32_t* __restrict__ base_idx,
                                                        const int64_t* __restrict__ rows, int64_t n, const int64_t* __restrict__ item_map,
                                                        int64_t n_map, const int64_t* __restrict__ ptr, int32_t* __restrict__ idx_out) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += n_waves) {
    const int64_t r = rows[i];
    if (r < 0) continue;   // (wave-uniform)
    const int64_t b = base_ptr[r], e = base_ptr[r + 1], end = ptr[i + 1];
    int64_t at = ptr[i];
    for (int64_t p0 = b; p0 < e; p0 += 64) {   // every lane walks every step: the ballot is the whole wave's
      const int64_t p = p0 + lane;
      const int64_t m = p < e ? geng_map_item(item_map, n_map, base_idx[p]) : -1;
      const unsigned long long mask = __ballot(m >= 0);
      const int before = __popcll(mask & ((1ull << lane) - 1ull));
      if (m >= 0 && at + before < end) idx_out[at + before] = (int32_t)m;
      at += __popcll(mask);
    }
  }
}

// REBASE: n row pointers of another CSR in place (first = the source's pointer at the run's first row)
__global__ __launch_bounds__(256) void geng_rebase_kernel(int64_t* __restrict__ ptr, int64_t n, int64_t first, int64_t base) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) ptr[i] = ptr[i] - first + base;
}

}  // namespace mals
