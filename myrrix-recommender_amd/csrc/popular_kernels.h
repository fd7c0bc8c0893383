// popular_kernels.h -- device side of mals_most_popular_items (include/myrrix_als.h; host side in popular_host.h), gfx950,
// wave64.  ServerRecommender.mostPopularItems (ServerRecommender.java:611-673, scored by MostPopularItemsIterator.java:
// 51-67) in four steps:
//   COUNT   count[i] = the number of counted users whose known-item set holds i: one pass over a CSR of user rows into a
//           uint32 array of n_items, one wave per row, with a per-row skip bitset.  An entry counts iff no earlier entry of
//           its row equals it (the rows are SETS, :639-645); for a strictly ascending row no entry has an equal
//           predecessor, so the ascending kernel counts every entry of a row it has checked to be ascending.  Increments
//           are vector atomics on global memory (global_atomic_add_u32 without return).
//   KEY     count -> a 64-bit selection key: the order-preserving image of the value in the high word (score_key), the
//           complemented item index in the low word, so that "largest key first" is "best first, equal values in ascending
//           item index".  A non-candidate has key 0 (no candidate has: the high word of a finite float's image is never 0).
//   SELECT  the how_many largest keys by an 8-pass radix select over the 64 bits (histogram, pick, collect as topn_hist /
//           pick / collect do for 32-bit scores).  Keys of candidates are distinct (the index is part of them), so after the
//           eighth pass the prefix IS the how_many-th largest key and the collect pass takes exactly the keys >= it: no tie
//           cap, nothing of the key row goes to the host.
//   ADD     the sum of the members' partial count arrays (a group), saturating.
// Included by mals_serving.hip after topn_kernels.h (score_key, TopnRescore, topn_rs_filtered, topn_rs_affine, topn_tagged).
#pragma once

namespace mals {

constexpr unsigned POPULAR_MAX_COUNT = 16777216u;   // 2^24: where FastByIDFloatMap.increment(id, 1.0f) stops moving (below)

struct PopularSelect {
  unsigned long long prefix;   // digits decided so far (in place, high bits); after 8 passes the how_many-th largest key
  uint32_t remaining;          // rank of that key among the candidates that match the prefix
  uint32_t taken;              // collect: keys written
};

// 1 into *unsorted if any row of the CSR is not strictly ascending (one wave per row; a plain store: every writer writes 1)
__global__ __launch_bounds__(256) void popular_ascending_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ idx, int64_t n_rows,
                                                                int* __restrict__ unsorted) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  bool bad = false;
  for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_rows; r += n_waves) {
    const int64_t b = row_ptr[r], e = row_ptr[r + 1];
    for (int64_t p = b + 1 + lane; p < e; p += 64) bad |= idx[p] <= idx[p - 1];
  }
  if (bad) *unsorted = 1;
}

// One wave per row of the CSR, lanes over its entries.  skip (nullable): bit r set = row r is not counted (a tag user, or a
// user whose current set comes from the override CSR).  ASCENDING: every row is strictly ascending (checked by
// popular_ascending_kernel, or built so), every entry counts; else an entry counts iff no earlier entry of its row equals
// it (quadratic in the row length: only correct).  Item indices outside [0, n_items) are ignored, never written.  pairs:
// the (user, item) pairs counted, one atomic per wave.
template <bool ASCENDING>
__global__ __launch_bounds__(256) void popular_count_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ idx, int64_t n_rows,
                                                            const uint32_t* __restrict__ skip, int64_t n_items, uint32_t* __restrict__ count,
                                                            unsigned long long* __restrict__ pairs) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  unsigned long long mine = 0;
  for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_rows; r += n_waves) {
    if (skip != nullptr && ((skip[r >> 5] >> (r & 31)) & 1u) != 0u) continue;
    const int64_t b = row_ptr[r], e = row_ptr[r + 1];
    for (int64_t p = b + lane; p < e; p += 64) {
      const int32_t it = idx[p];
      if (it < 0 || (int64_t)it >= n_items) continue;
      if (!ASCENDING) {
        bool seen = false;
        for (int64_t q = b; q < p && !seen; ++q) seen = idx[q] == it;
        if (seen) continue;
      }
      atomicAdd(&count[it], 1u);
      ++mine;
    }
  }
  // the wave's total in lane 0 (DPP-free: six shuffles)
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
  if (lane == 0 && mine) atomicAdd(pairs, mine);
}

// dst[i] = min(dst[i] + src[i], 2^32 - 1): a saturated sum stays >= 2^24, where the value saturates anyway
__global__ void popular_add_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = dst[i], s = a + src[i];
  dst[i] = s < a ? 0xffffffffu : s;
}

// The value of item i (ServerRecommender.java:644): itemCounts.increment(itemID, 1.0f) count(i) times from 0.0f.  Below
// 2^24 every partial sum is an integer fp32 holds exactly; at 2^24 the next sum, 2^24 + 1, lies halfway between 2^24 and
// 2^24 + 2 and rounds to the even one, 2^24, so the value stays there: (float)min(count, 2^24).
// Then, in the reference's order: count 0 = not in itemCounts (:636-648), a userTagID is removed (:657-667), and with a
// rescorer MostPopularItemsIterator.java:56-63: a filtered item is skipped, value = (float)rescore(id, value) with
// rescore = fl(fl(scale_i * (double)value) + offset_i) in fp64 without contraction (topn_rs_affine), and a value that is
// not finite after the cast is skipped -- never an error here (there is no checkState in this iterator).
template <bool RS>
__global__ __launch_bounds__(256) void popular_key_kernel(const uint32_t* __restrict__ count, int64_t n_items, const uint32_t* __restrict__ tag_bits,
                                                          TopnRescore rs, unsigned long long* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  const uint32_t c = count[i];
  unsigned long long key = 0ull;
  if (c != 0u && !topn_tagged(tag_bits, i)) {
    float value = (float)(c < POPULAR_MAX_COUNT ? c : POPULAR_MAX_COUNT);
    bool keep = true;
    if (RS) {
      keep = !topn_rs_filtered(rs, i);
      if (keep) {
        const bool arr = i < rs.n_rows;
        const double s = arr && rs.scale ? rs.scale[i] : rs.us, o = arr && rs.offset ? rs.offset[i] : rs.uo;
        value = (float)topn_rs_affine(s, (double)value, o);
        keep = fabsf(value) < __builtin_huge_valf();
      }
    }
    if (keep) key = ((unsigned long long)score_key(value) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
  }
  keys[i] = key;
}

__global__ void popular_select_init_kernel(PopularSelect* __restrict__ st, unsigned* __restrict__ hist, int how_many) {
  if (threadIdx.x == 0) *st = PopularSelect{0ull, (uint32_t)how_many, 0u};
  hist[threadIdx.x] = 0u;   // 256 threads
}

// pass p looks at bits [56 - 8p, 64 - 8p) of the keys that match the prefix of the earlier passes
__global__ __launch_bounds__(256) void popular_hist_kernel(const unsigned long long* __restrict__ keys, int64_t n, int pass,
                                                           const PopularSelect* __restrict__ st, unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const unsigned long long mask = pass == 0 ? 0ull : (~0ull << (shift + 8));
  const unsigned long long prefix = st->prefix;
  const int lane = threadIdx.x & 63;
  for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < n; i0 += (int64_t)gridDim.x * 256) {   // whole waves iterate together
    const int64_t i = i0 + threadIdx.x;
    const unsigned long long key = i < n ? keys[i] : 0ull;
    const bool cand = key != 0ull && (key & mask) == prefix;
    const int digit = (int)((key >> shift) & 255);
    // counts crowd into a few digits of the value bytes: equal digits of a wave are added by one lane (as topn_hist_kernel)
    uint64_t peers = __ballot(cand);
    if (!peers) continue;
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (digit >> bit) & 1;
      const uint64_t m = __ballot(one);
      peers &= one ? m : ~m;
    }
    if (cand && (peers & ((1ull << lane) - 1)) == 0) atomicAdd(&h[digit], (unsigned)__popcll(peers));
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// one workgroup: the digit in which the how_many-th largest key lies; the histogram is cleared for the next pass
__global__ __launch_bounds__(256) void popular_pick_kernel(PopularSelect* __restrict__ st, unsigned* __restrict__ hist, int pass) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = hist[threadIdx.x];
  hist[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int shift = 56 - 8 * pass;
    unsigned rem = st->remaining, d = 255;
    for (;; --d) {
      if (h[d] >= rem || d == 0) break;   // fewer candidates than asked for: ends at digit 0
      rem -= h[d];
    }
    st->prefix |= (unsigned long long)d << shift;
    st->remaining = rem;
  }
}

// out: the keys >= the prefix (candidates only), at most how_many of them, in no order
__global__ __launch_bounds__(256) void popular_collect_kernel(const unsigned long long* __restrict__ keys, int64_t n, PopularSelect* __restrict__ st,
                                                              int how_many, unsigned long long* __restrict__ out) {
  const unsigned long long thr = st->prefix;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned long long key = keys[i];
    if (key == 0ull || key < thr) continue;
    const unsigned p = atomicAdd(&st->taken, 1u);
    if ((int)p < how_many) out[p] = key;
  }
}

}  // namespace mals
