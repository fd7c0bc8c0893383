// split_kernels.h -- stable multi-way split of records (user id, item id, value: 20 bytes) into <= 256 buckets, the hot
// path of the sharded ingest (ingest_group_host.h): every record by its owner rank (user-id splitters), every entry by the
// rank that owns its item (the item bounds of the group).  One pass that writes every bucket's run contiguously, instead of
// one compaction pass per bucket.
//
//   1. split_count_kernel: a tile of SPLIT_TILE records; bucket = upper_bound of the key in the splitters (LDS), one byte per
//      record; per-tile bucket counts from wave64 ballots (one LDS add per distinct bucket per wave and round, no atomic per
//      record).  Counts are laid out bucket-major, so that
//   2. the 64-bit exclusive scan over buckets x tiles (big_scan64_*) gives every (bucket, tile) run its output offset;
//   3. split_scatter_kernel: the tile again, a stable rank per record (ballot peers + v_mbcnt), staged in LDS grouped by
//      bucket, then written out run by run.
// Stream order is kept inside every bucket: tiles ascend, waves own ascending quarters of a tile, rounds ascend in a wave,
// lanes ascend in a round.
#pragma once

namespace mals {

constexpr int SPLIT_TILE = 1024;           // 256 threads: 4 waves x 4 rounds x 64 lanes
constexpr int SPLIT_MAX_BUCKETS = 256;

__device__ __forceinline__ unsigned split_bucket(int64_t key, const int64_t* spl, int n_spl) {
  int lo = 0, hi = n_spl;  // upper bound: how many splitters are <= key
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (spl[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return (unsigned)lo;
}

// lanes of this wave whose (active, byte) equal this lane's: eight ballots over the bits of the byte
__device__ __forceinline__ uint64_t split_peers(unsigned b, bool active) {
  uint64_t m = __ballot(active);
#pragma unroll
  for (int bit = 0; bit < 8; ++bit) {
    const bool on = (b >> bit) & 1u;
    const uint64_t x = __ballot(active && on);
    m &= on ? x : ~x;
  }
  return m;
}

__device__ __forceinline__ unsigned split_rank_below(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// counts[b * n_tiles + tile] = records of the tile in bucket b; dest[i] = bucket of record i
__global__ __launch_bounds__(256) void split_count_kernel(const int64_t* __restrict__ key, int64_t n, const int64_t* __restrict__ splitters, int n_spl,
                                                          int64_t n_tiles, uint8_t* __restrict__ dest, unsigned* __restrict__ counts) {
  __shared__ int64_t spl[SPLIT_MAX_BUCKETS];
  __shared__ unsigned cnt[SPLIT_MAX_BUCKETS];
  const int nb = n_spl + 1;
  for (int b = threadIdx.x; b < SPLIT_MAX_BUCKETS; b += 256) {
    if (b < n_spl) spl[b] = splitters[b];
    cnt[b] = 0u;
  }
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t base = (int64_t)blockIdx.x * SPLIT_TILE + w * (SPLIT_TILE / 4);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = base + r * 64 + lane;
    const bool active = i < n;
    const unsigned b = active ? split_bucket(key[i], spl, n_spl) : 0u;
    if (active) dest[i] = (uint8_t)b;
    const uint64_t peers = split_peers(b, active);
    if (active && split_rank_below(peers) == 0u) atomicAdd(&cnt[b], (unsigned)__popcll(peers));   // the lowest lane of its bucket
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += 256) counts[(int64_t)b * n_tiles + blockIdx.x] = cnt[b];
}

// out[offsets[b * n_tiles + tile] + j] = the j-th record of the tile in bucket b
__global__ __launch_bounds__(256) void split_scatter_kernel(const uint8_t* __restrict__ dest, int64_t n, int nb, int64_t n_tiles,
                                                            const int64_t* __restrict__ offsets, const int64_t* __restrict__ in_a,
                                                            const int64_t* __restrict__ in_b, const float* __restrict__ in_c,
                                                            int64_t* __restrict__ out_a, int64_t* __restrict__ out_b, float* __restrict__ out_c) {
  __shared__ unsigned wcnt[4][SPLIT_MAX_BUCKETS];   // per wave: records per bucket, then the waves' exclusive prefix
  __shared__ unsigned start[SPLIT_MAX_BUCKETS];     // tile-local start of bucket b
  __shared__ int64_t sa[SPLIT_TILE], sb[SPLIT_TILE];
  __shared__ float sc[SPLIT_TILE];
  __shared__ uint8_t sd[SPLIT_TILE];
  for (int b = threadIdx.x; b < SPLIT_MAX_BUCKETS; b += 256) wcnt[0][b] = wcnt[1][b] = wcnt[2][b] = wcnt[3][b] = 0u;
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t t0 = (int64_t)blockIdx.x * SPLIT_TILE;
  const int64_t base = t0 + w * (SPLIT_TILE / 4);
  unsigned bk[4], rk[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = base + r * 64 + lane;
    const bool active = i < n;
    const unsigned b = active ? dest[i] : 0u;
    const uint64_t peers = split_peers(b, active);
    const unsigned below = split_rank_below(peers);
    bk[r] = b;
    rk[r] = active ? wcnt[w][b] + below : 0u;
    // one wave per row of wcnt: every lane has read it (in program order) before the lowest lane of each bucket adds
    if (active && below == 0u) wcnt[w][b] += (unsigned)__popcll(peers);
    __builtin_amdgcn_wave_barrier();   // the next round reads what this one added (one wave per row: in-order LDS)
  }
  __syncthreads();
  unsigned tot = 0;
  if (threadIdx.x < nb) {
    const unsigned c0 = wcnt[0][threadIdx.x], c1 = wcnt[1][threadIdx.x], c2 = wcnt[2][threadIdx.x], c3 = wcnt[3][threadIdx.x];
    wcnt[0][threadIdx.x] = 0u;
    wcnt[1][threadIdx.x] = c0;
    wcnt[2][threadIdx.x] = c0 + c1;
    wcnt[3][threadIdx.x] = c0 + c1 + c2;
    tot = c0 + c1 + c2 + c3;
  }
  const unsigned st = block_exclusive_scan_256(tot);
  if (threadIdx.x < nb) start[threadIdx.x] = st;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = base + r * 64 + lane;
    if (i < n) {
      const unsigned p = start[bk[r]] + wcnt[w][bk[r]] + rk[r];
      sa[p] = in_a[i];
      sb[p] = in_b[i];
      sc[p] = in_c[i];
      sd[p] = (uint8_t)bk[r];
    }
  }
  __syncthreads();
  const int tile_n = (int)((n - t0) < SPLIT_TILE ? (n - t0) : SPLIT_TILE);
  for (int p = threadIdx.x; p < tile_n; p += 256) {
    const unsigned b = sd[p];
    const int64_t o = offsets[(int64_t)b * n_tiles + blockIdx.x] + (p - (int64_t)start[b]);
    out_a[o] = sa[p];
    out_b[o] = sb[p];
    out_c[o] = sc[p];
  }
}

}  // namespace mals
