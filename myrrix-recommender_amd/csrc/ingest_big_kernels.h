// ingest_big_kernels.h -- the kernels of the partitioned finish (ingest_big_host.h tells how the pieces fit): cutting the
// records into user ranges, merging ascending id tables without a sort, and R^T item range by item range.  The group finish
// (ingest_group_host.h) borrows the 64-bit scan.  Expects before it: ingest_kernels.h (MALS_GRID_STRIDE, id_to_key, the scan
// helpers).
#pragma once

namespace mals {

constexpr int BIG_TILE = 2048;  // records (or entries) per workgroup of the selection kernels: 256 threads x 8

// part[i] = number of splitters <= user_ids[i] (splitters ascending and distinct): equal ids share a range, ranges ascend
__global__ void big_assign_part_kernel(const int64_t* __restrict__ user_ids, int64_t n, const int64_t* __restrict__ splitters, int n_split,
                                       uint8_t* __restrict__ part) {
  MALS_GRID_STRIDE(i, n) {
    const int64_t u = user_ids[i];
    int lo = 0, hi = n_split;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (splitters[mid] <= u) lo = mid + 1; else hi = mid;
    }
    part[i] = (uint8_t)lo;
  }
}
// records per range, all ranges in one read: hist[256] (block-private LDS counts, then global atomics)
__global__ __launch_bounds__(256) void big_part_histogram_kernel(const uint8_t* __restrict__ part, int64_t n, unsigned long long* __restrict__ hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  MALS_GRID_STRIDE(i, n) atomicAdd(&h[part[i]], 1u);
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}
// tile_counts[t] = records of range p in tile t
// (a thread's 8 range bytes are ONE 8-byte load -- the array is padded past n --, a thread's 8 columns two 16-byte loads:
// eight strided 1- or 4-byte loads per thread ran these kernels at 0.2-0.9 TB/s)
__device__ __forceinline__ unsigned big_match8(const uint8_t* __restrict__ part, int64_t b, int64_t n, uint8_t p, bool (&m)[8]) {
  const uint64_t w = b < n ? *reinterpret_cast<const uint64_t*>(part + b) : 0ull;
  unsigned c = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    m[j] = b + j < n && (uint8_t)(w >> (8 * j)) == p;
    c += m[j] ? 1u : 0u;
  }
  return c;
}
__device__ __forceinline__ void big_load8(const int32_t* __restrict__ col, int64_t e, int64_t nnz, int32_t (&c)[8]) {
  if (e + 8 <= nnz) {
    const int4 lo = *reinterpret_cast<const int4*>(col + e), hi = *reinterpret_cast<const int4*>(col + e + 4);
    c[0] = lo.x, c[1] = lo.y, c[2] = lo.z, c[3] = lo.w, c[4] = hi.x, c[5] = hi.y, c[6] = hi.z, c[7] = hi.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = e + j < nnz ? col[e + j] : -1;
  }
}
__global__ __launch_bounds__(256) void big_count_part_kernel(const uint8_t* __restrict__ part, int64_t n, uint8_t p, unsigned* __restrict__ tile_counts) {
  const int64_t b = (int64_t)blockIdx.x * BIG_TILE + threadIdx.x * 8;
  bool m[8];
  const unsigned c = big_match8(part, b, n, p, m);
  unsigned total;
  block_exclusive_scan(c, &total);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}
// the records of range p, in stream order, into the partition buffers (tile_offsets = exclusive scan of the tile counts)
__global__ __launch_bounds__(256) void big_compact_part_kernel(const uint8_t* __restrict__ part, int64_t n, uint8_t p,
                                                               const unsigned* __restrict__ tile_offsets, const int64_t* __restrict__ user,
                                                               const int64_t* __restrict__ item, const float* __restrict__ value,
                                                               int64_t* __restrict__ pu, int64_t* __restrict__ pi, float* __restrict__ pv) {
  const int64_t b = (int64_t)blockIdx.x * BIG_TILE + threadIdx.x * 8;
  bool m[8];
  const unsigned c = big_match8(part, b, n, p, m);
  unsigned pos = tile_offsets[blockIdx.x] + block_exclusive_scan(c, nullptr);
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (m[j]) {
      pu[pos] = user[b + j];
      pi[pos] = item[b + j];
      pv[pos] = value[b + j];
      ++pos;
    }
}
// every S-th user id as a sort key
__global__ void big_sample_kernel(const int64_t* __restrict__ user_ids, int64_t n, int64_t n_sample, uint64_t* __restrict__ keys, unsigned* __restrict__ pay) {
  MALS_GRID_STRIDE(j, n_sample) {
    int64_t i = (int64_t)((double)j * ((double)n / (double)n_sample));   // (any spread of positions does: it is a sample)
    i = i < 0 ? 0 : (i >= n ? n - 1 : i);
    keys[j] = id_to_key(user_ids[i]);
    pay[j] = 0u;
  }
}
__global__ void big_keys_to_ids_kernel(const uint64_t* __restrict__ keys, int64_t n, int64_t* __restrict__ ids) {
  MALS_GRID_STRIDE(i, n) ids[i] = key_to_id(keys[i]);
}
// the kept pairs of a partition: local row (dense among the partition's live users), LOCAL item rank as the column
__global__ void big_compact_pairs_kernel(const uint64_t* __restrict__ keys, const unsigned* __restrict__ keep, const unsigned* __restrict__ keep_scan,
                                         const float* __restrict__ pair_val, int64_t n, const unsigned* __restrict__ new_u,
                                         int32_t* __restrict__ row, int32_t* __restrict__ col, float* __restrict__ val) {
  MALS_GRID_STRIDE(i, n) {
    if (!keep[i]) continue;
    const unsigned q = keep_scan[i];
    row[q] = (int32_t)new_u[(unsigned)(keys[i] >> 32)];
    col[q] = (int32_t)(unsigned)(keys[i] & 0xffffffffu);
    if (val) val[q] = pair_val[i];
  }
}
// out[r] = base + local[r]
__global__ void big_add_base_kernel(const int64_t* __restrict__ local, int64_t n, int64_t base, int64_t* __restrict__ out) {
  MALS_GRID_STRIDE(i, n) out[i] = base + local[i];
}
// ---- merging ascending id tables without a sort ------------------------------------------------------------------------
// lower_bound of x in the ascending table
__device__ __forceinline__ int64_t big_lower_bound(const int64_t* __restrict__ table, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (table[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// fresh[i] = 1 where b[i] is not in a
__global__ void big_fresh_kernel(const int64_t* __restrict__ b, int64_t nb, const int64_t* __restrict__ a, int64_t na, unsigned* __restrict__ fresh) {
  MALS_GRID_STRIDE(i, nb) {
    const int64_t q = big_lower_bound(a, na, b[i]);
    fresh[i] = (q < na && a[q] == b[i]) ? 0u : 1u;
  }
}
__global__ void big_compact_fresh_kernel(const int64_t* __restrict__ b, int64_t nb, const unsigned* __restrict__ fresh, const unsigned* __restrict__ fresh_scan,
                                         int64_t* __restrict__ out) {
  MALS_GRID_STRIDE(i, nb)
    if (fresh[i]) out[fresh_scan[i]] = b[i];
}
// union of two DISJOINT ascending tables: an element's position = its own index + how many of the other table precede it
__global__ void big_merge_place_kernel(const int64_t* __restrict__ mine, int64_t n_mine, const int64_t* __restrict__ other, int64_t n_other,
                                       int64_t* __restrict__ out) {
  MALS_GRID_STRIDE(i, n_mine) out[i + big_lower_bound(other, n_other, mine[i])] = mine[i];
}
// alive_glob[map[l]] |= alive_local[l]
__global__ void big_mark_alive_kernel(const unsigned* __restrict__ alive_local, const int64_t* __restrict__ map, int64_t n_local,
                                      unsigned* __restrict__ alive_glob) {
  MALS_GRID_STRIDE(l, n_local)
    if (alive_local[l] && __atomic_load_n(&alive_glob[map[l]], __ATOMIC_RELAXED) == 0u) alive_glob[map[l]] = 1u;
}
// local item rank -> dense item index of the result
__global__ void big_final_map_kernel(const int64_t* __restrict__ map, int64_t n_local, const unsigned* __restrict__ new_i, int32_t* __restrict__ out) {
  MALS_GRID_STRIDE(l, n_local) out[l] = (int32_t)new_i[map[l]];
}
__global__ void big_remap_kernel(int32_t* __restrict__ col, int64_t n, const int32_t* __restrict__ final_map) {
  MALS_GRID_STRIDE(i, n) col[i] = final_map[col[i]];
}
// ---- R^T ------------------------------------------------------------------------------------------------------------------
// entries per item, from every `stride`-th entry: the item ranges of R^T are CUT by this estimate (an exact count of all
// entries is 5e9 atomics, a fifth of them on a few thousand popular items: 324 ms at 2.5e9 entries, a quarter of the whole
// finish); what a range really holds is counted exactly when it is selected, and R^T's offsets come out of the sorted ranges
__global__ void big_item_sample_kernel(const int32_t* __restrict__ col, int64_t nnz, int64_t stride, unsigned* __restrict__ cnt) {
  const int64_t n_s = (nnz + stride - 1) / stride;
  MALS_GRID_STRIDE(i, n_s) atomicAdd(&cnt[col[i * stride]], 1u);
}
// exclusive scan uint32 -> int64 offsets (out has n + 1 entries): tile sums, one block over them, apply
__global__ __launch_bounds__(256) void big_scan64_reduce_kernel(const unsigned* __restrict__ in, int64_t n, unsigned long long* __restrict__ tile_sums) {
  const int64_t b = (int64_t)blockIdx.x * SC_TILE + threadIdx.x * 8;
  unsigned v[8], s = 0;
  scan_load8(in, b, n, v);
#pragma unroll
  for (int i = 0; i < 8; ++i) s += v[i];   // a tile holds 2048 counts below 2^31 / 2048 each in every real input; summed in 64 bits below
  __shared__ unsigned long long acc;
  if (threadIdx.x == 0) acc = 0;
  __syncthreads();
  atomicAdd(&acc, (unsigned long long)s);
  __syncthreads();
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = acc;
}
__global__ void big_scan64_sums_kernel(unsigned long long* __restrict__ sums, int64_t n_tiles, unsigned long long* __restrict__ grand_total) {
  // one thread: a few million additions at most (n_items / 2048 tiles)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  unsigned long long run = 0;
  for (int64_t t = 0; t < n_tiles; ++t) {
    const unsigned long long v = sums[t];
    sums[t] = run;
    run += v;
  }
  *grand_total = run;
}
__global__ __launch_bounds__(256) void big_scan64_apply_kernel(const unsigned* __restrict__ in, int64_t n, const unsigned long long* __restrict__ tile_offsets,
                                                               const unsigned long long* __restrict__ grand_total, int64_t* __restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * SC_TILE + threadIdx.x * 8;
  unsigned v[8], s = 0;
  scan_load8(in, b, n, v);
#pragma unroll
  for (int i = 0; i < 8; ++i) s += v[i];
  unsigned long long pre = tile_offsets[blockIdx.x] + (unsigned long long)block_exclusive_scan(s, nullptr);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (b + i < n) out[b + i] = (int64_t)pre;
    pre += v[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = (int64_t)*grand_total;
}
// tile_counts[t] = entries of tile t whose item lies in [a, b)
__global__ __launch_bounds__(256) void big_count_items_kernel(const int32_t* __restrict__ col, int64_t nnz, int32_t a, int32_t b,
                                                              unsigned* __restrict__ tile_counts) {
  const int64_t e = (int64_t)blockIdx.x * BIG_TILE + threadIdx.x * 8;
  int32_t cc[8];
  big_load8(col, e, nnz, cc);
  unsigned c = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) c += (cc[j] >= a && cc[j] < b) ? 1u : 0u;
  unsigned total;
  block_exclusive_scan(c, &total);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}
// the row of entry e: the last r with row_ptr[r] <= e, searched in [lo, hi]
__device__ __forceinline__ int64_t big_row_of(const int64_t* __restrict__ row_ptr, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (row_ptr[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// tile_row[t] = the row of the first entry of entry tile t (tile_row[n_tiles] = the last row): once per finish, one thread per
// tile.  (Searched inside big_select_items_kernel by one thread per workgroup it was 50 dependent loads in front of a
// barrier, per tile and per item range: 20 ms per range at 2.5e9 entries, a third of the finish.)
__global__ void big_tile_rows_kernel(const int64_t* __restrict__ row_ptr, int64_t n_rows, int64_t nnz, int64_t n_tiles, int32_t* __restrict__ tile_row) {
  MALS_GRID_STRIDE(t, n_tiles + 1)
    tile_row[t] = (t == n_tiles || t * BIG_TILE >= nnz) ? (int32_t)(n_rows - 1) : (int32_t)big_row_of(row_ptr, 0, n_rows - 1, t * BIG_TILE);
}
// the selected entries, in (user, item) order, as sort keys ((item - a) << 32 | user) with the value bits as payload
__global__ __launch_bounds__(256) void big_select_items_kernel(const int32_t* __restrict__ col, const float* __restrict__ val, int64_t nnz,
                                                               const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ tile_row, int32_t a, int32_t b,
                                                               const unsigned* __restrict__ tile_offsets, uint64_t* __restrict__ keys,
                                                               unsigned* __restrict__ pay) {
  const int64_t e0 = (int64_t)blockIdx.x * BIG_TILE;
  const int64_t r_lo = tile_row[blockIdx.x], r_hi = tile_row[blockIdx.x + 1];
  const int64_t e = e0 + threadIdx.x * 8;
  int32_t cc[8];
  big_load8(col, e, nnz, cc);
  bool m[8];
  unsigned c = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    m[j] = cc[j] >= a && cc[j] < b;   // (entries past nnz read as -1: outside every range)
    c += m[j] ? 1u : 0u;
  }
  unsigned pos = tile_offsets[blockIdx.x] + block_exclusive_scan(c, nullptr);
  int64_t row = -1;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (m[j]) {
      // (a thread's 8 entries are consecutive: the row only moves forward)
      if (row < 0 || row_ptr[row + 1] <= e + j) row = big_row_of(row_ptr, row < 0 ? r_lo : row, r_hi, e + j);
      keys[pos] = ((uint64_t)(uint32_t)(cc[j] - a) << 32) | (uint32_t)row;
      pay[pos] = __float_as_uint(val[e + j]);
      ++pos;
    }
}
__global__ void big_transpose_write_kernel(const uint64_t* __restrict__ keys, const unsigned* __restrict__ pay, int64_t n, int32_t* __restrict__ t_row,
                                           int32_t* __restrict__ t_col, float* __restrict__ t_val) {
  MALS_GRID_STRIDE(i, n) {
    t_row[i] = (int32_t)(keys[i] >> 32);          // the item, counted from the range's first
    t_col[i] = (int32_t)(keys[i] & 0xffffffffu);  // the user
    t_val[i] = __uint_as_float(pay[i]);
  }
}
__global__ void big_add_base_inplace_kernel(int64_t* __restrict__ p, int64_t n, int64_t base) {
  MALS_GRID_STRIDE(i, n) p[i] += base;
}

}  // namespace mals
