// lsh_kernels.h -- the reference's candidate filter on the device: LocationSensitiveHash (online/src/net/myrrix/online/
// candidate/LocationSensitiveHash.java), which ServerRecommender.multithreadedTopN (ServerRecommender.java:443-508) asks
// for the items a query may see when model.lsh.sampleRatio < 1 (CandidateFilterFactory.java:50-71).
//
//   build        (LSH:89-152) H = num_hashes random +-1 vectors [H][features] (booleans), the mean vector of Y (fp64 sum of
//                the fp32 rows / rows, LSH:154-167), and per row of Y its bit signature;
//   signature    (toBitSignature, LSH:169-190) per hash h in order: total = 0.0; per feature f in order delta = (double)v[f] -
//                mean[f], total += delta or total -= delta; bit = total > 0.0 (strictly); l = (l << 1) | bit -- hash 0 ends up
//                the most significant of the H bits.  Only fp64 adds and subtracts, in feature order: the kernels below do
//                exactly those (x - d is x + (-d) in IEEE arithmetic; there is no product to contract), so signatures are
//                bit-identical to the reference's given the same mean.
//   candidates   (getCandidateIterator, LSH:193-216) item i is a candidate of a query with vectors f_1..f_n iff
//                bitCount(sig_i ^ sig(f_j)) <= maxBitsDiffering for ANY j, or i is a new item (addItem, LSH:219-225; here: a row
//                of Y past the rows signed at build time, mals_grow_factor_rows).
// The random vectors reach the device as one 64-bit mask per feature (bit h = randomVectors[h][f]): a lane that owns hashes
// h0, h0 + step, ... reads one word per feature and computes delta once for all of them (lsh_totals).
// The mean, when the caller does not supply it, is a two-level fp64 sum in a FIXED order (LSH_MEAN_BLOCKS row ranges, inside a
// range the rows r = first + slot, first + slot + R, ...; then the partial sums in ascending order): the same bits on every
// run, within (rows + 1) 2^-53 sum|y| / rows of the exact mean like any order of fp64 additions (the reference's own order is
// its hash map's, which nobody can restate).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mals {

constexpr int LSH_MEAN_BLOCKS = 256;
constexpr int LSH_MEAN_SLOTS = 4;  // most interleaved row slots of a range: the last level adds 256 x 4 partial sums per feature at most
constexpr int LSH_NEW_ITEM_BIAS = -128;  // added to the popcount of a row without a signature: below every threshold, -1 included

// what the kernels of a pass read of the filter (isig NULL: no filter, every item a candidate)
struct TopnLsh {
  const uint64_t* isig = nullptr;   // signatures of rows [0, n_signed) of Y, as they were at build time
  int64_t n_signed = 0;
  const uint64_t* vsig = nullptr;   // signatures of the pass's query vectors (lsh_sign_vectors_kernel)
  const int32_t* vptr = nullptr;    // query q owns vectors [vptr[q], vptr[q + 1]) of the pass
  int32_t mb = 0;                   // maxBitsDiffering (LSH:98-108; may be -1: only new items)
};

// LSH:193-216 for one item and the vectors [v0, v1) of the pass
__device__ __forceinline__ bool lsh_candidate(const TopnLsh& l, int64_t item, int v0, int v1) {
  if (!l.isig || item >= l.n_signed) return true;
  const uint64_t s = l.isig[item];
  for (int v = v0; v < v1; ++v)
    if ((int)__popcll(s ^ l.vsig[v]) <= l.mb) return true;
  return false;
}

// toBitSignature's inner loops (LSH:172-182) for the NH hashes h0, h0 + hstep, ... of one vector, f in
// order; total[j] += delta or -= delta by bit h0 + j hstep of mask[f].  (A hash index past 63 reads bit 0 of a zero: its total
// is never looked at.)
template <int NH>
__device__ __forceinline__ void lsh_totals(const float* __restrict__ v, const double* __restrict__ mean, const uint64_t* __restrict__ mask,
                                           int k, int h0, int hstep, double (&total)[NH]) {
#pragma unroll
  for (int j = 0; j < NH; ++j) total[j] = 0.0;
  for (int f = 0; f < k; ++f) {
    const double delta = (double)v[f] - mean[f];
    const uint64_t m = mask[f];
#pragma unroll
    for (int j = 0; j < NH; ++j) {
      const int h = h0 + j * hstep;
      const bool plus = h < 64 && ((m >> h) & 1ull) != 0ull;
      total[j] += plus ? delta : -delta;
    }
  }
}

// ---- the mean of Y (LSH:154-167), in a fixed order ----------------------------------------------------------------------
// part[(b R + slot) k + f] = sum of Y[r][f] over the rows r = b chunk + slot, + R, ... of range b; R = lsh_mean_slots(k)
__host__ __device__ __forceinline__ int lsh_mean_slots(int k) { return 256 / k < LSH_MEAN_SLOTS ? 256 / k : LSH_MEAN_SLOTS; }
__global__ __launch_bounds__(256) void lsh_mean_partial_kernel(const float* __restrict__ Y, int64_t n, int k, double* __restrict__ part) {
  const int R = lsh_mean_slots(k);
  const int slot = threadIdx.x / k, f = threadIdx.x % k;
  if (slot >= R) return;
  const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
  double s = 0.0;
  for (int64_t r = r0 + slot; r < r1; r += R) s += (double)Y[r * k + f];
  part[((int64_t)blockIdx.x * R + slot) * k + f] = s;
}
__global__ void lsh_mean_final_kernel(const double* __restrict__ part, int n_part, int k, int64_t n, double* __restrict__ mean) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= k) return;
  double s = 0.0;
  for (int p = 0; p < n_part; ++p) s += part[(int64_t)p * k + f];
  mean[f] = s / (double)n;
}

// ---- the signatures of Y (LSH:126-127): Y is read once ------------------------------------------------------------------
// A workgroup takes 64 rows at a time: staged in LDS with coalesced loads ([64][k + 1]: a lane walking its own row hits 64
// different banks), then lane = row, wave w = the hashes w, w + 4, ...: NH fp64 totals per lane in registers (NH = 16 covers
// H = 64: 32 registers).  The four waves' bits meet in LDS.
template <int NH>
__global__ __launch_bounds__(256) void lsh_sign_rows_kernel(const float* __restrict__ Y, int64_t n, int k, const double* __restrict__ mean,
                                                            const uint64_t* __restrict__ mask, int H, uint64_t* __restrict__ sig) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  float* ys = reinterpret_cast<float*>(smem);  // [64][k + 1]
  __shared__ double smean[128];
  __shared__ uint64_t smask[128];
  __shared__ uint64_t spart[4][64];
  const int pitch = k + 1, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if ((int)threadIdx.x < k) {
    smean[threadIdx.x] = mean[threadIdx.x];
    smask[threadIdx.x] = mask[threadIdx.x];
  }
  for (int64_t i0 = (int64_t)blockIdx.x * 64; i0 < n; i0 += (int64_t)gridDim.x * 64) {
    const int rows = (int)(n - i0 < 64 ? n - i0 : 64);
    __syncthreads();
    for (int e = threadIdx.x; e < rows * k; e += 256) ys[(e / k) * pitch + (e % k)] = Y[i0 * k + e];
    __syncthreads();
    uint64_t bits = 0;
    if (lane < rows) {
      double total[NH];
      lsh_totals<NH>(ys + lane * pitch, smean, smask, k, w, 4, total);
#pragma unroll
      for (int j = 0; j < NH; ++j) {
        const int h = w + 4 * j;
        if (h < H && total[j] > 0.0) bits |= 1ull << (H - 1 - h);
      }
    }
    spart[w][lane] = bits;
    __syncthreads();
    if (w == 0 && lane < rows) sig[i0 + lane] = spart[0][lane] | spart[1][lane] | spart[2][lane] | spart[3][lane];
  }
}

// ---- the signatures of query vectors (LSH:194-197) ----------------------------------------------------------------------
// One wave per vector (row vrow[v] of vecs; vrow NULL: row v), lane = hash.  The first lane of the launch also leaves the
// pass's view of the filter where the streaming kernels look for it (behind the query image; NULL: nowhere).
__global__ __launch_bounds__(64) void lsh_sign_vectors_kernel(const float* __restrict__ vecs, const int64_t* __restrict__ vrow, int n_vecs, int k,
                                                              const double* __restrict__ mean, const uint64_t* __restrict__ mask, int H,
                                                              uint64_t* __restrict__ vsig, TopnLsh* __restrict__ trailer, TopnLsh view) {
  const int v = blockIdx.x, h = threadIdx.x;
  if (trailer && v == 0 && h == 0) *trailer = view;
  if (v >= n_vecs) return;
  double total[1];
  lsh_totals<1>(vecs + (vrow ? vrow[v] : (int64_t)v) * k, mean, mask, k, h, 0, total);
  const uint64_t lanes = __ballot(h < H && total[0] > 0.0);  // bit h = hash h
  if (h == 0) vsig[v] = __brevll(lanes) >> (64 - H);           // hash 0 the most significant of the H bits
}

// filter path, in front of topn_threshold_kernel: a sample bucket won by a non-candidate is dropped whole, as one won by a
// known item is (only a query of several vectors has any: the sample tested the others item by item).  bmax / bidx: the
// sample's rows, n_row buckets per query.
__global__ __launch_bounds__(256) void lsh_drop_buckets_kernel(TopnLsh l, int64_t n_row, float* __restrict__ bmax, const uint32_t* __restrict__ bidx) {
  const int q = blockIdx.y;
  const int v0 = l.vptr[q], v1 = l.vptr[q + 1];
  if (v1 - v0 == 1) return;  // tested in the stream
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_row; i += (int64_t)gridDim.x * 256) {
    const int64_t at = (int64_t)q * n_row + i;
    if (bmax[at] > -__builtin_huge_valf() && !lsh_candidate(l, (int64_t)bidx[at], v0, v1)) bmax[at] = -__builtin_huge_valf();
  }
}
// filter path, behind topn_rescore_kernel: pairs[q][p] of a candidate-list entry that is none of the query's LSH candidates
// becomes 0, the value of a struck item (LSH:193-216, whatever the streaming tests let through)
__global__ __launch_bounds__(256) void lsh_strike_pairs_kernel(TopnLsh l, const unsigned* __restrict__ count, int count_stride, int cap,
                                                               const uint32_t* __restrict__ cand, uint64_t* __restrict__ pairs) {
  const int q = blockIdx.y;
  const unsigned cq = count[(size_t)q * count_stride];
  const unsigned n = cq < (unsigned)cap ? cq : (unsigned)cap;
  const int v0 = l.vptr[q], v1 = l.vptr[q + 1];
  for (unsigned p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
    const int64_t at = (int64_t)q * cap + p;
    if (!lsh_candidate(l, (int64_t)cand[at], v0, v1)) pairs[at] = 0ull;
  }
}

// dense path: the non-candidates of every query's score row
__global__ __launch_bounds__(256) void lsh_mask_dense_kernel(TopnLsh l, int n_queries, int64_t n_items, float* __restrict__ scores) {
  const int q = blockIdx.y;
  if (q >= n_queries) return;
  const int v0 = l.vptr[q], v1 = l.vptr[q + 1];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * 256)
    if (!lsh_candidate(l, i, v0, v1)) scores[(int64_t)q * n_items + i] = -__builtin_huge_valf();
}

}  // namespace mals
