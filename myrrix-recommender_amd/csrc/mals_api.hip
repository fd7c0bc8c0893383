// mals_api.hip -- the solver's host side of libmyrrix_als.so: its part of the C-ABI declared in include/myrrix_als.h (the
// serving calls are in mals_serving.hip).
// One handle = one GPU (mals_handle.h).  Holds the CSR shard of each side, the factor replicas, the Gramians and
// the work lists, and launches the gfx950 kernels of als_kernels.h on the handle's stream.
// No CPU fallback exists: every compute entry point needs a HIP device and fails with
// MALS_HIP_ERROR otherwise.
#include "../../include/myrrix_als.h"
#include "als_kernels.h"
#include "dual_kernels.h"
#include "lds_kernels.h"
#include "host_eigen.h"
#include "host_solver.h"
#include "mals_internal.h"
#include "mals_handle.h"
#include "hip_buffer.h"
#include "work_plan.h"
#include "convergence.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#ifndef MALS_D4
#define MALS_D4 4
#endif
using namespace mals;

namespace {

// the shard's own device copy: s.n_local rows, s.nnz entries
int alloc_matrix(mals_handle h, SideState& s) {
  HIPCHK(h, s.row_ptr_own.alloc((size_t)(s.n_local + 1)));
  HIPCHK(h, s.col_own.alloc((size_t)std::max<int64_t>(s.nnz, 1)));
  HIPCHK(h, s.val_own.alloc((size_t)std::max<int64_t>(s.nnz, 1)));
  s.row_ptr = s.row_ptr_own.get();
  s.col = s.col_own.get();
  s.val = s.val_own.get();
  return MALS_OK;
}

int64_t slot_floats(int T) { return (int64_t)(tri(T) * 4 + T) * 64; }

// ---- banded cuts of long dense rows (band_plan.h) ------------------------------------------------
// Default size of a band of the gather table; MALS_BAND_BYTES overrides it, 0 = no banding.  Chosen by the sweep of
// profiles/HISTORY.md, round 7.
constexpr int64_t BAND_BYTES_DEFAULT = 64ll << 20;
constexpr int BAND_CHECK_SLICES = 16;

struct BandRow {   // a row long enough to be banded
  int64_t begin;   // offset of its first entry in col
  int64_t len;
};

// Grid (rows, BAND_CHECK_SLICES).  Every workgroup checks its slice of the row's adjacent column pairs (unsorted[row]
// = 1 where one descends); the first slice's also finds, per band boundary b, the first entry whose column is in band
// b or later: off[row][b], b = 0 .. n_bands (meaningless for an unsorted row; still inside [0, len]).
__global__ __launch_bounds__(256) void band_cuts_kernel(const int32_t* __restrict__ col, const BandRow* __restrict__ rows, int n_bands,
                                                        int64_t band_rows, int64_t* __restrict__ off, int* __restrict__ unsorted) {
  const BandRow r = rows[blockIdx.x];
  const int32_t* c = col + r.begin;
  const int64_t pairs = r.len - 1;
  const int64_t per = (pairs + gridDim.y - 1) / gridDim.y;
  const int64_t p0 = (int64_t)blockIdx.y * per < pairs ? (int64_t)blockIdx.y * per : pairs, p1 = p0 + per < pairs ? p0 + per : pairs;
  bool descends = false;
  for (int64_t i = p0 + threadIdx.x; i < p1; i += 256) descends |= c[i] > c[i + 1];
  if (descends) unsorted[blockIdx.x] = 1;  // (every writer stores the same value)
  if (blockIdx.y != 0) return;
  for (int b = threadIdx.x; b <= n_bands; b += 256) {
    const int64_t first_col = (int64_t)b * band_rows;
    int64_t lo = 0, hi = r.len;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if ((int64_t)c[mid] < first_col) lo = mid + 1; else hi = mid;
    }
    off[(int64_t)blockIdx.x * (n_bands + 1) + b] = b == n_bands ? r.len : lo;
  }
}

// Which rows of the shard are banded and where their columns cross the bands: one kernel and one copy back per list build.
int find_band_cuts(mals_handle h, const SideState& s, BandCuts& bc) {
  const char* e = std::getenv("MALS_BAND_BYTES");   // read at every build: the tests switch it between two handles
  const int64_t band_bytes = e ? std::atoll(e) : BAND_BYTES_DEFAULT;
  if (band_bytes <= 0 || s.nnz == 0) return MALS_OK;
  const int k = h->cfg.features;
  const int64_t ld = k % 16 ? 16 * (int64_t)h->T : k;   // row stride of the table the kernels gather from (solve_chunks)
  bc.band_rows = std::max<int64_t>(1, band_bytes / (4 * ld));
  bc.n_bands = std::max<int64_t>(1, ((int64_t)s.col_max + bc.band_rows) / bc.band_rows);  // bands that hold a referenced row
  if (bc.n_bands > (1 << 20)) bc.n_bands = 1;   // (a band of a few rows: nothing to keep cached)
  if (bc.n_bands == 1) return MALS_OK;
  const char* m = std::getenv("MALS_BAND_MIN_ENTRIES");
  bc.min_avg = std::max<int64_t>(1, m ? std::atoll(m) : band_min_avg(slot_floats(h->T), k));
  const std::vector<int64_t>& rp = s.h_row_ptr;
  std::vector<BandRow> rows;
  for (int64_t r = 0; r < s.n_local; ++r) {
    const int64_t len = rp[r + 1] - rp[r];
    if (band_row_eligible(len, h->cfg.segment_nnz, bc.n_bands, bc.min_avg)) {
      bc.row.push_back(r);
      rows.push_back(BandRow{rp[r], len});
    }
  }
  if (rows.empty()) return MALS_OK;
  // (len >= min_avg * n_bands: the offsets are at most 2 nnz / min_avg words)
  const size_t n_off = rows.size() * (size_t)(bc.n_bands + 1);
  DeviceBuffer<BandRow> d_rows;
  DeviceBuffer<int64_t> d_off;
  DeviceBuffer<int> d_unsorted;
  HIPCHK(h, d_rows.alloc(rows.size()));
  HIPCHK(h, d_off.alloc(n_off));
  HIPCHK(h, d_unsorted.alloc(rows.size()));
  HIPCHK(h, hipMemcpyAsync(d_rows.get(), rows.data(), sizeof(BandRow) * rows.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(d_unsorted.get(), 0, sizeof(int) * rows.size(), h->stream));
  hipLaunchKernelGGL(band_cuts_kernel, dim3((unsigned)rows.size(), BAND_CHECK_SLICES), dim3(256), 0, h->stream, s.col, d_rows.get(),
                     (int)bc.n_bands, bc.band_rows, d_off.get(), d_unsorted.get());
  HIPCHK(h, hipGetLastError());
  bc.off.resize(n_off);
  bc.unsorted.resize(rows.size());
  HIPCHK(h, hipMemcpyAsync(bc.off.data(), d_off.get(), sizeof(int64_t) * n_off, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(bc.unsorted.data(), d_unsorted.get(), sizeof(int) * rows.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MALS_OK;
}

// What the list plan and the solve need to know about a shard's entries, found on the device where they live: the value
// statistics, the column range and the band cuts of the long rows.
int scan_shard(mals_handle h, SideState& s, BandCuts& bc) {
  s.max_abs_val = 0.f;
  s.mean_abs_val = 0.0;
  s.local_mean_abs_val = 0.0;
  if (s.nnz > 0) {  // one pass over the values: bounds the Gramian weights (gather_scale_kernel)
    HIPCHK(h, hipMemsetAsync(h->d_maxabs.get(), 0, 4 * sizeof(unsigned), h->stream));
    const unsigned blocks = (unsigned)std::min<int64_t>(4096, (s.nnz + 255) / 256);
    hipLaunchKernelGGL(max_abs_kernel, dim3(blocks), dim3(256), 0, h->stream, s.val, s.nnz, h->d_maxabs.get(),
                       reinterpret_cast<double*>(h->d_maxabs.get() + 2));
    HIPCHK(h, hipGetLastError());
    unsigned raw[4];
    HIPCHK(h, hipMemcpyAsync(raw, h->d_maxabs.get(), sizeof(raw), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::memcpy(&s.max_abs_val, &raw[0], sizeof(float));
    double sum = 0.0;
    std::memcpy(&sum, &raw[2], sizeof(double));
    s.mean_abs_val = sum / (double)s.nnz;
    s.local_mean_abs_val = s.mean_abs_val;
  }
  s.local_max_abs_val = s.max_abs_val;
  s.col_min = 0;
  s.col_max = -1;
  if (s.nnz > 0) {  // the same pass over the column indices: an index outside the opposite replica would be an
                    // out-of-bounds device access in the gather (and a write in the top-N mask)
    const int init[2] = {std::numeric_limits<int>::max(), std::numeric_limits<int>::min()};
    HIPCHK(h, hipMemcpyAsync(h->d_colrange.get(), init, sizeof(init), hipMemcpyHostToDevice, h->stream));
    const unsigned blocks = (unsigned)std::min<int64_t>(4096, (s.nnz + 255) / 256);
    hipLaunchKernelGGL(col_range_kernel, dim3(blocks), dim3(256), 0, h->stream, s.col, s.nnz, h->d_colrange.get());
    HIPCHK(h, hipGetLastError());
    int range[2];
    HIPCHK(h, hipMemcpyAsync(range, h->d_colrange.get(), sizeof(range), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    s.col_min = range[0];
    s.col_max = range[1];
    if (s.col_min < 0) return fail(h, MALS_INVALID_ARG, "negative column index");
  }
  if (int rc = find_band_cuts(h, s, bc)) return rc;
  {
    const char* e = std::getenv("MALS_BAND_FRONT");  // A/B: 0 = the strided 16x grid
    s.band_front = !e || std::atoi(e) != 0;
  }
  return MALS_OK;
}

// The planned lists onto the device (and, under MALS_DEBUG_LISTS, what they hold onto stderr).
int upload_work_lists(mals_handle h, SideState& s, const WorkPlan& plan, const BandCuts& bc) {
  s.chunks = plan.chunks;
  s.n_dual_rows = plan.n_dual_rows;
  if (std::getenv("MALS_DEBUG_LISTS")) {  // work decomposition of the upload (tuning aid)
    int64_t nd[4] = {0, 0, 0, 0}, ed[4] = {0, 0, 0, 0}, na = 0, nz = 0, n_long = 0;   // (rowsC also holds the slot groups)
    for (const ChunkRange& cr : s.chunks) {
      n_long += cr.nC;
      for (int c = 0; c < 4; ++c) {
        nd[c] += cr.nD[c];
        ed[c] += cr.nnzD[c];
      }
      na += cr.nA;
      nz += cr.nZ;
    }
    std::fprintf(stderr, "[lists] rows %lld: direct %lld (%lld entries), dual 1-16: %lld (%lld) 17-32: %lld (%lld) 33-48: %lld (%lld) 49-64: %lld (%lld), "
                         "zero-filled %lld, segments %lld of %lld long rows (%lld entries)\n",
                 (long long)s.n_local, (long long)na, (long long)plan.nnzA, (long long)nd[0], (long long)ed[0], (long long)nd[1], (long long)ed[1], (long long)nd[2],
                 (long long)ed[2], (long long)nd[3], (long long)ed[3], (long long)nz, (long long)plan.itemsB.size(), (long long)n_long, (long long)plan.nnzB);
    int64_t e_band = 0;
    for (const ChunkRange& cr : s.chunks) e_band += cr.nnzBand;
    std::fprintf(stderr, "[lists] bands %lld of %lld table rows (at least %lld entries per band): %lld banded rows (%lld entries) in %lld segments, "
                         "%lld long enough but unsorted\n",
                 (long long)bc.n_bands, (long long)bc.band_rows, (long long)bc.min_avg, (long long)plan.n_banded_rows, (long long)e_band,
                 (long long)plan.n_banded_segs, (long long)plan.n_unsorted);
  }
  if (!plan.itemsA.empty()) {
    HIPCHK(h, s.itemsA.alloc(plan.itemsA.size()));
    HIPCHK(h, hipMemcpy(s.itemsA.get(), plan.itemsA.data(), sizeof(WorkItem) * plan.itemsA.size(), hipMemcpyHostToDevice));
  }
  if (!plan.itemsB.empty()) {
    HIPCHK(h, s.itemsB.alloc(plan.itemsB.size()));
    HIPCHK(h, hipMemcpy(s.itemsB.get(), plan.itemsB.data(), sizeof(WorkItem) * plan.itemsB.size(), hipMemcpyHostToDevice));
    HIPCHK(h, s.rowsC.alloc(plan.rowsC.size()));
    HIPCHK(h, hipMemcpy(s.rowsC.get(), plan.rowsC.data(), sizeof(RowC) * plan.rowsC.size(), hipMemcpyHostToDevice));
    HIPCHK(h, s.scratch.alloc((size_t)(plan.n_slots * slot_floats(h->T))));
  }
  return MALS_OK;
}

// mals_set_chunk_rows, or the configuration's (0 = the shard in one chunk)
int64_t wanted_chunk_rows(mals_handle h, const SideState& s) { return s.chunk_rows_override >= 0 ? s.chunk_rows_override : h->cfg.chunk_rows; }

// Split the rows of a shard into the three work lists (DESIGN.md "work decomposition"), chunk by chunk: work_plan.h.
int build_work_lists(mals_handle h, SideState& s) {
  BandCuts bc;
  WorkPlan plan;
  s.n_dual_rows = 0;
  if (int rc = scan_shard(h, s, bc)) return rc;
  if (const char* why = plan_work_lists(s.h_row_ptr.data(), s.n_local, h->cfg.segment_nnz, wanted_chunk_rows(h, s), h->dual_blocks, h->n_cu, bc, plan))
    return fail(h, MALS_INVALID_ARG, why);
  return upload_work_lists(h, s, plan, bc);
}

int validate_matrix(mals_handle h, int side) {
  SideState& s = h->side[side];
  if (s.h_row_ptr.size() != (size_t)s.n_local + 1 || s.h_row_ptr[0] != 0 || s.h_row_ptr[(size_t)s.n_local] != s.nnz)
    return fail(h, MALS_INVALID_ARG, "row_ptr must have n_rows_local+1 entries, start at 0 and end at nnz");
  return MALS_OK;
}

// col_idx must index rows of the OPPOSITE side's factor replica (checked again at solve time: the
// replica may be declared after the matrix)
int validate_columns(mals_handle h, int side) {
  const SideState& s = h->side[side];
  const SideState& o = h->side[1 - side];
  if (s.nnz > 0 && o.n_total > 0 && (int64_t)s.col_max >= o.n_total)
    return fail(h, MALS_INVALID_ARG, "column index outside the opposite side's factor replica");
  return MALS_OK;
}

// ---- timing ------------------------------------------------------------------------------------
int begin_timed(mals_handle h, int kind, double bytes, PendingEvent& pe) {
  pe.kind = kind;
  pe.bytes = bytes;
  if (!h->timing) return MALS_OK;
  HIPCHK(h, pe.ev.ensure());   // (a pe whose pair end_timed moved out is empty again)
  HIPCHK(h, hipEventRecord(pe.ev.begin, h->stream));
  return MALS_OK;
}
int end_timed(mals_handle h, PendingEvent& pe) {
  if (!h->timing) return MALS_OK;
  HIPCHK(h, hipEventRecord(pe.ev.end, h->stream));
  h->pending.push_back(std::move(pe));
  return MALS_OK;
}
// the list leaves the handle first: on whichever path this returns, h->pending is empty and every event destroyed once
int drain_events(mals_handle h) {
  const std::vector<PendingEvent> pending = std::move(h->pending);
  h->pending.clear();
  for (const PendingEvent& pe : pending) {
    HIPCHK(h, hipEventSynchronize(pe.ev.end));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, pe.ev.begin, pe.ev.end));
    mals_stats& st = h->stats;
    switch (pe.kind) {
      case 0: st.rows_ms += ms; st.rows_launches += 1; st.rows_bytes += pe.bytes; break;
      case 1: st.segments_ms += ms; st.segments_launches += 1; st.segments_bytes += pe.bytes; break;
      case 2: st.finish_ms += ms; st.finish_launches += 1; st.finish_bytes += pe.bytes; break;
      case 4: st.dual_ms += ms; st.dual_launches += 1; st.dual_bytes += pe.bytes; break;
      case 5: st.rotate_ms += ms; st.rotate_launches += 1; st.rotate_bytes += pe.bytes; break;
      default: st.gramian_ms += ms; st.gramian_launches += 1; st.gramian_bytes += pe.bytes; break;
    }
  }
  return MALS_OK;
}

// ---- kernel dispatch ---------------------------------------------------------------------------
// The runtime feature-block count h->T as a compile-time constant: calls f(std::integral_constant<int, T>) for the T in
// MIN_T .. 8 that it is (the rotations and the dual kernels exist from T = 2 on) and returns what f returns.
template <int MIN_T = 1, typename F>
int dispatch_T(mals_handle h, F&& f) {
  if (h->T == MIN_T) return f(std::integral_constant<int, MIN_T>());
  if constexpr (MIN_T < 8) return dispatch_T<MIN_T + 1>(h, f);
  return fail(h, MALS_INVALID_ARG, "unsupported feature count");
}
// gather depth D of the fp32 persistent kernels (rows whose gathers are in flight at once) per T
constexpr int gather_depth(int T) { return T <= 3 ? 4 : T == 4 ? MALS_D4 : 2; }

// fp64 kernel below this many rows, split-f16 kernel (slabs of 512 rows = 32 accumulation steps, fp64 sum over the
// slabs) from there on: even when a few rows dominate G (no averaging over slabs) the fp32 slab sums stay within
// 6e-8 x sqrt(32) of it (als_kernels.h, gramian_split_kernel)
constexpr int64_t GRAMIAN_SPLIT_MIN_ROWS = 262144;
// Rows a wave of gramian_split_kernel sums in fp32 before its partial goes to the fp64 stages.  512 keeps a 262144-row matrix
// at 128 workgroups; from 4M rows on the 10 KB partial per slab (200 MB written and read again at 10M rows, a sixth of the
// input; a second one only for the slabs the kernel cuts) is worth more than the extra waves: 2048 there (10M x 64: 0.67 -> 0.53 ms; 0.54 with the second launch for cut slabs).  fp32 roundings per accumulator and slab:
// 3 per 32-row step, 192 at 2048 rows -- 8e-7 relative at random, averaged over thousands of slabs in fp64.
inline int64_t gramian_slab_rows(int64_t n_rows) {
  static const int64_t forced = std::getenv("MALS_GRAMIAN_SLAB_ROWS") ? std::atoll(std::getenv("MALS_GRAMIAN_SLAB_ROWS")) : 0;  // tuning override (a multiple of 64)
  if (forced > 0) return forced;
  int64_t slab = 512;
  while (slab < 2048 && n_rows / (2 * slab) / 4 >= 1024) slab *= 2;
  return slab;
}

template <int T>
int launch_gramian_T(mals_handle h, SideState& s, const float* M, int64_t n_rows, double* G_out, float* Gf_out, unsigned* ymax) {
  const int k = h->cfg.features;
  const int elems = tri(T) * 256;
  static const bool force_f64 = std::getenv("MALS_GRAMIAN_F64") != nullptr;  // A/B
  if (n_rows >= GRAMIAN_SPLIT_MIN_ROWS && !force_f64) {
    const int64_t slab_rows = gramian_slab_rows(n_rows);
    int64_t n_slabs = (n_rows + slab_rows - 1) / slab_rows;
    n_slabs = (n_slabs + 3) & ~(int64_t)3;  // whole workgroups
    constexpr int GROUPS = 64;              // first-stage sums (doubles) behind the slab partials (floats)
    // a partial per slab, room for a second one (written and read only for the slabs the kernel cuts in two), the groups' sums, the cut row per slab
    const size_t slab_bytes = sizeof(float) * (size_t)n_slabs * tri(T) * 256;
    const size_t bytes = 2 * slab_bytes + sizeof(double) * (size_t)GROUPS * tri(T) * 256 + sizeof(int) * (size_t)n_slabs;
    if (s.partials.capacity() < bytes) HIPCHK(h, s.partials.alloc(bytes));
    float* pf = reinterpret_cast<float*>(s.partials.get());
    float* pf2 = reinterpret_cast<float*>(s.partials.get() + slab_bytes);
    double* pd = reinterpret_cast<double*>(s.partials.get() + 2 * slab_bytes);  // slab_bytes is a multiple of 1024
    int* has2 = reinterpret_cast<int*>(s.partials.get() + 2 * slab_bytes + sizeof(double) * (size_t)GROUPS * tri(T) * 256);
    hipLaunchKernelGGL((gramian_split_kernel<T, false>), dim3((unsigned)(n_slabs / 4)), dim3(256), 0, h->stream, M, n_rows, k,
                       slab_rows, pf, has2, ymax);
    // the rows behind the cuts of the first pass (a quiet step after a loud one), summed on their own; waves of slabs without one return
    hipLaunchKernelGGL((gramian_split_kernel<T, true>), dim3((unsigned)(n_slabs / 4)), dim3(256), 0, h->stream, M, n_rows, k,
                       slab_rows, pf2, has2, ymax);
    hipLaunchKernelGGL(gramian_reduce_slabs_kernel, dim3((unsigned)((elems + 255) / 256), GROUPS), dim3(256), 0, h->stream, pf, pf2, has2, n_slabs,
                       elems, GROUPS, pd);
    hipLaunchKernelGGL((gramian_finalize_kernel<T, false>), dim3(elems / 64), dim3(256), 0, h->stream, pd, (int64_t)GROUPS, k, G_out, Gf_out);
    HIPCHK(h, hipGetLastError());
    return MALS_OK;
  }
  // waves: at least 64 rows each, at most 1024 waves (the finalize pass costs per partial).  (256 rows each until round 3: a 17 770-row Y then ran on 72 of the
  // chip's 1024 SIMDs for 174 us at k = 100, C2's two matrices for 44 us each -- 7 % of its iteration.)
  int64_t n_waves = std::min<int64_t>(1024, std::max<int64_t>(1, (n_rows + 63) / 64));
  n_waves = (n_waves + 3) & ~(int64_t)3;
  int64_t rows_per_wave = (n_rows + n_waves - 1) / n_waves;
  rows_per_wave = std::max<int64_t>(4, (rows_per_wave + 3) & ~(int64_t)3);
  const size_t bytes = sizeof(double) * (size_t)n_waves * tri(T) * 256;
  if (s.partials.capacity() < bytes) HIPCHK(h, s.partials.alloc(bytes));
  double* partials = reinterpret_cast<double*>(s.partials.get());
  // the fp64 kernel (small matrices: the diagonal's bound is at most 9 binades loose there) records no maximum; tracking
  // it cost the latency-bound kernel 20-40 % (measured on C2).  "Unknown" = a word above 3e38 that survives every max.
  if (ymax) HIPCHK(h, hipMemsetAsync(ymax, 0x7f, sizeof(unsigned), h->stream));
  hipLaunchKernelGGL((gramian_partial_kernel<T>), dim3((unsigned)(n_waves / 4)), dim3(256), 0, h->stream, M, n_rows, k,
                     rows_per_wave, partials);
  hipLaunchKernelGGL((gramian_finalize_kernel<T, true, 16>), dim3(elems / 16), dim3(256), 0, h->stream, partials, n_waves,
                     k, G_out, Gf_out);
  HIPCHK(h, hipGetLastError());
  return MALS_OK;
}

int launch_gramian(mals_handle h, SideState& s, const float* M, int64_t n_rows, double* G_out, float* Gf_out, unsigned* ymax = nullptr) {
  return dispatch_T(h, [&](auto t) { return launch_gramian_T<t()>(h, s, M, n_rows, G_out, Gf_out, ymax); });
}

// Grid of the persistent kernels.  Work item i goes to wave i mod W of a length-sorted list, so every
// wave gets the same mix of row lengths; W is 16x the resident capacity (CUs x blocks/CU from the
// occupancy query), never more than the work needs.  Measured on C4 (profiles/): exactly-resident
// grids lose ~10% to waves that run slower than their peers (nothing rebalances a static
// assignment), 12-16x oversubscription lets the dispatcher level that out and each wave still
// walks >100 rows, which keeps the cross-row prefetch effective; beyond 16x nothing changes.
// block: threads per workgroup, one work item per wave.  resident_per_cu: the workgroups a CU holds where the caller
// knows (the LDS-staged kernels), 0 = ask the occupancy query.
template <typename K>
int persistent_grid(mals_handle h, K kernel, int64_t n_work, unsigned* grid, bool front = false, int block = 256, int resident_per_cu = 0) {
  const int64_t groups = (n_work + block / 64 - 1) / (block / 64);
  if (front) {  // banded segments: one item per wave, workgroups dispatched in list order -- the resident waves then work
                // on one contiguous stretch of the list, i.e. on one or two bands of the table, where the strided
                // assignment has as many bands in flight as the list is longer than the grid
    *grid = (unsigned)std::max<int64_t>(1, groups);
    return MALS_OK;
  }
  int per_cu = resident_per_cu;
  if (!per_cu) HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0));
  if (per_cu < 1) per_cu = 1;
  per_cu *= 16;
  if (const char* e = std::getenv("MALS_BLOCKS_PER_CU")) per_cu = std::max(1, std::atoi(e)) * (256 / block);  // tuning override (in 256-thread blocks)
  const int64_t cap = (int64_t)h->n_cu * per_cu;
  *grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(groups, cap));
  return MALS_OK;
}

// what one launch_solve call covers: the rows list (+ zero-fill) / the dual lists through the direct kernel / the long
// rows (segments + finish).  The three are independent of each other (disjoint output rows, read-only inputs).
enum { LISTS_ROWS = 1, LISTS_DUAL_ROWS = 2, LISTS_LONG = 4 };

// The kernels that run a chunk's lists, and how they are launched: what differs between the families launch_solve_TF
// chooses from.  An fp32 twin (std::nullptr_t: none) follows its split-precision kernel with flag bit 3: exactly one of
// the two does the work (gather_scale_kernel's range flag), the other returns at once.
template <typename KR, typename KS, typename KRF, typename KSF, typename KC, typename KCF, typename KP>
struct ListKernels {
  KR rows;         // list A
  KS segments;     // list B
  KRF rows_f32;    // their fp32-gather twins
  KSF segments_f32;
  KC finish;       // list C
  KCF finish_f32;  // the finish kernel of the twins' partial slots where those differ in layout (flag bit 3 again)
  KP prereduce;
  int block;            // threads per workgroup of rows / segments
  int resident_per_cu;  // persistent_grid
};
template <typename KR, typename KS, typename KRF, typename KSF, typename KC, typename KCF, typename KP>
ListKernels(KR, KS, KRF, KSF, KC, KCF, KP, int, int) -> ListKernels<KR, KS, KRF, KSF, KC, KCF, KP>;

// One persistent launch, plus -- for a split-precision kernel -- its fp32-gather twin right behind it.
template <typename K, typename KF>
int launch_persistent(mals_handle h, K kernel, KF fallback, int block, int resident_per_cu, const SolveParams& p, int kind, double bytes, bool front) {
  PendingEvent pe;
  unsigned grid = 1;
  if (int rc = persistent_grid(h, kernel, p.n_work, &grid, front, block, resident_per_cu)) return rc;
  if (int rc = begin_timed(h, kind, bytes, pe)) return rc;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, h->stream, p);
  if constexpr (!std::is_same<KF, std::nullptr_t>::value) {
    SolveParams pf = p;
    pf.flags |= 8;
    if (int rc = persistent_grid(h, fallback, p.n_work, &grid)) return rc;
    // the twin almost always returns at once: a resident-sized grid keeps that at a few microseconds (a full 16x
    // oversubscribed grid of empty workgroups costs 15-30); when it does run it only loses the oversubscription
    grid = std::min<unsigned>(grid, (unsigned)h->n_cu * 8u);
    hipLaunchKernelGGL(fallback, dim3(grid), dim3(256), 0, h->stream, pf);
  }
  return end_timed(h, pe);
}

template <typename LK>
int launch_lists(mals_handle h, SideState& s, SolveParams p, int chunk, int which, const LK& fam) {
  const double per = 4.0 * p.k + 8.0;  // gathered row + col idx + value; written row + row_ptr
  const ChunkRange& cr = s.chunks[(size_t)chunk];
  const bool own = which & LISTS_ROWS, longs = which & LISTS_LONG, dual_rows_too = which & LISTS_DUAL_ROWS;
  const WorkItem *A = s.itemsA.get() + cr.offA, *B = s.itemsB.get() + cr.offB;
  const int64_t n_plain = cr.nB - cr.nBand, n_dual = cr.n_dual();
  struct Run {
    const WorkItem* items;
    int64_t n;
    double bytes;
    int kind;    // 0 = rows (list A), 1 = segments (list B): kernel and timing kind
    bool front;
  };
  const Run runs[4] = {
      {B, longs ? n_plain : 0, (double)(cr.nnzB - cr.nnzBand) * per, 1, false},
      {B + n_plain, longs ? cr.nBand : 0, (double)cr.nnzBand * per, 1, s.band_front},  // the banded tail of list B, band by band
      {A, own ? cr.nA : 0, (double)cr.nnzA * per + (double)cr.nA * per, 0, false},
      // the dual lists through the direct kernel (the half-iteration does not qualify)
      {A + cr.nA, dual_rows_too ? n_dual : 0, (double)cr.nnz_dual() * per + (double)n_dual * per, 0, false}};
  for (const Run& r : runs) {
    if (!r.n) continue;
    p.n_work = r.n;
    p.items = r.items;
    if (int rc = r.kind ? launch_persistent(h, fam.segments, fam.segments_f32, fam.block, fam.resident_per_cu, p, 1, r.bytes, r.front)
                        : launch_persistent(h, fam.rows, fam.rows_f32, fam.block, fam.resident_per_cu, p, 0, r.bytes, r.front))
      return rc;
  }
  if (longs && cr.nC) {
    PendingEvent pe;
    if (int rc = begin_timed(h, 2, (double)cr.nC * per, pe)) return rc;
    if (cr.nP) {
      p.n_work = cr.nP;
      p.rowsC = s.rowsC.get() + cr.offP;
      hipLaunchKernelGGL(fam.prereduce, dim3((unsigned)((cr.nP + 3) / 4)), dim3(256), 0, h->stream, p);
    }
    p.n_work = cr.nC;
    p.rowsC = s.rowsC.get() + cr.offC;
    hipLaunchKernelGGL(fam.finish, dim3((unsigned)((cr.nC + 3) / 4)), dim3(256), 0, h->stream, p);
    if constexpr (!std::is_same<decltype(fam.finish_f32), std::nullptr_t>::value) {
      SolveParams pf = p;
      pf.flags |= 8;
      hipLaunchKernelGGL(fam.finish_f32, dim3((unsigned)((cr.nC + 3) / 4)), dim3(256), 0, h->stream, pf);
    }
    if (int rc = end_timed(h, pe)) return rc;
  }
  if (own && cr.nZ) {
    hipLaunchKernelGGL(zero_rows_kernel, dim3((unsigned)((cr.nZ + 31) / 32)), dim3(256), 0, h->stream,  // 8 rows per wave
                       A + cr.nA + n_dual, cr.nZ, p.k, p.out);
  }
  HIPCHK(h, hipGetLastError());
  return MALS_OK;
}

template <int T, bool FULL>
int launch_solve_TF(mals_handle h, SideState& s, const SolveParams& p, int chunk, int which) {
  constexpr int D = gather_depth(T);
  constexpr auto rows_f32 = als_persistent_kernel<T, D, 0, FULL>;
  constexpr auto segments_f32 = als_persistent_kernel<T, D, 1, FULL>;
  if constexpr (T == 8 && FULL) {
    // k = 128 through the LDS-staged kernels (lds_kernels.h): one wave per workgroup, LDS-limited to 8 per CU.  Their
    // partial slots are in the kernels' own feature order, the fp32 twins' (range flag 0) in the plain one: both finish
    // kernels are enqueued and the range flag decides on the device which of the two runs (bit 3 again: "only if the
    // split-precision launch did not run").
    if (h->split_f16 && h->lds_gather && p.Gperm)
      return launch_lists(h, s, p, chunk, which, ListKernels{als_lds_kernel_h<0>, als_lds_kernel_h<1>, rows_f32, segments_f32, als_finish_kernel<T, true>,
                                                             als_finish_kernel<T, false>, als_prereduce_kernel<T>, 64, 8});
  }
  if constexpr (T == 4) {
    if (h->split3)
      return launch_lists(h, s, p, chunk, which, ListKernels{als_persistent_kernel_h<T, 0, FULL, 3>, als_persistent_kernel_h<T, 1, FULL, 3>, rows_f32,
                                                             segments_f32, als_finish_kernel<T>, nullptr, als_prereduce_kernel<T>, 256, 0});
  }
  if (h->split_f16)
    return launch_lists(h, s, p, chunk, which, ListKernels{als_persistent_kernel_h<T, 0, FULL>, als_persistent_kernel_h<T, 1, FULL>, rows_f32,
                                                           segments_f32, als_finish_kernel<T>, nullptr, als_prereduce_kernel<T>, 256, 0});
  return launch_lists(h, s, p, chunk, which,
                      ListKernels{rows_f32, segments_f32, nullptr, nullptr, als_finish_kernel<T>, nullptr, als_prereduce_kernel<T>, 256, 0});
}

// the direct kernels over a chunk's lists (LISTS_*)
int launch_solve(mals_handle h, SideState& s, const SolveParams& p, int chunk, int which) {
  return dispatch_T(h, [&](auto t) {
    return p.k == 16 * t() ? launch_solve_TF<t(), true>(h, s, p, chunk, which) : launch_solve_TF<t(), false>(h, s, p, chunk, which);
  });
}

// ---- refinement of the rows the solving kernels marked (als_refine_kernel) -------------------------
int launch_refine(mals_handle h, const RefineParams& q) {
  // reads the marks on the device: no host round trip.  A resident-sized grid; a chunk without marked rows costs
  // one pass over its flag bytes.
  const int64_t rows = q.row_end - q.row_begin;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + 255) / 256, (int64_t)h->n_cu * 8));
  return dispatch_T(h, [&](auto t) -> int {
    hipLaunchKernelGGL((als_refine_kernel<t()>), dim3(grid), dim3(256), 0, h->stream, q);
    HIPCHK(h, hipGetLastError());
    return MALS_OK;
  });
}

// The reference's M^T M (MU:219-239 rounds every product to fp32) for the refinement of marked rows; the kernel
// returns at once unless a row has been marked in this half-iteration and the matrix is not there yet.
int launch_gramian_ref(mals_handle h, const SideState& o) {
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((o.n_total + 63) / 64, (int64_t)h->n_cu * 2));
  return dispatch_T(h, [&](auto t) -> int {
    hipLaunchKernelGGL(gramian_ref_latch_kernel, dim3(1), dim3(1), 0, h->stream, h->d_gref_state.get());
    hipLaunchKernelGGL((gramian_ref_kernel<t()>), dim3(grid), dim3(256), 0, h->stream, o.F, o.n_total, h->cfg.features, h->d_gref_state.get(),
                       h->d_gref_part.get(), h->d_Gref.get());
    HIPCHK(h, hipGetLastError());
    return MALS_OK;
  });
}

int launch_exact(mals_handle h, const RefineParams& q, int level) {
  const int k = h->cfg.features;
  const size_t lds = sizeof(double) * ((size_t)k * (k + 1) + 2 * (size_t)k) + sizeof(float) * (size_t)k + sizeof(int) * 256;
  if (!h->exact_ready) {
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&als_exact_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    h->exact_ready = true;
  }
  const int64_t rows = q.row_end - q.row_begin;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + 255) / 256, (int64_t)h->n_cu * 4));
  hipLaunchKernelGGL((als_exact_kernel<0>), dim3(grid), dim3(256), lds, h->stream, q, level);
  HIPCHK(h, hipGetLastError());
  return MALS_OK;
}

// ---- dual path (dual_kernels.h) ------------------------------------------------------------------
template <bool LISTED, bool F64>
int launch_rotate(mals_handle h, const RotateParams& rp) {
  const int64_t tiles = (rp.n_rows + (F64 ? 31 : 63)) / (F64 ? 32 : 64);
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((tiles + 3) / 4, (int64_t)h->n_cu * 16));
  return dispatch_T<2>(h, [&](auto t) -> int {
    hipLaunchKernelGGL((rotate_rows_kernel<t(), LISTED, F64>), dim3(grid), dim3(256), 0, h->stream, rp);
    HIPCHK(h, hipGetLastError());
    return MALS_OK;
  });
}

template <bool LISTED>
int launch_rotate_split(mals_handle h, const RotateSplitParams& rp) {
  return dispatch_T<2>(h, [&](auto t) -> int {
    const int rows_per_wave = 16 * rotate_split_tiles(t());
    const int64_t tiles = (rp.n_rows + rows_per_wave - 1) / rows_per_wave;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((tiles + 3) / 4, (int64_t)h->n_cu * 16));
    hipLaunchKernelGGL((rotate_rows_split_kernel<t(), LISTED>), dim3(grid), dim3(256), 0, h->stream, rp);
    HIPCHK(h, hipGetLastError());
    return MALS_OK;
  });
}

// the same rotation on the f16 matrix pipe: Bs = Q (or Q^T) as split operands (split_rotation_operand) in place of B / Bf, and
// a bound on |src|, on the device (bound_bits) or known to the host
RotateSplitParams rotate_split_params(const RotateParams& rp, const int32_t* Bs, const unsigned* bound_bits, float bound_host) {
  RotateSplitParams sp;
  sp.src = rp.src;
  sp.dst = rp.dst;
  sp.Bs = reinterpret_cast<const i32x4*>(Bs);
  sp.items = rp.items;
  sp.dmax = rp.dmax;
  sp.zbound = rp.zbound;
  sp.bound_bits = bound_bits;
  sp.bound_host = bound_host;
  sp.n_rows = rp.n_rows;
  sp.k = rp.k;
  sp.src_stride = rp.src_stride;
  sp.dst_stride = rp.dst_stride;
  sp.dst_cols = rp.dst_cols;
  return sp;
}

// fp32 -> f16 bit pattern, round to nearest even (the compiler's conversion) / toward zero
uint16_t half_rne(float v) {
  const _Float16 x = (_Float16)v;
  uint16_t b;
  std::memcpy(&b, &x, 2);
  return b;
}
uint16_t half_rtz(float v) {
  uint16_t b = half_rne(v);
  _Float16 x;
  std::memcpy(&x, &b, 2);
  if (std::fabs((float)x) > std::fabs(v)) --b;  // one step toward zero: f16 magnitudes order like their bit patterns
  return b;
}
float half_to_float(uint16_t b) {
  _Float16 x;
  std::memcpy(&x, &b, 2);
  return (float)x;
}

// Q (or Q^T), times 2^13, as the split-f16 B operands of rotate_rows_split_kernel: Bs[q][t][hi|lo][lane][4 dwords],
// lane (g,c) slot s = element [32 q + 8 g + s][16 t + c]
void split_rotation_operand(const double* B, int k, int KP, int T, std::vector<int32_t>& out) {
  const int KC = (T + 1) / 2;
  out.assign((size_t)KC * T * 2 * 64 * 4, 0);
  for (int q = 0; q < KC; ++q)
    for (int t = 0; t < T; ++t)
      for (int lane = 0; lane < 64; ++lane) {
        const int g = lane >> 4, c = lane & 15;
        uint16_t hi[8], lo[8];
        for (int s8 = 0; s8 < 8; ++s8) {
          const int f = 32 * q + 8 * g + s8;
          const float v = f < k ? (float)(B[(size_t)f * KP + 16 * t + c] * 8192.0) : 0.f;
          hi[s8] = half_rtz(v);
          lo[s8] = half_rne(v - half_to_float(hi[s8]));
        }
        int32_t* oh = &out[(((size_t)(q * T + t) * 2 + 0) * 64 + lane) * 4];
        int32_t* ol = &out[(((size_t)(q * T + t) * 2 + 1) * 64 + lane) * 4];
        for (int e = 0; e < 4; ++e) {
          oh[e] = (int32_t)((uint32_t)hi[2 * e] | ((uint32_t)hi[2 * e + 1] << 16));
          ol[e] = (int32_t)((uint32_t)lo[2 * e] | ((uint32_t)lo[2 * e + 1] << 16));
        }
      }
}

template <int T, int TN>
int launch_dual_TN(mals_handle h, DualParams dp) {
  unsigned grid = 1;
  if (int rc = persistent_grid(h, als_dual_kernel<T, TN>, dp.n_work, &grid)) return rc;
  hipLaunchKernelGGL((als_dual_kernel<T, TN>), dim3(grid), dim3(256), 0, h->stream, dp);
  HIPCHK(h, hipGetLastError());
  return MALS_OK;
}
template <int T>
int launch_dual_T(mals_handle h, const DualParams& dp, int tn) {
  if constexpr (dual_max_blocks(T) >= 1) { if (tn == 1) return launch_dual_TN<T, 1>(h, dp); }
  if constexpr (dual_max_blocks(T) >= 2) { if (tn == 2) return launch_dual_TN<T, 2>(h, dp); }
  if constexpr (dual_max_blocks(T) >= 3) { if (tn == 3) return launch_dual_TN<T, 3>(h, dp); }
  if constexpr (dual_max_blocks(T) >= 4) { if (tn == 4) return launch_dual_TN<T, 4>(h, dp); }
  return fail(h, MALS_INVALID_ARG, "no dual kernel for this row class");
}
int launch_dual(mals_handle h, const DualParams& dp, int tn) {
  return dispatch_T<2>(h, [&](auto t) { return launch_dual_T<t()>(h, dp, tn); });
}

// Once per half-iteration, in two halves.  HOST: G (opposite side, already on its way to h_G) -> eigendecomposition
// -> everything the device needs, staged in one pinned block.  A group computes it on ONE member and hands the block
// to the others (`from`): after the all-reduce every member holds the same G, and a k x k eigenproblem solved once
// per member by the one thread that drives them all would only delay the later members' kernels.  DEVICE:
// asynchronous uploads out of the block + the rotated copy of the opposite factors.  Both run AFTER the direct
// kernels of the first chunk have been enqueued, so the host work hides under them.  Sets h->dual_ok.
double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct EigStage {  // views into mals_handle_s::eig_stage
  double* Q;
  float* Qf;
  float* lam;
  int32_t* Bs;
  size_t nQ, nLam, nBs;  // elements: 2 KP^2, 2 KP, KC T 2 64 4 per operand
};
EigStage eig_views(mals_handle h) {
  const size_t KP = (size_t)16 * h->T, KC = (size_t)(h->T + 1) / 2;
  EigStage e;
  e.nQ = 2 * KP * KP;
  e.nLam = 2 * KP;
  e.nBs = KC * h->T * 2 * 64 * 4;
  char* b = h->eig_stage.get();
  e.Q = reinterpret_cast<double*>(b);
  e.Qf = reinterpret_cast<float*>(b + sizeof(double) * e.nQ);
  e.lam = e.Qf + e.nQ;
  e.Bs = reinterpret_cast<int32_t*>(e.lam + e.nLam);
  return e;
}
int ensure_eig_stage(mals_handle h) {
  if (h->eig_stage) return MALS_OK;
  const size_t KP = (size_t)16 * h->T, KC = (size_t)(h->T + 1) / 2;
  const size_t bytes = sizeof(double) * 2 * KP * KP + sizeof(float) * (2 * KP * KP + 2 * KP) + sizeof(int32_t) * 2 * KC * h->T * 2 * 64 * 4;
  HIPCHK(h, h->eig_stage.alloc(bytes));
  return MALS_OK;
}

int prepare_dual_host(mals_handle h, int side, mals_handle from) {
  SideState& o = h->side[1 - side];
  const int k = h->cfg.features, KP = 16 * h->T;
  h->dual = HalfStamp{side, o.G_version};
  h->dual_ok = false;
  h->eig_ok = false;
  if (int rc = ensure_eig_stage(h)) return rc;
  // h_G <- o.G was enqueued before the direct kernels, behind everything of the previous half-iteration: once it is
  // in, the uploads that read the block last time are done as well and the block may be rewritten
  HIPCHK(h, hipEventSynchronize(h->ev_G));
  h->tl[1] = now_us();
  if (from && from != h) {  // the same G, decomposed by another member of the group
    if (from->eig_stage.capacity() != h->eig_stage.capacity()) return fail(h, MALS_INVALID_ARG, "members of a group must share features");
    std::memcpy(h->eig_stage.get(), from->eig_stage.get(), h->eig_stage.capacity());
    h->eig_ok = from->eig_ok;
    h->eig_gmax = from->eig_gmax;
    h->rotate_f64 = from->rotate_f64;
    h->rotate_split = from->rotate_split;
    h->tl[2] = now_us();
    return MALS_OK;
  }
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<double> evals((size_t)k), V((size_t)k * k);
  const bool ok = mals::symmetric_eigen(h->h_G.get(), k, evals.data(), V.data());
  h->stats.eigen_host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  h->tl[2] = now_us();
  if (!ok) return MALS_OK;
  double lmin = evals[0], lmax = evals[0];
  for (int f = 0; f < k; ++f) {
    lmin = std::min(lmin, evals[(size_t)f]);
    lmax = std::max(lmax, evals[(size_t)f]);
  }
  const double la = h->cfg.lambda * h->cfg.alpha;
  // A_u = G + lambda alpha n_u I must be safely positive definite for every n_u >= 1 (then W_u is too,
  // and the direct path could not have flagged the row either); tiny negative eigenvalues of a
  // rank-deficient G are rounding
  if (!(lmin + la >= 1.0e-4)) return MALS_OK;
  EigStage e = eig_views(h);
  std::fill(e.Q, e.Q + e.nQ, 0.0);
  for (int f = 0; f < k; ++f)
    for (int j = 0; j < k; ++j) {
      e.Q[(size_t)f * KP + j] = V[(size_t)f * k + j];                        // forward: y' = y Q
      e.Q[(size_t)KP * KP + (size_t)f * KP + j] = V[(size_t)j * k + f];      // back: x = x' Q^T
    }
  for (int f = 0; f < KP; ++f) {
    const double l = f < k ? std::max(evals[(size_t)f], 0.0) : 0.0;
    e.lam[(size_t)f] = (float)l;
    e.lam[(size_t)KP + f] = (float)(1.0 / std::sqrt(l + la));
  }
  for (size_t i = 0; i < e.nQ; ++i) e.Qf[i] = (float)e.Q[i];
  // fp32 rotation unless the spectrum is wide enough for a rotated coordinate to be a small difference of
  // large products (dual_kernels.h, rotate_rows_kernel)
  h->rotate_f64 = (lmax + la) > 1.0e5 * (std::max(lmin, 0.0) + la);
  if (const char* ev = std::getenv("MALS_ROTATE_F64")) h->rotate_f64 = std::atoi(ev) != 0;  // tests / A-B
  h->rotate_split = k % 8 == 0 && !std::getenv("MALS_ROTATE_NO_SPLIT");
  if (std::getenv("MALS_DEBUG_LISTS"))  // which of the rotation kernels this half-iteration runs (prepare_dual_device, launch_dual_chunk)
    std::fprintf(stderr, "[lists] rotation forward %s, back %s\n", h->rotate_f64 ? "fp64" : (h->rotate_split ? "split" : "fp32"), h->rotate_split ? "split" : "fp32");
  if (h->rotate_split) {
    std::vector<int32_t> Bs;
    for (int op = 0; op < 2; ++op) {
      split_rotation_operand(e.Q + (size_t)op * KP * KP, k, KP, h->T, Bs);
      std::memcpy(e.Bs + (size_t)op * e.nBs, Bs.data(), sizeof(int32_t) * e.nBs);
    }
  }
  double gmax = 0.0;   // max |y_f| <= sqrt(max_f G_ff)
  for (int f = 0; f < k; ++f) gmax = std::max(gmax, h->h_G.get()[(size_t)f * k + f]);
  h->eig_gmax = gmax;
  h->eig_ok = true;
  return MALS_OK;
}

int prepare_dual_device(mals_handle h, int side) {
  SideState& o = h->side[1 - side];
  const int k = h->cfg.features, KP = 16 * h->T;
  h->dual_ok = false;
  if (!h->eig_ok) return MALS_OK;
  const EigStage e = eig_views(h);
  if (!h->d_eig) {  // one device block with the layout of the pinned one: ONE upload per half-iteration instead of four
    HIPCHK(h, h->d_eig.alloc(h->eig_stage.capacity()));
    char* d = h->d_eig.get();
    h->d_Q = reinterpret_cast<double*>(d);
    h->d_Qf = reinterpret_cast<float*>(d + (reinterpret_cast<char*>(e.Qf) - h->eig_stage.get()));
    h->d_lam = reinterpret_cast<float*>(d + (reinterpret_cast<char*>(e.lam) - h->eig_stage.get()));
    h->d_Bs = reinterpret_cast<int32_t*>(d + (reinterpret_cast<char*>(e.Bs) - h->eig_stage.get()));
  }
  // {z bound of the dual kernels, x' bound of the un-rotation of the even chunks, of the odd chunks}: a chunk's un-rotation
  // picks its operand scale from the bound its OWN dual kernels left -- with the chunks on two alternating streams a
  // shared slot made the scale (hence the f16 split of small components) depend on how far the other stream had got
  if (!h->d_zbound) HIPCHK(h, h->d_zbound.alloc(3));
  HIPCHK(h, h->d_Mr.reserve((size_t)o.n_total * KP, h->stream));
  // pinned source, rewritten no earlier than the next half-iteration's prepare_dual_host (which waits for this stream)
  HIPCHK(h, hipMemcpyAsync(h->d_eig.get(), h->eig_stage.get(), h->eig_stage.capacity(), hipMemcpyHostToDevice, h->stream));
  h->Bs_stride = e.nBs;
  HIPCHK(h, hipMemsetAsync(h->d_zbound.get(), 0, 3 * sizeof(unsigned), h->stream));
  RotateParams rp;
  rp.src = o.F;
  rp.dst = h->d_Mr.get();
  rp.B = h->d_Q;
  rp.Bf = h->d_Qf;
  rp.items = nullptr;
  rp.dmax = h->d_lam + KP;
  rp.zbound = h->d_zbound.get();
  rp.n_rows = o.n_total;
  rp.k = k;
  rp.src_stride = k;
  rp.dst_stride = KP;
  rp.dst_cols = KP;
  PendingEvent pe;
  if (int rc = begin_timed(h, 5, (double)o.n_total * (4.0 * k + 4.0 * KP), pe)) return rc;
  if (h->rotate_split && !h->rotate_f64) {
    if (int rc = launch_rotate_split<false>(h, rotate_split_params(rp, h->d_Bs, nullptr, (float)std::sqrt(h->eig_gmax)))) return rc;
  } else if (int rc = h->rotate_f64 ? launch_rotate<false, true>(h, rp) : launch_rotate<false, false>(h, rp)) {
    return rc;
  }
  if (int rc = end_timed(h, pe)) return rc;
  h->dual_ok = true;
  return MALS_OK;
}

// the dual lists of one chunk: als_dual_kernel per row class, then x = Q x' in place
int launch_dual_chunk(mals_handle h, int side, int chunk) {
  SideState& s = h->side[side];
  const ChunkRange& cr = s.chunks[(size_t)chunk];
  const int k = h->cfg.features, KP = 16 * h->T;
  const double per = 4.0 * k + 8.0;
  DualParams dp;
  dp.col = s.col;
  dp.val = s.val;
  dp.Mr = h->d_Mr.get();
  dp.lam = h->d_lam;
  dp.zbound = h->d_zbound.get();
  dp.out = s.F + s.row_offset * k;
  dp.bad_row = h->d_bad.get() + side;
  dp.k = k;
  dp.alpha = (float)h->cfg.alpha;
  dp.lambda_alpha = (float)(h->cfg.lambda * h->cfg.alpha);
  dp.sqrt_w_max = (float)std::sqrt(std::fabs(h->cfg.alpha) * (double)s.max_abs_val);
  dp.xbound = h->d_zbound.get() + 1 + (chunk & 1);
  HIPCHK(h, hipMemsetAsync(dp.xbound, 0, sizeof(unsigned), h->stream));  // same stream as the chunk two back, whose un-rotation is done
  dp.any_marked = h->d_gref_state.get();
  dp.refine_flag = h->refine_limit > 0.f ? s.refine.get() : nullptr;
  dp.refine_limit = h->refine_limit;
  const WorkItem* base = s.itemsA.get() + cr.offA + cr.nA;
  int64_t off = 0;
  PendingEvent pe;
  // (Two classes in flight at a time on two streams -- one class's tail under the next one's head -- was built in round 4
  // and measured flat on c4rank, 11.37 vs 11.36 ms: the dual kernels are issue bound, not tail bound.)
  for (int cls = 3; cls >= 0; --cls) {  // descending length, as stored
    if (!cr.nD[cls]) continue;
    dp.items = base + off;
    dp.n_work = cr.nD[cls];
    if (int rc = begin_timed(h, 4, (double)cr.nnzD[cls] * per + (double)cr.nD[cls] * per, pe)) return rc;
    if (int rc = launch_dual(h, dp, cls + 1)) return rc;
    if (int rc = end_timed(h, pe)) return rc;
    off += cr.nD[cls];
  }
  RotateParams rp;
  rp.src = dp.out;
  rp.dst = dp.out;
  rp.B = h->d_Q + (size_t)KP * KP;
  rp.Bf = h->d_Qf + (size_t)KP * KP;
  rp.items = base;
  rp.dmax = nullptr;
  rp.zbound = nullptr;
  rp.n_rows = cr.n_dual();
  rp.k = k;
  rp.src_stride = k;
  rp.dst_stride = k;
  rp.dst_cols = k;
  if (int rc = begin_timed(h, 5, (double)cr.n_dual() * 8.0 * k, pe)) return rc;
  if (h->rotate_split) {
    if (int rc = launch_rotate_split<true>(h, rotate_split_params(rp, h->d_Bs + h->Bs_stride, dp.xbound, 0.f))) return rc;
  } else if (int rc = launch_rotate<true, false>(h, rp)) {
    return rc;
  }
  return end_timed(h, pe);
}

int ensure_gramian_buffers(mals_handle h, SideState& s) {
  const int k = h->cfg.features;
  if (!s.G) HIPCHK(h, s.G.alloc((size_t)k * k));
  if (!s.Gf) HIPCHK(h, s.Gf.alloc((size_t)tri(h->T) * 256));
  if (!s.d_ymax) HIPCHK(h, s.d_ymax.alloc(YMAX_SLOTS));
  return MALS_OK;
}

}  // namespace

// ================================================================================================
extern "C" {

int mals_abi_version(void) { return MALS_ABI_VERSION; }

int mals_default_config(mals_config* cfg) {
  if (!cfg) return MALS_INVALID_ARG;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->struct_size = (int32_t)sizeof(mals_config);
  cfg->features = 30;   // MatrixFactorizer.java:34 DEFAULT_FEATURES
  cfg->alpha = 1.0;     // ALS:71
  cfg->lambda = 0.1;    // ALS:73
  cfg->singularity_threshold = 1.0e-5;
  cfg->flags = 0;
  cfg->device = 0;
  cfg->segment_nnz = 0;
  cfg->chunk_rows = 0;
  cfg->gramian_mode = MALS_GRAMIAN_AUTO;
  cfg->solve_mode = MALS_SOLVE_AUTO;
  return MALS_OK;
}

static thread_local std::string t_create_error;
void malsi_set_create_error(const char* text) { t_create_error = text ? text : ""; }
static int create_fail(int code, const std::string& msg) {
  t_create_error = msg;
  return code;
}
int mals_create_error(char* buf, size_t cap) {
  if (buf && cap > 0) {
    const size_t n = std::min(cap - 1, t_create_error.size());
    std::memcpy(buf, t_create_error.data(), n);
    buf[n] = 0;
  }
  return (int)t_create_error.size();
}
int mals_group_create_error(char* buf, size_t cap) { return mals_create_error(buf, cap); }

int mals_create(const mals_config* cfg, mals_handle* out) {
  if (!cfg || !out) return create_fail(MALS_INVALID_ARG, "mals_create: null config or output pointer");
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(mals_config))
    return create_fail(MALS_INVALID_ARG, "mals_create: mals_config.struct_size " + std::to_string(cfg->struct_size) + " is not this library's " +
                                             std::to_string(sizeof(mals_config)) + " (mals_default_config fills it)");
  if (cfg->features <= 0 || cfg->features > 128)   // ALS:139
    return create_fail(MALS_INVALID_ARG, "mals_create: features must be in 1..128, got " + std::to_string(cfg->features));
  if (!(cfg->lambda >= 0.0) || !std::isfinite(cfg->alpha)) return create_fail(MALS_INVALID_ARG, "mals_create: lambda must be >= 0 and alpha finite");
  int n_dev = 0;
  {
    const hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0) {
      (void)hipGetLastError();
      return create_fail(MALS_HIP_ERROR, std::string("mals_create: no HIP device (hipGetDeviceCount: ") + hipGetErrorString(e) +
                                             "); a GPU is required, there is no CPU fallback");
    }
  }
  if (cfg->device < 0 || cfg->device >= n_dev)
    return create_fail(MALS_HIP_ERROR, "mals_create: device ordinal " + std::to_string(cfg->device) + " outside 0.." + std::to_string(n_dev - 1));
  std::unique_ptr<mals_handle_s> owner(new (std::nothrow) mals_handle_s());   // an error return below destroys what was built
  const mals_handle h = owner.get();
  if (!h) return create_fail(MALS_OOM, "mals_create: out of host memory");
  h->cfg = *cfg;
  h->cfg.flags &= 3;
#ifdef MALS_PROFILING
  if (const char* dbg = std::getenv("MALS_DEBUG_FLAGS")) h->cfg.flags |= (std::atoi(dbg) & 0xff) << 8;  // ablations
#endif
  if (h->cfg.segment_nnz <= 0) h->cfg.segment_nnz = 4096;
  if (h->cfg.chunk_rows < 0) h->cfg.chunk_rows = 0;
  h->cfg.segment_nnz = (h->cfg.segment_nnz + 3) & ~3;
  h->T = (cfg->features + 15) / 16;
  switch (cfg->gramian_mode) {
    case MALS_GRAMIAN_AUTO: h->split_f16 = h->T >= 2; break;  // k <= 16: one tile, the fp32 products are not the bottleneck (k = 30: split is 8 % faster, measured)
    case MALS_GRAMIAN_FP32: h->split_f16 = false; break;
    case MALS_GRAMIAN_SPLIT_F16: h->split_f16 = true; break;
    case MALS_GRAMIAN_SPLIT3_F16:
      if (h->T != 4) return create_fail(MALS_INVALID_ARG, "mals_create: MALS_GRAMIAN_SPLIT3_F16 is built for 49..64 features");
      h->split_f16 = h->split3 = true;
      break;
    default: return create_fail(MALS_INVALID_ARG, "mals_create: unknown gramian_mode");
  }
  // a negative alpha (accepted by the reference, ALS:506-509) has no real sqrt(alpha |r|): fp32 gather
  if (cfg->alpha < 0.0) h->split_f16 = false;
  switch (cfg->solve_mode) {
    case MALS_SOLVE_AUTO: h->dual_blocks = h->T >= 3 ? dual_max_blocks(h->T) : 0; break;
    case MALS_SOLVE_DIRECT: h->dual_blocks = 0; break;
    case MALS_SOLVE_DUAL: h->dual_blocks = dual_max_blocks(h->T); break;
    default: return create_fail(MALS_INVALID_ARG, "mals_create: unknown solve_mode");
  }
  if (h->cfg.flags != 0 || !(cfg->alpha > 0.0)) h->dual_blocks = 0;  // the dual path covers the default mode only
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0)
      h->n_cu = prop.multiProcessorCount;
  }
  std::memset(&h->stats, 0, sizeof(h->stats));
  h->stats.struct_size = (int32_t)sizeof(mals_stats);
  hipError_t st = hipSetDevice(cfg->device);
  if (st == hipSuccess) st = h->d_bad.alloc(4);
  if (st == hipSuccess) st = h->h_bad.alloc(4);
  if (st == hipSuccess) st = h->d_zscale.alloc(4);
  if (st == hipSuccess) st = h->d_maxabs.alloc(4);
  if (st == hipSuccess) st = h->d_colrange.alloc(2);
  if (st == hipSuccess) st = h->d_refined.alloc(1);
  if (st == hipSuccess) st = h->d_gref_state.alloc(4);
  if (st == hipSuccess) st = hipMemset(h->d_gref_state.get(), 0, 4 * sizeof(int));
  if (st == hipSuccess) st = hipMemset(h->d_refined.get(), 0, sizeof(unsigned long long));
  if (st == hipSuccess) st = hipMemset(h->d_zscale.get(), 0, 4 * sizeof(float));   // (mals_get_gather_scale before any split-precision gather: zeros)
  if (st == hipSuccess) st = hipMemset(h->d_bad.get(), 0xff, 4 * sizeof(unsigned long long));
  if (st != hipSuccess) return create_fail(MALS_HIP_ERROR, "mals_create: device " + std::to_string(cfg->device) + ": " + hipGetErrorString(st));
  if (const char* e = std::getenv("MALS_REFINE_LIMIT")) h->refine_limit = std::max(0.f, (float)std::atof(e));
  if (h->ev_ready.ensure(hipEventDisableTiming) != hipSuccess || h->ev_refine.ensure(hipEventDisableTiming) != hipSuccess)
    return create_fail(MALS_HIP_ERROR, "mals_create: creating the handle's events failed");
  h->lds_gather = h->cfg.features == 128;   // the LDS-staged rows / segments kernels (lds_kernels.h); MALS_LDS_GATHER=0: A/B against the register-staged ones
  if (const char* e = std::getenv("MALS_LDS_GATHER")) h->lds_gather = h->lds_gather && std::atoi(e) != 0;
  if (const char* e = std::getenv("MALS_OVERLAP")) h->overlap = std::atoi(e) != 0;
  if (h->overlap) {
    bool ok = h->ev_fork.ensure(hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2 && ok; ++i) ok = h->aux[i].ensure() == hipSuccess && h->ev_join[i].ensure(hipEventDisableTiming) == hipSuccess;
    if (!ok) h->overlap = false;
  }
#ifdef MALS_PROFILING
  if (std::getenv("MALS_DEBUG_TRACE")) {
    (void)h->d_trace.alloc(64 * 64 * 6);
    (void)hipMemset(h->d_trace.get(), 0, 64 * 64 * 6 * sizeof(unsigned long long));
  }
#endif
  t_create_error.clear();
  malsi_serving_create(h);
  *out = owner.release();
  return MALS_OK;
}

int mals_destroy(mals_handle h) {
  if (!h) return MALS_INVALID_ARG;
  (void)hipSetDevice(h->cfg.device);
  malsi_serving_stop_front(h);
  (void)hipStreamSynchronize(h->stream);
  for (const Stream& a : h->aux)
    if (a) (void)hipStreamSynchronize(a);
  if (h->d_trace) {  // dump the last launch's per-phase cycle stamps (profiling aid)
    std::vector<unsigned long long> t(64 * 64 * 6);
    (void)hipMemcpy(t.data(), h->d_trace.get(), t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    for (int r = 0; r < 64; r += 21)
      for (int w = 0; w < 4; w += 1) {
        const unsigned long long* o = &t[(size_t)(r * 64 + w) * 6];
        std::fprintf(stderr, "[trace] iter %2d wave %2d len %5llu gather %7llu chol %7llu solve+store %7llu gap_to_prev_end %lld\n", r, w, o[4],
                     o[1] - o[0], o[2] - o[1], o[3] - o[2], r ? (long long)(o[0] - t[(size_t)((r - 1) * 64 + w) * 6 + 3]) : 0ll);
      }
    for (int w = 0; w < 4; ++w) {  // shader clock: s_memtime ticks per 100 MHz wall tick over 63 traced rows
      const unsigned long long* a = &t[(size_t)w * 6];
      const unsigned long long* b = &t[(size_t)(63 * 64 + w) * 6];
      if (b[5] > a[5]) std::fprintf(stderr, "[trace] wave %d: %llu cycles in %llu wall ticks (100 MHz) = %.0f MHz; %.0f cycles per row\n", w, b[3] - a[3], b[5] - a[5], 100.0 * (double)(b[3] - a[3]) / (double)(b[5] - a[5]), (double)(b[3] - a[3]) / 63.0);
    }
  }
  malsi_serving_free(h);
  delete h;   // every buffer, event and stream the handle owns, with its device current
  return MALS_OK;
}

int mals_features(mals_handle h) { return h ? h->cfg.features : 0; }

const char* mals_last_error(mals_handle h) { return h ? h->err.c_str() : "null handle"; }

int mals_set_stream(mals_handle h, void* hip_stream) {
  if (!h) return MALS_INVALID_ARG;
  h->stream = (hipStream_t)hip_stream;
  return MALS_OK;
}

int mals_set_factor_rows(mals_handle h, int side, int64_t n_rows_total) {
  CHECK_SIDE(h, side);
  if (n_rows_total <= 0) return fail(h, MALS_INVALID_ARG, "n_rows_total must be positive");
  if (int rc = use_device(h)) return rc;
  SideState& s = h->side[side];
  s.F = nullptr;
  const size_t n = (size_t)n_rows_total * (size_t)h->cfg.features;
  HIPCHK(h, s.F_own.alloc(n));
  s.F = s.F_own.get();
  HIPCHK(h, hipMemsetAsync(s.F, 0, sizeof(float) * n, h->stream));
  s.n_total = n_rows_total;
  s.G_valid = false;
  ++s.F_epoch;
  if (side == MALS_SIDE_X) h->grown_users_end.store(-1);   // a new replica: no grown users
  malsi_generation_drop_recent(h, side);                         // ... and no rows written since the last load
  malsi_ids_drop(h, side);                                       // ... and no ids: the rows are not the ones they named
  if (side == MALS_SIDE_X) popular_touch(h, false);
  if (side == MALS_SIDE_Y) h->lsh.clear();                 // ... and its rows are not the ones the candidate filter signed
  return MALS_OK;
}

int mals_bind_factors(mals_handle h, int side, float* device_ptr, int64_t n_rows_total) {
  CHECK_SIDE(h, side);
  if (!device_ptr || n_rows_total <= 0) return fail(h, MALS_INVALID_ARG, "null buffer or non-positive row count");
  if (int rc = use_device(h)) return rc;
  SideState& s = h->side[side];
  s.F_own.reset();
  s.F = device_ptr;
  s.n_total = n_rows_total;
  s.G_valid = false;
  ++s.F_epoch;
  if (side == MALS_SIDE_X) h->grown_users_end.store(-1);   // a new replica: no grown users
  malsi_generation_drop_recent(h, side);                         // ... and no rows written since the last load
  malsi_ids_drop(h, side);                                       // ... and no ids: the rows are not the ones they named
  if (side == MALS_SIDE_X) popular_touch(h, false);
  if (side == MALS_SIDE_Y) h->lsh.clear();
  return MALS_OK;
}

int mals_factor_device_ptr(mals_handle h, int side, void** out_device_ptr, int64_t* out_n_rows_total) {
  CHECK_SIDE(h, side);
  if (out_device_ptr) *out_device_ptr = h->side[side].F;
  if (out_n_rows_total) *out_n_rows_total = h->side[side].n_total;
  return h->side[side].F ? MALS_OK : fail(h, MALS_INVALID_ARG, "factor replica not allocated");
}

int mals_set_matrix(mals_handle h, int side, int64_t row_offset, int64_t n_rows_local, int64_t nnz, const int64_t* row_ptr,
                    const int32_t* col_idx, const float* val, int mem_kind) {
  CHECK_SIDE(h, side);
  if (row_offset < 0 || n_rows_local < 0 || nnz < 0 || !row_ptr || (nnz > 0 && (!col_idx || !val)))
    return fail(h, MALS_INVALID_ARG, "bad matrix arguments");
  if (n_rows_local > std::numeric_limits<int32_t>::max())
    return fail(h, MALS_INVALID_ARG, "at most 2^31-1 local rows per handle");
  if (int rc = use_device(h)) return rc;
  SideState& s = h->side[side];
  HIPCHK(h, hipStreamSynchronize(h->stream));
  free_matrix(s);
  if (side == MALS_SIDE_X) malsi_clear_known_items(h);  // they were a CSR over the OLD local rows (and maybe borrowed arrays)
  if (side == MALS_SIDE_X) malsi_popular_new_generation(h, true);   // ... and the tag users named the old rows
  s.row_offset = row_offset;
  s.n_local = n_rows_local;
  s.nnz = nnz;
  s.h_row_ptr.resize((size_t)n_rows_local + 1);
  if (mem_kind == MALS_MEM_DEVICE) {
    HIPCHK(h, hipMemcpy(s.h_row_ptr.data(), row_ptr, sizeof(int64_t) * (size_t)(n_rows_local + 1), hipMemcpyDeviceToHost));
    s.row_ptr = const_cast<int64_t*>(row_ptr);
    s.col = const_cast<int32_t*>(col_idx);
    s.val = const_cast<float*>(val);
  } else if (mem_kind == MALS_MEM_HOST) {
    std::memcpy(s.h_row_ptr.data(), row_ptr, sizeof(int64_t) * (size_t)(n_rows_local + 1));
    if (int rc = alloc_matrix(h, s)) return rc;
    HIPCHK(h, hipMemcpy(s.row_ptr, row_ptr, sizeof(int64_t) * (size_t)(n_rows_local + 1), hipMemcpyHostToDevice));
    if (nnz) {
      HIPCHK(h, hipMemcpy(s.col, col_idx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
      HIPCHK(h, hipMemcpy(s.val, val, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice));
    }
  } else {
    return fail(h, MALS_INVALID_ARG, "mem_kind must be MALS_MEM_HOST or MALS_MEM_DEVICE");
  }
  if (int rc = validate_matrix(h, side)) {
    free_matrix(s);
    return rc;
  }
  if (int rc = build_work_lists(h, s)) {
    free_matrix(s);
    return rc;
  }
  if (int rc = validate_columns(h, side)) {
    free_matrix(s);
    return rc;
  }
  s.has_matrix = true;
  return MALS_OK;
}

int mals_begin_matrix(mals_handle h, int side, int64_t row_offset, int64_t n_rows_local, int64_t nnz) {
  CHECK_SIDE(h, side);
  if (row_offset < 0 || n_rows_local < 0 || nnz < 0) return fail(h, MALS_INVALID_ARG, "bad matrix arguments");
  if (n_rows_local > std::numeric_limits<int32_t>::max())
    return fail(h, MALS_INVALID_ARG, "at most 2^31-1 local rows per handle");
  if (int rc = use_device(h)) return rc;
  SideState& s = h->side[side];
  HIPCHK(h, hipStreamSynchronize(h->stream));
  free_matrix(s);
  if (side == MALS_SIDE_X) malsi_clear_known_items(h);
  if (side == MALS_SIDE_X) malsi_popular_new_generation(h, true);
  s.row_offset = row_offset;
  s.n_local = n_rows_local;
  s.nnz = nnz;
  s.h_row_ptr.assign((size_t)n_rows_local + 1, 0);
  if (int rc = alloc_matrix(h, s)) return rc;
  s.append_rows = 0;
  s.append_nnz = 0;
  s.appending = true;
  return MALS_OK;
}

int mals_append_rows(mals_handle h, int side, int64_t n_rows, const int64_t* row_ptr_chunk, const int32_t* col_idx,
                     const float* val) {
  CHECK_SIDE(h, side);
  SideState& s = h->side[side];
  if (!s.appending) return fail(h, MALS_INVALID_ARG, "mals_append_rows without mals_begin_matrix");
  if (n_rows < 0 || !row_ptr_chunk || row_ptr_chunk[0] != 0) return fail(h, MALS_INVALID_ARG, "bad chunk");
  const int64_t cn = row_ptr_chunk[n_rows];
  if (s.append_rows + n_rows > s.n_local || s.append_nnz + cn > s.nnz || (cn > 0 && (!col_idx || !val)))
    return fail(h, MALS_INVALID_ARG, "chunk exceeds the declared matrix size");
  if (int rc = use_device(h)) return rc;
  for (int64_t r = 0; r < n_rows; ++r) {
    if (row_ptr_chunk[r + 1] < row_ptr_chunk[r]) return fail(h, MALS_INVALID_ARG, "row_ptr must be non-decreasing");
    s.h_row_ptr[(size_t)(s.append_rows + r + 1)] = s.append_nnz + row_ptr_chunk[r + 1];
  }
  if (cn) {
    HIPCHK(h, hipMemcpy(s.col + s.append_nnz, col_idx, sizeof(int32_t) * (size_t)cn, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(s.val + s.append_nnz, val, sizeof(float) * (size_t)cn, hipMemcpyHostToDevice));
  }
  s.append_rows += n_rows;
  s.append_nnz += cn;
  return MALS_OK;
}

int mals_end_matrix(mals_handle h, int side) {
  CHECK_SIDE(h, side);
  SideState& s = h->side[side];
  if (!s.appending) return fail(h, MALS_INVALID_ARG, "mals_end_matrix without mals_begin_matrix");
  s.appending = false;
  if (s.append_rows != s.n_local || s.append_nnz != s.nnz) {
    free_matrix(s);
    return fail(h, MALS_INVALID_ARG, "appended rows/entries do not match the declared matrix size");
  }
  if (int rc = use_device(h)) return rc;
  HIPCHK(h, hipMemcpy(s.row_ptr, s.h_row_ptr.data(), sizeof(int64_t) * (size_t)(s.n_local + 1), hipMemcpyHostToDevice));
  if (int rc = build_work_lists(h, s)) {
    free_matrix(s);
    return rc;
  }
  if (int rc = validate_columns(h, side)) {
    free_matrix(s);
    return rc;
  }
  s.has_matrix = true;
  if (side == MALS_SIDE_X) popular_touch(h, true);   // the rows of R are there now
  return MALS_OK;
}

int mals_get_value_bound(mals_handle h, int side, float* max_abs_value) {
  CHECK_SIDE(h, side);
  if (!h->side[side].has_matrix || !max_abs_value) return fail(h, MALS_INVALID_ARG, "matrix of this side not set");
  *max_abs_value = h->side[side].max_abs_val;
  return MALS_OK;
}

int mals_set_value_bound(mals_handle h, int side, float max_abs_value) {
  CHECK_SIDE(h, side);
  SideState& s = h->side[side];
  if (!s.has_matrix) return fail(h, MALS_INVALID_ARG, "matrix of this side not set");
  if (!(max_abs_value >= s.local_max_abs_val)) return fail(h, MALS_INVALID_ARG, "bound below the largest local |value|");
  s.max_abs_val = max_abs_value;
  return MALS_OK;
}

int mals_get_value_stats(mals_handle h, int side, float* max_abs_value, double* sum_abs_value, int64_t* n_values) {
  CHECK_SIDE(h, side);
  const SideState& s = h->side[side];
  if (!s.has_matrix) return fail(h, MALS_INVALID_ARG, "matrix of this side not set");
  if (max_abs_value) *max_abs_value = s.local_max_abs_val;
  if (sum_abs_value) *sum_abs_value = s.local_mean_abs_val * (double)s.nnz;
  if (n_values) *n_values = s.nnz;
  return MALS_OK;
}

int mals_set_value_stats(mals_handle h, int side, float max_abs_value, double mean_abs_value) {
  CHECK_SIDE(h, side);
  if (!(mean_abs_value >= 0.0) || !std::isfinite(mean_abs_value)) return fail(h, MALS_INVALID_ARG, "mean |value| must be finite and >= 0");
  if (int rc = mals_set_value_bound(h, side, max_abs_value)) return rc;
  h->side[side].mean_abs_val = mean_abs_value;
  return MALS_OK;
}

int mals_set_factors(mals_handle h, int side, int64_t row_begin, int64_t n_rows, const float* host_rows) {
  CHECK_SIDE(h, side);
  SideState& s = h->side[side];
  if (!s.F) return fail(h, MALS_INVALID_ARG, "factor replica not allocated");
  if (row_begin < 0 || n_rows < 0 || row_begin + n_rows > s.n_total || !host_rows)
    return fail(h, MALS_INVALID_ARG, "row range outside the factor replica");
  if (int rc = use_device(h)) return rc;
  const int k = h->cfg.features;
  HIPCHK(h, hipMemcpyAsync(s.F + row_begin * k, host_rows, sizeof(float) * (size_t)n_rows * k, hipMemcpyHostToDevice,
                           h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  s.G_valid = false;
  ++s.F_epoch;
  return MALS_OK;
}

int mals_get_factors(mals_handle h, int side, int64_t row_begin, int64_t n_rows, float* host_out) {
  CHECK_SIDE(h, side);
  SideState& s = h->side[side];
  if (!s.F) return fail(h, MALS_INVALID_ARG, "factor replica not allocated");
  if (row_begin < 0 || n_rows < 0 || row_begin + n_rows > s.n_total || !host_out)
    return fail(h, MALS_INVALID_ARG, "row range outside the factor replica");
  if (int rc = use_device(h)) return rc;
  const int k = h->cfg.features;
  HIPCHK(h, hipMemcpyAsync(host_out, s.F + row_begin * k, sizeof(float) * (size_t)n_rows * k, hipMemcpyDeviceToHost,
                           h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MALS_OK;
}

int mals_get_rows(mals_handle h, int side, const int64_t* row_idx, int32_t n, float* host_out) {
  CHECK_SIDE(h, side);
  SideState& s = h->side[side];
  if (!s.F) return fail(h, MALS_INVALID_ARG, "factor replica not allocated");
  if (n < 0 || (n > 0 && (!row_idx || !host_out))) return fail(h, MALS_INVALID_ARG, "bad row list");
  if (n == 0) return MALS_OK;
  for (int i = 0; i < n; ++i)
    if (row_idx[i] < 0 || row_idx[i] >= s.n_total) return fail(h, MALS_INVALID_ARG, "row index outside the factor replica");
  if (int rc = use_device(h)) return rc;
  const int k = h->cfg.features;
  if (h->d_idx.capacity() < (size_t)n || h->d_rows.capacity() < (size_t)n * k) {
    h->d_idx.reset();
    h->d_rows.reset();
    HIPCHK(h, h->d_idx.alloc((size_t)n));
    HIPCHK(h, h->d_rows.alloc((size_t)n * k));
  }
  HIPCHK(h, hipMemcpyAsync(h->d_idx.get(), row_idx, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, h->stream, s.F, h->d_idx.get(), n, k,
                     h->d_rows.get());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(host_out, h->d_rows.get(), sizeof(float) * (size_t)n * k, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MALS_OK;
}

int mals_gramian(mals_handle h, int side, double* host_G) {
  CHECK_SIDE(h, side);
  SideState& s = h->side[side];
  if (!s.F) return fail(h, MALS_INVALID_ARG, "factor replica not allocated");  // MU:220-222 null/empty M
  if (int rc = use_device(h)) return rc;
  if (int rc = ensure_gramian_buffers(h, s)) return rc;
  PendingEvent pe;
  // only the split-f16 kernel (large matrices) records the maximum; below its threshold not even the two memsets are
  // spent (C2 is 50 launches of a few microseconds each)
  const bool with_max = s.n_total >= GRAMIAN_SPLIT_MIN_ROWS;
  if (with_max) HIPCHK(h, hipMemsetAsync(s.d_ymax.get(), 0, sizeof(unsigned) * YMAX_SLOTS, h->stream));
  if (int rc = begin_timed(h, 3, (double)s.n_total * 4.0 * h->cfg.features, pe)) return rc;
  if (int rc = launch_gramian(h, s, s.F, s.n_total, s.G.get(), s.Gf.get(), with_max ? s.d_ymax.get() : nullptr)) return rc;
  if (int rc = end_timed(h, pe)) return rc;
  s.G_valid = true;
  ++s.G_version;
  s.ymax_version = with_max ? s.G_version : 0;   // every element of the replica went through the kernel: its maximum is exact
  if (host_G) {
    const int k = h->cfg.features;
    HIPCHK(h, hipMemcpyAsync(host_G, s.G.get(), sizeof(double) * (size_t)k * k, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return MALS_OK;
}

int malsi_gramian_partial(mals_handle h, int side, int64_t row_begin, int64_t n_rows, double* device_out, unsigned* device_max) {
  CHECK_SIDE(h, side);
  SideState& s = h->side[side];
  if (!s.F) return fail(h, MALS_INVALID_ARG, "factor replica not allocated");
  if (row_begin < 0 || n_rows <= 0 || row_begin + n_rows > s.n_total || !device_out)
    return fail(h, MALS_INVALID_ARG, "row range outside the factor replica");
  if (int rc = use_device(h)) return rc;
  PendingEvent pe;
  if (int rc = begin_timed(h, 3, (double)n_rows * 4.0 * h->cfg.features, pe)) return rc;
  if (int rc = launch_gramian(h, s, s.F + row_begin * h->cfg.features, n_rows, device_out, nullptr, device_max)) return rc;
  return end_timed(h, pe);
}

int mals_gramian_partial(mals_handle h, int side, int64_t row_begin, int64_t n_rows, double* device_out) {
  return malsi_gramian_partial(h, side, row_begin, n_rows, device_out, nullptr);
}

// device_max: YMAX_SLOTS device words (malsi_ymax_slots()) whose maximum is the bit pattern of max |element| over ALL rows the installed G was formed from (the
// group's all-reduced maximum of the members' malsi_gramian_partial maxima), or NULL when the caller has none
int malsi_set_gramian(mals_handle h, int side, const double* G, int mem_kind, const unsigned* device_max) {
  CHECK_SIDE(h, side);
  if (!G) return fail(h, MALS_INVALID_ARG, "null Gramian");
  SideState& s = h->side[side];
  if (int rc = use_device(h)) return rc;
  if (int rc = ensure_gramian_buffers(h, s)) return rc;
  const int k = h->cfg.features;
  HIPCHK(h, hipMemcpyAsync(s.G.get(), G, sizeof(double) * (size_t)k * k,
                           mem_kind == MALS_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(gramian_pack_kernel, dim3((unsigned)tri(h->T)), dim3(256), 0, h->stream, s.G.get(), k, h->T, s.Gf.get());
  HIPCHK(h, hipGetLastError());
  if (device_max) HIPCHK(h, hipMemcpyAsync(s.d_ymax.get(), device_max, sizeof(unsigned) * YMAX_SLOTS, hipMemcpyDeviceToDevice, h->stream));
  if (mem_kind != MALS_MEM_DEVICE) HIPCHK(h, hipStreamSynchronize(h->stream));
  s.G_valid = true;
  ++s.G_version;
  s.ymax_version = device_max ? s.G_version : 0;
  return MALS_OK;
}

int mals_set_gramian(mals_handle h, int side, const double* G, int mem_kind) { return malsi_set_gramian(h, side, G, mem_kind, nullptr); }

// fork: the side streams start behind everything enqueued on the main stream so far; join: the main stream continues
// behind whatever was put on them.  A scope swaps h->stream so that every launch helper (and its timing events) lands
// on the side stream.
struct SideStream {
  mals_handle h;
  hipStream_t saved;
  SideStream(mals_handle hh, int i) : h(hh), saved(hh->stream) {
    if (h->overlap && h->forked[i]) h->stream = h->aux[i];
  }
  ~SideStream() { h->stream = saved; }
};
static int fork_streams(mals_handle h) {
  if (!h->overlap) return MALS_OK;
  HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
  for (int i = 0; i < 2; ++i) {
    HIPCHK(h, hipStreamWaitEvent(h->aux[i], h->ev_fork, 0));
    h->forked[i] = true;
  }
  return MALS_OK;
}
static int join_streams(mals_handle h) {
  if (!h->overlap) return MALS_OK;
  for (int i = 0; i < 2; ++i) {
    if (!h->forked[i]) continue;
    HIPCHK(h, hipEventRecord(h->ev_join[i], h->aux[i]));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join[i], 0));
    h->forked[i] = false;
  }
  return MALS_OK;
}

// phase: the whole of every chunk (ALL); or, for callers that drive several handles from one thread (mals_group.cpp),
// one chunk in two calls -- BEGIN enqueues everything that does not need the eigendecomposition of the dual path and
// returns (h->dual_pending says whether anything is left), the caller provides the decomposition (prepare_dual_host,
// once per group), END enqueues the rest.  BEGIN + host + END = ALL.
enum { SOLVE_ALL = 0, SOLVE_BEGIN = 1, SOLVE_END = 2 };

// ---- solve_chunks in steps: argument checks, the once-per-half-iteration setup, the parameter block, one chunk, the
// chunk's refinement block; the driver behind them

static int solve_check_args(mals_handle h, int side, int chunk_begin, int chunk_end) {
  const SideState& s = h->side[side];
  const SideState& o = h->side[1 - side];
  if (!s.has_matrix) return fail(h, MALS_INVALID_ARG, "matrix of this side not set");
  if (!s.F || !o.F) return fail(h, MALS_INVALID_ARG, "factor replicas not allocated");
  if (s.row_offset + s.n_local > s.n_total) return fail(h, MALS_INVALID_ARG, "matrix rows exceed the factor replica");
  if (int rc = validate_columns(h, side)) return rc;
  // the split-precision gather takes its scale from the Gramian's diagonal even when W does not start from G
  const bool use_g = !(h->cfg.flags & MALS_FLAG_LOSS_IGNORES_UNSPECIFIED) || h->split_f16;
  if (use_g && !o.G_valid) return fail(h, MALS_INVALID_ARG, "Gramian of the opposite side not computed");
  if (chunk_begin < 0 || chunk_end > (int)s.chunks.size() || chunk_begin >= chunk_end)
    return fail(h, MALS_INVALID_ARG, "chunk index out of range");
  return MALS_OK;
}

// dual path (dual_kernels.h): the reference's default mode only
// ... and only when it pays: the rotation of the gathered matrix costs ~1/30 of what a dual row saves
// (measured, k = 64 and 128), so a side with few short rows against a huge opposite matrix (the item half of
// C5: 1.25M long rows per rank gathering from 100M users) stays on the direct kernels
static bool dual_wanted(mals_handle h, const SideState& s, const SideState& o) {
  const bool dual_pays = h->cfg.solve_mode == MALS_SOLVE_DUAL || s.n_dual_rows * 32 >= o.n_total;
  return s.n_dual_rows > 0 && dual_pays && h->cfg.flags == 0 && h->cfg.alpha > 0.0 && o.G_valid;
}

// What a half-iteration sets up once, enqueued by the first call that solves one of its chunks: the padded gather table,
// the permuted Gramian image, the refinement marks' block, the operand scale and -- g_to_host -- the copy of G that the
// dual path's eigendecomposition reads.  Marks the call's chunks as solved from this setup.
static int solve_setup(mals_handle h, int side, int chunk_begin, int chunk_end, bool g_to_host) {
  SideState& s = h->side[side];
  SideState& o = h->side[1 - side];
  const int k = h->cfg.features;
  // A new half-iteration?  The opposite factors do not change while a half-iteration's chunks are solved (in any
  // order): "new" = the side, the opposite Gramian or the opposite uploads changed, or a chunk comes round again.
  const HalfStamp now{side, o.G_version};
  bool new_half = h->pad != now || h->pad_epoch != o.F_epoch || h->pad_done.size() != s.chunks.size();
  for (int c = chunk_begin; c < chunk_end && !new_half; ++c) new_half = h->pad_done[(size_t)c] != 0;
  if (new_half) {
    h->pad = now;
    h->pad_epoch = o.F_epoch;
    h->pad_done.assign(s.chunks.size(), 0);
    h->tl[0] = now_us();
    h->tl[1] = h->tl[2] = 0.0;
    // nothing marked yet, no reference-rounded Gramian yet, no arrival counted (gramian_ref_kernel)
    HIPCHK(h, hipMemsetAsync(h->d_gref_state.get(), 0, 3 * sizeof(int), h->stream));
  }
  for (int c = chunk_begin; c < chunk_end; ++c) h->pad_done[(size_t)c] = 1;
  if (k % 16 != 0) {
    const int ld = 16 * h->T;
    const size_t need = (size_t)o.n_total * (size_t)ld;
    if (need > h->d_Mp.capacity()) {
      new_half = true;   // the copy is gone
      HIPCHK(h, h->d_Mp.reserve(need, h->stream));
    }
    if (new_half) {
      PendingEvent pe;
      if (int rc = begin_timed(h, 5, (double)o.n_total * 4.0 * (k + ld), pe)) return rc;
      const int64_t n4 = o.n_total * (ld / 4);
      const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, (int64_t)h->n_cu * 32);
      hipLaunchKernelGGL(pad_rows_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, h->stream, o.F, o.n_total, k, ld, h->d_Mp.get());
      HIPCHK(h, hipGetLastError());
      if (int rc = end_timed(h, pe)) return rc;
    }
  }
  if (h->lds_gather && h->split_f16 && k == 128) {
    if (!h->d_Gperm) HIPCHK(h, h->d_Gperm.alloc((size_t)tri(8) * 256));
    if (h->gperm != now) {
      if (h->cfg.flags & MALS_FLAG_LOSS_IGNORES_UNSPECIFIED) {  // W does not start from G (ALS:524-539): an image of zeros
        HIPCHK(h, hipMemsetAsync(h->d_Gperm.get(), 0, sizeof(float) * (size_t)tri(8) * 256, h->stream));
      } else {
        hipLaunchKernelGGL(gramian_perm_kernel, dim3((unsigned)tri(8)), dim3(256), 0, h->stream, o.G.get(), k, h->d_Gperm.get());
        HIPCHK(h, hipGetLastError());
      }
      h->gperm = now;
    }
  }
  HIPCHK(h, s.refine.reserve((size_t)s.n_local, h->stream));
  if (h->split_f16 && (h->zs != now || h->zs_bound != s.max_abs_val || h->zs_mean != s.mean_abs_val)) {
    // once per half-iteration, not per chunk: the scale only depends on G and on the value bound
    const double base_w = (h->cfg.flags & MALS_FLAG_LOSS_IGNORES_UNSPECIFIED) ? 1.0 : 0.0;
    const double w_max = base_w + ((h->cfg.flags & MALS_FLAG_RECONSTRUCT_R) ? 0.0 : std::fabs(h->cfg.alpha) * (double)s.max_abs_val);
    const double w_mean = base_w + ((h->cfg.flags & MALS_FLAG_RECONSTRUCT_R) ? 0.0 : std::fabs(h->cfg.alpha) * s.mean_abs_val);
    int force = -1;  // MALS_FORCE_RANGE_FLAG=0/1 (tests): override the range decision
    if (const char* e = std::getenv("MALS_FORCE_RANGE_FLAG")) force = std::atoi(e) != 0;
    hipLaunchKernelGGL(gather_scale_kernel, dim3(1), dim3(64), 0, h->stream, o.G.get(), k, (float)std::sqrt(w_max), (float)std::sqrt(w_mean),
                       (double)o.n_total, force, (o.ymax_version != 0 && o.ymax_version == o.G_version) ? o.d_ymax.get() : nullptr, h->d_zscale.get());
    HIPCHK(h, hipGetLastError());
    h->zs = now;
    h->zs_bound = s.max_abs_val;
    h->zs_mean = s.mean_abs_val;
  }
  if (g_to_host) {  // the Gramian goes to the host first so that its eigendecomposition runs while the direct kernels of
                    // the first chunk execute
    if (!h->h_G) HIPCHK(h, h->h_G.alloc((size_t)k * k));
    HIPCHK(h, h->ev_G.ensure(hipEventDisableTiming));
    HIPCHK(h, hipMemcpyAsync(h->h_G.get(), o.G.get(), sizeof(double) * (size_t)k * k, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_G, h->stream));
  }
  return MALS_OK;
}

// The parameter block of the side's direct kernels, from what solve_setup left (no device work); a launch adds its list.
static SolveParams solve_params(mals_handle h, int side) {
  SideState& s = h->side[side];
  SideState& o = h->side[1 - side];
  const int k = h->cfg.features;
  SolveParams p;
  p.row_ptr = s.row_ptr;
  p.col = s.col;
  p.val = s.val;
  p.M = o.F;
  p.ldm = k;
  if (k % 16 != 0) {
    p.M = h->d_Mp.get();
    p.ldm = 16 * h->T;
  }
  p.Gf = o.Gf.get();
  p.Gperm = h->lds_gather && h->split_f16 && k == 128 ? h->d_Gperm.get() : nullptr;
  p.out = s.F + s.row_offset * k;
  p.items = nullptr;
  p.rowsC = s.rowsC.get();
  p.scratch = s.scratch.get();
  p.bad_row = h->d_bad.get() + side;
  p.suspect = h->d_bad.get() + 2 + side;
  p.any_marked = h->d_gref_state.get();
  p.refine_flag = s.refine.get();
  // under lossIgnoresUnspecified W has no Gramian under it and every marked row goes to the fp64 restatement, which
  // also reproduces that mode's fp32-rounded products: the estimate is at its weakest there (measured 100x and more
  // below cond(W) for rows with about as many entries as features), so the bar is lower
  p.refine_limit = (h->cfg.flags & MALS_FLAG_LOSS_IGNORES_UNSPECIFIED) ? h->refine_limit / 16.f : h->refine_limit;
  p.gramian_weight = 0.25f;
  if (h->cfg.flags & MALS_FLAG_RECONSTRUCT_R) {   // no confidence weights: W = G + rho I (or the plain sum of y y^T)
    p.gramian_weight = 1.f;
    p.refine_limit *= 0.25f;
  }
  p.n_work = 0;
  p.trace = h->d_trace.get();
  p.trace_start = 0;
  if (const char* ts = std::getenv("MALS_DEBUG_TRACE")) p.trace_start = std::atoi(ts);
  if (const char* ts = std::getenv("MALS_DEBUG_TRACE_SIDE")) if (std::atoi(ts) != side) p.trace = nullptr;
  p.k = k;
  p.flags = h->cfg.flags;
  p.alpha = (float)h->cfg.alpha;
  p.lambda_alpha = (float)(h->cfg.lambda * h->cfg.alpha);  // ALS:435
  p.sing_threshold = (float)h->cfg.singularity_threshold;
  p.zscale = h->d_zscale.get();
  return p;
}

// One chunk's kernels, between the fork and the join of the side streams.  prepare_dual: the chunk is the first of a
// half-iteration whose dual path is still to be prepared -- its direct lists go first, the eigendecomposition of G runs
// on the host under them (SOLVE_BEGIN: returns there with h->dual_pending set, the caller provides it; SOLVE_END resumes
// behind it), then the device half of the preparation and the dual lists.  *dual_now: the chunk's dual lists ran on the
// dual path.
static int solve_one_chunk(mals_handle h, int side, const SolveParams& p, int c, int phase, bool want_dual, bool prepare_dual, bool* dual_now) {
  SideState& s = h->side[side];
  const SideState& o = h->side[1 - side];
  const ChunkRange& cr = s.chunks[(size_t)c];
  const bool resume = phase == SOLVE_END;
  if (!resume && p.refine_flag && cr.row1 > cr.row0)
    HIPCHK(h, hipMemsetAsync(s.refine.get() + cr.row0, 0, (size_t)(cr.row1 - cr.row0), h->stream));
  // (per chunk, not per call: once the first chunk of a multi-chunk call has prepared the dual path the later ones use it)
  const HalfStamp now{side, o.G_version};
  *dual_now = want_dual && h->dual_ok && h->dual == now;
  if (!resume)
    if (int rc = fork_streams(h)) return rc;
  if (prepare_dual) {
    if (!resume) {
      {
        SideStream long_rows(h, 0);
        if (int rc = launch_solve(h, s, p, c, LISTS_LONG)) return rc;
      }
      if (int rc = launch_solve(h, s, p, c, LISTS_ROWS)) return rc;   // direct lists first ...
      if (phase == SOLVE_BEGIN) {                                     // ... the caller decomposes G under them
        h->dual_pending = true;
        h->dual_pending_side = side;
        h->dual_pending_chunk = c;
        return MALS_OK;
      }
      if (int rc = prepare_dual_host(h, side, nullptr)) return rc;    // ... host eigendecomposition under them
    } else if (h->dual != now) {
      return fail(h, MALS_INVALID_ARG, "solve END without the eigendecomposition of this half-iteration");
    }
    h->dual_pending = false;
    {
      SideStream dual_rows(h, 1);
      if (int rc = prepare_dual_device(h, side)) return rc;
      HIPCHK(h, hipEventRecord(h->ev_ready, h->stream));   // (with MALS_OVERLAP: the side stream the rotation is on)
      *dual_now = h->dual_ok;
      if (*dual_now) {
        if (int rc = launch_dual_chunk(h, side, c)) return rc;
      } else if (cr.n_dual()) {  // does not qualify: the dual lists through the direct kernel after all
        if (int rc = launch_solve(h, s, p, c, LISTS_DUAL_ROWS)) return rc;
      }
    }
  } else {
    {
      SideStream long_rows(h, 0);
      if (int rc = launch_solve(h, s, p, c, LISTS_LONG)) return rc;
    }
    if (*dual_now && cr.n_dual()) {
      SideStream dual_rows(h, 1);
      if (int rc = launch_dual_chunk(h, side, c)) return rc;
    }
    if (int rc = launch_solve(h, s, p, c, *dual_now ? LISTS_ROWS : (LISTS_ROWS | LISTS_DUAL_ROWS))) return rc;
  }
  return join_streams(h);
}

// The chunk's refinement block, behind every kernel of the chunk (the un-rotation of the dual rows included): the rows
// the solving kernels marked, re-solved.
static int refine_chunk(mals_handle h, int side, const SolveParams& p, const ChunkRange& cr) {
  const SideState& o = h->side[1 - side];
  if (!p.refine_flag || cr.row1 <= cr.row0) return MALS_OK;
  if (h->refine_recorded) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_refine, 0));   // one chunk's block at a time
  if (!h->d_Gref) {   // before the parameter block below takes the pointers
    const size_t kp2 = (size_t)(16 * h->T) * (size_t)(16 * h->T);
    HIPCHK(h, h->d_Gref.alloc(kp2));
    HIPCHK(h, h->d_gref_part.alloc(kp2 * (size_t)h->n_cu * 2));
  }
  RefineParams q;
  q.p = p;
  q.G = o.G.get();
  q.Gref = h->d_Gref.get();
  q.gref_state = h->d_gref_state.get();
  q.n_refined = h->d_refined.get();
  q.row_begin = cr.row0;
  q.row_end = cr.row1;
  q.alpha = h->cfg.alpha;
  q.lambda_alpha = h->cfg.lambda * h->cfg.alpha;
  const bool no_gramian = h->cfg.flags & MALS_FLAG_LOSS_IGNORES_UNSPECIFIED;
  if (!no_gramian)   // something marked in this half-iteration: M^T M once more, rounded like the reference's
    if (int rc = launch_gramian_ref(h, o)) return rc;
  if (!no_gramian && h->refine_limit > 0.f)
    if (int rc = launch_refine(h, q)) return rc;      // marks 1; may raise a mark to 2
  if (int rc = launch_exact(h, q, no_gramian ? 1 : 2)) return rc;
  HIPCHK(h, hipEventRecord(h->ev_refine, h->stream));
  h->refine_recorded = true;
  return MALS_OK;
}

static int solve_chunks(mals_handle h, int side, int chunk_begin, int chunk_end, int phase = SOLVE_ALL) {
  if (int rc = solve_check_args(h, side, chunk_begin, chunk_end)) return rc;
  SideState& s = h->side[side];
  SideState& o = h->side[1 - side];
  const bool resume = phase == SOLVE_END;
  if (resume) {
    if (!h->dual_pending) return MALS_OK;  // BEGIN did the whole chunk
    if (h->dual_pending_side != side || h->dual_pending_chunk != chunk_begin || chunk_end != chunk_begin + 1)
      return fail(h, MALS_INVALID_ARG, "solve END does not match the pending BEGIN");
  } else {
    h->dual_pending = false;  // a BEGIN whose END never came belongs to a half-iteration that was abandoned on an error
  }
  if (int rc = use_device(h)) return rc;
  if (s.n_local == 0) return MALS_OK;
  const bool want_dual = dual_wanted(h, s, o);
  const bool dual_stale = resume || (want_dual && h->dual != HalfStamp{side, o.G_version});
  if (!resume)
    if (int rc = solve_setup(h, side, chunk_begin, chunk_end, dual_stale)) return rc;
  const SolveParams p = solve_params(h, side);
  if (phase == SOLVE_BEGIN && chunk_end != chunk_begin + 1) return fail(h, MALS_INVALID_ARG, "solve BEGIN takes one chunk");
  // everything a half-iteration sets up once is enqueued by now unless the dual preparation is still to come (solve_one_chunk)
  if (!resume && !(want_dual && dual_stale)) HIPCHK(h, hipEventRecord(h->ev_ready, h->stream));
  for (int c = chunk_begin; c < chunk_end; ++c) {
    const ChunkRange& cr = s.chunks[(size_t)c];
    bool dual_now = false;
    if (int rc = solve_one_chunk(h, side, p, c, phase, want_dual, want_dual && dual_stale && c == chunk_begin, &dual_now)) return rc;
    if (phase == SOLVE_BEGIN && h->dual_pending) return MALS_OK;   // the host's turn; END takes the chunk up again
    if (int rc = refine_chunk(h, side, p, cr)) return rc;
    h->stats.rows_solved += cr.nA + cr.nC + cr.n_dual() + cr.nZ;
    h->stats.nnz_gathered += cr.nnzA + cr.nnzB + cr.nnz_dual();
    if (dual_now) h->stats.rows_dual += cr.n_dual();
  }
  // this side's factors changed: its Gramian is stale.  (The OPPOSITE side's Gramian stays valid
  // for the remaining chunks of this half-iteration.)
  s.G_valid = false;
  ++s.F_epoch;
  return MALS_OK;
}

int mals_solve_side(mals_handle h, int side) {
  CHECK_SIDE(h, side);
  return solve_chunks(h, side, 0, (int)h->side[side].chunks.size());
}

int mals_solve_chunk(mals_handle h, int side, int32_t chunk) {
  CHECK_SIDE(h, side);
  return solve_chunks(h, side, chunk, chunk + 1);
}

// ---- csrc/mals_internal.h: the two-call form of mals_solve_chunk for mals_group.cpp (not part of the C-ABI)
int malsi_solve_chunk_begin(mals_handle h, int side, int32_t chunk) {
  CHECK_SIDE(h, side);
  return solve_chunks(h, side, chunk, chunk + 1, SOLVE_BEGIN);
}
int malsi_solve_chunk_end(mals_handle h, int side, int32_t chunk) {
  CHECK_SIDE(h, side);
  return solve_chunks(h, side, chunk, chunk + 1, SOLVE_END);
}
int malsi_dual_pending(mals_handle h) { return h && h->dual_pending ? 1 : 0; }
void* malsi_ready_event(mals_handle h) { return h ? (void*)h->ev_ready.get() : nullptr; }
int malsi_ymax_slots(void) { return YMAX_SLOTS; }
int malsi_dual_host(mals_handle h, int side, mals_handle from) {
  CHECK_SIDE(h, side);
  if (!h->dual_pending || h->dual_pending_side != side) return fail(h, MALS_INVALID_ARG, "no chunk is waiting for the eigendecomposition");
  if (int rc = use_device(h)) return rc;
  return prepare_dual_host(h, side, from);
}

int mals_get_gather_scale(mals_handle h, float* out4) {
  if (!h || !out4) return MALS_INVALID_ARG;
  if (int rc = use_device(h)) return rc;
  HIPCHK(h, hipMemcpyAsync(out4, h->d_zscale.get(), 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MALS_OK;
}

int mals_get_timeline(mals_handle h, double* out4) {
  if (!h || !out4) return MALS_INVALID_ARG;
  for (int i = 0; i < 4; ++i) out4[i] = h->tl[i];
  return MALS_OK;
}

int mals_set_chunk_rows(mals_handle h, int side, int64_t chunk_rows) {
  CHECK_SIDE(h, side);
  if (chunk_rows < 0) return fail(h, MALS_INVALID_ARG, "chunk_rows must be >= 0");
  h->side[side].chunk_rows_override = chunk_rows;
  return MALS_OK;
}

int mals_num_chunks(mals_handle h, int side, int32_t* n_chunks) {
  CHECK_SIDE(h, side);
  if (!h->side[side].has_matrix) return fail(h, MALS_INVALID_ARG, "matrix of this side not set");
  if (n_chunks) *n_chunks = (int32_t)h->side[side].chunks.size();
  return MALS_OK;
}

namespace {

// The reference's SingularMatrixSolverException carries RRQR's getRank(0.01) of the failing row's
// system (CMLSS:47).  Error path only: rebuild that one k x k system on the host in fp64 from the
// row's entries, the current opposite factors and their Gramian (ALS:450-492).  0 = unknown.
// the row's k x k system in fp64 (ALS:450-492); false = could not be rebuilt
bool build_row_system(mals_handle h, int side, int64_t local_row, std::vector<double>& W) {
  SideState& s = h->side[side];
  SideState& o = h->side[1 - side];
  const int k = h->cfg.features;
  if (!s.has_matrix || local_row < 0 || local_row >= s.n_local || !o.F) return false;
  const int64_t e0 = s.h_row_ptr[local_row], n_u = s.h_row_ptr[local_row + 1] - e0;
  std::vector<int32_t> col((size_t)n_u);
  std::vector<float> val((size_t)n_u);
  std::vector<int64_t> idx((size_t)n_u);
  std::vector<float> rows((size_t)n_u * k);
  W.assign((size_t)k * k, 0.0);
  if (n_u > 0) {
    if (n_u > (int64_t)INT32_MAX) return false;
    if (hipMemcpy(col.data(), s.col + e0, sizeof(int32_t) * (size_t)n_u, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (hipMemcpy(val.data(), s.val + e0, sizeof(float) * (size_t)n_u, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (int64_t e = 0; e < n_u; ++e) idx[e] = col[e];
    if (mals_get_rows(h, 1 - side, idx.data(), (int32_t)n_u, rows.data()) != MALS_OK) return false;
  }
  const bool reconstruct = h->cfg.flags & MALS_FLAG_RECONSTRUCT_R;
  if (!(h->cfg.flags & MALS_FLAG_LOSS_IGNORES_UNSPECIFIED)) {
    if (!o.G.get() || hipMemcpy(W.data(), o.G.get(), sizeof(double) * W.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
  }
  for (int64_t e = 0; e < n_u; ++e) {
    const float* y = rows.data() + (size_t)e * k;
    double w = 0.0;
    if (h->cfg.flags & MALS_FLAG_LOSS_IGNORES_UNSPECIFIED) w += 1.0;             // ALS:524-539
    if (!reconstruct) w += h->cfg.alpha * std::fabs((double)val[e]);             // ALS:471-477
    for (int r = 0; r < k; ++r)
      for (int c = 0; c < k; ++c) W[(size_t)r * k + c] += w * (double)y[r] * (double)y[c];
  }
  for (int d = 0; d < k; ++d) W[(size_t)d * k + d] += h->cfg.lambda * h->cfg.alpha * (double)n_u;  // ALS:488
  return true;
}

int apparent_rank_of_row(mals_handle h, int side, int64_t local_row) {
  std::vector<double> W;
  if (!build_row_system(h, side, local_row, W)) return 0;
  return mals::PivotedQR(W.data(), h->cfg.features, h->cfg.singularity_threshold).rank(0.01);
}

}  // namespace

int mals_check(mals_handle h) {
  if (!h) return MALS_INVALID_ARG;
  if (int rc = use_device(h)) return rc;
  HIPCHK(h, hipMemcpyAsync(h->h_bad.get(), h->d_bad.get(), 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // The kernels' verdict is "a Cholesky pivot <= threshold"; the reference's is "a diagonal element of R of the
  // column-pivoted QR <= threshold" (CMLSS:43-54), which can already hold when the smallest (unpivoted) Cholesky
  // pivot is still 100x the threshold (measured: 63 x 63 Gramian of 63 rows, pivot 5e-5, |R_dd| 2e-6).  So the row with
  // the smallest pivot within 1024x of the threshold is put to the reference's own test here, in fp64 on the host.
  for (int sd = 0; sd < 2; ++sd) {
    const unsigned long long key = h->h_bad.get()[2 + sd];
    if (h->h_bad.get()[sd] != ~0ull || key == ~0ull) continue;
    const int64_t row = (int64_t)(key & 0xffffffffull);
    SideState& s = h->side[sd];
    std::vector<double> W;
    if (row < s.n_local && s.h_row_ptr[(size_t)row + 1] - s.h_row_ptr[(size_t)row] <= 200000 && build_row_system(h, sd, row, W) &&
        !mals::PivotedQR(W.data(), h->cfg.features, h->cfg.singularity_threshold).non_singular())
      h->h_bad.get()[sd] = (unsigned long long)row;
  }
  if (h->h_bad.get()[2] != ~0ull || h->h_bad.get()[3] != ~0ull)
    HIPCHK(h, hipMemsetAsync(h->d_bad.get() + 2, 0xff, 2 * sizeof(unsigned long long), h->stream));
  for (int sd = 0; sd < 2; ++sd) {
    if (h->h_bad.get()[sd] != ~0ull) {
      h->sing_side = sd;
      h->sing_row = h->side[sd].row_offset + (int64_t)h->h_bad.get()[sd];
      h->sing_rank = apparent_rank_of_row(h, sd, (int64_t)h->h_bad.get()[sd]);
      HIPCHK(h, hipMemsetAsync(h->d_bad.get(), 0xff, 2 * sizeof(unsigned long long), h->stream));
      char buf[160];
      std::snprintf(buf, sizeof(buf), "near-singular system (pivot <= %g) for row %lld of side %c", h->cfg.singularity_threshold,
                    (long long)h->sing_row, sd == MALS_SIDE_X ? 'X' : 'Y');
      return fail(h, MALS_SINGULAR, buf);
    }
  }
  return MALS_OK;
}

int mals_singular_info(mals_handle h, int32_t* side, int64_t* row, int32_t* apparent_rank) {
  if (!h) return MALS_INVALID_ARG;
  if (side) *side = h->sing_side;
  if (row) *row = h->sing_row;
  if (apparent_rank) *apparent_rank = h->sing_rank;
  return MALS_OK;
}

// ---- Generation.recomputeSolver (mals_solver_s: mals_handle.h) ------------
int mals_solver_create(const double* A, int32_t n, double singularity_threshold, mals_solver* out, int32_t* apparent_rank_out) {
  if (out) *out = nullptr;
  if (!A || !out || n <= 0) return MALS_INVALID_ARG;
  mals_solver s = new (std::nothrow) mals_solver_s{mals::PivotedQR(A, n, singularity_threshold)};
  if (!s) return MALS_OOM;
  if (!s->qr.non_singular()) {  // CMLSS:43-54
    if (apparent_rank_out) *apparent_rank_out = s->qr.rank(0.01);
    delete s;
    return MALS_SINGULAR;
  }
  *out = s;
  return MALS_OK;
}

int mals_solver_dim(mals_solver s) { return s ? s->qr.dim() : 0; }

int mals_solver_solve_dtof(mals_solver s, const double* b, float* x) {
  if (!s || !b || !x) return MALS_INVALID_ARG;
  std::vector<double> t((size_t)s->qr.dim());
  s->qr.solve(b, t.data());
  for (int i = 0; i < s->qr.dim(); ++i) x[i] = (float)t[i];  // CommonsMathSolver.java:40-42
  return MALS_OK;
}

int mals_solver_solve_ftod(mals_solver s, const float* b, double* x) {
  if (!s || !b || !x) return MALS_INVALID_ARG;
  std::vector<double> t(b, b + s->qr.dim());  // CommonsMathSolver.java:48-51
  s->qr.solve(t.data(), x);
  return MALS_OK;
}

int mals_solver_destroy(mals_solver s) {
  delete s;
  return MALS_OK;
}

int mals_recompute_solver(mals_handle h, int side, mals_solver* out, double* inf_norm_out) {
  CHECK_SIDE(h, side);
  if (!out) return fail(h, MALS_INVALID_ARG, "out must not be NULL");
  *out = nullptr;
  if (inf_norm_out) *inf_norm_out = 0.0;
  SideState& s = h->side[side];
  if (!s.F || s.n_total == 0) return MALS_OK;  // Generation.java:145-147: no solver for an empty matrix
  const int k = h->cfg.features;
  std::vector<double> G((size_t)k * k);
  if (int rc = mals_gramian(h, side, G.data())) return rc;  // Generation.java:148
  const double norm = mals::max_abs_column_sum(G.data(), k);  // :149
  if (inf_norm_out) *inf_norm_out = norm;
  if (!(norm >= 1.0)) {  // :150-153 (a NaN norm is ill-conditioned too)
    char buf[96];
    std::snprintf(buf, sizeof(buf), "infNorm: %g; try decreasing model.als.lambda", norm);
    return fail(h, MALS_ILL_CONDITIONED, buf);
  }
  int32_t rank = 0;
  const int rc = mals_solver_create(G.data(), k, h->cfg.singularity_threshold, out, &rank);
  if (rc == MALS_SINGULAR) {
    h->sing_side = side;
    h->sing_row = -1;
    h->sing_rank = rank;
    char buf[96];
    std::snprintf(buf, sizeof(buf), "Apparent rank: %d", rank);
    return fail(h, rc, buf);
  }
  return rc == MALS_OK ? MALS_OK : fail(h, rc, "mals_solver_create failed");
}

int mals_half_iteration(mals_handle h, int side) {
  CHECK_SIDE(h, side);
  if (!(h->cfg.flags & MALS_FLAG_LOSS_IGNORES_UNSPECIFIED) || h->split_f16 || !h->side[1 - side].G_valid) {
    if (int rc = mals_gramian(h, 1 - side, nullptr)) return rc;  // ALS:342 / ALS:369
  }
  if (int rc = mals_solve_side(h, side)) return rc;                // ALS:344 / ALS:371
  return mals_check(h);                                            // ALS:346-361 f
}

int mals_sample_dots(mals_handle h, const int64_t* test_users, int32_t n_test_users, const int64_t* test_items, int32_t n_test_items,
                     double* host_out) {
  if (!h) return MALS_INVALID_ARG;
  SideState& x = h->side[MALS_SIDE_X];
  SideState& y = h->side[MALS_SIDE_Y];
  if (!x.F || !y.F) return fail(h, MALS_INVALID_ARG, "factor replicas not allocated");
  if (n_test_users < 0 || n_test_items < 0 || (n_test_users > 0 && !test_users) || (n_test_items > 0 && !test_items) ||
      (int64_t)n_test_users * n_test_items > (1 << 24))
    return fail(h, MALS_INVALID_ARG, "bad convergence sample");
  const int64_t n = (int64_t)n_test_users * n_test_items;
  if (n == 0) return MALS_OK;
  if (!host_out) return fail(h, MALS_INVALID_ARG, "null output");
  for (int i = 0; i < n_test_users; ++i)
    if (test_users[i] < 0 || test_users[i] >= x.n_total) return fail(h, MALS_INVALID_ARG, "test user outside the factor replica");
  for (int j = 0; j < n_test_items; ++j)
    if (test_items[j] < 0 || test_items[j] >= y.n_total) return fail(h, MALS_INVALID_ARG, "test item outside the factor replica");
  if (int rc = use_device(h)) return rc;
  const size_t n_idx = (size_t)(n_test_users + n_test_items);
  if (h->d_sd.capacity() < (size_t)n || h->d_sd_idx.capacity() < n_idx) {
    h->d_sd.reset();
    h->d_sd_idx.reset();
    HIPCHK(h, h->d_sd.alloc((size_t)n));
    HIPCHK(h, h->d_sd_idx.alloc(n_idx));
  }
  HIPCHK(h, hipMemcpyAsync(h->d_sd_idx.get(), test_users, sizeof(int64_t) * (size_t)n_test_users, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_sd_idx.get() + n_test_users, test_items, sizeof(int64_t) * (size_t)n_test_items, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(sample_dots_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, x.F, y.F, h->d_sd_idx.get(),
                     h->d_sd_idx.get() + n_test_users, n_test_users, n_test_items, h->cfg.features, h->d_sd.get());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(host_out, h->d_sd.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MALS_OK;
}

}  // extern "C"

namespace {

// mals_factorize's side of the loop in convergence.h: one handle, its own cancel flag, n_local rows per half
struct HandleFactorize {
  mals_handle h;
  int64_t rows0 = 0, nnz0 = 0;
  int fail(int code, const char* msg) { return ::fail(h, code, msg); }
  void clear_cancel() { h->cancelled.store(0); }
  int cancelled() { return h->cancelled.load() ? ::fail(h, MALS_CANCELLED, "cancelled") : MALS_OK; }
  int half_iteration(int side) { return mals_half_iteration(h, side); }
  int sample_dots(const int64_t* users, int32_t n_users, const int64_t* items, int32_t n_items, double* out) {
    return mals_sample_dots(h, users, n_users, items, n_items, out);
  }
  mals_iteration_fn callback(void** user) {
    *user = h->iter_user;
    return h->iter_fn;
  }
  void count(int point) {
    if (point == 0) rows0 = h->stats.rows_solved, nnz0 = h->stats.nnz_gathered;
  }
  void report(mals_iteration_info* info) {
    info->x_rows = h->side[MALS_SIDE_X].n_local;
    info->y_rows = h->side[MALS_SIDE_Y].n_local;
    info->entries_gathered = h->stats.nnz_gathered - nnz0;
    info->algorithmic_bytes = (double)info->entries_gathered * (4.0 * h->cfg.features + 8.0) +
                              (double)(h->stats.rows_solved - rows0) * (4.0 * h->cfg.features + 8.0);
    info->devices = 1;
  }
};

}  // namespace

extern "C" {

int mals_factorize(mals_handle h, double convergence_threshold, int32_t max_iterations, int32_t random_y, int32_t iterate,
                   const int64_t* test_users, int32_t n_test_users, const int64_t* test_items, int32_t n_test_items,
                   int32_t* iterations_out, double* convergence_out) {
  if (!h) return MALS_INVALID_ARG;
  HandleFactorize d{h};
  return factorize_loop(d, convergence_threshold, max_iterations, random_y, iterate, test_users, n_test_users, test_items, n_test_items,
                        iterations_out, convergence_out);
}

int mals_reconstruction_error(mals_handle h, double* sum_out, int64_t* count_out) {
  if (!h || !sum_out || !count_out) return MALS_INVALID_ARG;
  SideState& s = h->side[MALS_SIDE_X];
  SideState& o = h->side[MALS_SIDE_Y];
  if (!s.has_matrix || !s.F || !o.F) return fail(h, MALS_INVALID_ARG, "needs the user-side matrix and both factor replicas");
  if (int rc = use_device(h)) return rc;
  *sum_out = 0.0;
  *count_out = 0;
  if (s.n_local == 0) return MALS_OK;
  const unsigned grid = (unsigned)std::min<int64_t>((s.n_local + 3) / 4, (int64_t)h->n_cu * 32);
  const size_t n_waves = (size_t)grid * 4;
  DeviceBuffer<double> sums;
  DeviceBuffer<unsigned long long> counts;
  HIPCHK(h, sums.alloc(n_waves));
  HIPCHK(h, counts.alloc(n_waves));
  double* d_sum = sums.get();
  unsigned long long* d_cnt = counts.get();
  int rc = dispatch_T(h, [&](auto t) -> int {
    hipLaunchKernelGGL((reconstruction_kernel<t()>), dim3(grid), dim3(256), 0, h->stream, s.row_ptr, s.col,
                       s.F + s.row_offset * h->cfg.features, o.F, h->cfg.features, s.n_local, d_sum, d_cnt);
    HIPCHK(h, hipGetLastError());
    return MALS_OK;
  });
  std::vector<double> hs(n_waves);
  std::vector<unsigned long long> hc(n_waves);
  if (rc == MALS_OK) {
    hipError_t e = hipMemcpyAsync(hs.data(), d_sum, sizeof(double) * n_waves, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hc.data(), d_cnt, sizeof(unsigned long long) * n_waves, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) rc = fail(h, MALS_HIP_ERROR, hipGetErrorString(e));
  }
  sums.reset();
  counts.reset();
  if (rc != MALS_OK) return rc;
  double sum = 0.0;
  unsigned long long cnt = 0;
  for (size_t w = 0; w < n_waves; ++w) {  // fixed order: deterministic
    sum += hs[w];
    cnt += hc[w];
  }
  *sum_out = sum;
  *count_out = (int64_t)cnt;
  return MALS_OK;
}

int mals_symmetric_eigen(const double* A, int32_t n, double* evals_out, double* V_out) {
  if (!A || !evals_out || !V_out || n <= 0) return MALS_INVALID_ARG;
  return mals::symmetric_eigen(A, n, evals_out, V_out) ? MALS_OK : MALS_INVALID_ARG;
}

int mals_cancel(mals_handle h) {
  if (!h) return MALS_INVALID_ARG;
  h->cancelled.store(1);
  return MALS_OK;
}

int mals_set_iteration_callback(mals_handle h, mals_iteration_fn fn, void* user) {
  if (!h) return MALS_INVALID_ARG;
  h->iter_fn = fn;
  h->iter_user = user;
  return MALS_OK;
}

int mals_enable_timing(mals_handle h, int32_t on) {
  if (!h) return MALS_INVALID_ARG;
  h->timing = on != 0;
  return MALS_OK;
}

int mals_reset_stats(mals_handle h) {
  if (!h) return MALS_INVALID_ARG;
  if (int rc = use_device(h)) return rc;
  if (int rc = drain_events(h)) return rc;
  std::memset(&h->stats, 0, sizeof(h->stats));
  h->stats.struct_size = (int32_t)sizeof(mals_stats);
  HIPCHK(h, hipMemsetAsync(h->d_refined.get(), 0, sizeof(unsigned long long), h->stream));
  return MALS_OK;
}

int mals_get_stats(mals_handle h, mals_stats* out) {
  if (!h || !out) return MALS_INVALID_ARG;
  if (int rc = use_device(h)) return rc;
  if (int rc = drain_events(h)) return rc;
  unsigned long long refined = 0;
  HIPCHK(h, hipMemcpyAsync(&refined, h->d_refined.get(), sizeof(refined), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->stats.rows_refined = (int64_t)refined;
  *out = h->stats;
  return MALS_OK;
}

int mals_set_refine_limit(mals_handle h, double limit) {
  if (!h || !(limit >= 0.0)) return h ? fail(h, MALS_INVALID_ARG, "refine limit must be >= 0") : MALS_INVALID_ARG;
  h->refine_limit = (float)limit;
  return MALS_OK;
}

}  // extern "C"
