// work_plan.h -- which rows every solving kernel sees: a shard's rows split into the work lists (DESIGN.md "work
// decomposition"), chunk by chunk.  Host only, no HIP, pure integer work on the shard's row_ptr:
// tests/cpp/test_work_plan.cpp builds it on its own.  als_kernels.h includes it for the list entries the kernels read.
#pragma once

#include "band_plan.h"

#include <algorithm>
#include <cstdint>
#include <limits>
#include <utility>
#include <vector>

namespace mals {

struct WorkItem {   // one row (list A) or one segment of a long row (list B); 16 bytes, s_load_dwordx4
  int64_t begin;    // absolute offset into col/val
  int32_t len;      // entries
  int32_t id;       // list A: local row; list B: scratch slot
};
struct RowC {       // a long row to be finished from its segment partials: slots first_slot + i * stride, i < nseg
  int64_t first_slot;
  int32_t row;
  int32_t nseg;
  int32_t stride;   // 1, or the group length once als_prereduce_kernel has summed every group of slots into its first
  int32_t pad_;
};
// A wave sums a row's partial slots one after the other (a dependent chain of ~0.7 us each): the most popular item of
// C4 (7M entries, 1 700 segments) kept the finish kernel running for 1.15 ms with everything else long done.  Rows with
// more than FINISH_GROUP segments are first reduced group-wise, one wave per group of FINISH_GROUP consecutive slots,
// in place (als_prereduce_kernel); the finish kernel then walks the group leaders.
constexpr int FINISH_GROUP = 32;

// Which rows of the shard are long enough to be banded (band_plan.h) and where their columns cross the bands; found on
// the device (the columns live there).  n_bands = 1: no banding.
struct BandCuts {
  int64_t n_bands = 1, band_rows = 0, min_avg = 0;
  std::vector<int64_t> row;      // the rows long enough, ascending
  std::vector<int64_t> off;      // [row.size()][n_bands + 1]
  std::vector<int> unsorted;     // [row.size()]
};

// the lists are stored chunk-major (contiguous ranges of chunk_rows rows of the shard), each
// chunk sorted by length; a chunk can be solved on its own so that the caller can overlap the
// exchange of finished chunks with the solve of the next one
// itemsA of a chunk: [nA rows for the direct kernel, longest first, then ONE representative empty
// row] [the dual classes: nD[3] rows with 48 < len <= 64, nD[2] ..., nD[0] rows with len <= 16 --
// descending length throughout] [nZ further empty rows: x = 0, same verdict as the representative]
struct ChunkRange {
  int64_t row0 = 0, row1 = 0;  // the chunk's rows of the shard
  int64_t offA = 0, nA = 0, nnzA = 0, offB = 0, nB = 0, nnzB = 0, offC = 0, nC = 0;
  int64_t offP = 0, nP = 0;  // groups of partial slots reduced ahead of the finish kernel (entries of rowsC as well)
  int64_t nD[4] = {0, 0, 0, 0}, nnzD[4] = {0, 0, 0, 0}, nZ = 0;
  int64_t nBand = 0, nnzBand = 0;  // the tail of list B (included in nB, nnzB): segments cut at the gather table's bands
  int64_t n_dual() const { return nD[0] + nD[1] + nD[2] + nD[3]; }
  int64_t nnz_dual() const { return nnzD[0] + nnzD[1] + nnzD[2] + nnzD[3]; }
};

struct WorkPlan {
  std::vector<WorkItem> itemsA;  // rows no longer than segment_nnz, longest first
  std::vector<WorkItem> itemsB;  // segments of the long rows, longest first; behind them the chunk's banded segments
                                 // (band_plan.h), band by band
  std::vector<RowC> rowsC;       // per chunk: its long rows, then their slot groups
  std::vector<ChunkRange> chunks;
  int64_t n_slots = 0;           // partial slots of the shard (the ids of list B)
  int64_t nnzA = 0, nnzB = 0;    // entries handled by the rows kernel / the segments kernel
  int64_t n_dual_rows = 0;
  int64_t n_banded_rows = 0, n_banded_segs = 0, n_unsorted = 0;  // MALS_DEBUG_LISTS
};

// Rows per chunk: chunk_rows, or the whole shard for 0.
inline int64_t plan_chunk_rows(int64_t chunk_rows, int64_t n_local) { return chunk_rows > 0 ? chunk_rows : std::max<int64_t>(n_local, 1); }

// row_ptr: n_local + 1 offsets.  dual_blocks: rows with 1 .. 16 * dual_blocks entries go to the dual classes (0 = none).
// Returns nullptr, or why the shard cannot be planned (plan is then unspecified).
inline const char* plan_work_lists(const int64_t* rp, int64_t n, int seg, int64_t chunk_rows_wanted, int dual_blocks, int n_cu,
                                   const BandCuts& bc, WorkPlan& plan) {
  plan = WorkPlan();
  const int64_t chunk_rows = plan_chunk_rows(chunk_rows_wanted, n);
  const int n_chunks = (int)std::max<int64_t>(1, (n + chunk_rows - 1) / chunk_rows);
  std::vector<WorkItem>& order = plan.itemsA;
  std::vector<WorkItem>& segs = plan.itemsB;
  std::vector<RowC>& rowsC = plan.rowsC;
  std::vector<std::pair<int32_t, WorkItem>> band_segs;  // (band, segment) of the chunk's banded rows
  std::vector<BandPiece> pieces;
  std::vector<RowC> groups;
  size_t bc_next = 0;  // cursor into bc.row (the chunks visit the rows in ascending order)
  order.reserve((size_t)n);
  int64_t& slot = plan.n_slots;
  plan.chunks.assign((size_t)n_chunks, ChunkRange());
  std::vector<int64_t> count((size_t)seg + 2);
  for (int c = 0; c < n_chunks; ++c) {
    ChunkRange& cr = plan.chunks[(size_t)c];
    const int64_t r0 = cr.row0 = std::min(n, c * chunk_rows), r1 = cr.row1 = std::min(n, (c + 1) * chunk_rows);
    cr.offA = (int64_t)order.size();
    cr.offB = (int64_t)segs.size();
    cr.offC = (int64_t)rowsC.size();
    // counting sort of the chunk's short rows by length, longest first (stable: ascending row inside a length)
    std::fill(count.begin(), count.end(), 0);
    const int64_t dual_len = 16 * (int64_t)dual_blocks;  // rows with 1..dual_len entries: dual lists
    int64_t n_short = 0, n_direct = 0, n_empty = 0;
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t len = rp[r + 1] - rp[r];
      if (len < 0) return "row_ptr must be non-decreasing";
      if (len <= seg) {
        ++count[(size_t)(seg - len)];
        ++n_short;
        if (len == 0) {
          ++n_empty;
        } else if (len <= dual_len) {
          const int cls = (int)((len - 1) >> 4);
          ++cr.nD[cls];
          cr.nnzD[cls] += len;
        } else {
          ++n_direct;
          cr.nnzA += len;
        }
      } else {
        cr.nnzB += len;
      }
    }
    // How the long rows (more than segment_nnz entries) are cut: segments of up to segment_nnz entries when that gives
    // at least one per SIMD, shorter ones otherwise -- a wave takes ~20 ns per entry, and the user half of C2 (a handful
    // of rows above 4 096 entries) ran FOUR waves for 80 us on the critical path (round 3: 80 -> 22 us).  Each segment
    // costs a partial slot, written and read back one after the other by the finish kernel's one wave per row: with
    // six times the segments on C2's item half the finish kernel went from 23 to 70 us and ate the gain -- hence only
    // for lists that cannot even give every SIMD a segment, and never below 512 entries.
    int64_t seg_b = seg;
    {
      const int64_t want_segments = (int64_t)n_cu * 4;
      const int64_t lo = std::min<int64_t>(512, seg);
      seg_b = std::max<int64_t>(lo, std::min<int64_t>(seg, (cr.nnzB + want_segments - 1) / want_segments));
      seg_b = (seg_b + 31) & ~(int64_t)31;                   // whole 32-entry super-steps
      if (seg_b > seg) seg_b = seg;
    }
    int64_t acc = cr.offA;
    for (size_t b = 0; b < count.size(); ++b) {
      const int64_t cnt = count[b];
      count[b] = acc;
      acc += cnt;
    }
    order.resize((size_t)(cr.offA + n_short));
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t len = rp[r + 1] - rp[r];
      if (len <= seg) {
        WorkItem& w = order[(size_t)count[(size_t)(seg - len)]++];
        w.begin = rp[r];
        w.len = (int32_t)len;
        w.id = (int32_t)r;
      } else {
        const int64_t nseg = (len + seg_b - 1) / seg_b;
        int64_t per = (len + nseg - 1) / nseg;
        per = (per + 3) & ~(int64_t)3;  // whole 4-entry steps
        RowC rc;
        rc.first_slot = slot;
        rc.row = (int32_t)r;
        rc.nseg = 0;
        rc.stride = 1;
        rc.pad_ = 0;
        // A row long enough to be cut at the gather table's bands (band_plan.h), with ascending columns: its pieces,
        // slots in entry order like any other row's.  Everything else: cuts by count.
        pieces.clear();
        if (bc_next < bc.row.size() && bc.row[bc_next] == r) {
          if (bc.unsorted[bc_next]) ++plan.n_unsorted;
          else if (!band_plan_row(&bc.off[bc_next * (size_t)(bc.n_bands + 1)], bc.n_bands, len, seg, pieces)) pieces.clear();
          ++bc_next;
        }
        if (!pieces.empty()) {
          ++plan.n_banded_rows;
          plan.n_banded_segs += (int64_t)pieces.size();
          cr.nnzBand += len;
          for (const BandPiece& pc : pieces) {
            if (slot >= std::numeric_limits<int32_t>::max()) return "too many row segments";
            WorkItem sg;
            sg.begin = rp[r] + pc.begin;
            sg.len = pc.len;
            sg.id = (int32_t)slot++;
            band_segs.emplace_back(pc.band, sg);
            ++rc.nseg;
          }
        } else {
          for (int64_t b = 0; b < len; b += per) {
            if (slot >= std::numeric_limits<int32_t>::max()) return "too many row segments";
            WorkItem sg;
            sg.begin = rp[r] + b;
            sg.len = (int32_t)std::min(per, len - b);
            sg.id = (int32_t)slot++;
            segs.push_back(sg);
            ++rc.nseg;
          }
        }
        if (rc.nseg > FINISH_GROUP) {  // group sums first (als_prereduce_kernel), the finish kernel walks the leaders
          // (groups of max(8, sqrt(segments)) slots, more rows grouped: finish + group sums 0.29 -> 0.35 ms on C4 -- every
          // group sum is a slot read and written once more)
          const int32_t grp_len = FINISH_GROUP;
          for (int32_t g0 = 0; g0 < rc.nseg; g0 += grp_len) {
            RowC grp;
            grp.first_slot = rc.first_slot + g0;
            grp.row = (int32_t)r;
            grp.nseg = std::min<int32_t>(grp_len, rc.nseg - g0);
            grp.stride = 1;
            grp.pad_ = 0;
            groups.push_back(grp);
          }
          rc.nseg = (rc.nseg + grp_len - 1) / grp_len;
          rc.stride = grp_len;
        }
        rowsC.push_back(rc);
      }
    }
    // Every empty row has the same system (W = G, b = 0: ALS:447-494 with no entries): x = 0, and the
    // verdict "singular" is shared.  One representative (the smallest row) goes through the kernel, right
    // behind the direct rows; the others are only zero-filled.
    const int64_t n_dual = cr.n_dual();
    if (n_empty > 0 && n_dual > 0) {
      auto first = order.begin() + (size_t)(cr.offA + n_direct);
      std::rotate(first, first + (size_t)n_dual, first + (size_t)n_dual + 1);
    }
    cr.nA = n_direct + (n_empty > 0 ? 1 : 0);
    cr.nZ = n_empty > 0 ? n_empty - 1 : 0;
    plan.n_dual_rows += n_dual;
    cr.nBand = (int64_t)band_segs.size();
    cr.nB = (int64_t)segs.size() - cr.offB + cr.nBand;
    cr.nC = (int64_t)rowsC.size() - cr.offC;
    cr.offP = (int64_t)rowsC.size();  // the chunk's slot groups sit behind its rows in the same array
    cr.nP = (int64_t)groups.size();
    rowsC.insert(rowsC.end(), groups.begin(), groups.end());
    groups.clear();
    // longest segments first; behind them the banded ones by band, longest first inside a band (both stable in row order)
    std::stable_sort(segs.begin() + cr.offB, segs.end(), [](const WorkItem& a, const WorkItem& b) { return a.len > b.len; });
    std::stable_sort(band_segs.begin(), band_segs.end(), [](const std::pair<int32_t, WorkItem>& a, const std::pair<int32_t, WorkItem>& b) {
      return a.first != b.first ? a.first < b.first : a.second.len > b.second.len;
    });
    for (const std::pair<int32_t, WorkItem>& bs : band_segs) segs.push_back(bs.second);
    band_segs.clear();
    plan.nnzA += cr.nnzA;
    plan.nnzB += cr.nnzB;
  }
  return nullptr;
}

}  // namespace mals
