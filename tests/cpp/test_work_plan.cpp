// The list planner of the solve (csrc/work_plan.h) on random row-length mixes.  Stand-alone host program, built with
// -fsanitize=address,undefined by tests/test_work_plan.py.  usage: test_work_plan <seed>
//
// A shard per segment_nnz in {64, 192, 512, 4096}: a zipf-like body of row lengths plus the forced lengths 0, 1, 16, 17, 64,
// 65, seg, seg + 1, 32 seg + 1 and one row of more than 32 * 32 * seg / 8 entries; planned with chunk rows {0, 1, 7, 100},
// dual_blocks {0, 1, 4}, n_cu {4, 256}, without and with band cuts (synthetic ascending offsets, some rows "unsorted").
// Checked per plan, chunk by chunk, against counts taken from row_ptr alone:
//   * every local row appears exactly once among the direct rows, the one representative empty row, the dual classes, the
//     zero-filled rows and RowC;
//   * list A is in non-increasing length, the representative (the chunk's first empty row) sits directly behind the direct
//     rows, the dual classes run 49-64 ... 1-16 in that order with the right per-class counts and entry sums;
//   * the segments of every long row partition it exactly, each with 1 .. segment_nnz entries, count-cut ones in whole
//     4-entry steps except the last, slots consecutive in entry order and unique over the shard;
//   * plain segments in non-increasing length, banded ones behind them by band and then by length (the bands from
//     band_plan_row over the same offsets); nBand and nnzBand agree with what is there;
//   * rows of more than FINISH_GROUP segments: groups of at most FINISH_GROUP slots tile the row's slots, the row's nseg and
//     stride describe the leaders, offP and nP address exactly those groups;
//   * n_dual_rows, nnzA, nnzB and the banding counters equal the counts from row_ptr.
// A decreasing row_ptr is refused.  (The other refusal, 2^31 segments, needs a shard of that size.)
// Also prints "cuts <length> <segment_nnz> <start> ..." for a few count-cut rows: tests/test_work_plan.py compares them
// with tests/rows_cases.segment_cuts.
#include "../../myrrix-recommender_amd/csrc/work_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace mals;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (++failures <= 20) {                             \
        std::fprintf(stderr, "FAIL %s: ", #cond);         \
        std::fprintf(stderr, __VA_ARGS__);                \
        std::fprintf(stderr, "\n");                       \
      }                                                   \
    }                                                     \
  } while (0)

struct Case {
  int seg, dual_blocks, n_cu;
  int64_t chunk_rows;
  bool banded;
};

static std::vector<int64_t> row_lengths(std::mt19937_64& rng, int64_t seg) {
  std::uniform_real_distribution<double> u(1.0e-4, 1.0);
  const int64_t n = 1000 + (int64_t)(rng() % 500);
  std::vector<int64_t> len((size_t)n);
  for (int64_t& l : len) l = std::min<int64_t>((int64_t)std::pow(u(rng), -1.3) - 1, 6 * seg + 7);
  const int64_t forced[] = {0, 1, 16, 17, 64, 65, seg, seg + 1, 32 * seg + 1, 32 * 32 * seg / 8 + 1 + (int64_t)(rng() % 100)};
  for (int64_t f : forced) len[(size_t)(rng() % (uint64_t)n)] = f;
  len[0] = 0;   // (a forced length may have been overwritten by a later one: 0 and the two longest are put back)
  len[(size_t)n / 2] = forced[8];
  len[(size_t)n - 1] = forced[9];
  return len;
}

// band cuts as the device scan would report them: the eligible rows, ascending offsets per band boundary, a few unsorted
static BandCuts synthetic_cuts(std::mt19937_64& rng, const std::vector<int64_t>& rp, int64_t seg) {
  BandCuts bc;
  bc.n_bands = 6;
  bc.band_rows = 1000;
  bc.min_avg = 8;
  for (size_t r = 0; r + 1 < rp.size(); ++r) {
    const int64_t len = rp[r + 1] - rp[r];
    if (!band_row_eligible(len, seg, bc.n_bands, bc.min_avg)) continue;
    bc.row.push_back((int64_t)r);
    bc.unsorted.push_back(rng() % 4 == 0);
    std::vector<int64_t> off((size_t)bc.n_bands + 1, 0);
    for (int64_t b = 1; b < bc.n_bands; ++b) off[(size_t)b] = rng() % 3 == 0 ? off[(size_t)b - 1] : (int64_t)(rng() % (uint64_t)(len + 1));
    off[(size_t)bc.n_bands] = len;
    std::sort(off.begin(), off.end());
    bc.off.insert(bc.off.end(), off.begin(), off.end());
  }
  return bc;
}

static void check_plan(const Case& cs, const std::vector<int64_t>& rp, const BandCuts& bc, const WorkPlan& plan) {
  const int64_t n = (int64_t)rp.size() - 1, seg = cs.seg, dual_len = 16 * (int64_t)cs.dual_blocks;
  const int failures_before = failures;
  auto len_of = [&](int64_t r) { return rp[(size_t)r + 1] - rp[(size_t)r]; };
  const int64_t chunk_rows = cs.chunk_rows > 0 ? cs.chunk_rows : std::max<int64_t>(n, 1);
  const int64_t n_chunks = std::max<int64_t>(1, (n + chunk_rows - 1) / chunk_rows);
  CHECK((int64_t)plan.chunks.size() == n_chunks, "%zu chunks, expected %lld", plan.chunks.size(), (long long)n_chunks);
  if ((int64_t)plan.chunks.size() != n_chunks) return;
  std::vector<int> seen((size_t)n, 0), slot_seen((size_t)plan.n_slots, 0);
  // where every slot's segment is: position in list B, and whether in a banded tail
  std::vector<int64_t> slot_pos((size_t)plan.n_slots, -1);
  for (size_t i = 0; i < plan.itemsB.size(); ++i) {
    const int32_t id = plan.itemsB[i].id;
    CHECK(id >= 0 && id < plan.n_slots, "segment %zu has slot %d of %lld", i, id, (long long)plan.n_slots);
    if (id < 0 || id >= plan.n_slots) return;
    ++slot_seen[(size_t)id];
    slot_pos[(size_t)id] = (int64_t)i;
  }
  for (int64_t sl = 0; sl < plan.n_slots; ++sl) CHECK(slot_seen[(size_t)sl] == 1, "slot %lld used %d times", (long long)sl, slot_seen[(size_t)sl]);
  CHECK((int64_t)plan.itemsB.size() == plan.n_slots, "%zu segments, %lld slots", plan.itemsB.size(), (long long)plan.n_slots);
  if (failures != failures_before) return;
  int64_t tot_dual = 0, tot_nnzA = 0, tot_nnzB = 0, tot_banded_rows = 0, tot_banded_segs = 0, tot_unsorted = 0, endA = 0, endB = 0, endC = 0;
  size_t bc_next = 0;
  std::vector<int32_t> band_of((size_t)plan.n_slots, -1);
  std::vector<BandPiece> pieces;
  for (int64_t c = 0; c < n_chunks; ++c) {
    const ChunkRange& cr = plan.chunks[(size_t)c];
    const int64_t r0 = std::min(n, c * chunk_rows), r1 = std::min(n, (c + 1) * chunk_rows);
    CHECK(cr.row0 == r0 && cr.row1 == r1, "chunk %lld rows [%lld, %lld), expected [%lld, %lld)", (long long)c, (long long)cr.row0, (long long)cr.row1,
          (long long)r0, (long long)r1);
    // ---- what row_ptr says about the chunk
    int64_t nD[4] = {0, 0, 0, 0}, eD[4] = {0, 0, 0, 0}, n_direct = 0, e_direct = 0, n_empty = 0, first_empty = -1, n_long = 0, e_long = 0;
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t len = len_of(r);
      if (len == 0) {
        if (!n_empty++) first_empty = r;
      } else if (len > seg) {
        ++n_long;
        e_long += len;
      } else if (len <= dual_len) {
        ++nD[(len - 1) >> 4];
        eD[(len - 1) >> 4] += len;
      } else {
        ++n_direct;
        e_direct += len;
      }
    }
    // ---- list A
    CHECK(cr.offA == endA && cr.offB == endB && cr.offC == endC, "chunk %lld does not start where the one before ends", (long long)c);
    CHECK(cr.nA == n_direct + (n_empty ? 1 : 0) && cr.nZ == (n_empty ? n_empty - 1 : 0), "chunk %lld: nA %lld nZ %lld, %lld direct %lld empty", (long long)c,
          (long long)cr.nA, (long long)cr.nZ, (long long)n_direct, (long long)n_empty);
    CHECK(cr.nnzA == e_direct, "chunk %lld nnzA %lld, expected %lld", (long long)c, (long long)cr.nnzA, (long long)e_direct);
    for (int cls = 0; cls < 4; ++cls)
      CHECK(cr.nD[cls] == nD[cls] && cr.nnzD[cls] == eD[cls], "chunk %lld class %d: %lld rows %lld entries, expected %lld, %lld", (long long)c, cls,
            (long long)cr.nD[cls], (long long)cr.nnzD[cls], (long long)nD[cls], (long long)eD[cls]);
    endA = cr.offA + cr.nA + cr.n_dual() + cr.nZ;
    CHECK(endA <= (int64_t)plan.itemsA.size(), "chunk %lld: list A ends at %lld of %zu", (long long)c, (long long)endA, plan.itemsA.size());
    if (endA > (int64_t)plan.itemsA.size()) return;
    int64_t class_end[4];  // one past the last position of the classes 3, 2, 1, 0 (in that order) inside the chunk's dual part
    class_end[0] = cr.nD[3];
    class_end[1] = class_end[0] + cr.nD[2];
    class_end[2] = class_end[1] + cr.nD[1];
    class_end[3] = class_end[2] + cr.nD[0];
    for (int64_t i = cr.offA; i < endA; ++i) {
      const WorkItem& w = plan.itemsA[(size_t)i];
      CHECK(w.id >= r0 && w.id < r1, "chunk %lld holds row %d", (long long)c, w.id);
      if (w.id < r0 || w.id >= r1) return;
      ++seen[(size_t)w.id];
      CHECK(w.begin == rp[(size_t)w.id] && w.len == len_of(w.id), "row %d listed at %lld with %d entries", w.id, (long long)w.begin, w.len);
      const int64_t at = i - cr.offA;
      if (at < cr.nA) {   // direct rows, the representative last
        const bool rep = n_empty && at == cr.nA - 1;
        CHECK(rep ? (w.len == 0 && w.id == first_empty) : (w.len > dual_len && w.len <= seg), "direct position %lld of chunk %lld: row %d, %d entries",
              (long long)at, (long long)c, w.id, w.len);
      } else if (at < cr.nA + cr.n_dual()) {
        const int64_t d = at - cr.nA;
        const int cls = d < class_end[0] ? 3 : d < class_end[1] ? 2 : d < class_end[2] ? 1 : 0;
        CHECK(w.len >= 1 && (w.len - 1) >> 4 == cls, "dual position %lld of chunk %lld (class %d): %d entries", (long long)d, (long long)c, cls, w.len);
      } else {
        CHECK(w.len == 0, "zero-filled row %d has %d entries", w.id, w.len);
      }
      if (i > cr.offA && !(n_empty && at == cr.nA))   // (the representative, empty, stands in front of the dual classes)
        CHECK(plan.itemsA[(size_t)i - 1].len >= w.len, "list A of chunk %lld ascends at %lld", (long long)c, (long long)at);
    }
    // ---- lists B and C
    endB = cr.offB + cr.nB;
    endC = cr.offP + cr.nP;
    CHECK(endB <= (int64_t)plan.itemsB.size() && endC <= (int64_t)plan.rowsC.size() && cr.offP == cr.offC + cr.nC && cr.nBand <= cr.nB,
          "chunk %lld: list B or C out of range", (long long)c);
    if (endB > (int64_t)plan.itemsB.size() || endC > (int64_t)plan.rowsC.size() || cr.offP != cr.offC + cr.nC || cr.nBand > cr.nB) return;
    CHECK(cr.nC == n_long && cr.nnzB == e_long, "chunk %lld: %lld long rows %lld entries, expected %lld, %lld", (long long)c, (long long)cr.nC,
          (long long)cr.nnzB, (long long)n_long, (long long)e_long);
    const int64_t band0 = endB - cr.nBand;   // first banded position
    int64_t n_segs = 0, e_band = 0, n_band_segs = 0, next_group = cr.offP;
    for (int64_t i = cr.offC; i < cr.offC + cr.nC; ++i) {
      const RowC& rc = plan.rowsC[(size_t)i];
      CHECK(rc.row >= r0 && rc.row < r1 && len_of(rc.row) > seg, "chunk %lld finishes row %d", (long long)c, rc.row);
      if (rc.row < r0 || rc.row >= r1) return;
      ++seen[(size_t)rc.row];
      if (i > cr.offC) CHECK(plan.rowsC[(size_t)i - 1].row < rc.row, "list C of chunk %lld not in row order", (long long)c);
      const int64_t len = len_of(rc.row);
      // is the row banded?  (the planner's rule, from the cuts alone)
      while (bc_next < bc.row.size() && bc.row[bc_next] < rc.row) ++bc_next;
      pieces.clear();
      if (bc_next < bc.row.size() && bc.row[bc_next] == rc.row) {
        if (bc.unsorted[bc_next]) ++tot_unsorted;
        else if (!band_plan_row(&bc.off[bc_next * (size_t)(bc.n_bands + 1)], bc.n_bands, len, seg, pieces)) pieces.clear();
      }
      const bool banded = !pieces.empty();
      // its segments: consecutive slots from first_slot, in entry order, until the row is covered
      int64_t at = 0, k = 0;
      for (; at < len; ++k) {
        const int64_t sl = rc.first_slot + k;
        CHECK(sl < plan.n_slots, "row %d runs out of slots", rc.row);
        if (sl >= plan.n_slots) return;
        const int64_t pos = slot_pos[(size_t)sl];
        const WorkItem& sg = plan.itemsB[(size_t)pos];
        CHECK(pos >= cr.offB && pos < endB && (pos >= band0) == banded, "row %d segment %lld at position %lld of list B (banded: %d)", rc.row, (long long)k,
              (long long)pos, (int)banded);
        CHECK(sg.begin == rp[(size_t)rc.row] + at, "row %d segment %lld begins at %lld, expected %lld", rc.row, (long long)k, (long long)sg.begin,
              (long long)(rp[(size_t)rc.row] + at));
        CHECK(sg.len >= 1 && sg.len <= seg && at + sg.len <= len, "row %d segment %lld has %d entries", rc.row, (long long)k, sg.len);
        if (sg.len < 1 || sg.begin != rp[(size_t)rc.row] + at) return;
        if (!banded && at + sg.len < len) CHECK(sg.len % 4 == 0, "row %d segment %lld: %d entries, no whole 4-entry steps", rc.row, (long long)k, sg.len);
        if (banded) {
          CHECK((size_t)k < pieces.size() && pieces[(size_t)k].begin == at && pieces[(size_t)k].len == sg.len, "row %d segment %lld is not piece %lld", rc.row,
                (long long)k, (long long)k);
          if ((size_t)k < pieces.size()) band_of[(size_t)sl] = pieces[(size_t)k].band;
        }
        at += sg.len;
      }
      CHECK(at == len && (!banded || (size_t)k == pieces.size()), "row %d: segments cover %lld of %lld entries", rc.row, (long long)at, (long long)len);
      n_segs += k;
      if (banded) {
        ++tot_banded_rows;
        e_band += len;
        n_band_segs += k;
      }
      if (k > FINISH_GROUP) {
        const int64_t n_groups = (k + FINISH_GROUP - 1) / FINISH_GROUP;
        CHECK(rc.nseg == n_groups && rc.stride == FINISH_GROUP, "row %d: %lld segments, nseg %d stride %d", rc.row, (long long)k, rc.nseg, rc.stride);
        for (int64_t g = 0; g < n_groups; ++g, ++next_group) {
          CHECK(next_group < endC, "row %d: group %lld missing", rc.row, (long long)g);
          if (next_group >= endC) return;
          const RowC& gr = plan.rowsC[(size_t)next_group];
          CHECK(gr.first_slot == rc.first_slot + g * FINISH_GROUP && gr.nseg == std::min<int64_t>(FINISH_GROUP, k - g * FINISH_GROUP) && gr.stride == 1 &&
                    gr.row == rc.row,
                "row %d group %lld: slots %lld + %d, stride %d", rc.row, (long long)g, (long long)gr.first_slot, gr.nseg, gr.stride);
        }
      } else {
        CHECK(rc.nseg == k && rc.stride == 1, "row %d: %lld segments, nseg %d stride %d", rc.row, (long long)k, rc.nseg, rc.stride);
      }
    }
    CHECK(next_group == endC, "chunk %lld: %lld groups beyond those of its rows", (long long)c, (long long)(endC - next_group));
    CHECK(n_segs == cr.nB && n_band_segs == cr.nBand && e_band == cr.nnzBand, "chunk %lld: nB %lld nBand %lld nnzBand %lld, found %lld, %lld, %lld", (long long)c,
          (long long)cr.nB, (long long)cr.nBand, (long long)cr.nnzBand, (long long)n_segs, (long long)n_band_segs, (long long)e_band);
    for (int64_t i = cr.offB + 1; i < endB; ++i) {
      const WorkItem &a = plan.itemsB[(size_t)i - 1], &b = plan.itemsB[(size_t)i];
      if (i < band0) CHECK(a.len >= b.len, "plain segments of chunk %lld ascend at %lld", (long long)c, (long long)(i - cr.offB));
      if (i > band0) {
        const int32_t ba = band_of[(size_t)a.id], bb = band_of[(size_t)b.id];
        CHECK(ba < bb || (ba == bb && a.len >= b.len), "banded segments of chunk %lld out of order at %lld: band %d len %d, then band %d len %d", (long long)c,
              (long long)(i - cr.offB), ba, a.len, bb, b.len);
      }
    }
    tot_dual += cr.n_dual();
    tot_nnzA += cr.nnzA;
    tot_nnzB += cr.nnzB;
    tot_banded_segs += n_band_segs;
  }
  for (int64_t r = 0; r < n; ++r) CHECK(seen[(size_t)r] == 1, "row %lld listed %d times", (long long)r, seen[(size_t)r]);
  CHECK(endA == (int64_t)plan.itemsA.size() && endB == (int64_t)plan.itemsB.size() && endC == (int64_t)plan.rowsC.size(), "entries behind the last chunk");
  CHECK(plan.n_dual_rows == tot_dual && plan.nnzA == tot_nnzA && plan.nnzB == tot_nnzB, "totals: dual %lld nnzA %lld nnzB %lld", (long long)plan.n_dual_rows,
        (long long)plan.nnzA, (long long)plan.nnzB);
  CHECK(plan.n_banded_rows == tot_banded_rows && plan.n_banded_segs == tot_banded_segs && plan.n_unsorted == tot_unsorted,
        "banding counters %lld %lld %lld, found %lld %lld %lld", (long long)plan.n_banded_rows, (long long)plan.n_banded_segs, (long long)plan.n_unsorted,
        (long long)tot_banded_rows, (long long)tot_banded_segs, (long long)tot_unsorted);
}

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 1u;
  std::mt19937_64 rng(seed);
  int64_t n_plans = 0, n_grouped = 0, n_banded = 0;
  WorkPlan plan;
  for (int seg : {64, 192, 512, 4096}) {
    const std::vector<int64_t> len = row_lengths(rng, seg);
    std::vector<int64_t> rp(len.size() + 1, 0);
    for (size_t r = 0; r < len.size(); ++r) rp[r + 1] = rp[r] + len[r];
    const BandCuts none, cuts = synthetic_cuts(rng, rp, seg);
    for (int64_t chunk_rows : {0, 1, 7, 100})
      for (int dual_blocks : {0, 1, 4})
        for (int n_cu : {4, 256})
          for (bool banded : {false, true}) {
            const Case cs{seg, dual_blocks, n_cu, chunk_rows, banded};
            const BandCuts& bc = banded ? cuts : none;
            const char* why = plan_work_lists(rp.data(), (int64_t)len.size(), seg, chunk_rows, dual_blocks, n_cu, bc, plan);
            CHECK(!why, "seg %d chunk rows %lld dual %d cus %d banded %d refused: %s", seg, (long long)chunk_rows, dual_blocks, n_cu, (int)banded, why);
            if (why) continue;
            const int before = failures;
            check_plan(cs, rp, bc, plan);
            if (failures != before && before < 20)
              std::fprintf(stderr, "  (seg %d chunk rows %lld dual %d cus %d banded %d)\n", seg, (long long)chunk_rows, dual_blocks, n_cu, (int)banded);
            ++n_plans;
            n_banded += plan.n_banded_rows;
            for (const ChunkRange& cr : plan.chunks) n_grouped += cr.nP;
          }
    // a row_ptr that descends
    std::vector<int64_t> bad = rp;
    std::swap(bad[bad.size() / 2], bad[bad.size() / 2 + 1]);
    if (bad != rp) CHECK(plan_work_lists(bad.data(), (int64_t)len.size(), seg, 7, 4, 256, none, plan) != nullptr, "a decreasing row_ptr was accepted");
  }
  {  // an empty shard: one empty chunk
    const int64_t rp0[1] = {0};
    CHECK(!plan_work_lists(rp0, 0, 64, 0, 4, 256, BandCuts(), plan) && plan.chunks.size() == 1 && plan.itemsA.empty() && plan.n_slots == 0, "empty shard");
  }
  // the count cuts of single rows, for the Python restatement the exact-rows tests rest on
  const int64_t pairs[][2] = {{65, 64}, {129, 64}, {1000, 64}, {2049, 64}, {4129, 64}, {193, 192}, {577, 192}, {4129, 192}, {513, 512}, {4129, 512}};
  for (const auto& pr : pairs) {
    const int64_t rp1[2] = {0, pr[0]};
    const char* why = plan_work_lists(rp1, 1, (int)pr[1], 0, 4, 256, BandCuts(), plan);
    CHECK(!why, "single row refused");
    if (why) continue;
    std::vector<int64_t> starts;
    for (const WorkItem& sg : plan.itemsB) starts.push_back(sg.begin);
    std::sort(starts.begin(), starts.end());
    std::printf("cuts %lld %lld", (long long)pr[0], (long long)pr[1]);
    for (int64_t b : starts) std::printf(" %lld", (long long)b);
    std::printf("\n");
  }
  std::printf("plans %lld grouped %lld banded %lld failures %d\n", (long long)n_plans, (long long)n_grouped, (long long)n_banded, failures);
  return failures ? 1 : 0;
}
