// band_plan.h -- where a long, dense row is cut when its segments follow the bands of the gather table (host only, no
// HIP: tests/cpp/test_band_plan.cpp builds it on its own).
//
// The gather table (the opposite side's factor replica) is cut into n_bands contiguous row ranges of band_rows rows.
// A row whose columns ascend reads the table front to back, so a segment that ends where a band ends reads one band
// only; the segments of all such rows, run band by band, keep the random gather inside a stretch of the table that the
// last-level cache holds.  Which rows are cut this way depends on the row's own length and on
// constants, never on what else is in the chunk: chunked and un-chunked lists cut a row alike.
#pragma once

#include <cstdint>
#include <vector>

namespace mals {

struct BandPiece {
  int64_t begin;  // offset of the first entry inside the row
  int32_t len;    // entries, 1 .. segment_nnz
  int32_t band;   // the band the piece reads (the last one it touches: see band_plan_row)
};

// Entries per band, on average, from which banding a row pays.  Every piece costs a partial slot, written by the
// segments kernel and read back by the finish kernel: 2 * slot_floats * 4 bytes, against 4 k + 8 bytes per entry of the
// piece itself.  The slots may cost a tenth of the entries' traffic at most: 853 entries at k = 64 (slot 2816 floats).
inline int64_t band_min_avg(int64_t slot_floats, int k) {
  const int64_t slot_bytes = 2 * slot_floats * 4, entry_bytes = 4 * (int64_t)k + 8;
  return (10 * slot_bytes + entry_bytes - 1) / entry_bytes;
}

// The length rule of a banded row (the other condition, ascending columns, is checked on the device).
inline bool band_row_eligible(int64_t len, int64_t segment_nnz, int64_t n_bands, int64_t min_avg) {
  return n_bands > 1 && len > segment_nnz && len / n_bands >= min_avg;
}

// Pieces smaller than this are not worth a slot of their own: they ride with the next band's piece.
inline int64_t band_min_piece(int64_t len, int64_t n_bands) { return len / n_bands / 4; }

// off[b] = first entry of the row with a column in band b or later (off[0] = 0, off[n_bands] = len, non-decreasing).
// Appends the row's pieces in entry order and returns true; returns false (nothing appended) when off is not such a
// sequence.  Band by band: an empty band gives no piece; a piece below band_min_piece() is carried into the next band's
// (so a piece holds fewer than band_min_piece() entries from bands before its own, and none from a later one); a piece
// above segment_nnz is cut by count, in whole 4-entry steps, and all its parts belong to the band.  At most n_bands
// more pieces than ceil(len / segment_nnz).
inline bool band_plan_row(const int64_t* off, int64_t n_bands, int64_t len, int64_t segment_nnz, std::vector<BandPiece>& out) {
  if (n_bands < 1 || len < 1 || segment_nnz < 1 || off[0] != 0 || off[n_bands] != len) return false;
  for (int64_t b = 0; b < n_bands; ++b)
    if (off[b + 1] < off[b]) return false;
  const int64_t min_piece = band_min_piece(len, n_bands);
  int64_t begin = 0;
  for (int64_t b = 0; b < n_bands; ++b) {
    const int64_t end = off[b + 1], piece = end - begin;
    if (piece == 0) continue;
    if (piece < min_piece && end < len) continue;  // carried (entries behind it exist: a later band takes it along)
    const int64_t nseg = (piece + segment_nnz - 1) / segment_nnz;
    int64_t per = (piece + nseg - 1) / nseg;
    per = (per + 3) & ~(int64_t)3;
    if (per > segment_nnz) per = segment_nnz;
    for (int64_t a = begin; a < end; a += per) {
      BandPiece p;
      p.begin = a;
      p.len = (int32_t)(end - a < per ? end - a : per);
      p.band = (int32_t)b;
      out.push_back(p);
    }
    begin = end;
  }
  return true;
}

}  // namespace mals
