// The piece planner of the banded long rows (csrc/band_plan.h) on random sorted rows.  Stand-alone host program, built
// with -fsanitize=address,undefined by tests/test_band_plan.py.  usage: test_band_plan <seed> <rows>
//
// Checked for every row:
//   * the pieces partition the row exactly, in entry order;
//   * no piece is empty or longer than segment_nnz;
//   * no piece crosses a band: it holds no entry of a band behind its own, and fewer than band_min_piece() entries of
//     the bands before it (the small pieces the planner carries into the next band; none at all when that is 0);
//   * at most n_bands more pieces than ceil(len / segment_nnz), the count of today's cuts at their longest;
//   * the same row gives the same pieces alone and behind other rows' pieces in the same output vector.
#include "../../myrrix-recommender_amd/csrc/band_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using mals::BandPiece;

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

static std::vector<int64_t> offsets(const std::vector<int32_t>& col, int64_t n_bands, int64_t band_rows) {
  std::vector<int64_t> off((size_t)n_bands + 1);
  for (int64_t b = 0; b <= n_bands; ++b)
    off[(size_t)b] = b == n_bands ? (int64_t)col.size()
                                  : std::lower_bound(col.begin(), col.end(), b * band_rows, [](int32_t c, int64_t v) { return (int64_t)c < v; }) - col.begin();
  return off;
}

static bool same(const BandPiece& a, const BandPiece& b) { return a.begin == b.begin && a.len == b.len && a.band == b.band; }

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 1u;
  const int n_rows = argc > 2 ? std::atoi(argv[2]) : 2000;
  std::mt19937_64 rng(seed);
  std::vector<BandPiece> shared;   // every row's pieces, one behind the other
  int64_t n_pieces = 0, n_carried = 0;
  for (int it = 0; it < n_rows; ++it) {
    const int64_t n_bands = 2 + (int64_t)(rng() % 40);
    const int64_t band_rows = 1 + (int64_t)(rng() % 300);
    const int64_t n_cols = n_bands * band_rows - (int64_t)(rng() % band_rows);  // the last band may be short
    const int64_t seg = 1 + (int64_t)(rng() % 200);
    // a row: every column with probability p inside a random window of the table, so that bands are empty, thin or full;
    // every fourth row with repeated columns (ascending, not strictly)
    std::vector<int32_t> col;
    const int64_t w0 = (int64_t)(rng() % (uint64_t)n_cols), w1 = w0 + 1 + (int64_t)(rng() % (uint64_t)(n_cols - w0));
    const double p = (double)(1 + rng() % 100) / 100.0;
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (int64_t c = (it % 3 == 0 ? 0 : w0); c < (it % 3 == 0 ? n_cols : w1); ++c) {
      const bool thin = it % 5 == 0 && (c / band_rows) % 2 == 1;   // every other band nearly empty
      if (u(rng) < (thin ? p / 50.0 : p)) {
        col.push_back((int32_t)c);
        if (it % 4 == 0 && u(rng) < 0.1) col.push_back((int32_t)c);
      }
    }
    const int64_t len = (int64_t)col.size();
    if (len == 0) continue;
    const std::vector<int64_t> off = offsets(col, n_bands, band_rows);
    std::vector<BandPiece> alone;
    const bool ok = mals::band_plan_row(off.data(), n_bands, len, seg, alone);
    CHECK(ok, "row %d refused", it);
    if (!ok) continue;
    const size_t before = shared.size();
    CHECK(mals::band_plan_row(off.data(), n_bands, len, seg, shared), "row %d refused the second time", it);
    CHECK(shared.size() - before == alone.size(), "row %d: %zu pieces alone, %zu behind other rows", it, alone.size(), shared.size() - before);
    for (size_t i = 0; i < alone.size() && before + i < shared.size(); ++i)
      CHECK(same(alone[i], shared[before + i]), "row %d piece %zu differs behind other rows", it, i);
    const int64_t min_piece = mals::band_min_piece(len, n_bands);
    int64_t at = 0;
    int32_t last_band = -1;
    for (size_t i = 0; i < alone.size(); ++i) {
      const BandPiece& pc = alone[i];
      CHECK(pc.begin == at, "row %d piece %zu begins at %lld, expected %lld", it, i, (long long)pc.begin, (long long)at);
      CHECK(pc.len >= 1 && pc.len <= seg, "row %d piece %zu has %d entries (segment_nnz %lld)", it, i, pc.len, (long long)seg);
      CHECK(pc.band >= last_band && pc.band < n_bands, "row %d piece %zu band %d after %d", it, i, pc.band, last_band);
      last_band = pc.band;
      if (pc.len < 1) break;
      const int64_t lo = (int64_t)pc.band * band_rows, hi = lo + band_rows;
      int64_t before_band = 0;
      for (int64_t e = pc.begin; e < pc.begin + pc.len && e < len; ++e) {
        CHECK(col[(size_t)e] < hi, "row %d piece %zu (band %d) holds column %d of a later band", it, i, pc.band, col[(size_t)e]);
        before_band += col[(size_t)e] < lo;
      }
      CHECK(before_band == 0 || before_band < min_piece, "row %d piece %zu (band %d) holds %lld entries of earlier bands, limit %lld", it, i,
            pc.band, (long long)before_band, (long long)min_piece);
      n_carried += before_band > 0;
      at += pc.len;
    }
    CHECK(at == len, "row %d: pieces cover %lld of %lld entries", it, (long long)at, (long long)len);
    const int64_t by_count = (len + seg - 1) / seg;
    CHECK((int64_t)alone.size() <= by_count + n_bands, "row %d: %zu pieces, %lld by count, %lld bands", it, alone.size(), (long long)by_count,
          (long long)n_bands);
    n_pieces += (int64_t)alone.size();
  }
  // what the planner must refuse: offsets that are no cut positions
  {
    std::vector<BandPiece> out;
    const int64_t bad1[] = {0, 5, 3, 10}, bad2[] = {1, 5, 7, 10}, bad3[] = {0, 5, 7, 9};
    CHECK(!mals::band_plan_row(bad1, 3, 10, 4, out) && out.empty(), "descending offsets accepted");
    CHECK(!mals::band_plan_row(bad2, 3, 10, 4, out) && out.empty(), "offsets that do not start at 0 accepted");
    CHECK(!mals::band_plan_row(bad3, 3, 10, 4, out) && out.empty(), "offsets that do not end at len accepted");
  }
  // the length rule and its constant at the flagship shape (k = 64: slots of (10 * 4 + 4) * 64 floats)
  CHECK(mals::band_min_avg(2816, 64) == 854, "min_avg %lld", (long long)mals::band_min_avg(2816, 64));
  CHECK(!mals::band_row_eligible(100000, 4096, 1, 854), "one band is never banded");
  CHECK(!mals::band_row_eligible(4096, 4096, 2, 1), "a row of segment_nnz entries is not long");
  CHECK(mals::band_row_eligible(854 * 40, 4096, 40, 854) && !mals::band_row_eligible(854 * 40 - 1, 4096, 40, 854), "length rule");
  std::printf("rows %d pieces %lld carried %lld failures %d\n", n_rows, (long long)n_pieces, (long long)n_carried, failures);
  return failures ? 1 : 0;
}
