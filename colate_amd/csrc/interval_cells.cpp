// colate_amd/csrc/interval_cells.cpp -- the host side of the interval cells (interval_cells.h): the threshold table, the
// argument checks, the host twin of interval_cells_kernel.hip (one pass over the records, two counted searches and two
// additions per SNP), and the step from the dense per-block cell sums to rows, which the device call shares.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "interval_cells.h"
#include "age_bins.hpp"

using colate::fail;

namespace colate_ic {

namespace {
inline float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, sizeof(f));
  return f;
}
inline int bin_libm(float x) { return colate_drv::age_bin_index((double)x, 10.0); }  // (the ages are floats, widened as the walk widens them)
}  // namespace

int build_thresholds(float* T) {
  const uint32_t top = 0x7f7fffffu;  // the largest finite float
  for (int n = 1; n <= kBins; n++) {
    uint32_t a = 0, b = top;  // bin(a) < n <= bin(b): 0.0 is in bin 0, the largest float far beyond the grid
    if (!(bin_libm(from_bits(a)) < n && bin_libm(from_bits(b)) >= n)) return fail(COLATE_EINVAL, "age bins: no bracket for step %d", n);
    while (b - a > 1) {
      const uint32_t mid = a + (b - a) / 2;
      if (bin_libm(from_bits(mid)) >= n) b = mid; else a = mid;
    }
    T[n - 1] = from_bits(b);
    // the two neighbouring floats: one below still in front of the step, one above behind it; and the step is one bin high
    if (bin_libm(from_bits(b - 1)) != n - 1 || bin_libm(from_bits(b)) != n || bin_libm(from_bits(b + 1)) < n)
      return fail(COLATE_EINVAL, "age bins: step %d of the library expression is not a single step at %.9g", n, (double)T[n - 1]);
    if (n > 1 && !(T[n - 2] < T[n - 1])) return fail(COLATE_EINVAL, "age bins: steps %d and %d coincide", n - 1, n);
  }
  return COLATE_OK;
}

int check_cells_args(long long n, const IntervalRec* recs, const int* block, int nb, int max_rows, const int* kinds,
                     const double* age_begin, const double* age_end, const double* tables, const long long* dropped) {
  if (n < 0 || nb < 1 || max_rows < 0) return fail(COLATE_EINVAL, "bad sizes n=%lld nb=%d max_rows=%d", n, nb, max_rows);
  if (nb > COLATE_INTERVAL_MAX_BLOCKS) return fail(COLATE_ELIMIT, "nb=%d above %d genome blocks", nb, COLATE_INTERVAL_MAX_BLOCKS);
  if ((n > 0 && (!recs || !block)) || !dropped || (max_rows > 0 && (!kinds || !age_begin || !age_end || !tables)))
    return fail(COLATE_EINVAL, "NULL pointer argument");
  const double dmax = std::numeric_limits<double>::max();
  for (long long i = 0; i < n; i++) {
    const IntervalRec& r = recs[i];
    if (!(r.begin >= 0.0f) || !(r.end >= 0.0f)) return fail(COLATE_EINVAL, "record %lld: negative age or not a number", i);
    if (!(r.begin <= r.end)) return fail(COLATE_EINVAL, "record %lld: begin %.9g > end %.9g", i, (double)r.begin, (double)r.end);
    if (!(r.w_sh >= 0.0) || !(r.w_sh <= dmax) || !(r.w_ns >= 0.0) || !(r.w_ns <= dmax))
      return fail(COLATE_EINVAL, "record %lld: the weights must be finite and not negative", i);
    if (block[i] < 0 || block[i] >= nb) return fail(COLATE_EINVAL, "record %lld: block %d outside [0, %d)", i, block[i], nb);
    if (i > 0 && block[i] < block[i - 1]) return fail(COLATE_EINVAL, "record %lld: block indices out of order (%d after %d)", i, block[i], block[i - 1]);
  }
  return COLATE_OK;
}

void block_ranges(long long n, const int* block, int nb, long long* off) {
  long long i = 0;
  for (int k = 0; k < nb; k++) {
    off[k] = i;
    while (i < n && block[i] == k) i++;
  }
  off[nb] = n;
}

void host_cells(long long n, const IntervalRec* recs, const long long* off, int nb, const float* T, double* cells,
                long long* dropped_per_block) {
  std::memset(cells, 0, sizeof(double) * (size_t)nb * 2 * kCells);
  for (int k = 0; k < nb; k++) {
    double* const sh = cells + (size_t)k * 2 * kCells;
    double* const ns = sh + kCells;
    long long nd = 0;
    for (long long i = off[k]; i < off[k + 1]; i++) {
      const int c = cell_of(T, recs[i].begin, recs[i].end);
      if (c == kDropped) {
        nd++;
        continue;
      }
      sh[c] += recs[i].w_sh;
      ns[c] += recs[i].w_ns;
    }
    dropped_per_block[k] = nd;
  }
  (void)n;
}

int compact_cells(int nb, const double* cells, int max_rows, int* kinds, double* age_begin, double* age_end, double* tables) {
  std::vector<int> rows;  // kind * kCells + triangular index, in row order: kind, bb, be
  for (int kind = 0; kind < 2; kind++)
    for (int bb = 0; bb < kBins; bb++)
      for (int be = bb; be < kBins; be++) {
        const int c = kind * kCells + be * (be + 1) / 2 + bb;
        bool any = false;
        for (int k = 0; k < nb && !any; k++) any = cells[(size_t)k * 2 * kCells + c] > 0.0;
        if (any) rows.push_back(c);
      }
  const int R = (int)rows.size();
  if (R > max_rows) return fail(COLATE_EINVAL, "%d rows, room for %d", R, max_rows);
  double grid[COLATE_MAX_AGE_BINS];
  if (colate_age_grid(grid, COLATE_MAX_AGE_BINS) != kBins) return fail(COLATE_EINVAL, "the age grid has not %d points", kBins);
  for (int r = 0; r < R; r++) {
    const int c = rows[r] % kCells;
    int be = 0;
    while ((be + 1) * (be + 2) / 2 <= c) be++;
    const int bb = c - be * (be + 1) / 2;
    kinds[r] = rows[r] / kCells, age_begin[r] = grid[bb], age_end[r] = grid[be];
    for (int k = 0; k < nb; k++) tables[(size_t)k * R + r] = cells[(size_t)k * 2 * kCells + rows[r]];
  }
  return R;
}

}  // namespace colate_ic

using namespace colate_ic;

extern "C" {

int colate_interval_bin_thresholds(float* T185) {
  if (!T185) return fail(COLATE_EINVAL, "NULL pointer argument");
  float T[kBins];
  if (int rc = build_thresholds(T)) return rc;
  std::memcpy(T185, T, sizeof(T));
  return COLATE_OK;
}

int colate_interval_cells_tile(void) { return kTile; }

int colate_interval_cells_host(long long n, const colate_interval_rec* recs, const int* block, int nb, int max_rows, int* kinds,
                               double* age_begin, double* age_end, double* tables, long long* dropped) {
  if (int rc = check_cells_args(n, recs, block, nb, max_rows, kinds, age_begin, age_end, tables, dropped)) return rc;
  float T[kBins];
  if (int rc = build_thresholds(T)) return rc;
  std::vector<long long> off((size_t)nb + 1), nd((size_t)nb);
  block_ranges(n, block, nb, off.data());
  std::vector<double> cells((size_t)nb * 2 * kCells);
  host_cells(n, recs, off.data(), nb, T, cells.data(), nd.data());
  const int R = compact_cells(nb, cells.data(), max_rows, kinds, age_begin, age_end, tables);
  if (R < 0) return R;
  long long total = 0;
  for (long long d : nd) total += d;
  *dropped = total;
  return R;
}

}  // extern "C"
