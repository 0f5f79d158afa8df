// colate_amd/csrc/interval_cells.h -- what a used SNP becomes for the interval-dated fit (internal to libcolate_amd.so).
//
// `Colate --mode mut` follows coal.cpp:2245-2297: every SNP a pair uses spreads its weight over 100 ages drawn uniformly
// between the mutation's lower and upper age.  The interval fit (colate_bootstrap_em_interval_batch) treats that uniform
// distribution exactly, so here a used SNP is ONE observation of each kind and nothing is drawn:
//   * its ages are snapped to the 185-point age grid: bb = bin(age_begin), be = bin(age_end), bin = age_bin_index(x, 10)
//     (age_bins.hpp) on the float ages as the walk holds them; the cell (kind, bb, be), bb <= be, is the row
//     [age_bin[bb], age_bin[be]] of that kind; be >= 185 drops the SNP (counted);
//   * bin() is a step function of a float: T[n], n = 1 .. 185, is the smallest float whose age_bin_index is >= n (located
//     once on the host by bisection over float bit patterns on the library expression itself, checked at both neighbours),
//     and bin(x) = #{n : T[n] <= x}.  Host twin and kernel count against the same table: no log on the device, no guard
//     band, nothing handed back;
//   * THE SUMMATION CONTRACT: for every (genome block, kind, bb, be) the sum starts at 0.0 and adds the SNPs' weights in
//     the order of the records (the walk's: chromosome, then file order), every addition rounded.  No floating-point
//     atomics, no partial sums combined in another order -- on the device (interval_cells_kernel.hip) as on the host
//     (interval_cells.cpp), like the W[b][r] contract of bootstrap_kernel.hip.
#pragma once
#include <cstddef>
#include <cstdint>

#include "colate_amd.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COLATE_IC_HD __host__ __device__
#else
#define COLATE_IC_HD
#endif

namespace colate_ic {

using IntervalRec = colate_interval_rec;  // {float begin, end; double w_sh, w_ns}: one used SNP
static_assert(sizeof(IntervalRec) == 24, "IntervalRec");

constexpr int kBins = COLATE_INTERVAL_BINS;         // points of the age grid (colate_age_grid)
constexpr int kCells = kBins * (kBins + 1) / 2;     // (bb, be) with bb <= be: 17205 per kind
constexpr int kTile = 1024;                         // cells of the triangle one workgroup keeps in LDS (x 2 kinds x 8 B = 16 KB)
constexpr int kTiles = (kCells + kTile - 1) / kTile;
constexpr int kDropped = -1;                        // cell index of a record beyond the age grid

// #{n in 1 .. kBins : T[n - 1] <= x}: the age bin of x, with every value beyond the grid returned as kBins
COLATE_IC_HD inline int bin_of(const float* T, float x) {
  int n = 0;
  for (int step = 128; step > 0; step >>= 1)
    if (n + step <= kBins && T[n + step - 1] <= x) n += step;
  return n;
}
// the triangular index of the cell (bb, be), bb <= be < kBins; kDropped for be >= kBins
COLATE_IC_HD inline int cell_of(const float* T, float begin, float end) {
  const int be = bin_of(T, end);
  if (be >= kBins) return kDropped;
  return be * (be + 1) / 2 + bin_of(T, begin);
}

// T[0 .. kBins): T[n - 1] = the smallest float x with age_bin_index(x, 10) >= n.  COLATE_OK, or COLATE_EINVAL where the
// library expression is not the step function the bisection assumes (a threshold fails at one of its two neighbours).
int build_thresholds(float* T);

// What both cells calls refuse before anything is staged (COLATE_EINVAL; message in colate_last_error()).
int check_cells_args(long long n, const IntervalRec* recs, const int* block, int nb, int max_rows, const int* kinds,
                     const double* age_begin, const double* age_end, const double* tables, const long long* dropped);

// off[0 .. nb]: records [off[k], off[k + 1]) belong to block k (block[] does not decrease)
void block_ranges(long long n, const int* block, int nb, long long* off);

// From the dense per-block sums cells[nb][2][kCells] to rows: those with a positive sum in at least one block, ordered by
// kind, bb, be.  Returns R, or COLATE_EINVAL (nothing written) where R exceeds max_rows.
int compact_cells(int nb, const double* cells, int max_rows, int* kinds, double* age_begin, double* age_end, double* tables);

// the host twin's single pass: cells[nb][2][kCells] (zeroed here), dropped_per_block[nb]
void host_cells(long long n, const IntervalRec* recs, const long long* off, int nb, const float* T, double* cells,
                long long* dropped_per_block);

}  // namespace colate_ic

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
// Device pointers; recs[n], off[nb + 1], T[kBins]; cell_idx[n] is scratch; cells[nb][2][kCells] and dropped[nb] are
// written in full.  Two kernels on `stream`: one thread per record bins it, then one wave per (block, tile) sums.
hipError_t colate_interval_cells_launch(long long n, const colate_ic::IntervalRec* recs, const long long* off, int nb,
                                        const float* T, int* cell_idx, double* cells, unsigned long long* dropped,
                                        hipStream_t stream);
#endif
