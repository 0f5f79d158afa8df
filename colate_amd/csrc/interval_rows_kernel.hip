// colate_amd/csrc/interval_rows_kernel.hip -- from the dense cell sums of many groups to each group's rows, on the GPU
// (colate_interval_fit_groups; interval_cells.h: what a cell is; interval_cells.cpp, compact_cells: the host's row pick).
//
// A row of a group is a cell (kind, bb, be) whose sum is positive in at least one of the group's genome blocks; the rows
// are ordered by kind, bb, be.  The dense sums are stored per kind in the triangular order be * (be + 1) / 2 + bb, which
// is another order, so position and cell are mapped explicitly.  Two kernels, back to back on one stream:
//   * interval_rows_flag_kernel: a thread per (group, cell of both kinds) reads the cell in all the group's blocks --
//     consecutive threads read consecutive doubles -- and writes one byte: positive somewhere or not;
//   * interval_rows_rank_kernel: ONE workgroup per group walks the 2 * 185 lines (kind, bb) of the row order, lane t of a
//     line holding the cell be = bb + t.  The rank of a flagged cell is the number of flagged cells in front of it: those
//     of earlier lines (a running count that every thread keeps alike), of earlier waves of its line (wave totals through
//     LDS) and of earlier lanes of its wave (a ballot and a popcount).  Integers only: the order is exact by construction.
//     The thread of a flagged cell writes the row: its cell index, its kind and its two ages from the age grid.
// Control flow of the rank kernel: the loop runs over the 370 lines, which every thread counts alike; the one barrier of a
// line is reached by every wave; ballots are taken with all 64 lanes of every wave active (a lane beyond the line's end
// holds "not flagged").  The wave totals alternate between two LDS buffers, so a line's totals are not overwritten
// before every wave has passed the next line's barrier.
#include <hip/hip_runtime.h>

#include "em_kernels.h"
#include "interval_cells.h"

using namespace colate_ic;

namespace {

constexpr int kFlagThreads = 256;
constexpr int kRankWaves = 4;  // 256 lanes >= the 185 cells of the longest line
static_assert(kRankWaves * 64 >= kBins, "a line of the row order fits one pass of the workgroup");

__global__ __launch_bounds__(kFlagThreads) void interval_rows_flag_kernel(const double* __restrict__ cells,
                                                                          const int* __restrict__ seg_off,
                                                                          unsigned char* __restrict__ flags) {
  const int g = blockIdx.y;
  const int c = blockIdx.x * kFlagThreads + threadIdx.x;  // kind * kCells + triangular index
  if (c >= 2 * kCells) return;
  const int s0 = seg_off[g], s1 = seg_off[g + 1];
  bool any = false;
  for (int s = s0; s < s1; s++) any = any || cells[(size_t)s * 2 * kCells + c] > 0.0;
  flags[(size_t)g * 2 * kCells + c] = any ? 1 : 0;
}

__global__ __launch_bounds__(kRankWaves * 64) void interval_rows_rank_kernel(
    const unsigned char* __restrict__ flags, const int* __restrict__ seg_off, const unsigned long long* __restrict__ seg_dropped,
    const double* __restrict__ age_grid, const long long* __restrict__ row_off, const int* __restrict__ row_cap,
    int* __restrict__ cell_of_row, int* __restrict__ kinds, double* __restrict__ age_begin, double* __restrict__ age_end,
    int* __restrict__ R, long long* __restrict__ dropped) {
  __shared__ int s_total[2][kRankWaves];
  __shared__ double s_grid[kBins];
  const int g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned char* const f = flags + (size_t)g * 2 * kCells;
  const long long base = row_off[g];
  const int cap = row_cap[g];
  const unsigned long long below = (1ull << lane) - 1ull;  // the lanes in front of this one
  for (int i = tid; i < kBins; i += kRankWaves * 64) s_grid[i] = age_grid[i];
  __syncthreads();
  int count = 0;  // rows of the lines in front of this one (the same in every thread)
  for (int line = 0; line < 2 * kBins; line++) {
    const int kind = line / kBins, bb = line % kBins;
    const int be = bb + tid;
    const int c = kind * kCells + be * (be + 1) / 2 + bb;
    const bool flagged = be < kBins && f[c] != 0;
    const unsigned long long mask = __ballot(flagged);
    if (lane == 0) s_total[line & 1][wave] = __popcll(mask);
    __syncthreads();
    int in_front = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kRankWaves; w++) {
      const int t = s_total[line & 1][w];
      in_front += w < wave ? t : 0;
      total += t;
    }
    const int r = count + in_front + __popcll(mask & below);
    if (flagged && r < cap) {  // (r < cap always: a record flags at most one cell of each kind, and cap covers that)
      cell_of_row[base + r] = c;
      kinds[base + r] = kind;
      age_begin[base + r] = s_grid[bb];
      age_end[base + r] = s_grid[be];
    }
    count += total;
  }
  if (tid == 0) {
    R[g] = count;
    unsigned long long nd = 0;
    for (int s = seg_off[g]; s < seg_off[g + 1]; s++) nd += seg_dropped[s];
    dropped[g] = (long long)nd;
  }
}

}  // namespace

hipError_t colate_interval_rows_launch(int groups, const double* cells, const int* seg_off, const unsigned long long* seg_dropped,
                                       const double* age_grid, const long long* row_off, const int* row_cap,
                                       unsigned char* flags, int* cell_of_row, int* kinds, double* age_begin, double* age_end,
                                       int* R, long long* dropped, hipStream_t stream) {
  if (groups < 1 || groups > 65535) return hipErrorInvalidValue;  // (gridDim.y of the flag kernel)
  const unsigned tiles = (2 * kCells + kFlagThreads - 1) / kFlagThreads;
  hipLaunchKernelGGL(interval_rows_flag_kernel, dim3(tiles, (unsigned)groups), dim3(kFlagThreads), 0, stream, cells, seg_off, flags);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(interval_rows_rank_kernel, dim3((unsigned)groups), dim3(kRankWaves * 64), 0, stream, flags, seg_off,
                     seg_dropped, age_grid, row_off, row_cap, cell_of_row, kinds, age_begin, age_end, R, dropped);
  return hipGetLastError();
}
