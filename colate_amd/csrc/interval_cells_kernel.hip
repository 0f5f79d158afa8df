// colate_amd/csrc/interval_cells_kernel.hip -- the used SNPs of one pair summed into the cells of the interval-dated fit
// on the GPU (interval_cells.h: what a cell is, the threshold table, and the summation contract).
//
// Two kernels, back to back on one stream:
//   * interval_cells_bin_kernel: a thread per record; the 185 thresholds sit in LDS, two counted searches give the
//     record's cell index (an integer: nothing here depends on order);
//   * interval_cells_sum_kernel: ONE wave per (genome block, tile of kTile cells of the triangle).  It keeps its tile's
//     sums of both kinds in LDS (16 KB) and scans the block's cell indices 64 records at a time, lane l holding record
//     base + l.  Records of a batch that fall into the same cell must be added in lane order: every such lane gets its
//     rank among the lanes of its cell (ballots: integers, one round per distinct cell of the batch), and round r adds the
//     lanes of rank r -- at most one lane per cell and round, so a round is a plain read-add-write of LDS, and a cell's
//     running sum goes from a lane to the next one through LDS with a barrier between the rounds.  Batches follow each
//     other in record order, so every cell's chain is the contract's: from 0.0, record after record, each addition rounded.
//     No floating-point atomics, no partial sums.  The workgroup is one wave and every branch around a barrier is taken on
//     a ballot or on the loop counters, which all lanes share: every barrier is reached by the whole workgroup.
//     The tile goes to global memory once, at the end; nothing written here is read back by this launch.
#include <hip/hip_runtime.h>

#include "interval_cells.h"

using namespace colate_ic;

namespace {

__global__ __launch_bounds__(256) void interval_cells_bin_kernel(long long n, const IntervalRec* __restrict__ recs,
                                                                 const float* __restrict__ T, int* __restrict__ cell_idx) {
  __shared__ float sT[kBins];
  for (int i = threadIdx.x; i < kBins; i += blockDim.x) sT[i] = T[i];
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) cell_idx[i] = cell_of(sT, recs[i].begin, recs[i].end);
}

__global__ __launch_bounds__(64) void interval_cells_sum_kernel(const IntervalRec* __restrict__ recs,
                                                                const long long* __restrict__ off,
                                                                const int* __restrict__ cell_idx, double* __restrict__ cells,
                                                                unsigned long long* __restrict__ dropped) {
  __shared__ double s_sh[kTile], s_ns[kTile];
  const int lane = threadIdx.x;
  const int blk = blockIdx.x / kTiles, tile = blockIdx.x % kTiles;
  const int lo = tile * kTile, hi = min(lo + kTile, kCells);
  for (int i = lane; i < kTile; i += 64) s_sh[i] = 0.0, s_ns[i] = 0.0;
  __syncthreads();
  const long long r0 = off[blk], r1 = off[blk + 1];
  const unsigned long long below = (1ull << lane) - 1ull;  // the lanes in front of this one
  unsigned long long ndrop = 0;
  for (long long base = r0; base < r1; base += 64) {
    const long long i = base + lane;
    const int c = i < r1 ? cell_idx[i] : -2;  // (-2: no record)
    if (tile == 0) ndrop += (unsigned long long)__popcll(__ballot(c == kDropped));
    const bool mine = c >= lo && c < hi;
    unsigned long long left = __ballot(mine);
    if (left == 0) continue;
    double w_sh = 0.0, w_ns = 0.0;
    if (mine) w_sh = recs[i].w_sh, w_ns = recs[i].w_ns;
    int rank = 0, rounds = 0;
    while (left != 0) {  // one turn per distinct cell of the batch
      const int j = __ffsll((long long)left) - 1;
      const int cj = __shfl(c, j);
      const bool same_cell = mine && c == cj;
      const unsigned long long same = __ballot(same_cell);  // (lane j is in it: the loop ends)
      if (same_cell) rank = __popcll(same & below);
      rounds = max(rounds, (int)__popcll(same));
      left &= ~same;
    }
    for (int r = 0; r < rounds; r++) {
      if (mine && rank == r) {
        s_sh[c - lo] += w_sh;
        s_ns[c - lo] += w_ns;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  double* const out = cells + (size_t)blk * 2 * kCells;
  for (int i = lane; i < hi - lo; i += 64) out[lo + i] = s_sh[i], out[kCells + lo + i] = s_ns[i];
  if (tile == 0 && lane == 0) dropped[blk] = ndrop;
}

}  // namespace

hipError_t colate_interval_cells_launch(long long n, const IntervalRec* recs, const long long* off, int nb, const float* T,
                                        int* cell_idx, double* cells, unsigned long long* dropped, hipStream_t stream) {
  if (n > 0) {
    const long long grid = (n + 255) / 256;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(interval_cells_bin_kernel, dim3((unsigned)grid), dim3(256), 0, stream, n, recs, T, cell_idx);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if ((long long)nb * kTiles > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(interval_cells_sum_kernel, dim3((unsigned)(nb * kTiles)), dim3(64), 0, stream, recs, off, cell_idx, cells,
                     dropped);
  return hipGetLastError();
}
