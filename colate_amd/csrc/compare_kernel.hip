// colate_amd/csrc/compare_kernel.hip -- `Colate --mode compare_tmp --samples` on the GPU (compare_tmp.h: the contract;
// compare_tmp.cpp: the host twin): the two kernels of the pair stage and the host code that drives them over the resident
// inputs of the pair walks (walk_resident.hpp).
//
//   * compare_planes_kernel: one lane per (sample, searched row).  A wave holds the 64 rows of one plane word of one
//     sample: each lane reads idx[s][i] and the position of the row in front (-1 at a chromosome's first row), forms the two
//     predicates, and two ballots -- 64 bits on wave64 -- are the words of `hit` and `fixed & hit`, which lane 0 writes to
//     planes[S][2][words] in HBM.  Every chromosome starts on a word, so a word never holds rows of two chromosomes; lanes
//     beyond the chromosome's end hold "no".
//   * compare_pairs_kernel: one workgroup per (pair, chromosome).  Wave k takes the windows k, k + 4, ... of the chromosome;
//     its lanes stride over the words of the window's row range, the first and the last word masked to the range; the two
//     popcounts are reduced over the wave by shuffles and lane 0 writes mismatch[p][w] and snps[p][w].  Every output has one
//     owner; a workgroup reads nothing another workgroup of the same launch writes.
// No atomics, no floating point, no LDS, no barrier.  The window row ranges come from the host (window_rows), once per call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "compare_tmp.h"
#include "em_job.hpp"
#include "walk_resident.hpp"

using namespace colate;
using namespace colate_cmp;
using colate_iw::DeviceInputs;

namespace {

__global__ __launch_bounds__(kPlaneTile) void compare_planes_kernel(DeviceInputs in, unsigned long long* __restrict__ planes) {
  const int lane = threadIdx.x & 63;
  const long long gw = (long long)blockIdx.x * (kPlaneTile / 64) + (threadIdx.x >> 6);  // the word: alike in the whole wave
  if (gw >= in.words) return;
  const int s = blockIdx.y;
  int c = 0;
  while (c + 1 < in.C && in.word_off[c + 1] <= gw) c++;  // (the chromosome of the word; empty chromosomes own no word)
  const long long r0 = in.row_off[c];
  const long long i = (gw - in.word_off[c]) * 64 + lane, n = in.row_off[c + 1] - r0;
  bool hit = false, fix = false;
  if (i < n) {
    const Idx x = in.idx[(size_t)s * in.n + r0 + i];
    hit = hits(x, i == 0 ? -1 : in.rows[r0 + i - 1].pos);
    fix = hit && fixed(x);
  }
  const unsigned long long h = __ballot(hit), f = __ballot(fix);
  if (lane == 0) {
    planes[(size_t)s * 2 * in.words + gw] = h;
    planes[((size_t)s * 2 + 1) * in.words + gw] = f;
  }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(kPairWaves * 64) void compare_pairs_kernel(DeviceInputs in, int p0, const unsigned long long* __restrict__ planes,
                                                                        const long long* __restrict__ win_off, const int* __restrict__ win_row,
                                                                        int* __restrict__ mismatch, int* __restrict__ snps) {
  const int c = blockIdx.x % in.C, j = blockIdx.x / in.C;  // (pair p0 + j, chromosome c)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const colate_iw::Pair pr = in.pairs[p0 + j];
  const long long w0 = in.word_off[c], Wt = win_off[in.C], o0 = win_off[c];
  const int W = (int)(win_off[c + 1] - o0);
  const int* const b = win_row + o0 + c;
  const unsigned long long* const hT = planes + (size_t)pr.target * 2 * in.words + w0;
  const unsigned long long* const hR = planes + (size_t)pr.reference * 2 * in.words + w0;
  const unsigned long long* const fT = hT + in.words;
  const unsigned long long* const fR = hR + in.words;
  for (int w = wave; w < W; w += kPairWaves) {
    const long long r0 = b[w], r1 = b[w + 1];
    int n = 0, mm = 0;
    if (r1 > r0)
      for (long long k = (r0 >> 6) + lane; k <= (r1 - 1) >> 6; k += 64) {
        const unsigned long long both = hT[k] & hR[k] & range_bits(k, r0, r1);
        n += __popcll(both);
        mm += __popcll(both & (fT[k] ^ fR[k]));
      }
    n = wave_sum(n), mm = wave_sum(mm);
    if (lane == 0) {
      const size_t at = (size_t)j * (size_t)Wt + (size_t)(o0 + w);
      mismatch[at] = mm, snps[at] = n;
    }
  }
}

thread_local int g_chunks = 0;
thread_local double g_kernel_s = 0.0;

// bytes of the two output arrays a chunk of pairs may take on the device (COLATE_COMPARE_BUDGET: bytes, for the tests)
long long output_budget() {
  if (const char* e = std::getenv("COLATE_COMPARE_BUDGET")) return std::max(1LL, std::atoll(e));
  return 256LL << 20;
}

}  // namespace

namespace colate_cmp {

hipError_t planes_launch(const DeviceInputs& in, unsigned long long* planes, hipStream_t stream) {
  if (in.words < 1 || in.S < 1) return hipSuccess;
  const long long blocks = (in.words + kPlaneTile / 64 - 1) / (kPlaneTile / 64);
  if (blocks > 0x7fffffffLL || in.S > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(compare_planes_kernel, dim3((unsigned)blocks, (unsigned)in.S), dim3(kPlaneTile), 0, stream, in, planes);
  return hipGetLastError();
}

hipError_t pairs_launch(const DeviceInputs& in, int p0, int p1, const unsigned long long* planes, const long long* win_off,
                        const int* win_row, int* mismatch, int* snps, hipStream_t stream) {
  if (p1 <= p0 || in.C < 1) return hipSuccess;
  const long long grid = (long long)(p1 - p0) * in.C;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(compare_pairs_kernel, dim3((unsigned)grid), dim3(kPairWaves * 64), 0, stream, in, p0, planes, win_off, win_row, mismatch,
                     snps);
  return hipGetLastError();
}

int compare_view_device(const View& v, long long cap, long long* win_off, int* mismatch, int* snps) {
  if (int rc = check_outputs(cap, win_off, mismatch, snps)) return rc;
  if (int rc = check_view(v)) return rc;
  if (v.S > 65535) return fail(COLATE_ELIMIT, "S=%d above the grid of the plane kernel (65535)", v.S);
  std::vector<long long> woff;
  std::vector<int> win_row;
  window_rows(v, woff, win_row);
  const long long Wt = woff[(size_t)v.C];
  if (int rc = check_capacity(v.P, Wt, cap)) return rc;
  if (int rc = ensure_device()) return rc;
  ProfRange range("colate_compare_samples: H2D + planes; per chunk of pairs the window popcounts + D2H");
  g_chunks = 0, g_kernel_s = 0.0;
  if (int rc = thread_workspace().reserve(256, 256)) return rc;  // (the workspace's stream: no second one)
  hipStream_t stream = thread_workspace().stream;
  colate_iw::KernelTimer timer(stream);
  colate_iw::Resident res;
  DeviceBuffers buf;
  const colate_iw::StreamSync sync_at_exit{stream};
  colate_iw::View iv;
  iv.C = v.C, iv.row_off = v.row_off, iv.rows = v.rows, iv.S = v.S, iv.idx = v.idx, iv.M = 0, iv.P = v.P, iv.pairs = v.pairs, iv.nbpb = 1;
  if (int rc = res.upload(iv, stream)) return rc;
  // pairs per chunk: the two output arrays of a chunk within the budget, and the grid within 2^31 workgroups
  const long long per_pair = std::max(1LL, 2 * Wt * (long long)sizeof(int));
  const long long chunk = std::max(1LL, std::min<long long>({(long long)v.P, output_budget() / per_pair, 0x7fffffffLL / v.C}));
  unsigned long long* d_planes = nullptr;
  long long* d_win_off = nullptr;
  int *d_win_row = nullptr, *d_mm = nullptr, *d_n = nullptr;
  HIP_TRY(buf.device(d_planes, (size_t)v.S * 2 * (size_t)res.in.words)); HIP_TRY(buf.device(d_win_off, woff.size()));
  HIP_TRY(buf.device(d_win_row, win_row.size())); HIP_TRY(buf.device(d_mm, (size_t)(chunk * Wt))); HIP_TRY(buf.device(d_n, (size_t)(chunk * Wt)));
  HIP_TRY(colate_iw::h2d(stream, d_win_off, woff.data(), sizeof(long long) * woff.size()));
  HIP_TRY(colate_iw::h2d(stream, d_win_row, win_row.data(), sizeof(int) * win_row.size()));
  HIP_TRY(timer.mark());
  if (hipError_t e = planes_launch(res.in, d_planes, stream)) return hip_fail(e, "compare planes kernel launch");
  HIP_TRY(timer.mark());
  for (long long p0 = 0; p0 < v.P; p0 += chunk) {  // (a chunk's outputs are copied out before the next launch overwrites them: one stream)
    const long long p1 = std::min<long long>(v.P, p0 + chunk);
    HIP_TRY(timer.mark());
    if (hipError_t e = pairs_launch(res.in, (int)p0, (int)p1, d_planes, d_win_off, d_win_row, d_mm, d_n, stream))
      return hip_fail(e, "compare pairs kernel launch");
    HIP_TRY(timer.mark());
    const size_t bytes = sizeof(int) * (size_t)((p1 - p0) * Wt);
    HIP_TRY(hipMemcpyAsync(mismatch + p0 * Wt, d_mm, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(snps + p0 * Wt, d_n, bytes, hipMemcpyDeviceToHost, stream));
    g_chunks++;
  }
  HIP_TRY(hipStreamSynchronize(stream));  // the one host wait
  g_kernel_s = timer.seconds();
  std::memcpy(win_off, woff.data(), sizeof(long long) * woff.size());
  return COLATE_OK;
}

}  // namespace colate_cmp

extern "C" {
int colate_compare_samples_chunks(void) { return g_chunks; }
double colate_compare_samples_kernel_seconds(void) { return g_kernel_s; }
}
