// colate_amd/csrc/fill_samples_kernel.hip -- the table fill of `Colate --mode mut --samples` on the GPU (fill_samples.h: the
// contract; fill_samples.cpp: the host twin): the two kernels this path adds and the host code that drives it.
//
// Per chunk of pairs, on one stream: the write pass of the pair walk (interval_walk_kernel.hip, its FillRec form) leaves the
// chunk's records, their side array and the per-(pair, block) record ranges `off` in HBM; then
//   * fill_frow_kernel: ONE wave per segment = (pair, block) sums row 0 of the F tables.  The 185 float thresholds sit in LDS
//     (bin(end) = the number of thresholds <= end: no log on the device), and so does the segment's [2][A] tile.  The records are
//     scanned 64 at a time, lane l holding record base + l; a lane takes part when its record is on the F path (begin <= 0) and
//     its bin is below A.  Lanes of one batch that hit the same bin must add in lane order: every such lane gets its rank among
//     the lanes of its bin (ballots: integers, one turn per distinct bin of the batch), and round r is a plain read-add-write of
//     LDS by the lanes of rank r -- at most one lane per bin and round --, with a barrier between rounds.  Every bin's chain is
//     the contract's: from 0.0, record after record, each addition rounded.  No floating-point atomics, no partial sums.  The
//     workgroup is one wave and every branch around a barrier is taken on a ballot or a loop counter.
//   * fill_jobs_kernel: one thread per segment writes the FillJob of fill_sample_kernel: its records, and the offset of the
//     first one's uniforms in the seed's stream -- 100 times the record's rank in its pair.
//   * fill_sample_kernel (fill_kernel.hip, unchanged) draws the ages.
// Nothing written by one kernel of the chunk is read by another workgroup of the same launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <cmath>
#include <random>
#include <thread>
#include <vector>

#include "age_bins.hpp"
#include "colate_amd.h"
#include "colate_internal.h"
#include "em_job.hpp"
#include "fill_device.h"
#include "fill_samples.h"
#include "interval_cells.h"
#include "interval_groups.h"
#include "uniform_stream.hpp"
#include "walk_resident.hpp"

using namespace colate;
using namespace colate_iw;
using colate_drv::FillJob;
using colate_drv::FillRec;
using colate_ic::kBins;

namespace {

__global__ __launch_bounds__(64) void fill_frow_kernel(const FillRec* __restrict__ recs, const FillSide* __restrict__ side,
                                                       const long long* __restrict__ off, const float* __restrict__ T,
                                                       double* __restrict__ frow) {
  __shared__ float sT[kBins];
  __shared__ double s_sum[2][kBins];
  const int lane = threadIdx.x;
  for (int i = lane; i < kBins; i += 64) sT[i] = T[i], s_sum[0][i] = 0.0, s_sum[1][i] = 0.0;
  __syncthreads();
  const long long seg = blockIdx.x;
  const long long r0 = off[seg], r1 = off[seg + 1];
  const unsigned long long below = (1ull << lane) - 1ull;  // the lanes in front of this one
  for (long long base = r0; base < r1; base += 64) {
    const long long i = base + lane;
    int b = -1;  // (-1: no record, not on the F path, or beyond the grid)
    if (i < r1 && recs[i].begin <= 0.0f) {
      b = colate_ic::bin_of(sT, recs[i].end);
      if (b >= kBins) b = -1;
    }
    const bool mine = b >= 0;
    unsigned long long left = __ballot(mine);
    if (left == 0) continue;
    double e_sh = 0.0, e_ns = 0.0;
    if (mine) e_sh = side[i].e_sh, e_ns = side[i].e_ns;
    int rank = 0, rounds = 0;
    while (left != 0) {  // one turn per distinct bin of the batch
      const int j = __ffsll((long long)left) - 1;
      const int bj = __shfl(b, j);
      const bool same_bin = mine && b == bj;
      const unsigned long long same = __ballot(same_bin);  // (lane j is in it: the loop ends)
      if (same_bin) rank = __popcll(same & below);
      rounds = max(rounds, (int)__popcll(same));
      left &= ~same;
    }
    for (int r = 0; r < rounds; r++) {
      if (mine && rank == r) {
        s_sum[0][b] += e_sh;
        s_sum[1][b] += e_ns;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  double* const out = frow + (size_t)seg * 2 * kBins;
  for (int i = lane; i < kBins; i += 64) out[i] = s_sum[0][i], out[kBins + i] = s_sum[1][i];
}

// seg_off[ng + 1]: the first segment of each pair of the chunk; pair_rec0[ng]: its first record in the chunk's records
__global__ __launch_bounds__(256) void fill_jobs_kernel(int nseg, int ng, const int* __restrict__ seg_off,
                                                        const long long* __restrict__ pair_rec0, const long long* __restrict__ off,
                                                        FillJob* __restrict__ jobs) {
  const int seg = blockIdx.x * blockDim.x + threadIdx.x;
  if (seg >= nseg) return;
  int lo = 0, hi = ng - 1;  // the last pair whose first segment is at or below seg (every pair has a block)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg_off[mid] <= seg) lo = mid; else hi = mid - 1;
  }
  const long long first = off[seg];
  jobs[seg] = FillJob{(uint64_t)first, (uint64_t)(colate_fs::kDraws * (first - pair_rec0[lo])), (uint32_t)(off[seg + 1] - first), (uint32_t)seg};
}

}  // namespace

namespace colate_fs {

namespace {

// The seed's uniforms [0, n) into d_U through two page-locked buffers that take turns: the words of a buffer come from the bulk
// generator, one after the other (0.6 ns a word); turning two words into a double costs more than that and has no order, so a
// few threads share it; the copy out of one buffer runs while the other is filled.  (The caller has checked the generator and the
// conversion against this machine's library: bulk_stream_ok.)
int upload_uniforms(unsigned seed, size_t n, double* d_U, DeviceBuffers& buf, hipStream_t stream) {
  constexpr size_t kRing = 8u << 20;  // doubles per buffer (64 MB)
  if (n == 0) return COLATE_OK;
  std::mt19937 g(seed);
  colate_drv::BulkMt19937 bulk;
  if (!bulk.load(g)) return fail(COLATE_EINVAL, "the generator's state could not be read");
  double* h[2] = {nullptr, nullptr};
  hipEvent_t ev[2];
  const size_t room = std::min(n, kRing);
  HIP_TRY(buf.pinned(h[0], room)); HIP_TRY(buf.pinned(h[1], room));
  HIP_TRY(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
  if (hipError_t e = hipEventCreateWithFlags(&ev[1], hipEventDisableTiming)) {
    (void)hipEventDestroy(ev[0]);
    return hip_fail(e, "hipEventCreate");
  }
  const size_t threads = std::min<size_t>(8, std::max(1u, std::thread::hardware_concurrency()));
  std::vector<uint32_t> w(2 * room);
  hipError_t err = hipSuccess;
  bool busy[2] = {false, false};
  int k = 0;
  for (size_t at = 0; at < n && err == hipSuccess; at += room, k ^= 1) {
    const size_t m = std::min(room, n - at);
    bulk.generate(w.data(), 2 * m);
    if (busy[k]) err = hipEventSynchronize(ev[k]);
    if (err != hipSuccess) break;
    double* const dst = h[k];
    const uint32_t* const src = w.data();
    const auto convert = [dst, src](size_t i0, size_t i1) {
      for (size_t i = i0; i < i1; i++) dst[i] = colate_drv::canonical_from_words(src[2 * i], src[2 * i + 1]);
    };
    const size_t share = (m + threads - 1) / threads;
    std::vector<std::thread> helpers;
    if (m >= (1u << 16))
      for (size_t t = 1; t < threads && t * share < m; t++) helpers.emplace_back(convert, t * share, std::min(m, (t + 1) * share));
    convert(0, helpers.empty() ? m : std::min(m, share));
    for (std::thread& t : helpers) t.join();
    err = hipMemcpyAsync(d_U + at, h[k], sizeof(double) * m, hipMemcpyHostToDevice, stream);
    if (err == hipSuccess) err = hipEventRecord(ev[k], stream), busy[k] = true;
  }
  for (int b = 0; b < 2; b++) {
    if (busy[b]) (void)hipEventSynchronize(ev[b]);
    (void)hipEventDestroy(ev[b]);
  }
  return err == hipSuccess ? COLATE_OK : hip_fail(err, "uniform stream upload");
}

}  // namespace

int fill_view_device(const View& v, int A, unsigned seed, Result& out) {
  if (int rc = check_fill(v, A)) return rc;
  if (int rc = ensure_device()) return rc;  // (marks the process: the runtime comes up here)
  ProfRange range("colate_fill_samples: H2D + walk count pass + uniform stream; per chunk walk write pass + F rows + jobs + age sampling + D2H");
  float T[kBins];
  if (int rc = colate_ic::build_thresholds(T)) return rc;
  const colate_drv::FastBin bands(A, 10.0);
  const bool device_ok = bands.ok() && colate_drv::bulk_stream_ok(seed);
  if (int rc = thread_workspace().reserve(256, 256)) return rc;  // (the workspace's stream: no second one)
  hipStream_t stream = thread_workspace().stream;
  KernelTimer timer(stream);
  Resident res;
  DeviceBuffers buf;
  // host arrays the stream copies from or into: they outlive the stream's work (sync_at_exit is declared behind them)
  std::vector<long long> rec0, pair_rec0;
  std::vector<int> seg0, seg_off, flags, blk0;
  std::vector<double> tab, frow;
  const StreamSync sync_at_exit{stream};
  if (int rc = res.upload(v, stream)) return rc;
  if (int rc = res.count(timer)) return rc;
  const int P = v.P, C = v.C;
  const size_t PC = (size_t)P * C;
  if (int rc = size_result(v, A, res.cnt.data(), res.last.data(), blk0, out)) return rc;
  out.chunks = 0, out.kernel_s = 0.0;
  if (!device_ok) {  // no located steps, or a stream the bulk form does not reproduce on this machine: all through the twin
    for (int p = 0; p < P; p++) twin_pair(v, p, A, seed, blk0.data() + (size_t)p * C, nullptr, out), out.handed_back[(size_t)p] = 1;
    return COLATE_OK;
  }
  long long max_used = 0;
  for (int p = 0; p < P; p++) max_used = std::max(max_used, out.used[(size_t)p]), out.words[(size_t)p] = 2ull * kDraws * (unsigned long long)out.used[(size_t)p];

  // ---- for the whole call: thresholds, guard bands, the uniform stream, the walk's first blocks
  float* d_T = nullptr;
  double *d_lo = nullptr, *d_hi = nullptr, *d_U = nullptr;
  int* d_blk0 = nullptr;
  const size_t n_uniforms = (size_t)kDraws * (size_t)max_used;
  HIP_TRY(buf.device(d_T, kBins)); HIP_TRY(buf.device(d_lo, (size_t)A + 2)); HIP_TRY(buf.device(d_hi, (size_t)A + 2));
  HIP_TRY(buf.device(d_U, n_uniforms + kDraws)); HIP_TRY(buf.device(d_blk0, PC));
  HIP_TRY(h2d(stream, d_T, T, sizeof(float) * kBins));
  HIP_TRY(h2d(stream, d_lo, bands.guard_lo(), sizeof(double) * ((size_t)A + 2)));
  HIP_TRY(h2d(stream, d_hi, bands.guard_hi(), sizeof(double) * ((size_t)A + 2)));
  HIP_TRY(h2d(stream, d_blk0, res.blk0.data(), sizeof(int) * PC));
  if (int rc = upload_uniforms(seed, n_uniforms, d_U, buf, stream)) return rc;

  // ---- the chunks: runs of consecutive pairs within the record budget; scratch once, for the largest
  const long long budget = std::max<long long>(
      1, colate_ic::env_budget_mb("COLATE_FILL_SAMPLES_RECS_MB", COLATE_FILL_SAMPLES_RECS_MB_DEFAULT) * (1LL << 20) / (long long)(sizeof(FillRec) + sizeof(FillSide)));
  const std::vector<std::pair<int, int>> chunks = plan_chunks(P, res.off.data(), budget);
  size_t max_recs = 0, max_segs = 0, max_pairs = 0;
  for (const auto& c : chunks) {
    size_t segs = 0;
    for (int p = c.first; p < c.second; p++) segs += (size_t)res.nb[(size_t)p];
    max_segs = std::max(max_segs, segs), max_pairs = std::max(max_pairs, (size_t)(c.second - c.first));
    max_recs = std::max(max_recs, (size_t)(res.off[(size_t)c.second] - res.off[(size_t)c.first]));
  }
  if (max_segs > 0x7fffffffull) return fail(COLATE_ELIMIT, "a chunk of %zu (pair, block) segments", max_segs);
  FillRec* d_recs = nullptr;
  FillSide* d_side = nullptr;
  FillJob* d_jobs = nullptr;
  long long *d_off = nullptr, *d_rec0 = nullptr, *d_pair_rec0 = nullptr;
  int *d_seg0 = nullptr, *d_seg_off = nullptr, *d_flags = nullptr;
  double *d_tab = nullptr, *d_frow = nullptr;
  HIP_TRY(buf.device(d_recs, max_recs)); HIP_TRY(buf.device(d_side, max_recs)); HIP_TRY(buf.device(d_jobs, max_segs));
  HIP_TRY(buf.device(d_off, max_segs + 1)); HIP_TRY(buf.device(d_rec0, max_pairs * C)); HIP_TRY(buf.device(d_seg0, max_pairs * C));
  HIP_TRY(buf.device(d_pair_rec0, max_pairs)); HIP_TRY(buf.device(d_seg_off, max_pairs + 1)); HIP_TRY(buf.device(d_flags, max_segs));
  HIP_TRY(buf.device(d_tab, max_segs * 2 * A)); HIP_TRY(buf.device(d_frow, max_segs * 2 * A));
  tab.resize(max_segs * 2 * A), frow.resize(max_segs * 2 * A), flags.resize(max_segs);

  for (const auto& c : chunks) {
    const int p0 = c.first, p1 = c.second, ng = p1 - p0;
    const size_t k0 = (size_t)p0 * C, nk = (size_t)ng * C;
    const long long n = res.off[(size_t)p1] - res.off[(size_t)p0];
    seg_off.assign(1, 0), pair_rec0.resize((size_t)ng), rec0.resize(nk), seg0.resize(nk);
    for (int j = 0; j < ng; j++) seg_off.push_back(seg_off.back() + res.nb[(size_t)(p0 + j)]), pair_rec0[(size_t)j] = res.off[(size_t)(p0 + j)] - res.off[(size_t)p0];
    const int nseg = seg_off.back();
    long long at = 0;
    for (size_t k = 0; k < nk; k++) {
      rec0[k] = at, at += res.cnt[k0 + k];
      seg0[k] = seg_off[k / C] + res.blk0[k0 + k];
    }
    if (at != n) return fail(COLATE_EHIP, "the walk's counts do not add up to the chunk's records (%lld, %lld)", at, n);
    HIP_TRY(h2d(stream, d_rec0, rec0.data(), sizeof(long long) * nk)); HIP_TRY(h2d(stream, d_seg0, seg0.data(), sizeof(int) * nk));
    HIP_TRY(h2d(stream, d_seg_off, seg_off.data(), sizeof(int) * seg_off.size()));
    HIP_TRY(h2d(stream, d_pair_rec0, pair_rec0.data(), sizeof(long long) * (size_t)ng));
    HIP_TRY(hipMemsetAsync(d_tab, 0, sizeof(double) * (size_t)nseg * 2 * A, stream));
    HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int) * (size_t)nseg, stream));
    HIP_TRY(timer.mark());
    if (hipError_t e = write_fill_launch(res.in, p0, p1, d_rec0, d_blk0 + k0, d_seg0, d_recs, d_side, d_off, nseg, n, stream))
      return hip_fail(e, "fill walk write kernel launch");
    hipLaunchKernelGGL(fill_frow_kernel, dim3((unsigned)nseg), dim3(64), 0, stream, d_recs, d_side, d_off, d_T, d_frow);
    if (hipError_t e = hipGetLastError()) return hip_fail(e, "F-row kernel launch");
    hipLaunchKernelGGL(fill_jobs_kernel, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, stream, nseg, ng, d_seg_off, d_pair_rec0, d_off, d_jobs);
    if (hipError_t e = hipGetLastError()) return hip_fail(e, "jobs kernel launch");
    if (hipError_t e = colate_drv::fill_sample_launch(d_jobs, nseg, d_recs, d_U, d_lo, d_hi, A, d_tab, d_flags, stream))
      return hip_fail(e, "age sampling kernel launch");
    HIP_TRY(timer.mark());
    // the chunk's one copy back: tables, F rows, flags
    HIP_TRY(hipMemcpyAsync(tab.data(), d_tab, sizeof(double) * (size_t)nseg * 2 * A, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(frow.data(), d_frow, sizeof(double) * (size_t)nseg * 2 * A, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(flags.data(), d_flags, sizeof(int) * (size_t)nseg, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int j = 0; j < ng; j++) {
      const int p = p0 + j;
      bool flagged = false;
      for (int s = seg_off[(size_t)j]; s < seg_off[(size_t)j + 1]; s++) flagged = flagged || flags[(size_t)s] != 0;
      if (flagged) {  // a sample inside a guard band, or one the reference would draw again: the twin fills the pair
        twin_pair(v, p, A, seed, blk0.data() + (size_t)p * C, nullptr, out);
        out.handed_back[(size_t)p] = 1;
        continue;
      }
      double* dst = out.tables.data() + out.table_off[(size_t)p];
      for (int s = seg_off[(size_t)j]; s < seg_off[(size_t)j + 1]; s++, dst += 4 * (size_t)A) {
        std::memcpy(dst, tab.data() + (size_t)s * 2 * A, sizeof(double) * 2 * (size_t)A);
        std::memcpy(dst + 2 * (size_t)A, frow.data() + (size_t)s * 2 * A, sizeof(double) * 2 * (size_t)A);
      }
    }
    out.chunks++;
  }
  out.kernel_s = timer.seconds();
  return COLATE_OK;
}

}  // namespace colate_fs
