// colate_amd/csrc/interval_device.cpp -- the device driver of the interval-dated fit over many groups: colate_interval_fit_groups
// (records from the caller's host arrays) and the device half of the pair walk (interval_walk.h; records from its write pass).
// No kernel lives here: everything goes through the *_launch functions, on the stream of the calling thread's workspace
// (em_job.hpp).  Read fit_groups_core first (the chunk loop, the fit launch), then GroupsFit::run_chunk (one chunk, its one wait).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <limits>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "em_job.hpp"
#include "em_kernels.h"
#include "device_stage.hpp"
#include "interval_cells.h"
#include "interval_groups.h"
#include "interval_walk.h"
#include "walk_resident.hpp"

using namespace colate;
using namespace colate_ic;
using colate_iw::h2d;
using colate_iw::KernelTimer;
using colate_iw::StreamSync;

static thread_local double g_interval_groups_kernel_s = 0.0;
extern "C" double colate_interval_fit_groups_kernel_seconds(void) { return g_interval_groups_kernel_s; }
extern "C" double colate_interval_fit_samples_kernel_seconds(void) { return g_interval_groups_kernel_s; }

namespace {

// The host side of a chunk.  The stream copies from these vectors asynchronously: a Chunk lives until the stream is idle.
struct Chunk {
  int g0 = 0, g1 = 0;  // groups [g0, g1)
  std::vector<int> seg_off, cap, src_int;
  std::vector<long long> row_off, src_ll;  // (src_*: whatever the records' source copies from)
  std::vector<ColateIntervalRowsJob> jobs;
};

// Where the records of a chunk of groups come from: the caller's host arrays (colate_interval_fit_groups) or the write pass of the
// pair walk (colate_interval_fit_samples).  On the timer's stream: the records of the chunk's groups at d_recs and, for its
// segments (group, block) in order, the nseg + 1 record ranges at d_off (c.seg_off[j]: the first segment of group c.g0 + j; n: the
// chunk's records).  Opens the chunk's timed interval with one timer.mark(): in front of its own kernels, or behind its copies.
using StageRecords = std::function<int(Chunk& c, long long n, IntervalRec* d_recs, long long* d_off, KernelTimer& timer)>;

// The device side of one grouped fit and the steps that use it, in the order fit_groups_core calls them.
struct GroupsFit {
  const int G, B, E;
  const long long* const rec_off;
  const int* const nb;
  KernelTimer& timer;
  const hipStream_t stream = timer.stream;
  DeviceBuffers buf;
  // for the whole call: inputs, the groups' descriptors, results ([G][B] rows)
  float* d_T = nullptr;
  double *d_grid = nullptr, *d_bw = nullptr, *d_ep = nullptr, *d_init = nullptr, *d_rates = nullptr, *d_ll = nullptr;
  int *d_iters = nullptr, *d_flags = nullptr;
  ColateIntervalGroup* d_desc = nullptr;
  std::vector<size_t> bw_off;  // [G]: the group's block weights in d_bw
  // the scratch of a chunk, sized for the largest and used by one chunk after the other in stream order
  IntervalRec* d_recs = nullptr;
  int *d_idx = nullptr, *d_seg_off = nullptr, *d_cap = nullptr, *d_R = nullptr;
  long long *d_off = nullptr, *d_row_off = nullptr, *d_dropped = nullptr;
  unsigned long long* d_seg_dropped = nullptr;
  double* d_cells = nullptr;
  unsigned char* d_flagbytes = nullptr;
  ColateIntervalRowsJob* d_jobs = nullptr;
  // what the chunks leave for the fit and the caller, [G]; each chunk's R and dropped arrive in its groups' places
  std::vector<ColateIntervalGroup> desc;
  std::vector<int> R;
  std::vector<long long> dropped;
  bool any_rows = false;

  // the call-lifetime arrays, and their inputs on the way
  int call_buffers(const float* T, const double* grid, const double* block_weights, const double* epochs, const double* init_rates) {
    size_t bw_total = 0;
    bw_off.resize((size_t)G), desc.resize((size_t)G), R.resize((size_t)G), dropped.resize((size_t)G);
    for (int g = 0; g < G; g++) bw_off[(size_t)g] = bw_total, bw_total += (size_t)B * nb[g];
    const size_t GB = (size_t)G * B, GE = (size_t)G * E;
    HIP_TRY(buf.device(d_T, kBins)); HIP_TRY(buf.device(d_grid, kBins)); HIP_TRY(buf.device(d_bw, bw_total));
    HIP_TRY(buf.device(d_ep, GE)); HIP_TRY(buf.device(d_init, GE)); HIP_TRY(buf.device(d_desc, (size_t)G));
    HIP_TRY(buf.device(d_rates, GB * E)); HIP_TRY(buf.device(d_ll, GB)); HIP_TRY(buf.device(d_iters, GB)); HIP_TRY(buf.device(d_flags, GB));
    HIP_TRY(h2d(stream, d_T, T, sizeof(float) * kBins)); HIP_TRY(h2d(stream, d_grid, grid, sizeof(double) * kBins));
    HIP_TRY(h2d(stream, d_bw, block_weights, sizeof(double) * bw_total));
    HIP_TRY(h2d(stream, d_ep, epochs, sizeof(double) * GE)); HIP_TRY(h2d(stream, d_init, init_rates, sizeof(double) * GE));
    return COLATE_OK;
  }

  int chunk_scratch(const std::vector<Chunk>& chunks) {
    size_t max_segs = 0, max_groups = 0, max_recs = 0;
    for (const Chunk& c : chunks) {
      size_t segs = 0;
      for (int g = c.g0; g < c.g1; g++) segs += (size_t)nb[g];
      max_segs = std::max(max_segs, segs), max_groups = std::max(max_groups, (size_t)(c.g1 - c.g0));
      max_recs = std::max(max_recs, (size_t)(rec_off[c.g1] - rec_off[c.g0]));
    }
    HIP_TRY(buf.device(d_recs, max_recs)); HIP_TRY(buf.device(d_idx, max_recs)); HIP_TRY(buf.device(d_off, max_segs + 1));
    HIP_TRY(buf.device(d_cells, max_segs * 2 * kCells)); HIP_TRY(buf.device(d_seg_dropped, max_segs));
    HIP_TRY(buf.device(d_seg_off, max_groups + 1)); HIP_TRY(buf.device(d_cap, max_groups)); HIP_TRY(buf.device(d_row_off, max_groups));
    HIP_TRY(buf.device(d_R, max_groups)); HIP_TRY(buf.device(d_dropped, max_groups)); HIP_TRY(buf.device(d_jobs, max_groups));
    HIP_TRY(buf.device(d_flagbytes, max_groups * 2 * kCells));
    return COLATE_OK;
  }

  // One chunk, in stream order: its offsets in; the source's records and ranges; cells; row pick; R and dropped out and THE ONE
  // HOST WAIT of the chunk (R sizes its W); then, where a group has rows, the jobs in and the grouped row bootstrap.  Timed: from
  // the source's mark to behind the row pick, and the row bootstrap.
  int run_chunk(Chunk& c, const StageRecords& stage) {
    const int ng = c.g1 - c.g0;
    const long long n = rec_off[c.g1] - rec_off[c.g0];
    c.seg_off.assign(1, 0), c.cap.resize((size_t)ng), c.row_off.resize((size_t)ng);
    long long rows_cap = 0;
    for (int j = 0; j < ng; j++) {
      const int g = c.g0 + j;
      c.seg_off.push_back(c.seg_off.back() + nb[g]);
      c.cap[(size_t)j] = row_cap(rec_off[g + 1] - rec_off[g]), c.row_off[(size_t)j] = rows_cap;
      rows_cap += c.cap[(size_t)j];
    }
    // the chunk's rows stay for the fit: room for every group's cap
    int *d_cell_of_row = nullptr, *d_kinds = nullptr;
    double *d_a0 = nullptr, *d_a1 = nullptr;
    HIP_TRY(buf.device(d_cell_of_row, (size_t)rows_cap)); HIP_TRY(buf.device(d_kinds, (size_t)rows_cap));
    HIP_TRY(buf.device(d_a0, (size_t)rows_cap)); HIP_TRY(buf.device(d_a1, (size_t)rows_cap));
    HIP_TRY(h2d(stream, d_seg_off, c.seg_off.data(), sizeof(int) * c.seg_off.size()));
    HIP_TRY(h2d(stream, d_cap, c.cap.data(), sizeof(int) * (size_t)ng));
    HIP_TRY(h2d(stream, d_row_off, c.row_off.data(), sizeof(long long) * (size_t)ng));
    if (int rc = stage(c, n, d_recs, d_off, timer)) return rc;
    hipError_t e = colate_interval_cells_launch(n, d_recs, d_off, c.seg_off.back(), d_T, d_idx, d_cells, d_seg_dropped, stream);
    if (e != hipSuccess) return hip_fail(e, "interval cells kernel launch");
    e = colate_interval_rows_launch(ng, d_cells, d_seg_off, d_seg_dropped, d_grid, d_row_off, d_cap, d_flagbytes, d_cell_of_row, d_kinds,
                                    d_a0, d_a1, d_R, d_dropped, stream);
    if (e != hipSuccess) return hip_fail(e, "interval rows kernel launch");
    HIP_TRY(timer.mark());
    HIP_TRY(hipMemcpyAsync(&R[(size_t)c.g0], d_R, sizeof(int) * (size_t)ng, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&dropped[(size_t)c.g0], d_dropped, sizeof(long long) * (size_t)ng, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    size_t w_total = 0;
    int max_R = 0;
    for (int j = 0; j < ng; j++) {
      const int Rg = R[(size_t)(c.g0 + j)];
      if (Rg < 0 || Rg > c.cap[(size_t)j])
        return fail(COLATE_EHIP, "group %d: the row pick returned %d rows, room for %d", c.g0 + j, Rg, c.cap[(size_t)j]);
      w_total += (size_t)B * Rg, max_R = std::max(max_R, Rg);
    }
    double* d_W = nullptr;
    HIP_TRY(buf.device(d_W, w_total));
    c.jobs.resize((size_t)ng);
    size_t w_at = 0;
    for (int j = 0; j < ng; j++) {
      const int g = c.g0 + j, Rg = R[(size_t)g];
      const long long ro = c.row_off[(size_t)j];
      c.jobs[(size_t)j] = ColateIntervalRowsJob{c.seg_off[(size_t)j], nb[g], Rg, d_cell_of_row + ro, d_bw + bw_off[(size_t)g], d_W + w_at};
      desc[(size_t)g] = ColateIntervalGroup{Rg, d_kinds + ro, d_a0 + ro, d_a1 + ro, d_W + w_at, d_ep + (size_t)g * E, d_init + (size_t)g * E};
      w_at += (size_t)B * Rg;
    }
    if (max_R == 0) return COLATE_OK;
    any_rows = true;
    HIP_TRY(h2d(stream, d_jobs, c.jobs.data(), sizeof(ColateIntervalRowsJob) * (size_t)ng));
    HIP_TRY(timer.mark());
    e = colate_bootstrap_rows_groups_launch(ng, B, max_R, d_jobs, d_cells, stream);
    if (e != hipSuccess) return hip_fail(e, "grouped row bootstrap kernel launch");
    HIP_TRY(timer.mark());
    return COLATE_OK;
  }

  // One fit launch for all groups (timed) and its results on their way to the host arrays; nothing where no group has rows.
  int launch_fit(int max_iter, int min_iter, double rel_tol, double rate_floor, double* rates, double* ll, int* iters, int* flags) {
    if (!any_rows) return COLATE_OK;
    const size_t GB = (size_t)G * B;
    HIP_TRY(h2d(stream, d_desc, desc.data(), sizeof(ColateIntervalGroup) * (size_t)G));
    HIP_TRY(timer.mark());
    const hipError_t e = colate_em_interval_fit_groups_launch(G, B, E, d_desc, max_iter, min_iter, rel_tol, rate_floor, d_rates, d_iters,
                                                              d_ll, d_flags, stream);
    if (e != hipSuccess) return hip_fail(e, "grouped interval EM kernel launch");
    HIP_TRY(timer.mark());
    HIP_TRY(hipMemcpyAsync(rates, d_rates, sizeof(double) * GB * E, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(ll, d_ll, sizeof(double) * GB, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(iters, d_iters, sizeof(int) * GB, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(flags, d_flags, sizeof(int) * GB, hipMemcpyDeviceToHost, stream));
    return COLATE_OK;
  }
};

// Many groups' cells, rows and fits in one pass (include/colate_amd.h), after the checks, on the timer's stream.  The groups go
// through the cells, the row pick and the row bootstrap in chunks (plan_chunks: dense cell sums within the budget, records within
// max_chunk_recs); the only thing the host waits for before the results is each chunk's R and dropped counts; then one launch fits
// all groups.  epochs / init_rates: [G][E].  Leaves the kernels' seconds, with whatever the timer held before, in
// g_interval_groups_kernel_s.  The results go to copies first: a call that fails leaves the outputs untouched.
int fit_groups_core(int G, int B, int E, const long long* rec_off, const int* nb, const double* block_weights, const double* epochs,
                    const double* init_rates, int max_iter, int min_iter, double rel_tol, double rate_floor, long long max_chunk_recs,
                    const StageRecords& stage, const float* T, KernelTimer& timer, int* out_R, long long* out_dropped, double* out_rates,
                    int* out_iters, double* out_loglik, int* out_flags) {
  double grid[COLATE_MAX_AGE_BINS];
  if (colate_age_grid(grid, COLATE_MAX_AGE_BINS) != kBins) return fail(COLATE_EINVAL, "the age grid has not %d points", kBins);
  const size_t budget_segs = (size_t)env_budget_mb("COLATE_INTERVAL_GROUPS_CELLS_MB", COLATE_INTERVAL_GROUPS_CELLS_MB_DEFAULT) *
                             (1u << 20) / (sizeof(double) * 2 * kCells);
  std::vector<Chunk> chunks;
  for (const std::pair<int, int>& r : plan_chunks(G, nb, rec_off, budget_segs, max_chunk_recs))
    chunks.emplace_back(), chunks.back().g0 = r.first, chunks.back().g1 = r.second;
  const size_t GB = (size_t)G * B;
  std::vector<double> rates(GB * E), ll(GB);
  std::vector<int> iters(GB), flags(GB);
  GroupsFit fit{G, B, E, rec_off, nb, timer};
  const StreamSync sync_at_exit{timer.stream};  // (behind the chunks, the result copies and the fit's buffers: see StreamSync)

  if (int rc = fit.call_buffers(T, grid, block_weights, epochs, init_rates)) return rc;
  if (int rc = fit.chunk_scratch(chunks)) return rc;
  for (Chunk& c : chunks)
    if (int rc = fit.run_chunk(c, stage)) return rc;
  if (int rc = fit.launch_fit(max_iter, min_iter, rel_tol, rate_floor, rates.data(), ll.data(), iters.data(), flags.data())) return rc;
  HIP_TRY(hipStreamSynchronize(timer.stream));
  g_interval_groups_kernel_s = timer.seconds();

  for (int g = 0; g < G; g++) {  // a group without rows keeps its starting rates
    const size_t o = (size_t)g * B;
    if (fit.R[(size_t)g] == 0)
      no_rows_results(B, E, init_rates + (size_t)g * E, rates.data() + o * E, iters.data() + o, ll.data() + o, flags.data() + o);
  }
  std::memcpy(out_R, fit.R.data(), sizeof(int) * (size_t)G), std::memcpy(out_dropped, fit.dropped.data(), sizeof(long long) * (size_t)G);
  std::memcpy(out_rates, rates.data(), sizeof(double) * GB * E), std::memcpy(out_loglik, ll.data(), sizeof(double) * GB);
  std::memcpy(out_iters, iters.data(), sizeof(int) * GB), std::memcpy(out_flags, flags.data(), sizeof(int) * GB);
  return COLATE_OK;
}

}  // namespace

extern "C" int colate_interval_fit_groups(int G, int B, int E, const long long* rec_off, const colate_interval_rec* recs, const int* block,
                                          const int* nb, const double* block_weights, const double* epochs, const double* init_rates,
                                          int max_iter, int min_iter, double rel_tol, double rate_floor, int* out_R,
                                          long long* out_dropped, double* out_rates, int* out_iters, double* out_loglik, int* out_flags) {
  float T[kBins];
  if (int rc = build_thresholds(T)) return rc;
  if (int rc = check_groups_args(G, B, E, rec_off, recs, block, nb, block_weights, epochs, init_rates, max_iter, min_iter, rel_tol,
                                 rate_floor, T, out_R, out_dropped, out_rates, out_iters, out_loglik, out_flags))
    return rc;
  if (int rc = ensure_device()) return rc;
  ProfRange range("colate_interval_fit_groups: per chunk H2D + cells + row pick + row bootstrap; one interval EM kernel + D2H");
  g_interval_groups_kernel_s = 0.0;
  if (int rc = thread_workspace().reserve(256, 256)) return rc;  // (the workspace's stream: no second one)
  hipStream_t stream = thread_workspace().stream;
  KernelTimer timer(stream);
  // the caller's records: uploaded chunk by chunk, the ranges from block_ranges on the host; the copies are not timed
  const StageRecords from_host = [=](Chunk& c, long long n, IntervalRec* d_recs, long long* d_off, KernelTimer& timer) -> int {
    const long long r0 = rec_off[c.g0];
    std::vector<long long>& coff = c.src_ll;
    for (int g = c.g0; g < c.g1; g++) {
      const long long ng_recs = rec_off[g + 1] - rec_off[g];
      std::vector<long long> off((size_t)nb[g] + 1);
      block_ranges(ng_recs, ng_recs ? block + rec_off[g] : nullptr, nb[g], off.data());
      for (int k = 0; k < nb[g]; k++) coff.push_back(rec_off[g] - r0 + off[(size_t)k]);
    }
    coff.push_back(n);
    HIP_TRY(h2d(timer.stream, d_recs, recs + r0, sizeof(IntervalRec) * (size_t)n));
    HIP_TRY(h2d(timer.stream, d_off, coff.data(), sizeof(long long) * coff.size()));
    HIP_TRY(timer.mark());
    return COLATE_OK;
  };
  return fit_groups_core(G, B, E, rec_off, nb, block_weights, epochs, init_rates, max_iter, min_iter, rel_tol, rate_floor,
                         std::numeric_limits<long long>::max(), from_host, T, timer, out_R, out_dropped, out_rates, out_iters, out_loglik,
                         out_flags);
}

// ---- the pair walk on the device (interval_walk.h)
namespace colate_iw {

int walk_view_device(const View& v, long long cap, long long* rec_off, int* nb, IntervalRec* recs, int* block) {
  if (int rc = check_walk_outputs(cap, rec_off, nb, recs, block)) return rc;
  if (int rc = check_view(v)) return rc;
  if (int rc = ensure_device()) return rc;
  ProfRange range("colate_interval_walk: H2D + count pass + write pass + D2H");
  if (int rc = thread_workspace().reserve(256, 256)) return rc;  // (the workspace's stream: no second one)
  hipStream_t stream = thread_workspace().stream;
  KernelTimer timer(stream);
  Resident res;
  DeviceBuffers buf;
  std::vector<long long> rec0;
  const StreamSync sync_at_exit{stream};
  if (int rc = res.upload(v, stream)) return rc;
  if (int rc = res.count(timer)) return rc;
  const size_t PC = (size_t)v.P * v.C;
  const long long total = res.off[(size_t)v.P];
  if (int rc = check_capacity(total, cap)) return rc;
  long long at = 0;
  for (size_t k = 0; k < PC; k++) rec0.push_back(at), at += res.cnt[k];
  long long* d_rec0 = nullptr;
  int *d_blk0 = nullptr, *d_block = nullptr;
  IntervalRec* d_recs = nullptr;
  HIP_TRY(buf.device(d_rec0, PC)); HIP_TRY(buf.device(d_blk0, PC)); HIP_TRY(buf.device(d_recs, (size_t)total)); HIP_TRY(buf.device(d_block, (size_t)total));
  HIP_TRY(hipMemcpyAsync(d_rec0, rec0.data(), sizeof(long long) * PC, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_blk0, res.blk0.data(), sizeof(int) * PC, hipMemcpyHostToDevice, stream));
  if (hipError_t e = write_launch(res.in, 0, v.P, d_rec0, d_blk0, nullptr, d_recs, d_block, nullptr, 0, total, stream))
    return hip_fail(e, "interval walk write kernel launch");
  if (total) {
    HIP_TRY(hipMemcpyAsync(recs, d_recs, sizeof(IntervalRec) * (size_t)total, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(block, d_block, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, stream));
  }
  HIP_TRY(hipStreamSynchronize(stream));
  std::memcpy(rec_off, res.off.data(), sizeof(long long) * res.off.size()), std::memcpy(nb, res.nb.data(), sizeof(int) * res.nb.size());
  return COLATE_OK;
}

int fit_samples_view_device(const View& v, const FitArgs& a) {
  if (int rc = check_fit_args(v, a)) return rc;
  float T[kBins];
  if (int rc = build_thresholds(T)) return rc;
  if (int rc = ensure_device()) return rc;
  ProfRange range("colate_interval_fit_samples: H2D + walk count pass; per chunk walk write pass + cells + row pick + row bootstrap; one interval EM kernel + D2H");
  g_interval_groups_kernel_s = 0.0;
  if (int rc = thread_workspace().reserve(256, 256)) return rc;  // (the workspace's stream: no second one)
  hipStream_t stream = thread_workspace().stream;
  KernelTimer timer(stream);  // the count pass and the grouped fit: one sum
  Resident res;
  DeviceBuffers buf;
  const StreamSync sync_at_exit{stream};
  if (int rc = res.upload(v, stream)) return rc;
  if (int rc = res.count(timer)) return rc;
  const int P = v.P;
  const size_t PC = (size_t)P * v.C;
  std::vector<double> weights;
  if (int rc = draw_pair_weights(a.seed, a.B, P, res.nb.data(), weights)) return rc;
  const long long max_chunk_recs = std::max<long long>(
      1, env_budget_mb("COLATE_INTERVAL_WALK_RECS_MB", COLATE_INTERVAL_WALK_RECS_MB_DEFAULT) * (1LL << 20) / (long long)(sizeof(IntervalRec) + sizeof(int)));
  long long* d_rec0 = nullptr;
  int *d_blk0 = nullptr, *d_seg0 = nullptr;
  HIP_TRY(buf.device(d_rec0, PC)); HIP_TRY(buf.device(d_blk0, PC)); HIP_TRY(buf.device(d_seg0, PC));
  HIP_TRY(hipMemcpyAsync(d_blk0, res.blk0.data(), sizeof(int) * PC, hipMemcpyHostToDevice, stream));
  // the records of a chunk of pairs straight from the write pass, which is timed with the chunk's other kernels
  const StageRecords from_walk = [&](Chunk& c, long long n, IntervalRec* d_recs, long long* d_off, KernelTimer& timer) -> int {
    HIP_TRY(timer.mark());
    const size_t C = (size_t)v.C, k0 = (size_t)c.g0 * C, nk = (size_t)(c.g1 - c.g0) * C;
    std::vector<long long>& rec0 = c.src_ll;
    std::vector<int>& seg0 = c.src_int;
    rec0.resize(nk), seg0.resize(nk);
    long long at = 0;
    for (size_t k = 0; k < nk; k++) {
      rec0[k] = at, at += res.cnt[k0 + k];
      seg0[k] = c.seg_off[k / C] + res.blk0[k0 + k];
    }
    if (at != n) return fail(COLATE_EHIP, "the walk's counts do not add up to the chunk's records (%lld, %lld)", at, n);
    HIP_TRY(hipMemcpyAsync(d_rec0, rec0.data(), sizeof(long long) * nk, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_seg0, seg0.data(), sizeof(int) * nk, hipMemcpyHostToDevice, stream));
    if (hipError_t e = write_launch(res.in, c.g0, c.g1, d_rec0, d_blk0 + k0, d_seg0, d_recs, nullptr, d_off, c.seg_off.back(), n, stream))
      return hip_fail(e, "interval walk write kernel launch");
    return COLATE_OK;
  };
  const std::vector<double> ep = repeat_rows(a.epochs, a.E, P), init = repeat_rows(a.init_rates, a.E, P);
  if (int rc = fit_groups_core(P, a.B, a.E, res.off.data(), res.nb.data(), weights.data(), ep.data(), init.data(), a.max_iter, a.min_iter,
                               a.rel_tol, a.rate_floor, max_chunk_recs, from_walk, T, timer, a.out_R, a.out_dropped, a.out_rates, a.out_iters,
                               a.out_loglik, a.out_flags))
    return rc;
  for (int p = 0; p < P; p++) a.out_nb[p] = res.nb[(size_t)p], a.out_used[p] = res.off[(size_t)p + 1] - res.off[(size_t)p];
  return COLATE_OK;
}

}  // namespace colate_iw
