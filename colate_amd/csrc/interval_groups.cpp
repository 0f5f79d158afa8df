// colate_amd/csrc/interval_groups.cpp -- the host side of colate_interval_fit_groups (interval_groups.h): the argument checks
// both forms run before anything is staged, and the host twin, which walks the groups through the host twins of the two
// calls it stands for (colate_interval_cells_host, colate_bootstrap_em_interval_batch_host).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "interval_groups.h"

using colate::fail;

namespace colate_ic {

namespace {

// the rows and tables of one group on the host (the host twin of the cells call, without its checks)
struct GroupRows {
  int R = 0;
  long long dropped = 0;
  std::vector<int> kinds;
  std::vector<double> age_begin, age_end, tables;
};
int group_rows_host(long long n, const IntervalRec* recs, const int* block, int nb, const float* T, GroupRows& out) {
  std::vector<long long> off((size_t)nb + 1), nd((size_t)nb);
  block_ranges(n, block, nb, off.data());
  std::vector<double> cells((size_t)nb * 2 * kCells);
  host_cells(n, recs, off.data(), nb, T, cells.data(), nd.data());
  const int cap = row_cap(n);
  out.kinds.resize((size_t)cap), out.age_begin.resize((size_t)cap), out.age_end.resize((size_t)cap), out.tables.resize((size_t)nb * cap);
  const int R = compact_cells(nb, cells.data(), cap, out.kinds.data(), out.age_begin.data(), out.age_end.data(), out.tables.data());
  if (R < 0) return R;
  out.R = R, out.dropped = 0;
  for (long long d : nd) out.dropped += d;
  return COLATE_OK;
}

int group_fail(int rc, int g) {
  const std::string why = colate_last_error();
  return fail(rc, "group %d: %s", g, why.c_str());
}

}  // namespace

std::vector<std::pair<int, int>> plan_chunks(int G, const int* nb, const long long* rec_off, size_t budget_segs, long long max_chunk_recs) {
  budget_segs = std::max<size_t>(1, budget_segs);
  std::vector<std::pair<int, int>> chunks;
  for (int g = 0; g < G;) {
    const int g0 = g;
    size_t segs = 0;
    do segs += (size_t)nb[g++];
    while (g < G && g - g0 < 65535 && segs + (size_t)nb[g] <= budget_segs && rec_off[g + 1] - rec_off[g0] <= max_chunk_recs);
    chunks.emplace_back(g0, g);
  }
  return chunks;
}

long long env_budget_mb(const char* name, long long default_mb) {
  const char* e = std::getenv(name);
  return e ? std::max(0LL, std::atoll(e)) : default_mb;
}

void no_rows_results(int B, int E, const double* init_rates, double* rates, int* iters, double* loglik, int* flags) {
  for (int b = 0; b < B; b++) {
    std::memcpy(rates + (size_t)b * E, init_rates, sizeof(double) * (size_t)E);
    iters[b] = 0, loglik[b] = 0.0, flags[b] = 0;
  }
}

int check_groups_args(int G, int B, int E, const long long* rec_off, const IntervalRec* recs, const int* block, const int* nb,
                      const double* block_weights, const double* epochs, const double* init_rates, int max_iter, int min_iter,
                      double rel_tol, double rate_floor, const float* T, const int* out_R, const long long* out_dropped,
                      const double* out_rates, const int* out_iters, const double* out_loglik, const int* out_flags) {
  if (G < 1 || B < 1 || E < 1) return fail(COLATE_EINVAL, "bad sizes G=%d B=%d E=%d (at least one group, one replicate and one epoch)", G, B, E);
  if (E > 1024) return fail(COLATE_ELIMIT, "E=%d above the compiled limit (1024)", E);
  if ((long long)G * B > 0x7fffffffLL) return fail(COLATE_ELIMIT, "G x B = %lld replicates", (long long)G * B);
  if (B > 65535) return fail(COLATE_ELIMIT, "B=%d above the grid of the grouped bootstrap kernel (65535)", B);
  if (!rec_off || !nb || !block_weights || !epochs || !init_rates || !out_R || !out_dropped || !out_rates || !out_iters ||
      !out_loglik || !out_flags)
    return fail(COLATE_EINVAL, "NULL pointer argument");
  if (rec_off[0] < 0) return fail(COLATE_EINVAL, "rec_off[0] = %lld is negative", rec_off[0]);
  for (int g = 0; g < G; g++)
    if (rec_off[g + 1] < rec_off[g]) return fail(COLATE_EINVAL, "rec_off decreases at group %d (%lld after %lld)", g, rec_off[g + 1], rec_off[g]);
  if (rec_off[G] > 0 && (!recs || !block)) return fail(COLATE_EINVAL, "NULL pointer argument");
  const double dmax = std::numeric_limits<double>::max();
  size_t w_off = 0;
  for (int g = 0; g < G; g++) {
    const long long n = rec_off[g + 1] - rec_off[g];
    const IntervalRec* r = n ? recs + rec_off[g] : nullptr;
    const int* blk = n ? block + rec_off[g] : nullptr;
    if (int rc = check_cells_args(n, r, blk, nb[g], 0, nullptr, nullptr, nullptr, nullptr, out_dropped)) return group_fail(rc, g);
    const double* ep = epochs + (size_t)g * E;
    const double* bw = block_weights + w_off;
    w_off += (size_t)B * nb[g];
    // the smallest age_begin of the group's rows, and per block the sums of the weights: bounds on the cell sums
    int bb_min = -1;
    float begin_min = 0.0f;
    bool have = false;
    double smax = 0.0;
    {
      double s_sh = 0.0, s_ns = 0.0;
      for (long long i = 0; i < n; i++) {
        if (i > 0 && blk[i] != blk[i - 1]) s_sh = 0.0, s_ns = 0.0;
        if (T[kBins - 1] <= r[i].end) continue;  // beyond the grid: dropped
        s_sh += r[i].w_sh, s_ns += r[i].w_ns;
        smax = std::max(smax, std::max(s_sh, s_ns));
        if ((r[i].w_sh > 0.0 || r[i].w_ns > 0.0) && (!have || r[i].begin < begin_min)) begin_min = r[i].begin, have = true;
      }
    }
    if (have) bb_min = bin_of(T, begin_min);
    double grid[COLATE_MAX_AGE_BINS];
    if (colate_age_grid(grid, COLATE_MAX_AGE_BINS) != kBins) return fail(COLATE_EINVAL, "the age grid has not %d points", kBins);
    const int kind0 = 0;
    const double a_min = have ? grid[bb_min] : ep[0];
    const std::vector<double> zeros((size_t)nb[g], 0.0);
    if (int rc = colate::check_bootstrap_interval_batch(B, nb[g], 1, E, &kind0, &a_min, &a_min, bw, zeros.data(), ep, init_rates + (size_t)g * E,
                                                        max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags))
      return group_fail(rc, g);
    // overflow: every cell sum is at most its block's sum of weights (times 1 + n * 2^-52 for the roundings)
    double wmax = 0.0;
    for (size_t i = 0; i < (size_t)B * nb[g]; i++) wmax = std::max(wmax, bw[i]);
    const double tbound = smax * (1.0 + (double)n * 0x1p-52);
    if (tbound <= dmax && wmax * tbound * (double)nb[g] <= 0x1.fffffffffffffp+1022) continue;
    GroupRows rows;
    if (int rc = group_rows_host(n, r, blk, nb[g], T, rows)) return group_fail(rc, g);
    if (rows.R == 0) continue;
    if (int rc = colate::check_bootstrap_interval_batch(B, nb[g], rows.R, E, rows.kinds.data(), rows.age_begin.data(), rows.age_end.data(), bw,
                                                        rows.tables.data(), ep, init_rates + (size_t)g * E, max_iter, min_iter, rel_tol,
                                                        rate_floor, out_rates, out_iters, out_loglik, out_flags))
      return group_fail(rc, g);
  }
  return COLATE_OK;
}

}  // namespace colate_ic

using namespace colate_ic;

extern "C" int colate_interval_fit_groups_host(int G, int B, int E, const long long* rec_off, const colate_interval_rec* recs,
                                               const int* block, const int* nb, const double* block_weights, const double* epochs,
                                               const double* init_rates, int max_iter, int min_iter, double rel_tol,
                                               double rate_floor, int* out_R, long long* out_dropped, double* out_rates,
                                               int* out_iters, double* out_loglik, int* out_flags, int math) {
  if (math != 0 && math != 1) return fail(COLATE_EINVAL, "math must be 0 (<cmath>) or 1 (em_math)");
  float T[kBins];
  if (int rc = build_thresholds(T)) return rc;
  if (int rc = check_groups_args(G, B, E, rec_off, recs, block, nb, block_weights, epochs, init_rates, max_iter, min_iter, rel_tol,
                                 rate_floor, T, out_R, out_dropped, out_rates, out_iters, out_loglik, out_flags))
    return rc;
  // (into copies: a call that fails at a later group leaves the outputs alone)
  const size_t GB = (size_t)G * B;
  std::vector<int> R((size_t)G), iters(GB), flags(GB);
  std::vector<long long> dropped((size_t)G);
  std::vector<double> rates(GB * E), ll(GB);
  size_t w_off = 0;
  for (int g = 0; g < G; g++) {
    const long long n = rec_off[g + 1] - rec_off[g];
    const double* bw = block_weights + w_off;
    w_off += (size_t)B * nb[g];
    GroupRows rows;
    if (int rc = group_rows_host(n, n ? recs + rec_off[g] : nullptr, n ? block + rec_off[g] : nullptr, nb[g], T, rows)) return rc;
    R[(size_t)g] = rows.R, dropped[(size_t)g] = rows.dropped;
    const size_t o = (size_t)g * B;
    if (rows.R == 0) {
      no_rows_results(B, E, init_rates + (size_t)g * E, rates.data() + o * E, iters.data() + o, ll.data() + o, flags.data() + o);
      continue;
    }
    if (int rc = colate_bootstrap_em_interval_batch_host(B, nb[g], rows.R, E, rows.kinds.data(), rows.age_begin.data(), rows.age_end.data(),
                                                         bw, rows.tables.data(), epochs + (size_t)g * E, init_rates + (size_t)g * E,
                                                         max_iter, min_iter, rel_tol, rate_floor, rates.data() + o * E, iters.data() + o,
                                                         ll.data() + o, flags.data() + o, math)) {
      const std::string why = colate_last_error();
      return fail(rc, "group %d: %s", g, why.c_str());
    }
  }
  std::memcpy(out_R, R.data(), sizeof(int) * R.size()), std::memcpy(out_dropped, dropped.data(), sizeof(long long) * dropped.size());
  std::memcpy(out_rates, rates.data(), sizeof(double) * rates.size()), std::memcpy(out_loglik, ll.data(), sizeof(double) * ll.size());
  std::memcpy(out_iters, iters.data(), sizeof(int) * iters.size()), std::memcpy(out_flags, flags.data(), sizeof(int) * flags.size());
  return COLATE_OK;
}
