// colate_amd/csrc/interval_groups.h -- what the two forms of colate_interval_fit_groups share (internal to libcolate_amd.so):
// the argument checks that run before anything is staged, and the host twin's pieces (interval_groups.cpp).
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "colate_amd.h"
#include "interval_cells.h"

namespace colate_ic {

// Everything colate_interval_cells and colate_bootstrap_em_interval_batch would refuse for any of the G groups, found
// without forming the cells where that is possible:
//   * sizes, NULLs, G < 1, a decreasing rec_off, the compiled limits;
//   * per group the records and blocks (check_cells_args), then epochs, starting rates, iteration limits and block
//     weights (check_bootstrap_interval_batch on one stand-in row at the smallest age_begin any of the group's rows can
//     have: the grid point of the smallest begin among its records that are within the grid and carry weight);
//   * an overflowing table entry or weighted block sum: excluded by a bound on the group's weights where that bound is
//     below DBL_MAX / 2, and only otherwise decided on the group's cells, formed on the host.
// T: the thresholds (build_thresholds).  The message names the group.
int check_groups_args(int G, int B, int E, const long long* rec_off, const IntervalRec* recs, const int* block, const int* nb,
                      const double* block_weights, const double* epochs, const double* init_rates, int max_iter, int min_iter,
                      double rel_tol, double rate_floor, const float* T, const int* out_R, const long long* out_dropped,
                      const double* out_rates, const int* out_iters, const double* out_loglik, const int* out_flags);

// room for the rows of a group of n records: a record flags at most one cell of each kind
inline int row_cap(long long n) { return (int)(2 * n < COLATE_INTERVAL_MAX_ROWS ? 2 * n : COLATE_INTERVAL_MAX_ROWS); }

// The chunks of a grouped device call: runs [g0, g1) of consecutive groups that share device scratch, covering [0, G) in order.
// A chunk holds at most 65535 groups (a grid dimension), at most budget_segs segments (nb summed; clamped to at least 1) and at
// most max_chunk_recs records (rec_off[g1] - rec_off[g0]); a group that exceeds a budget goes alone.
std::vector<std::pair<int, int>> plan_chunks(int G, const int* nb, const long long* rec_off, size_t budget_segs, long long max_chunk_recs);
// a budget in MB from the environment variable `name` (negative: 0), or default_mb where it is not set
long long env_budget_mb(const char* name, long long default_mb);

// row[E] repeated to [G][E]: one set of epochs or starting rates for all groups, as the grouped fit takes them
inline std::vector<double> repeat_rows(const double* row, int E, int G) {
  std::vector<double> out;
  for (int g = 0; g < G; g++) out.insert(out.end(), row, row + E);
  return out;
}

// the results of a group without rows: its starting rates, and zeros
void no_rows_results(int B, int E, const double* init_rates, double* rates, int* iters, double* loglik, int* flags);

}  // namespace colate_ic
