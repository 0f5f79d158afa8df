// colate_amd/csrc/colate_internal.h -- shared between the translation units of libcolate_amd.so
#pragma once
#include <cstddef>
#include <cstring>
namespace colate {
// records the message for colate_last_error() and returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// COLATE_OK, or COLATE_ENODEVICE with a message (there is no CPU fallback)
int ensure_device();
// the grids the kernel's contiguous-segment logic relies on: age_grid non-negative and non-decreasing, epochs
// non-decreasing, epochs[0] <= age_grid[0] (every host-pointer entry point runs this before anything is launched)
int check_grids(int E, int A, const double* age_grid, const double* epochs);
// the argument checks of colate_em_interval_calls[_host] (em_interval_host.cpp): sizes, NULLs, non-decreasing epochs,
// kinds 0 / 1, finite ages with 0 <= epochs[0] <= age_begin <= age_end
int check_interval_calls(int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                         const double* epochs, const double* rates, const double* weights, const double* out_num,
                         const double* out_den, const double* out_logl, const int* out_flags, const double* out_num_acc,
                         const double* out_den_acc, const double* out_ll);
// the argument checks of colate_em_interval_batch[_host] (em_interval_host.cpp): check_interval_calls for the rows and
// the grid, plus B, R >= 1, finite weights >= 0, the iteration limits, rel_tol, rate_floor and the starting rates
int check_interval_batch(int B, int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                         const double* weights, const double* epochs, const double* init_rates, int max_iter, int min_iter,
                         double rel_tol, double rate_floor, const double* out_rates, const int* out_iters,
                         const double* out_loglik, const int* out_flags);
// the argument checks of colate_bootstrap_em_interval_batch[_host] (em_interval_host.cpp): those of check_interval_batch with
// the block weights [B][nb] and the row tables [nb][R] for the weights: nb >= 1, every entry of both finite and >= 0, and no
// weighted block sum W[b][r] that overflows to infinity
int check_bootstrap_interval_batch(int B, int nb, int R, int E, const int* kinds, const double* age_begin,
                                   const double* age_end, const double* block_weights, const double* tables,
                                   const double* epochs, const double* init_rates, int max_iter, int min_iter,
                                   double rel_tol, double rate_floor, const double* out_rates, const int* out_iters,
                                   const double* out_loglik, const int* out_flags);
// Set (process-wide, never cleared) by every entry point that makes this process talk to the HIP runtime.  A process
// that has done so must not fork() children that use the GPU: `Colate --ranks N` (run_ranked, mut_driver.cpp) refuses
// when it is set (colate_device_touched, include/colate_amd.h).
void mark_device_touched();
// A named range for profilers (rocprofv3 --marker-trace): roctxRangePush / roctxRangePop, bound lazily with dlopen so that the
// library has no link-time dependency on a profiler; a no-op where librocprofiler-sdk-roctx / libroctx64 is not present.
struct ProfRange {
  explicit ProfRange(const char* name);
  ~ProfRange();
  ProfRange(const ProfRange&) = delete;
  ProfRange& operator=(const ProfRange&) = delete;
};
// rows [lo, hi) of a per-group [.][E] array (its first row is group `group_first`; row r belongs to group r / B) as
// the per-row [hi - lo][E] array the EM kernel reads
inline void expand_group_rows(const double* per_group, int B, int group_first, long lo, long hi, int E, double* per_row) {
  for (long r = lo; r < hi; r++)
    std::memcpy(per_row + (size_t)(r - lo) * E, per_group + (size_t)(r / B - group_first) * E, (size_t)E * sizeof(double));
}
}  // namespace colate
