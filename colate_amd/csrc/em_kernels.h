// colate_amd/csrc/em_kernels.h -- internal launch interface of the EM kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#define COLATE_EM_THREADS 256
#define COLATE_EM_MAX_E 1024  // up to 16 epochs per lane of a 64-lane wave (em_kernels_big.hip beyond 256)
#define COLATE_EM_MAX_A 256  // one age bin per thread

// per-replicate diagnostic flags (the reference aborts on the corresponding asserts)
#define COLATE_FLAG_NAN 1      // coal.cpp:3711-3712, coal_EM.cpp:128-129, 351
#define COLATE_FLAG_NEG 2      // coal.cpp:3713-3714
#define COLATE_FLAG_MAXITER 4  // iteration cap reached without meeting the stop rule
#define COLATE_FLAG_UNRESOLVED 8  // some trailing epochs are below the resolution of the reference's arithmetic
#define COLATE_UNRESOLVED_SHIFT 8 // out_flags >> 8 = number of such trailing epochs

struct ColateEmArgs {
  int B, E, A;
  int mode;                 // 0 = EM to convergence, 1 = one E-step
  const double* age_grid;   // [A]      device
  const double* cnt_sh;     // [B][A]   device
  const double* cnt_ns;     // [B][A]   device
  const double* epochs;     // [E] (epochs_stride 0) or [B][E] (epochs_stride E)
  long epochs_stride;
  const double* rates_in;   // initial rates (mode 0) / rates (mode 1); [E] or [B][E]
  long rates_stride;
  int max_iter, min_iter;
  double rel_tol, rate_floor;
  double* out_rates;  // [B][E] (mode 0)
  int* out_iters;     // [B]    (mode 0)
  double* out_ll;     // [B]
  int* out_flags;     // [B]
  double* out_num;    // [B][E] (mode 1)
  double* out_den;    // [B][E] (mode 1)
  double* ll_trace;   // [B][ll_trace_cap] or NULL: the log-likelihood of every iteration (diagnostic; general loop only)
  int ll_trace_cap;
};

size_t colate_em_lds_bytes(int E, int A);
hipError_t colate_em_launch(const ColateEmArgs& args, hipStream_t stream);
// which build of the kernel a launch of this shape picks on the current device:
// 0 = latency (max-ilp build), 1 = latency (default build), 2 = throughput (em_kernels.hip)
int colate_em_variant(int B, int E);
// force the build for E <= 128 (0, 1, 2 as above; anything else = automatic again)
void colate_em_set_forced_variant(int v);
// the instantiation behind that choice (em_build.hpp: one table, one function; colate_em_launch switches on the same
// result): for `mode` (0 = EM, 1 = one E-step) on the current device under the current forcing; NULL for sizes outside the table
struct EmBuild;
const EmBuild* colate_em_build(int mode, int B, int E);

// block bootstrap on the device (bootstrap_kernel.hip)
hipError_t colate_bootstrap_launch(int B, int nb, int A, const double* age_grid, double age,
                                   const double* weights, const double* sh_block, const double* ns_block,
                                   const double* sh_emp_block, const double* ns_emp_block, double* cnt_sh,
                                   double* cnt_ns, int* status, hipStream_t stream);
// the same for rows [row_lo, row_lo + rows) of G groups x B replicates with per-group tables / weights / ages
// (device arrays indexed from group `group_first`; bootstrap_groups_kernel)
hipError_t colate_bootstrap_groups_launch(int B, int row_lo, int rows, int group_first, int A, const double* age_grid,
                                          const int* group_nb, const long long* group_block_off,
                                          const long long* group_weight_off, const double* group_age,
                                          const double* weights, const double* sh_block, const double* ns_block,
                                          const double* sh_emp_block, const double* ns_emp_block, double* cnt_sh,
                                          double* cnt_ns, int* status, hipStream_t stream);

// the block bootstrap in front of the interval-dated fit (bootstrap_rows_kernel): W[B][R] = block_weights[B][nb] x
// tables[nb][R], per element from 0.0 over k ascending, multiply and add apart.  Device pointers.  _fits: the launch
// has a grid for this shape (B * ceil(R / 256) workgroups below 2^31)
hipError_t colate_bootstrap_rows_launch(int B, int nb, int R, const double* block_weights, const double* tables, double* W,
                                        hipStream_t stream);
bool colate_bootstrap_rows_fits(int B, int R);

// coal_EM::EM_shared / EM_notshared for R calls (kind, age_begin, age_end) against one (epochs[E], rates[E]), one
// wavefront per call (em_interval_kernel.hip; the arithmetic is em_interval.hpp).  Device pointers; weights NULL = no
// accumulated outputs.  The caller has validated the ages (colate::check_interval_calls).
hipError_t colate_em_interval_launch(int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                                     const double* epochs, const double* rates, const double* weights, double* out_num,
                                     double* out_den, double* out_logl, int* out_flags, double* out_num_acc,
                                     double* out_den_acc, double* out_ll, hipStream_t stream);

// colate_em_interval_batch: the EM fit on interval-dated mutations for B replicates that share R rows and weight them
// by weights[B][R], one persistent workgroup per replicate (em_interval_fit_kernel.hip; the calls are those of
// em_interval_kernel.hip, M-step and stop rule are em_interval_fit.hpp).  Device pointers; the caller has validated
// the arguments (colate::check_interval_batch).
#define COLATE_EM_INTERVAL_FIT_WAVES 8  // calls in flight per workgroup at E <= 256 (one beyond)
int colate_em_interval_fit_waves(int E);
hipError_t colate_em_interval_fit_launch(int B, int R, int E, const int* kinds, const double* age_begin,
                                         const double* age_end, const double* weights, const double* epochs,
                                         const double* init_rates, int max_iter, int min_iter, double rel_tol,
                                         double rate_floor, double* out_rates, int* out_iters, double* out_ll,
                                         int* out_flags, hipStream_t stream);

// ---- colate_interval_fit_groups: many groups' cells, rows and fits in one pass (all device pointers) ----
// What a workgroup of the grouped fit reads about its group: the group's R rows, W[B][R], epochs[E] and starting rates[E].
struct ColateIntervalGroup {
  int R;
  const int* kinds;
  const double *age_begin, *age_end;
  const double* W;
  const double *epochs, *init_rates;
};
// colate_em_interval_fit_launch for G groups x B replicates in one launch: workgroup i is replicate i % B of group
// i / B and writes row i of the four outputs.  A group with R < 1 runs no loop and writes nothing (the caller fills in).
hipError_t colate_em_interval_fit_groups_launch(int G, int B, int E, const ColateIntervalGroup* groups, int max_iter,
                                                int min_iter, double rel_tol, double rate_floor, double* out_rates,
                                                int* out_iters, double* out_ll, int* out_flags, hipStream_t stream);

// The rows of a group picked on the device (interval_rows_kernel.hip).  cells: the dense sums of
// colate_interval_cells_launch for the chunk's segments, [segments][2][17205]; group j of the chunk owns the segments
// [seg_off[j], seg_off[j + 1]) and has room for row_cap[j] rows from row_off[j] on in cell_of_row / kinds / age_begin /
// age_end.  flags: scratch, [groups][2 * 17205] bytes.  Out: the group's rows in row order (kind, bb, be) -- the cell
// index kind * 17205 + be * (be + 1) / 2 + bb, the kind and the two ages from age_grid[185] --, R[j], and dropped[j] = the
// sum of seg_dropped over the group's segments.
hipError_t colate_interval_rows_launch(int groups, const double* cells, const int* seg_off, const unsigned long long* seg_dropped,
                                       const double* age_grid, const long long* row_off, const int* row_cap,
                                       unsigned char* flags, int* cell_of_row, int* kinds, double* age_begin, double* age_end,
                                       int* R, long long* dropped, hipStream_t stream);

// bootstrap_rows_kernel for the groups of a chunk, reading the dense sums through the groups' row lists:
// W_j[b][r] = sum_k block_weights_j[b][k] * cells[seg0 + k][cell_of_row[r]], k ascending from 0.0, multiply and add apart.
struct ColateIntervalRowsJob {
  int seg0, nb, R;
  const int* cell_of_row;       // [R]
  const double* block_weights;  // [B][nb]
  double* W;                    // [B][R]
};
hipError_t colate_bootstrap_rows_groups_launch(int groups, int B, int max_R, const ColateIntervalRowsJob* jobs,
                                               const double* cells, hipStream_t stream);
