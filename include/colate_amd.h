/* include/colate_amd.h -- C ABI of libcolate_amd.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE path of leospeidel/Colate: `Colate --mode mut` on
 * precomputed .colate.in inputs, i.e. the block-bootstrap driver and the EM loop
 * that turns age-binned shared / not-shared mutation counts into pairwise
 * coalescence rates.  The reference has no FFI; its de-facto boundary is the C++
 * class `coal_EM` (include/coal/coal_EM.hpp:14-63) used at exactly one site,
 * include/coal/coal.cpp:3698-3721, inside the per-replicate EM loop
 * include/coal/coal.cpp:3675-3827.  Calling a GPU once per age bin would be
 * meaningless, so the replacement boundary is one coarse call per batch of
 * bootstrap replicates (colate_em_batch), plus the single E-step
 * (colate_em_estep) that corresponds to one pass of coal.cpp:3698-3733.
 * Mutations dated to an interval (coal_EM with age_begin < age_end, which the
 * reference wrote and tested but never put a loop around) have the same two
 * levels: colate_em_interval_calls is one E-step over a list of calls,
 * colate_em_interval_batch the whole EM fit for a batch of replicates, and
 * colate_bootstrap_em_interval_batch that fit with the block bootstrap in front
 * of it: per-block row tables and block weights in, rates out (the weighted
 * block sums run from 0.0 over the blocks in ascending order, multiply and add
 * apart; its speed has not been measured).  `Colate --mode mut_interval` is the
 * command line of the last one; colate_interval_fit_groups does it for many pairs
 * of samples in one pass, from their used SNPs to their rates.
 * INTEGRATION.md shows the patch a maintainer would apply to coal.cpp.
 *
 * Conventions: plain pointers and sizes, row-major, IEEE double; caller owns
 * every buffer; the library keeps no state between calls besides the selected
 * device.  Every function returns 0 on success or a negative COLATE_E* code and
 * never aborts; colate_last_error() gives a message.  "_device" variants take
 * pointers to device (HBM) memory and enqueue on a HIP stream without
 * synchronising; the plain variants take host pointers and are synchronous.
 * There is NO CPU fallback: without a usable HIP device the compute entry
 * points fail with COLATE_ENODEVICE.
 */
#ifndef COLATE_AMD_H
#define COLATE_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define COLATE_OK 0
#define COLATE_EINVAL (-1)    /* bad argument (sizes, NULL, unsorted grids, ...) */
#define COLATE_ENODEVICE (-2) /* no usable HIP device                            */
#define COLATE_EHIP (-3)      /* a HIP runtime call failed                       */
#define COLATE_ELIMIT (-4)    /* E above 1024 or A above 256 (compiled limits)   */
#define COLATE_EIO (-5)       /* file could not be read / written                */

/* per-replicate flags in out_flags[]: conditions on which the reference aborts
 * through assert() (coal.cpp:3711-3714, coal_EM.cpp:128-129, 351) or that it
 * cannot report (iteration cap) */
#define COLATE_FLAG_NAN 1
#define COLATE_FLAG_NEG 2
#define COLATE_FLAG_MAXITER 4
/* Not an error: the last COLATE_UNRESOLVED_EPOCHS(flags) epochs of this replicate are below the resolution of the
 * reference's own arithmetic -- the survival probability there is so small that the `integ` term of its denominators
 * (coal_EM.cpp:270-274, 445-449) is rounding residue, and the reference's printed rate changes by more than 1e-8
 * (relative; by orders of magnitude a few epochs further on) when its libm's exp()/log() return a neighbouring double.
 * Rates of such epochs are returned (deep in that regime they are the floor, as in the reference) but are outside the
 * 1e-6 parity claim; all other epochs are inside it.  out_flags == 0 therefore still means: clean and fully
 * reproducible.  With --bins 3,7,0.2 (23 epochs) no epoch is ever unresolved on whole-genome tables; with
 * --bins 2,7.95,0.05 (122 epochs) the last ~17 are (profiles/parity/).  The verdict is about the
 * fixed point: it is made for runs that end by the stop rule at the reference's tolerance (COLATE_DEFAULT_REL_TOL); a run cut
 * by max_iter (COLATE_FLAG_MAXITER) or stopped at a looser tolerance still carries its path. */
#define COLATE_FLAG_UNRESOLVED 8
/* the error-like bits (NAN | NEG | MAXITER): COLATE_STATUS_FLAGS(f) != 0 means "the reference would have aborted, or the
 * iteration cap ended the run"; COLATE_FLAG_UNRESOLVED is deliberately not part of it */
#define COLATE_STATUS_FLAGS(flags) ((flags) & 0x07)
#define COLATE_UNRESOLVED_EPOCHS(flags) ((int)((unsigned)(flags) >> 8))

/* compiled limits of the EM kernel: up to 16 epochs per lane of a 64-lane wave (the reference builds any number of epochs,
 * coal.cpp:3551-3632: `--bins 3,7,0.01` gives 404; beyond 256 a slower instantiation runs), one age bin per thread */
#define COLATE_MAX_EPOCHS 1024
#define COLATE_MAX_AGE_BINS 256

/* reference defaults (coal.cpp:3656, 3822, 3798-3803, 3636) */
#define COLATE_DEFAULT_MAX_ITER 100000
#define COLATE_DEFAULT_MIN_ITER 1000
#define COLATE_DEFAULT_REL_TOL 1e-7
#define COLATE_DEFAULT_RATE_FLOOR 5e-9
#define COLATE_DEFAULT_INIT_RATE (1.0 / 20000.0)

const char* colate_version(void);
const char* colate_last_error(void);
int colate_device_count(void);       /* >= 0, or COLATE_ENODEVICE */
int colate_set_device(int ordinal);  /* device used by the calling thread's later calls */
/* Creates the device's HIP context now (from any thread) instead of inside the first compute call: lets a host overlap
 * the few hundred ms a fresh process pays for it with its own input parsing.  No reference counterpart (CPU code). */
int colate_warm_up(int ordinal);
/* 1 once this process has talked to the HIP runtime through this library (any compute or device entry point), else 0.
 * Such a process must not fork() children that use the GPU: colate_mut_main refuses `--ranks N` (which forks one
 * process per GPU) when this is set -- start `Colate --ranks N` as a fresh process instead. */
int colate_device_touched(void);
/* Diagnostic: which build of the EM kernel a batch of this shape runs on the current device
 * (0 latency/max-ilp, 1 latency/default scheduler, 2 throughput), or a negative code. */
int colate_em_kernel_variant(int B, int E);
/* Diagnostic: force that choice for E <= 128 (0, 1 or 2; any other value = automatic again).  Process-wide.  The
 * environment variable COLATE_EM_VARIANT=latency-ilp|latency|throughput sets the initial value (read once). */
int colate_em_force_variant(int variant);
/* Diagnostic: the name of the instantiation behind that choice, `unit-kind/NCHxEROWS`: unit ilp |
 * default | big = the translation unit and its scheduler; kind free | capped | tput | estep; NCH epochs per lane;
 * EROWS 16-lane rows of epochs.  E.g. `ilp-capped/1x4`: what a batch of #CUs < B <= 2 #CUs replicates at 33 .. 64 epochs runs.
 * The launch switches on the same table entry that is named here.  Each call writes a NUL-terminated string into
 * name[cap] and returns its length, or a negative code.
 *   colate_em_kernel_build       the EM fit of B replicates x E epochs on the current device, under the current forcing
 *   colate_em_kernel_build_for   the same from given numbers, no device asked: mode 0 = EM fit, 1 = one E-step; cus = the
 *                                device's compute units (0 = unknown); forced = -1 or colate_em_force_variant's value
 *   colate_em_kernel_builds      every name the dispatch can return for `mode`, newline-separated */
int colate_em_kernel_build(int B, int E, char* name, int cap);
int colate_em_kernel_build_for(int mode, int B, int E, int cus, int forced, char* name, int cap);
int colate_em_kernel_builds(int mode, char* buf, int cap);

/* ---- the EM hot path ------------------------------------------------------
 * Replaces coal.cpp:3675-3827 (bootstrap EM driver: coal_EM construction,
 * EM_shared/EM_notshared per age bin, accumulation, M-step, floor, stop rule)
 * for B replicates at once.
 *   age_grid[A]            ascending age-bin representatives (coal.cpp:3126-3137; A = 185)
 *   cnt_shared[B][A], cnt_notshared[B][A]   bootstrap count tables (coal.cpp:3344-3451)
 *   epochs[E]              epoch starts in generations, epochs[0] <= age_grid[0], non-decreasing
 *   init_rates[E]          starting rates (coal.cpp:3636-3646)
 *   max_iter, min_iter, rel_tol, rate_floor   100000, 1000, 1e-7, 5e-9 in the reference
 *   out_rates[B][E], out_iters[B] (the reference's "Total iterations"), out_loglik[B], out_flags[B]
 */
int colate_em_batch(int B, int E, int A, const double* age_grid, const double* cnt_shared,
                    const double* cnt_notshared, const double* epochs, const double* init_rates,
                    int max_iter, int min_iter, double rel_tol, double rate_floor,
                    double* out_rates, int* out_iters, double* out_loglik, int* out_flags);

/* Same, all pointers in device memory, asynchronous on `hip_stream` (a
 * hipStream_t, NULL = default stream).  epochs_per_replicate / rates_per_replicate
 * != 0 select [B][E] layouts for epochs / init_rates (batched all-pairs, where
 * every (target, reference) pair brings its own epochs); 0 = one shared [E] row.
 * Host-side argument checks that need the data (sortedness) are skipped. */
int colate_em_batch_device(int B, int E, int A, const double* age_grid, const double* cnt_shared,
                           const double* cnt_notshared, const double* epochs,
                           int epochs_per_replicate, const double* init_rates,
                           int rates_per_replicate, int max_iter, int min_iter, double rel_tol,
                           double rate_floor, double* out_rates, int* out_iters,
                           double* out_loglik, int* out_flags, void* hip_stream);

/* Host-pointer variant with epochs[B][E] and init_rates[B][E] per replicate: one launch for many
 * (target, reference) pairs whose epochs differ (an ancient sample inserts its age as an epoch,
 * coal.cpp:3597-3624); all rows must have the same E.  Used by `Colate --pairs` (batched all-pairs). */
int colate_em_batch_rows(int B, int E, int A, const double* age_grid, const double* cnt_shared,
                         const double* cnt_notshared, const double* epochs, const double* init_rates,
                         int max_iter, int min_iter, double rel_tol, double rate_floor,
                         double* out_rates, int* out_iters, double* out_loglik, int* out_flags);

/* Host-pointer variant that shards the B replicates over several GPUs of the node from ONE
 * process: contiguous, balanced ranges (replicate i of device d = global lo_d + i), one stream per
 * device, all launches in flight together, results gathered in replicate order.  `devices` lists
 * `num_devices` HIP ordinals (an ordinal may repeat: its shards then share that GPU).  The
 * one-process-per-GPU form of the same sharding (torch.distributed + RCCL all-gather) is
 * colate_amd/distributed.py; there is no exchange between shards inside the EM. */
int colate_em_batch_sharded(int num_devices, const int* devices, int B, int E, int A,
                            const double* age_grid, const double* cnt_shared,
                            const double* cnt_notshared, const double* epochs,
                            const double* init_rates, int max_iter, int min_iter, double rel_tol,
                            double rate_floor, double* out_rates, int* out_iters, double* out_loglik,
                            int* out_flags);

/* The same sharding for the per-row form (epochs[B][E], init_rates[B][E], as colate_em_batch_rows):
 * the batched all-pairs run over several GPUs. */
int colate_em_batch_rows_sharded(int num_devices, const int* devices, int B, int E, int A,
                                 const double* age_grid, const double* cnt_shared,
                                 const double* cnt_notshared, const double* epochs,
                                 const double* init_rates, int max_iter, int min_iter, double rel_tol,
                                 double rate_floor, double* out_rates, int* out_iters,
                                 double* out_loglik, int* out_flags);

/* The same sharding for the two calls that bootstrap on the device: the arguments after `devices` are those of
 * colate_bootstrap_em_batch / colate_bootstrap_em_batch_groups below.  Every shard uploads only what its rows read
 * (its replicates' weights; in the groups form the tables, weights, ages and epochs of the groups its rows belong
 * to -- a shard may begin and end inside a group), runs the bootstrap kernel and the EM kernel on its device, and
 * the outputs (out_cnt_* included, may be NULL) come back in row order, bit-identical to the one-device call.  A
 * sample age outside the age grid in any shard fails the whole call (COLATE_EINVAL). */
int colate_bootstrap_em_batch_sharded(int num_devices, const int* devices, int B, int nb, int E, int A,
                                      const double* age_grid, double age, const double* weights,
                                      const double* sh_block, const double* ns_block, const double* sh_emp_block,
                                      const double* ns_emp_block, const double* epochs, const double* init_rates,
                                      int max_iter, int min_iter, double rel_tol, double rate_floor,
                                      double* out_rates, int* out_iters, double* out_loglik, int* out_flags,
                                      double* out_cnt_shared, double* out_cnt_notshared);
int colate_bootstrap_em_batch_groups_sharded(int num_devices, const int* devices, int G, int B, int E, int A,
                                             const double* age_grid, const int* group_nb, const double* group_age,
                                             const double* weights, const double* sh_block, const double* ns_block,
                                             const double* sh_emp_block, const double* ns_emp_block,
                                             const double* epochs, const double* init_rates, int max_iter,
                                             int min_iter, double rel_tol, double rate_floor, double* out_rates,
                                             int* out_iters, double* out_loglik, int* out_flags,
                                             double* out_cnt_shared, double* out_cnt_notshared);

/* One E-step = one pass of coal.cpp:3698-3733 for each of B replicates with the
 * rates given per replicate: rates[B][E] -> num_acc[B][E], den_acc[B][E]
 * (coal_rates_num / coal_rates_denom), loglik[B], flags[B]. */
int colate_em_estep(int B, int E, int A, const double* age_grid, const double* cnt_shared,
                    const double* cnt_notshared, const double* epochs, const double* rates,
                    double* num_acc, double* den_acc, double* loglik, int* flags);
int colate_em_estep_device(int B, int E, int A, const double* age_grid, const double* cnt_shared,
                           const double* cnt_notshared, const double* epochs, const double* rates,
                           double* num_acc, double* den_acc, double* loglik, int* flags,
                           void* hip_stream);

/* Interval-dated mutations: coal_EM::EM_shared (kinds[r] = 0) / EM_notshared (kinds[r] = 1) of the reference
 * (coal_EM.cpp:153-468) for R calls (age_begin[r], age_end[r]) against one (epochs[E], rates[E]) -- the reference's
 * exact treatment of a mutation whose age is uniform on its branch.  out_num[R][E], out_den[R][E] and out_logl[R] are
 * what one call of the reference leaves in num / denom and returns (zeros and 0 where its normaliser is not finite);
 * out_flags[R] carries COLATE_FLAG_NAN / COLATE_FLAG_NEG.  With weights[R] (NULL: none, the three outputs are not
 * touched) the calls are also summed as one E-step of coal.cpp:3704-3733 with weights for counts, rows with
 * weight > 0 in ascending order: out_num_acc[E], out_den_acc[E], *out_ll.
 * Refused (COLATE_EINVAL): age_begin > age_end, a negative, infinite or NaN age, an age before epochs[0].  An interval
 * may reach into the open last epoch: the reference's own test does (test_aDNA.cpp:187-208; coal_EM.cpp:406-416).
 * Rows with age_begin == age_end are allowed and give colate_em_estep's per-bin result (same formulas, to the last
 * few bits).
 * colate_em_interval_calls runs on the calling thread's device (one wavefront per call, csrc/em_interval_kernel.hip);
 * _host runs the same source (csrc/em_interval.hpp) on the CPU, math = 0 with <cmath> -- bit for bit the reference
 * on the same libm -- and math = 1 with the kernels' own exp / log -- bit for bit the device. */
int colate_em_interval_calls(int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                             const double* epochs, const double* rates, const double* weights, double* out_num,
                             double* out_den, double* out_logl, int* out_flags, double* out_num_acc,
                             double* out_den_acc, double* out_ll);
int colate_em_interval_calls_host(int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                                  const double* epochs, const double* rates, const double* weights, double* out_num,
                                  double* out_den, double* out_logl, int* out_flags, double* out_num_acc,
                                  double* out_den_acc, double* out_ll, int math);

/* The EM fit on interval-dated mutations: coal.cpp:3675-3827 with the R rows (kinds[r], age_begin[r], age_end[r]) of
 * colate_em_interval_calls for age bins, for B replicates that share the rows and weight row r by weights[b][r] (the
 * bootstrap-weighted count; finite, >= 0).  One iteration constructs coal_EM(epochs, rates_b), calls every row with
 * weights[b][r] > 0 in ascending r, sums num_acc[e] += w * num[e], den_acc[e] += w * den[e], ll += w * logl in that
 * order (a call whose normaliser is not finite contributes zeros and 0), then runs the M-step with its floor
 * (coal.cpp:3771-3815, regularise == 2: num == 0 -> the rate of the epoch before, 0 at e == 0; den == 0 -> unchanged)
 * and the stop test ll / prev_ll > 1 - rel_tol && iter > min_iter, prev_ll starting at log(0).
 * out_rates[B][E], out_iters[B], out_loglik[B], out_flags[B] as for colate_em_batch: out_iters is the reference's
 * "Total iterations", COLATE_FLAG_MAXITER says that max_iter ended the run, COLATE_FLAG_NAN / COLATE_FLAG_NEG are OR-ed
 * over all calls of all iterations.  COLATE_FLAG_UNRESOLVED is never set here: the tail model behind it (DESIGN.md
 * section 6) belongs to the point kernel of colate_em_batch, the interval fit has no such verdict.
 * Refused (COLATE_EINVAL, before anything is staged): what colate_em_interval_calls refuses for the rows and epochs,
 * B < 1, R < 1, a negative or non-finite weight, min_iter < 0, max_iter < 1, rel_tol not finite or <= 0,
 * rate_floor < 0, a negative or non-finite init_rates entry.  E <= COLATE_MAX_EPOCHS (COLATE_ELIMIT).
 * colate_em_interval_batch keeps the whole loop on the calling thread's device (one persistent workgroup per replicate,
 * csrc/em_interval_fit_kernel.hip; COLATE_ENODEVICE without one, there is no fall-back); _host is the same loop on the
 * CPU, math = 0 with <cmath> -- bit for bit the reference's loop on the same libm -- and math = 1 with the kernels' own
 * exp / log -- bit for bit the device. */
int colate_em_interval_batch(int B, int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                             const double* weights, const double* epochs, const double* init_rates, int max_iter,
                             int min_iter, double rel_tol, double rate_floor, double* out_rates, int* out_iters,
                             double* out_loglik, int* out_flags);
int colate_em_interval_batch_host(int B, int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                                  const double* weights, const double* epochs, const double* init_rates, int max_iter,
                                  int min_iter, double rel_tol, double rate_floor, double* out_rates, int* out_iters,
                                  double* out_loglik, int* out_flags, int math);
/* Diagnostic: how many rows a workgroup of colate_em_interval_batch calls at a time for this E (no device needed). */
int colate_em_interval_batch_waves(int E);

/* The block bootstrap in front of that fit: per genome block k a table of the R rows' weights, tables[nb][R], and per
 * replicate the block weights block_weights[B][nb] (colate_bootstrap_weights draws them); the fit runs on
 *   W[b][r] = sum_k block_weights[b][k] * tables[k][r]
 * -- coal.cpp:3358-3390 with rows for age bins.  Summation order (the contract, on the device and on the host): per
 * (b, r) the sum starts at 0.0 and runs over k ascending; every product is rounded, then added (no fused multiply-add,
 * no atomics, no tree).  colate_bootstrap_em_interval_batch stages the inputs once, runs the bootstrap kernel
 * (csrc/bootstrap_kernel.hip, one thread per (b, r)) and the fit kernel back to back on one stream -- W stays in device
 * memory, nothing is copied back or waited for before the results -- and returns what colate_em_interval_batch returns
 * on that W, bit for bit.  COLATE_ENODEVICE without a device, there is no fall-back.  _host: the same on the CPU (math
 * as for colate_em_interval_batch_host; math = 1 is bit for bit the device).  colate_bootstrap_rows_host: W alone, the
 * host twin of the bootstrap kernel.
 * Refused (COLATE_EINVAL, before anything is staged; the outputs are not touched): everything colate_em_interval_batch
 * refuses, nb < 1, a negative or non-finite block weight or table entry, a W entry that overflows to infinity.
 * Speed: not measured on a device yet (tools/em_interval_bootstrap_bench.py is the measurement: this call against W
 * formed on the host plus colate_em_interval_batch). */
int colate_bootstrap_em_interval_batch(int B, int nb, int R, int E, const int* kinds, const double* age_begin,
                                       const double* age_end, const double* block_weights, const double* tables,
                                       const double* epochs, const double* init_rates, int max_iter, int min_iter,
                                       double rel_tol, double rate_floor, double* out_rates, int* out_iters,
                                       double* out_loglik, int* out_flags);
int colate_bootstrap_em_interval_batch_host(int B, int nb, int R, int E, const int* kinds, const double* age_begin,
                                            const double* age_end, const double* block_weights, const double* tables,
                                            const double* epochs, const double* init_rates, int max_iter, int min_iter,
                                            double rel_tol, double rate_floor, double* out_rates, int* out_iters,
                                            double* out_loglik, int* out_flags, int math);
int colate_bootstrap_rows_host(int B, int nb, int R, const double* block_weights, const double* tables, double* W);

/* ---- from used SNPs to the rows and tables of that call (csrc/interval_cells.h) ----
 * `--mode mut` spreads a used SNP's weight over 100 ages drawn uniformly on [age_begin, age_end] (coal.cpp:2245-2297);
 * the interval fit treats that uniform distribution exactly, so here a used SNP is one observation of each kind and
 * nothing is drawn.  A record is one used SNP: its float ages as the walk holds them (age_begin clamped to the sample
 * age 0) and its weights f_DAF_target * DAF_ref / N_ref (shared) and the same with f_AAF_target (not shared).  Ages are
 * snapped to the 185-point age grid: bb = bin(begin), be = bin(end), bin(x) = max(0, (int)round(log(10 x) * 10) + 1)
 * (coal.cpp:2265) on the float widened to double; the cell (kind, bb, be) is the row age_begin = age_grid[bb], age_end =
 * age_grid[be] of that kind (bb == be: a point row; begin <= 0, the reference's F path: an ordinary row from 0); a
 * record with be >= 185 lies beyond the grid and is dropped.
 * colate_interval_bin_thresholds: T185[n - 1], n = 1 .. 185, is the smallest float whose bin is >= n -- located by
 * bisection over float bit patterns on the library expression and checked at both neighbouring floats (COLATE_EINVAL
 * where it is not such a step) -- so that bin(x) = #{n : T[n - 1] <= x}.  Both calls below bin through this table.
 * Summation order (the contract, on the device and on the host): per (genome block, kind, bb, be) the sum starts at 0.0
 * and adds the records' weights in record order, every addition rounded (no floating-point atomics, no partial sums).
 * block[n]: the genome block of every record, in [0, nb), not decreasing.  Out: the R rows are the cells with a positive
 * sum in at least one block, ordered by kind (0 = shared first), bb, be: kinds / age_begin / age_end[R] and
 * tables[nb][R] -- what colate_bootstrap_em_interval_batch takes --, *dropped the records beyond the grid.  Returns R
 * (>= 0; n = 0 gives 0) or a negative code.  The caller gives room for max_rows rows (tables: nb * max_rows doubles,
 * filled as [nb][R]); COLATE_INTERVAL_MAX_ROWS always suffices, R above max_rows is COLATE_EINVAL.
 * Refused (COLATE_EINVAL, before anything is staged; the outputs are not touched): a NaN or negative age, begin > end,
 * a negative or non-finite weight, a block index outside [0, nb) or out of order, nb < 1.  nb above
 * COLATE_INTERVAL_MAX_BLOCKS: COLATE_ELIMIT.
 * colate_interval_cells bins and sums on the calling thread's device (csrc/interval_cells_kernel.hip: a thread per
 * record, then one wave per (block, tile of the (bb, be) triangle) that resolves equal cells in lane order through
 * LDS); the rows are picked on the host after one copy.  COLATE_ENODEVICE without a device, there is no fall-back.
 * _host: the host twin, the same doubles.  colate_interval_cells_tile: diagnostic, the cells per tile of the kernel
 * (tile t covers the triangular indices be * (be + 1) / 2 + bb in [t * tile, (t + 1) * tile); no device needed).
 * Speed (one MI355X, tools/interval_cells_bench.py, profiles/interval/interval_cells_bench.json): 8.8 M records in 110
 * blocks take 0.035 s on the device (0.21 s for a process's first call) against 0.32 s for the host twin; 10 000 records
 * take about half a millisecond either way. */
#define COLATE_INTERVAL_BINS 185
#define COLATE_INTERVAL_MAX_ROWS (COLATE_INTERVAL_BINS * (COLATE_INTERVAL_BINS + 1))
#define COLATE_INTERVAL_MAX_BLOCKS 4096
typedef struct colate_interval_rec {
  float begin, end;
  double w_sh, w_ns;
} colate_interval_rec;
int colate_interval_bin_thresholds(float* T185);
int colate_interval_cells(long long n, const colate_interval_rec* recs, const int* block, int nb, int max_rows, int* kinds,
                          double* age_begin, double* age_end, double* tables, long long* dropped);
int colate_interval_cells_host(long long n, const colate_interval_rec* recs, const int* block, int nb, int max_rows,
                               int* kinds, double* age_begin, double* age_end, double* tables, long long* dropped);
int colate_interval_cells_tile(void);

/* ---- many groups' cells, rows and fits in one pass ----
 * colate_interval_fit_groups is, for each of G groups (a group: the used SNPs of one pair of samples),
 * colate_interval_cells on the group's records followed by colate_bootstrap_em_interval_batch on the rows and tables of
 * that call, with the group's block weights, epochs and starting rates -- in one call, without the dense cell sums or W
 * ever reaching the host.  Group g owns the records [rec_off[g], rec_off[g + 1]) of recs / block; block[i] is the genome
 * block of record i within its group, in [0, nb[g]), not decreasing within the group; block_weights holds the groups'
 * [B][nb[g]] arrays one after the other; epochs and init_rates are [G][E].
 * Contract, for every group g: out_R[g] and out_dropped[g] are what colate_interval_cells returns on the group's records;
 * out_rates[g][B][E], out_iters / out_loglik / out_flags[g][B] are, in every bit, what
 * colate_bootstrap_em_interval_batch returns on the rows and tables of that cells call -- the summation contracts above
 * are unchanged: cells from 0.0 in record order, W[b][r] from 0.0 over the blocks ascending with every product rounded and
 * then added, and the fit visits the rows with a positive weight in ascending r (kind, bb, be).  A group with no row
 * (out_R[g] = 0: no records, or all beyond the grid or without weight) keeps its starting rates; its iters, loglik and
 * flags are 0.
 * On the device (COLATE_ENODEVICE without one, there is no fall-back), all on one stream: the groups pass through the
 * cells kernels (csrc/interval_cells_kernel.hip, segments = (group, block)), the row pick (csrc/interval_rows_kernel.hip:
 * a flag per cell, then the rank of every flagged cell in row order by an integer scan) and the grouped row bootstrap
 * (csrc/bootstrap_kernel.hip, reading the dense sums through the row lists) in chunks -- runs of consecutive groups whose
 * dense sums (275 KB per segment) fit COLATE_INTERVAL_GROUPS_CELLS_MB_DEFAULT megabytes, or what the environment
 * variable COLATE_INTERVAL_GROUPS_CELLS_MB says; a larger group goes alone.  Per chunk the host waits once, for the
 * chunk's R and dropped counts, which size its W.  Then one launch of G x B persistent workgroups fits all groups
 * (csrc/em_interval_fit_kernel.hip: workgroup i is replicate i % B of group i / B; the body is that of
 * colate_em_interval_batch).  The chunking changes no bit.
 * _host: the host twin, group by group through colate_interval_cells_host and colate_bootstrap_em_interval_batch_host
 * (math as there; math = 1 is bit for bit the device).
 * Refused (COLATE_EINVAL, before anything is staged; the outputs are not touched; the message names the group): G < 1,
 * B < 1, a decreasing rec_off, and per group whatever the two calls refuse.  COLATE_ELIMIT: E above 1024, nb[g] above
 * COLATE_INTERVAL_MAX_BLOCKS, G x B at or above 2^31, B above 65535.
 * Speed: not measured on a device yet (tools/interval_pairs_bench.py is the measurement). */
#define COLATE_INTERVAL_GROUPS_CELLS_MB_DEFAULT 1024
int colate_interval_fit_groups(int G, int B, int E, const long long* rec_off, const colate_interval_rec* recs, const int* block,
                               const int* nb, const double* block_weights, const double* epochs, const double* init_rates,
                               int max_iter, int min_iter, double rel_tol, double rate_floor, int* out_R, long long* out_dropped,
                               double* out_rates, int* out_iters, double* out_loglik, int* out_flags);
/* Diagnostic: the seconds the kernels of the calling thread's last colate_interval_fit_groups took on the device (hip events
 * around the cells and row-pick kernels and the row bootstrap of every chunk, and around the fit; copies and waits excluded). */
double colate_interval_fit_groups_kernel_seconds(void);
int colate_interval_fit_groups_host(int G, int B, int E, const long long* rec_off, const colate_interval_rec* recs,
                                    const int* block, const int* nb, const double* block_weights, const double* epochs,
                                    const double* init_rates, int max_iter, int min_iter, double rel_tol, double rate_floor,
                                    int* out_R, long long* out_dropped, double* out_rates, int* out_iters, double* out_loglik,
                                    int* out_flags, int math);

/* ---- the pair walk over per-sample walk indices: every pair of a sample list (csrc/interval_walk.h) ----
 * What a pair's walk needs of a sample is one 8-byte entry per .mut row (colate_walk_idx: the position of the sample's
 * record in front of the row's lower bound, -2 for none, and the lower bound's counts where position and alleles match,
 * else 0, 0), so N samples need N such arrays, not N^2 arrays of records.  Inputs: the rows of C chromosomes back to
 * back, chromosome c owning rows [row_off[c], row_off[c + 1]), row_off[0] = 0, positions not negative and not
 * descending within a chromosome; idx[S][n], n = row_off[C]; masks[M][words], one bit per row (set: the row passes), each
 * chromosome starting on a 64-bit word (words = the sum over c of ceil(rows of c / 64); bit i & 63 of word i >> 6 of the
 * chromosome is its row i); pairs[P] of sample ids and mask ids (-1: no mask).
 * The walk, per pair and chromosome, rows in order, states searched = ref_pass = -1, pos(-1) = -1: a row whose bit is
 * clear in the target's or the reference's mask changes nothing; otherwise ref_from = searched, searched = i, and with
 * r = idx[reference][i] the row is skipped if r.DAF == 0 or r.prev_bp < pos(ref_from); otherwise tgt_from = ref_pass,
 * ref_pass = i, and with t = idx[target][i] it is skipped if (t.DAF | t.AAF) == 0 or t.prev_bp < pos(tgt_from);
 * otherwise it is used.  A used row is one colate_interval_rec: begin = (float)max(age_begin, 0), end = age_end,
 * f = roundf((float)((double)(float)t.DAF / ((t.DAF + t.AAF) / 2.0))), w_sh = (double)(f * (float)r.DAF) /
 * (double)(r.DAF + r.AAF), w_ns the same from t.AAF.  Its block within the chromosome is k(pos) = (pos - 1) /
 * num_bases_per_block (0 for pos <= 0); a chromosome has k(pos of its last used row) + 1 blocks, or 1 without a used
 * row; block[] numbers them through the pair's chromosomes, nb[p] is their number.  Records are ordered by chromosome,
 * then row.  This is, byte for byte, what the engine's walk of `--mode mut_interval` collects for the pair.
 * Out: rec_off[P + 1] (rec_off[0] = 0), nb[P], and the pairs' records and blocks back to back in recs / block, which
 * have room for cap records.  A total above cap is COLATE_ELIMIT with the needed total in colate_last_error(); nothing
 * is written then.
 * colate_interval_walk runs two passes on one stream of the calling thread's device (csrc/interval_walk_kernel.hip: one
 * workgroup per (pair, chromosome) walks colate_interval_walk_tile() rows at a time; a count pass, the offsets formed on
 * the host, a write pass); COLATE_ENODEVICE without a device, there is no fall-back.  _host: the host twin, a plain loop,
 * the same bytes.
 * Refused (COLATE_EINVAL, before anything is staged): NULL pointers, C, S or P < 1, M < 0, a sample or mask id out of
 * range, decreasing offsets, num_bases_per_block < 1, a position at or above 2^31 - num_bases_per_block, a negative or
 * descending position.
 * Speed: tools/interval_samples_bench.py is the measurement (README). */
typedef struct colate_walk_row {
  int pos;
  float age_begin, age_end;
} colate_walk_row;
typedef struct colate_walk_idx {
  int prev_bp;
  unsigned short DAF, AAF;
} colate_walk_idx;
typedef struct colate_walk_pair {
  int target, reference;           /* sample ids */
  int target_mask, reference_mask; /* mask ids, -1: none */
} colate_walk_pair;
int colate_interval_walk(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int M,
                         const unsigned long long* masks, int P, const colate_walk_pair* pairs, int num_bases_per_block, long long cap,
                         long long* rec_off, int* nb, colate_interval_rec* recs, int* block);
int colate_interval_walk_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int M,
                              const unsigned long long* masks, int P, const colate_walk_pair* pairs, int num_bases_per_block,
                              long long cap, long long* rec_off, int* nb, colate_interval_rec* recs, int* block);
int colate_interval_walk_tile(void); /* diagnostic: rows per step of a workgroup of the walk kernel (no device needed) */

/* The walk, then colate_interval_fit_groups on its records (group p = pair p), with the records never leaving the device:
 * per chunk of pairs the write pass of the walk puts the records and the per-(pair, block) record ranges where the cells
 * kernel reads them.  epochs[E] and init_rates[E] serve all pairs.  The call draws every pair's block weights itself, as
 * the command line does: pair p's [B][nb[p]] from a fresh std::mt19937 on `seed` through colate_bootstrap_weights, once
 * nb is known -- one host wait after the count pass, which also sizes the chunks: runs of consecutive pairs whose dense
 * cell sums fit COLATE_INTERVAL_GROUPS_CELLS_MB and whose records (28 bytes each with the cell index) fit
 * COLATE_INTERVAL_WALK_RECS_MB megabytes (default COLATE_INTERVAL_WALK_RECS_MB_DEFAULT); a larger pair goes alone.
 * Out, per pair: out_nb, out_used (its records), and out_R, out_dropped, out_rates[P][B][E], out_iters / out_loglik /
 * out_flags[P][B] -- in every bit what colate_interval_fit_groups returns on the records of colate_interval_walk with
 * those weights.  _host: colate_interval_walk_host followed by colate_interval_fit_groups_host (math as there).
 * Refused: what colate_interval_walk refuses; B or E < 1, epochs, starting rates and iteration limits as
 * colate_bootstrap_em_interval_batch refuses them (epochs[0] must not lie behind the first point of the age grid);
 * COLATE_ELIMIT: E above 1024, B above 65535, P x B at or above 2^31, a pair with more than COLATE_INTERVAL_MAX_BLOCKS
 * blocks.  The library forms the records itself (weights in [0, 2], blocks not decreasing), so the sums are bounded
 * analytically and no record is scanned on the host.
 * colate_interval_fit_samples_kernel_seconds: as colate_interval_fit_groups_kernel_seconds, with both walk passes. */
#define COLATE_INTERVAL_WALK_RECS_MB_DEFAULT 4096
int colate_interval_fit_samples(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int M,
                                const unsigned long long* masks, int P, const colate_walk_pair* pairs, int num_bases_per_block, int B,
                                int E, const double* epochs, const double* init_rates, unsigned int seed, int max_iter, int min_iter,
                                double rel_tol, double rate_floor, int* out_nb, long long* out_used, int* out_R, long long* out_dropped,
                                double* out_rates, int* out_iters, double* out_loglik, int* out_flags);
int colate_interval_fit_samples_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                                     int M, const unsigned long long* masks, int P, const colate_walk_pair* pairs,
                                     int num_bases_per_block, int B, int E, const double* epochs, const double* init_rates,
                                     unsigned int seed, int max_iter, int min_iter, double rel_tol, double rate_floor, int* out_nb,
                                     long long* out_used, int* out_R, long long* out_dropped, double* out_rates, int* out_iters,
                                     double* out_loglik, int* out_flags, int math);
double colate_interval_fit_samples_kernel_seconds(void);

/* ---- the table fill of `--mode mut` for every pair of a sample list, over the same walk indices (csrc/fill_samples.h) ----
 * Inputs and refusals are those of colate_interval_walk; A must be the 185 of colate_age_grid (COLATE_EINVAL otherwise).
 * Per pair the walk above picks the used rows and their genome blocks; the fill is coal.cpp:2221-2297 with age = ref_age
 * = 0 (coal.cpp:2074-2075): the pair owns a std::mt19937 on `seed` and draws uniform_real_distribution<double>(0, 1)
 * from it, row after row.  With begin = (float)max(age_begin, 0), end = age_end, f as above,
 * e = (double)(f * (float)r.DAF) / (double)(r.DAF + r.AAF) and w = (double)(f * (float)r.DAF) / ((double)(r.DAF + r.AAF)
 * * 100.0), each for the shared (t.DAF) and the not-shared (t.AAF) kind, and bin(x) = max(0, (int)round(log(10 x) * 10) +
 * 1): a row with begin <= 0 (the F path) adds e to the two row-0 tables at bin(end) where that is below A, then makes
 * 100 draws x = u * (end - begin) + begin (a separate multiply and add), clamps x at 0 and adds w of the not-shared kind
 * at bin(x) where that is below A; any other row makes draws until 100 of them have x >= 0 and bin(x) < A, each of
 * those adding both w at bin(x).  Every sum starts at 0.0 and adds in the order of the draws, each addition rounded.
 * Out, per pair p: out_nb[p], out_used[p] (its used rows); its tables [nb[p]][4][A] -- shared, not shared, shared row 0,
 * not-shared row 0 per block, the order of the engine's Block::t -- back to back in out_tables, which has room for
 * cap_blocks blocks (a total above it is COLATE_ELIMIT with the needed total in colate_last_error(); nothing is written
 * then); out_words[p]: the 32-bit words the pair's generator has given out when its fill ends (std::mt19937 g(seed);
 * g.discard(out_words[p]) is the run's generator there: two words per draw, 200 per used row unless a draw was repeated);
 * out_handed_back[p]: 1 where the device form had the host twin fill the pair (always 0 from _host).
 * _host: the host twin, a plain loop per pair with the library's generator, distribution and log(): right for every
 * input.  (Where no draw can ever be accepted the reference does not end; the twin stops after 100 x 100 x (rows + 1)
 * draws.)  out_near_band[p]: 1 where a draw of the pair lies inside a guard band of the located bin steps (64 ulps either
 * side, csrc/mut_pairs.cpp FastBin) or a draw was repeated -- the documented reasons for which the device hands a pair
 * back.
 * colate_fill_samples, all on one stream of the calling thread's device (COLATE_ENODEVICE without one): the inputs and the
 * count pass of the walk once; one host wait for the counts; the seed's uniforms [0, 100 x the largest out_used) uploaded
 * once for all pairs (record k of a pair reads them at 100 k); then chunks -- runs of consecutive pairs whose records (40
 * bytes each with the row-0 weights) fit COLATE_FILL_SAMPLES_RECS_MB megabytes (default
 * COLATE_FILL_SAMPLES_RECS_MB_DEFAULT), a larger pair alone, scratch allocated once for the largest --: the walk's write
 * pass forms the records in HBM, one wave per (pair, block) sums the row-0 tables in record order (thresholds of
 * colate_interval_bin_thresholds in LDS, no log, no floating-point atomics), one thread per (pair, block) writes the job of
 * the age-sampling kernel (csrc/fill_kernel.hip, the kernel of `--pairs`), that kernel runs, and tables, row-0 tables and
 * flags come back in one wait.  A pair with a flagged block is filled by the twin on the same inputs, so the results equal
 * _host's in every bit, whatever the chunking.  Where the located steps fail their self-check or the bulk generator does
 * not reproduce this machine's std::mt19937, every pair is handed back.
 * colate_fill_samples_chunks / _kernel_seconds: diagnostics of the calling thread's last call (0 from _host). */
#define COLATE_FILL_SAMPLES_RECS_MB_DEFAULT 4096
int colate_fill_samples(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int M,
                        const unsigned long long* masks, int P, const colate_walk_pair* pairs, int num_bases_per_block, int A,
                        unsigned int seed, long long cap_blocks, int* out_nb, long long* out_used, double* out_tables,
                        unsigned long long* out_words, int* out_handed_back);
int colate_fill_samples_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int M,
                             const unsigned long long* masks, int P, const colate_walk_pair* pairs, int num_bases_per_block, int A,
                             unsigned int seed, long long cap_blocks, int* out_nb, long long* out_used, double* out_tables,
                             unsigned long long* out_words, int* out_handed_back, int* out_near_band);
int colate_fill_samples_chunks(void);
double colate_fill_samples_kernel_seconds(void);

/* ---- `Colate --mode compare_tmp` for many pairs over the same walk indices (csrc/compare_tmp.h: the contract;
 * include/coal/coal.cpp:4297-4521) ----
 * For every pair and every window of every chromosome two counts: the searched rows both samples hit (snps) and, of those,
 * the rows on which the two disagree (mismatch).  The inputs are those of colate_interval_walk without masks: every row
 * given is a searched row (flipped == 0, one branch, age_begin < age_end, single-base alleles), its positions not
 * descending; a pair's mask ids must both be -1.  Sample s hits row i iff (idx.DAF | idx.AAF) != 0 and idx.prev_bp >= the
 * position of the row in front of i (-1 at a chromosome's first row); its allele there is fixed = (idx.AAF == 0) -- the
 * reference's draw `uniform < DAF / (AAF + DAF)` in integer division decides nothing else.  snps counts the rows both
 * samples hit, mismatch those of them with different `fixed`.  first_pos[C] / last_pos[C]: the positions of the first and
 * last raw rows of each chromosome's .mut file (first_pos not above the first row given, last_pos not below the last);
 * chromosome c has W_c = w(last_pos) + 1 windows with w(pos) = pos > first_pos ? (pos - first_pos - 1) / window : 0, and a
 * row belongs to window w(its position).  `window` >= 1 (the command line: 10 000 000).
 * Out: win_off[C + 1] (win_off[c + 1] - win_off[c] = W_c) and mismatch / snps as int[P][win_off[C]], each with room for
 * `cap` ints (P x win_off[C] above it is COLATE_ELIMIT with the needed number in colate_last_error(); nothing is written
 * then, nor after any other refusal).
 * _host: the host twin -- two bit planes per sample (hit, fixed & hit; every chromosome starts on a 64-bit word), two
 * popcounts per pair and window.  colate_compare_samples: the same on the calling thread's device (COLATE_ENODEVICE
 * without one), all on one stream with one host wait: a plane kernel (one lane per sample and row, ballots), then per chunk
 * of pairs -- the two output arrays of a chunk within 256 MB -- one workgroup per (pair, chromosome), a wave per window in
 * turn.  Integers only, no atomics: both forms give the same ints whatever the chunking.
 * colate_compare_samples_chunks / _kernel_seconds: diagnostics of the calling thread's last device call. */
int colate_compare_samples(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int P,
                           const colate_walk_pair* pairs, const int* first_pos, const int* last_pos, int window, long long cap,
                           long long* win_off, int* mismatch, int* snps);
int colate_compare_samples_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int P,
                                const colate_walk_pair* pairs, const int* first_pos, const int* last_pos, int window, long long cap,
                                long long* win_off, int* mismatch, int* snps);
int colate_compare_samples_chunks(void);
double colate_compare_samples_kernel_seconds(void);

/* ---- `Colate --mode count_topo` for many (cond, target, reference) triples over the same walk indices (csrc/count_topo.h:
 * the contract; include/coal/coal.cpp:4523-4781) ----
 * The rows are those of colate_interval_walk, every row a searched row of this mode (flipped == 0, one branch, age_begin <=
 * age_end, single-base alleles), positions not descending.  idx[S][rows]: the samples' walk indices; cond_idx[S][rows]: their
 * cond indices -- the counts of the record the sample's cursor stands on at that row, whether or not its position and alleles
 * are the row's (prev_bp is not read).  Sample s HITS row i iff (idx.DAF | idx.AAF) != 0 and QUALIFIES it iff cond_idx.DAF > 0.
 * A row qualifies for a triple iff the target hits, the reference hits and the cond sample qualifies; the triple's qualifying
 * row number k, counted over the chromosomes in order, reads uniforms[2 k] and uniforms[2 k + 1]: with d = (float)u promoted
 * back to double, pT = (double)DAF_T / (DAF_T + AAF_T) and pR likewise, the row's bit is set in `plus` iff d1 <= pT && d2 > pR
 * and in `minus` iff d1 > pT && d2 <= pR.  Every triple starts at uniforms[0]: the command line hands over the stream of the
 * run's std::mt19937 through uniform_real_distribution<double>(0, 1).
 * Out: word_off[C + 1] (chromosome c owns the words [word_off[c], word_off[c + 1]) of a plane, ceil(rows / 64) of them; bit
 * i & 63 of word i >> 6 is its row i), plus / minus as [P][word_off[C]] words with room for `cap` words each (COLATE_ELIMIT
 * with the needed number above it), draws[P]: the triple's qualifying rows.  A stream shorter than 2 x the largest draws[p]
 * is COLATE_ELIMIT with the needed length in colate_last_error().  Nothing is written after a refusal.
 * _host: the host twin.  colate_topo_samples: the same on the calling thread's device (COLATE_ENODEVICE without one), on one
 * stream: a plane kernel (one lane per array and row, ballots); a count kernel, one workgroup per (triple, chromosome); one
 * host wait for the counts, from which the host forms every triple's base rank per chromosome and uploads the longest stream
 * any triple needs once for all; then per chunk of triples -- the two output planes of a chunk within 256 MB
 * (COLATE_TOPO_BUDGET: bytes) -- the draw kernel, one workgroup per (triple, chromosome): a wave scans the popcounts of a tile
 * of 64 words (colate_topo_samples_tile() rows) for each word's base rank, then word by word, lane = row, reads the two
 * uniforms of its rank and the two index entries, compares and ballots.  No atomics, no compaction, no floating-point
 * reduction: both forms give the same bits whatever the chunking.
 * colate_topo_samples_chunks / _kernel_seconds: diagnostics of the calling thread's last device call. */
typedef struct colate_topo_triple {
  int cond, target, reference; /* sample ids */
} colate_topo_triple;
int colate_topo_samples(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                        const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms,
                        const double* uniforms, long long cap, long long* word_off, unsigned long long* plus,
                        unsigned long long* minus, long long* draws);
int colate_topo_samples_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                             const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms,
                             const double* uniforms, long long cap, long long* word_off, unsigned long long* plus,
                             unsigned long long* minus, long long* draws);
int colate_topo_samples_tile(void); /* rows of a tile of the draw kernel (no device needed) */
int colate_topo_samples_chunks(void);
double colate_topo_samples_kernel_seconds(void);

/* ---- the age profile of those draws: signed counts per epoch, no plane leaves the call (csrc/count_topo.h: age_epoch) ----
 * Inputs and draws as for colate_topo_samples.  epochs[E]: finite and strictly ascending, 1 <= E <= 1024 (the command line takes
 * them from colate_epochs_from_bins(spec, 0, years_per_gen), the epochs of a .coal).  The epoch of a row is the number of e in
 * 1 .. E - 1 with epochs[e] <= (double)mid, where mid = 0.5f * (age_begin + age_end) is formed in single precision; a NaN or
 * negative mid gives 0, +inf gives E - 1.  Out: counts[P][E][3] -- per triple and epoch the rows of that epoch set in `plus`, in
 * `minus`, and the qualifying rows (those that drew) -- and draws[P].  Integers only: no result depends on an order of operations.
 * Refused, by name and before anything is written: what colate_topo_samples refuses of its inputs and stream, E out of range, an
 * epoch that is not finite, neighbours that do not ascend, NULL outputs.
 * _host: the host twin.  colate_topo_profile: on the calling thread's device (COLATE_ENODEVICE without one), the staging, plane
 * kernel, count kernel and host wait of colate_topo_samples; a bins kernel, one lane per row, once for all triples (2 bytes per
 * row); then per chunk of triples -- 12 E bytes per (triple, chromosome), a chunk within 256 MB (COLATE_TOPO_BUDGET) -- the profile
 * kernel: the draw kernel's scan, ranks and draws, with every lane of a qualifying row adding to a 3 x E histogram in the
 * workgroup's LDS (integer adds), written out as the workgroup's own partials; one copy per chunk, and the host sums the
 * chromosomes in long long.  The same integers whatever the chunking.
 * colate_topo_profile_chunks / _kernel_seconds: diagnostics of the calling thread's last device call. */
int colate_topo_profile(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                        const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms,
                        const double* uniforms, int E, const double* epochs, long long* counts, long long* draws);
int colate_topo_profile_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                             const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms,
                             const double* uniforms, int E, const double* epochs, long long* counts, long long* draws);
int colate_topo_profile_chunks(void);
double colate_topo_profile_kernel_seconds(void);

/* ---- the age profile per genome block, and the block jackknife on it (csrc/count_topo.h: the blocks of this mode) ----
 * colate_topo_blocks: blk_off[C + 1] of the searched rows, no device.  With k(pos) = pos > 0 ? (pos - 1) / num_bases_per_block : 0
 * a chromosome owns k(pos of its last row) + 1 blocks (the largest k of its rows), or 1 without a row; a row's global block is
 * blk_off[c] + k(pos); blk_off[C] = nb.  A block without a row exists and is all zeros.  These blocks are a function of the rows
 * alone; they are not those of `--mode mut`, which depend on a pair's used rows.  Refused: num_bases_per_block < 1, a position at
 * or above 2^31 - num_bases_per_block, nb > 65535 (COLATE_ELIMIT with the needed number).
 * colate_topo_profile_blocks: inputs, epochs and draws as for colate_topo_profile -- a triple's qualifying row number k, counted
 * across the whole genome in order, reads uniforms[2 k] and uniforms[2 k + 1] whatever the blocks -- and counts[P][nb][E][3]: plus,
 * minus and qualifying per (triple, block, epoch).  The sum over a triple's blocks is colate_topo_profile's counts in every integer,
 * for every num_bases_per_block.  Refused, by name and before anything is written: what colate_topo_profile and colate_topo_blocks
 * refuse, an nb that is not blk_off[C], one triple's partials (12 E nb bytes) above 1 GB (COLATE_ELIMIT; no E <= 1024 with nb <=
 * 65535 reaches it).  _host: the host twin.  On the device (COLATE_ENODEVICE without one), one stream: the staging, plane kernel and
 * bins kernel of colate_topo_profile; every block as a segment (chromosome, first row, end row); a count kernel, one wave per
 * (triple, block), the segment's first and last word masked; one host wait, after which the host forms every block's base rank;
 * then per chunk of triples -- 12 E bytes per (triple, block), a chunk within 256 MB (COLATE_TOPO_BUDGET), one triple where its
 * partials alone are larger -- the profile kernel, one workgroup per (triple, block), over the segment's words with the same masks.
 * Integers only, no global atomics: the same integers whatever the chunking.
 * colate_topo_profile_blocks_chunks / _kernel_seconds: diagnostics of the calling thread's last device call.
 * colate_topo_jackknife: host only, the one copy of the statistic.  counts[nb][E][3] of one triple (none negative); out[E + 1][4]:
 * D, D_jack, se, Z per epoch and, in cell E, for the sum over the epochs; used[E + 1]: the blocks with plus + minus > 0.  Per cell,
 * over the used blocks j in ascending order, g of them, with a_j = plus, b_j = minus, n_j = a_j + b_j, A = sum a_j, M = sum b_j,
 * n = A + M as integers and every operation a rounded IEEE double in this order, nothing contracted: D = (double)(A - M) /
 * (double)n; theta_j = (double)((A - a_j) - (M - b_j)) / (double)(n - n_j); h_j = (double)n / (double)n_j; s = sum of
 * ((double)(n - n_j) / (double)n) * theta_j; D_jack = (double)g * D - s; v = sum of (d * d) / (h_j - 1.0) with d = (h_j * D -
 * (h_j - 1.0) * theta_j) - D_jack; se = sqrt(v / (double)g); Z = D_jack / se -- the weighted delete-one jackknife of Busing,
 * Meijer and van der Leeden (1999).  NaN stands for "not available": all four at n == 0, all but D at g < 2, Z where se is not
 * > 0. */
int colate_topo_blocks(int C, const long long* row_off, const colate_walk_row* rows, int num_bases_per_block, int* blk_off);
int colate_topo_profile_blocks(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                               const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms,
                               const double* uniforms, int E, const double* epochs, int num_bases_per_block, int nb,
                               long long* counts, long long* draws);
int colate_topo_profile_blocks_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                                    const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms,
                                    const double* uniforms, int E, const double* epochs, int num_bases_per_block, int nb,
                                    long long* counts, long long* draws);
int colate_topo_profile_blocks_chunks(void);
double colate_topo_profile_blocks_kernel_seconds(void);
int colate_topo_jackknife(int nb, int E, const long long* counts, double* out, int* used);

/* ---- the expected counts per genome block: what the sampled counts estimate, without a draw (csrc/count_topo.h: the expected
 * counts) ----
 * Inputs, epochs and blocks as for colate_topo_profile_blocks, without a stream of uniforms and without `draws`.  A row qualifies
 * as there.  At a qualifying row, with N_T = DAF_T + AAF_T and N_R = DAF_R + AAF_R, all unsigned integers,
 *   plus_fx = floor((DAF_T * AAF_R) * 2^30 / (N_T * N_R)),  minus_fx = floor((AAF_T * DAF_R) * 2^30 / (N_T * N_R)):
 * the probabilities pT (1 - pR) of a +1 line and (1 - pT) pR of a -1 line in units of 2^-30, rounded down; every intermediate fits 64
 * bits.  counts[P][nb][E][3]: sum plus_fx, sum minus_fx and the qualifying rows per (triple, block, epoch).  plus_fx + minus_fx <=
 * 2^30; where T and R are both fixed at a row it adds exactly 2^30 to plus (T all derived, R all ancestral), to minus (the converse)
 * or nothing, as the sampled form prints for every uniform in (0, 1); column 2 is column 2 of colate_topo_profile_blocks.  Each
 * addend is short of the exact product by less than 2^-30: a cell of n rows by less than n 2^-30.  Only integers are summed: the
 * same integers whatever the order, the chunking or the block size (finer blocks regrouped are the coarser ones).  With fewer than
 * 2^31 searched rows every sum stays below 2^62, and colate_topo_jackknife -- ratios of counts throughout -- takes one triple's
 * counts[nb][E][3] as they are.  Refused, by name and before anything is written: what colate_topo_profile_blocks refuses of the
 * same arguments, and row_off[C] >= 2^31 (COLATE_ELIMIT with the number).  _host: the host twin.  On the device (COLATE_ENODEVICE
 * without one), one stream and no host wait before the final copy: the staging, plane kernel and bins kernel of
 * colate_topo_profile; every block as a segment; then per chunk of triples -- 24 E bytes per (triple, block), a chunk within 256 MB
 * (COLATE_TOPO_BUDGET), one triple where its partials alone are larger -- one kernel, one workgroup per (triple, block) over the
 * segment's words, the first and last one masked: lane = row, two 64-bit integer quotients (a double quotient as the first guess, the exact integer remainder deciding), 64-bit
 * histograms in LDS, the workgroup's own 3 E integers out.  No count pass, no rank, no global atomics, no floating point in the result.
 * colate_topo_expected_blocks_chunks / _kernel_seconds: diagnostics of the calling thread's last device call. */
int colate_topo_expected_blocks(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                                const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, int E, const double* epochs,
                                int num_bases_per_block, int nb, long long* counts);
int colate_topo_expected_blocks_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                                     const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, int E,
                                     const double* epochs, int num_bases_per_block, int nb, long long* counts);
int colate_topo_expected_blocks_chunks(void);
double colate_topo_expected_blocks_kernel_seconds(void);

/* ---- host-side pieces of mut() around the hot path (CPU, no device needed) ----
 * coal.cpp:3126-3137: the 185-point age grid.  Returns A or COLATE_EINVAL if cap < A. */
int colate_age_grid(double* age_grid, int cap);

/* coal.cpp:3551-3632: epochs from `--bins x,y,step` (std::stof semantics), with the
 * ancient-sample rule; age = max(target_age, reference_age)/years_per_gen in
 * generations.  Returns E (>0) or a negative code; *ep_null as coal.cpp:3622. */
int colate_epochs_from_bins(const char* bins, double age, double years_per_gen, double* epochs,
                            int cap, int* ep_null);

/* coal.cpp:3508-3549 + 3638-3646: epochs and initial rates from a `--coal` file.
 * Returns E or a negative code. */
int colate_epochs_from_coal(const char* path, double age, double* epochs, double* init_rates,
                            int cap);

/* coal.cpp:3344-3451: block bootstrap.  Draws the multinomial block weights for
 * num_bootstrap replicates from std::mt19937 state `rng_state` (opaque, from
 * colate_rng_*), forms the weighted block sums and applies the F
 * redistribution of the age_begin<=0 mutations.  Tables are [nb][A]; the emp
 * tables hold row 0 of the reference's A*A tables (the only row it reads). */
void* colate_rng_create(unsigned int seed); /* std::mt19937, coal.cpp:3157-3162 */
void colate_rng_destroy(void* rng_state);
int colate_bootstrap_counts(void* rng_state, int num_bootstrap, int nb, int A,
                            const double* age_grid, double age, const double* sh_block,
                            const double* ns_block, const double* sh_emp_block,
                            const double* ns_emp_block, double* cnt_shared,
                            double* cnt_notshared);

/* coal.cpp:3350-3357 alone: the multinomial block weights w[num_bootstrap][nb] (all ones when
 * num_bootstrap == 1), drawn from the same std::mt19937 -- the host half of the GPU bootstrap below. */
int colate_bootstrap_weights(void* rng_state, int num_bootstrap, int nb, double* weights);

/* coal.cpp:3358-3451 alone, on the host, from weights drawn before (colate_bootstrap_weights): the weighted block sums
 * and the F redistribution.  colate_bootstrap_counts = colate_bootstrap_weights + this.  The host twin of the GPU
 * bootstrap below (bit-identical); what `--counts_only` runs, which needs no device. */
int colate_bootstrap_counts_from_weights(int num_bootstrap, int nb, int A, const double* age_grid, double age,
                                         const double* weights, const double* sh_block, const double* ns_block,
                                         const double* sh_emp_block, const double* ns_emp_block, double* cnt_shared,
                                         double* cnt_notshared);

/* coal.cpp:3358-3441 on the GPU: weighted block sums + F redistribution for B replicates, all
 * pointers in device memory (tables [nb][A], weights [B][nb], cnt_* [B][A]), asynchronous on
 * hip_stream; results are bit-identical to colate_bootstrap_counts.  `status` (device int, may be
 * NULL) receives 1 if the sample age lies outside the age grid. */
int colate_bootstrap_counts_device(int B, int nb, int A, const double* age_grid, double age,
                                   const double* weights, const double* sh_block, const double* ns_block,
                                   const double* sh_emp_block, const double* ns_emp_block,
                                   double* cnt_shared, double* cnt_notshared, int* status,
                                   void* hip_stream);

/* Block tables -> rates in one call, host pointers: uploads the [nb][A] tables and the weights
 * w[B][nb], runs the bootstrap kernel and the EM kernel back to back on the device (the count
 * tables never visit the host) and returns the EM outputs; out_cnt_shared / out_cnt_notshared
 * (each [B][A], may be NULL) additionally receive the count tables.  This is what `Colate --mode
 * mut` of colate_amd runs after reading the inputs (coal.cpp:3344-3451 + 3675-3827). */
int colate_bootstrap_em_batch(int B, int nb, int E, int A, const double* age_grid, double age,
                              const double* weights, const double* sh_block, const double* ns_block,
                              const double* sh_emp_block, const double* ns_emp_block,
                              const double* epochs, const double* init_rates, int max_iter,
                              int min_iter, double rel_tol, double rate_floor, double* out_rates,
                              int* out_iters, double* out_loglik, int* out_flags,
                              double* out_cnt_shared, double* out_cnt_notshared);

/* ---- batched all-pairs (BASELINE configs[4]) --------------------------------------------
 * The reference is run once per (target, reference) pair (coal.cpp:2071-2321 + 3071-3863 each time).  Here G pairs
 * ("groups") go through ONE bootstrap launch and ONE EM launch: group g has its own genome-block tables (group_nb[g]
 * blocks; the four tables of all groups are concatenated in group order, [sum_g nb_g][A]), its own sample age, its own
 * epochs[g][E] / init_rates[g][E] (an ancient sample inserts its age as an epoch, coal.cpp:3597-3624; all groups of a
 * call have the same E) and B bootstrap replicates with weights [B][nb_g], concatenated in group order as well.
 * Row r = g * B + i of every output is replicate i of group g; results are bit-identical to G separate
 * colate_bootstrap_em_batch calls.  out_cnt_* ([G*B][A], may be NULL) receive the count tables. */
int colate_bootstrap_em_batch_groups(int G, int B, int E, int A, const double* age_grid, const int* group_nb,
                                     const double* group_age, const double* weights, const double* sh_block,
                                     const double* ns_block, const double* sh_emp_block,
                                     const double* ns_emp_block, const double* epochs, const double* init_rates,
                                     int max_iter, int min_iter, double rel_tol, double rate_floor,
                                     double* out_rates, int* out_iters, double* out_loglik, int* out_flags,
                                     double* out_cnt_shared, double* out_cnt_notshared);
/* The bootstrap of rows [row_lo, row_hi) of such a batch, all pointers in device memory, asynchronous on hip_stream.
 * The group arrays describe groups [group_first, group_first + G) (every row must belong to one of them):
 * group_block_off[g] = number of genome blocks in front of group g in the tables given, group_weight_off[g] = number
 * of weights in front of its [B][nb_g] weights; cnt_*[row_hi - row_lo][A]; `status` (device int, required) receives 1
 * if a sample age lies outside the age grid. */
int colate_bootstrap_counts_groups_device(int G, int B, int group_first, int row_lo, int row_hi, int A,
                                          const double* age_grid, const int* group_nb,
                                          const long long* group_block_off, const long long* group_weight_off,
                                          const double* group_age, const double* weights, const double* sh_block,
                                          const double* ns_block, const double* sh_emp_block,
                                          const double* ns_emp_block, double* cnt_shared, double* cnt_notshared,
                                          int* status, void* hip_stream);

/* The host-pointer entry points above keep one device buffer, one pinned staging buffer and one stream per calling
 * thread between calls (grown on demand); this frees them. */
int colate_release_workspace(void);

/* ---- one process per GPU: replicate shards + ONE RCCL all-gather over xGMI -----------
 * The reference runs its replicates one after the other (coal.cpp:3675-3846); they are independent, so rank r of
 * `nranks` processes runs the contiguous range colate_shard_bounds(B, nranks, r) on ITS current device and a
 * single ncclAllGather of the packed results (rates, log-likelihood, iterations, flags: (8E + 16) bytes per
 * replicate) gives every rank all B results in replicate order -- bit-identical to the one-process run.  No other
 * exchange exists on the path.  Rank 0 obtains the 128-byte id (colate_comm_unique_id) and hands it to the others
 * by any means (a pipe, a file, MPI, torch.distributed's store); every rank then calls colate_comm_create after
 * selecting its device (colate_set_device).  RCCL (librccl.so.1) is loaded on first use.  `Colate --ranks N` is
 * the command-line form (it forks N such processes itself); colate_amd/distributed.py + bench.py are the
 * torch.distributed form of the same sharding. */
#define COLATE_COMM_ID_BYTES 128
int colate_shard_bounds(int B, int nranks, int rank, int* lo, int* hi);
int colate_comm_unique_id(void* id /* [COLATE_COMM_ID_BYTES] */);
int colate_comm_create(const void* id, int nranks, int rank, void** comm);
int colate_comm_destroy(void* comm);
/* colate_em_batch over the communicator: every rank passes the FULL host arrays (cnt_*[B][A]) and receives the
 * full outputs; it computes rows [lo, hi) only. */
int colate_em_batch_allgather(void* comm, int B, int E, int A, const double* age_grid, const double* cnt_shared,
                              const double* cnt_notshared, const double* epochs, const double* init_rates,
                              int max_iter, int min_iter, double rel_tol, double rate_floor, double* out_rates,
                              int* out_iters, double* out_loglik, int* out_flags);
/* colate_bootstrap_em_batch over the communicator (weights[B][nb] in full on every rank: they come from the
 * run's one std::mt19937 stream, which every rank replays identically from --seed). */
int colate_bootstrap_em_batch_allgather(void* comm, int B, int nb, int E, int A, const double* age_grid, double age,
                                        const double* weights, const double* sh_block, const double* ns_block,
                                        const double* sh_emp_block, const double* ns_emp_block, const double* epochs,
                                        const double* init_rates, int max_iter, int min_iter, double rel_tol,
                                        double rate_floor, double* out_rates, int* out_iters, double* out_loglik,
                                        int* out_flags);

/* colate_bootstrap_em_batch_groups over the communicator: the G * B rows are sharded like replicates
 * (colate_shard_bounds(G * B, nranks, rank)); a rank passes the arrays of the groups its rows belong to ONLY --
 * groups [group_first, group_first + group_count) with group_first = lo / B, group_count = (hi - 1) / B - lo / B + 1 --
 * so that it needs to read and fill the tables of those pairs alone; a rank without rows passes group_count = 0.
 * Every rank receives all G * B results.  `Colate --pairs FILE --ranks N` is the command-line form. */
int colate_bootstrap_em_batch_groups_allgather(void* comm, int G, int B, int group_first, int group_count, int E, int A,
                                               const double* age_grid, const int* group_nb, const double* group_age,
                                               const double* weights, const double* sh_block, const double* ns_block,
                                               const double* sh_emp_block, const double* ns_emp_block,
                                               const double* epochs, const double* init_rates, int max_iter,
                                               int min_iter, double rel_tol, double rate_floor, double* out_rates,
                                               int* out_iters, double* out_loglik, int* out_flags);

/* coal.cpp:3660-3672, 3830-3847: the .coal text (6 significant digits, trailing blank). */
int colate_write_coal(const char* path, int B, int E, const double* epochs, const double* rates,
                      int is_ancient, int ep_null);

/* `Colate --mode CondCoalRates` (coal.cpp:4786-4999, GetConditionalCoalescentRate): the per-block accumulators of the
 * conditional coalescence rates.  T trees of N haplotypes (2N-1 nodes each, Relate's labelling: leaves 0..N-1, root
 * 2N-2): parents[T][2N-1] (-1 at the root), branch_lengths[T][2N-1], factors[T] (each tree's weight as the reference's
 * float; -1 for its extra pass of the last tree), blocks[T] in [0, num_blocks).  G groups (group_of_hap[N]), the focal
 * haplotypes focal[F], the conditional ones cond[C] (C = 0: the empty conditional group), sample_ages[N] or NULL (the
 * modern path), epochs[E] and epochs_focal[EF] as floats.  Out: num / denom[num_blocks][EF][E][G] in double (the
 * reference's float addends summed in double).  N up to 16384 (COLATE_ELIMIT beyond).  The walks run on the calling
 * thread's device; COLATE_ENODEVICE without one.  _host: the same on the host (the CLI's host twin). */
int colate_condcoal_accumulate(int N, int T, const int* parents, const double* branch_lengths, const float* factors,
                               const int* blocks, int num_blocks, int G, const int* group_of_hap, int F, const int* focal,
                               int C, const int* cond, const double* sample_ages, int E, const float* epochs, int EF,
                               const float* epochs_focal, double* num, double* denom);
int colate_condcoal_accumulate_host(int N, int T, const int* parents, const double* branch_lengths, const float* factors,
                                    const int* blocks, int num_blocks, int G, const int* group_of_hap, int F,
                                    const int* focal, int C, const int* cond, const double* sample_ages, int E,
                                    const float* epochs, int EF, const float* epochs_focal, double* num, double* denom);

/* The same for P (focal group, conditional group) pairs in one pass over the trees (`Colate --mode CondCoalRates
 * --pairs`): focal_group[P] in [0, G), each with at least one haplotype (its focal haplotypes: all of the group's,
 * ascending), cond_group[P] in [-1, G) (-1: the empty conditional group).  blocks[T] must not decrease.  Out: num /
 * denom[P][num_blocks][EF][E][G]; pair p's part is bit for bit what colate_condcoal_accumulate (device) or
 * colate_condcoal_accumulate_host (_host) gives for that pair alone. */
int colate_condcoal_accumulate_pairs(int N, int T, const int* parents, const double* branch_lengths, const float* factors,
                                     const int* blocks, int num_blocks, int G, const int* group_of_hap, int P,
                                     const int* focal_group, const int* cond_group, const double* sample_ages, int E,
                                     const float* epochs, int EF, const float* epochs_focal, double* num, double* denom);
int colate_condcoal_accumulate_pairs_host(int N, int T, const int* parents, const double* branch_lengths,
                                          const float* factors, const int* blocks, int num_blocks, int G,
                                          const int* group_of_hap, int P, const int* focal_group, const int* cond_group,
                                          const double* sample_ages, int E, const float* epochs, int EF,
                                          const float* epochs_focal, double* num, double* denom);

/* `CoalRate --mode local_ancestry` (coal_tree.cpp:447-527, coal_LA::populate): the per-block sums of the pairwise
 * coalescence rates between groups.  T calls, each a tree of N haplotypes (parents / branch_lengths[T][2N-1] as above)
 * with a weight (weights[T], the bases it stands for; the sums take weight / 1e9), a block (blocks[T] in
 * [0, num_blocks), any order) and a group vector (group_vector_ids[T] in [0, S)); group_vectors[S][N] holds labels in
 * [0, G).  sample_ages[N] or NULL; epochs[E] in double, epochs[0] = 0, increasing.  Out: num / denom
 * [num_blocks][G][G][E], filled for g1 >= g2 (the rest 0) -- per (pair of leaves, epoch) what populate adds, summed from
 * exact pair counts ("CoalRate").  COLATE_EINVAL for a node older than epochs[E-1] or in an epoch below that
 * of a sample age under it; COLATE_ELIMIT for N above 16384, G above 65535 or E * G * (G + 1) / 2 of 2^31 or more.  The
 * counting runs on the calling thread's device: COLATE_ENODEVICE without one, and the device's own code (COLATE_ELIMIT where
 * a tree does not fit it, COLATE_EHIP for a runtime error) where its walker cannot be made -- there is no fall-back to the
 * host here; the `CoalRate` executable, by contrast, runs the host twin then after a line on stderr.  _host: the host twin,
 * bit for bit the same sums. */
int colate_coalrate_accumulate(int N, int T, const int* parents, const double* branch_lengths, const double* weights,
                               const int* blocks, int num_blocks, const int* group_vector_ids, int S,
                               const int* group_vectors, int G, const double* sample_ages, int E, const double* epochs,
                               double* num, double* denom);
int colate_coalrate_accumulate_host(int N, int T, const int* parents, const double* branch_lengths, const double* weights,
                                    const int* blocks, int num_blocks, const int* group_vector_ids, int S,
                                    const int* group_vectors, int G, const double* sample_ages, int E,
                                    const double* epochs, double* num, double* denom);

/* `CoalRate --mode tree` (coal_tree.cpp:100-178, coal_tree::populate): the per-block sums of the whole sample's
 * coalescence rate.  T calls, each a tree of N haplotypes (parents / branch_lengths[T][2N-1] as above) with a weight
 * (weights[T]) and a block (blocks[T] in [0, num_blocks), any order); sample_ages[N] or NULL; epochs[E] in double,
 * epochs[0] = 0, increasing.  Out: num / denom [num_blocks][E]: per epoch the internal nodes in it times weight / 1e9, and
 * weight * L * (L - 1) / 2 * (upper - lower) / 1e9 over the pieces between consecutive node times and epoch boundaries, L
 * the lineages alive there (csrc/coalrate_tree.h: the walk and the one summation order).  COLATE_EINVAL for a malformed
 * tree or a node older than epochs[E-1]; COLATE_ELIMIT for N above 16384.  The device call sorts the node times of every
 * tree in a HIP kernel on the calling thread's device: COLATE_ENODEVICE without one, the device walker's own code
 * (COLATE_ELIMIT for more epochs than its LDS holds, COLATE_EHIP for a runtime error) where it cannot be made; no fall-back
 * to the host here.  _host: the host twin, bit for bit the same sums. */
int colate_coalrate_tree_accumulate(int N, int T, const int* parents, const double* branch_lengths, const double* weights,
                                    const int* blocks, int num_blocks, const double* sample_ages, int E, const double* epochs,
                                    double* num, double* denom);
int colate_coalrate_tree_accumulate_host(int N, int T, const int* parents, const double* branch_lengths, const double* weights,
                                         const int* blocks, int num_blocks, const double* sample_ages, int E,
                                         const double* epochs, double* num, double* denom);

/* Diagnostics of the calling thread's last colate_coalrate_accumulate / colate_coalrate_tree_accumulate (the device calls;
 * each resets its own at its start): out[5] (or NULL) = the launches of the first kernel (cr_count / crt_sort: one per
 * chunk that holds a call), the smallest and the largest number of calls per workgroup over them, the lanes per call, and 1
 * where the prefix counts (local_ancestry) or the sort keys (tree) lay in LDS, 0 where in device memory.  All 0 after a call
 * that launched nothing (refused, failed before its first chunk, or every call of weight 0).  Returns the launches. */
int colate_coalrate_launch_shape(int* out);
int colate_coalrate_tree_launch_shape(int* out);

/* The `CoalRate` command line (CoalRate.cpp:6-58) for --mode local_ancestry and --mode tree: same option names, stderr
 * lines and OUTPUT.coal.  Returns the process exit code. */
int colate_coalrate_main(int argc, char** argv);

/* The whole `Colate --mode mut` command line for the .colate.in / .colate_mat
 * inputs (Colate.cpp:6-116 -> coal.cpp:3071-3863): same option names, same
 * stderr progress lines, same .coal output.  Returns the process exit code.
 * `--mode mut_interval --rows FILE (--bins x,y,s | --coal FILE) -o OUT [--num_bootstraps B] [--seed S]
 * [--years_per_gen Y] [--max_iter N] [--min_iter N]` (no reference counterpart) is colate_bootstrap_em_interval_batch
 * on a text file: FILE (plain or gzip) has one line `block kind age_begin age_end weight` per observation -- block a
 * non-negative integer, kind `shared` or `notshared`, ages in generations, weight finite and >= 0; blank lines and
 * lines starting with `#` are skipped.  Distinct block ids, ascending, are the table rows 0 .. nb-1; distinct (kind,
 * age_begin, age_end) triples (equal as parsed doubles), in order of first appearance, the R rows; repeated lines of
 * one cell add up in file order.  Epochs and starting rates as for `mut` at age 0; block weights from
 * colate_bootstrap_weights on std::mt19937(--seed).  Writes OUT.coal (colate_write_coal).  Without a device, or with
 * COLATE_DEVICE_INTERVAL=0, the math = 1 host twin runs after one line on stderr and writes the same bytes.  A
 * malformed line is an error that names its line number; nothing is written then.
 * `--mode mut_interval --mut P --target_tmp T --reference_tmp R [--chr FILE] [--target_mask PREFIX] [--reference_mask PREFIX]
 * [--write_rows FILE]` with the same fit options takes the inputs of `--mode mut` instead of --rows (both together: an
 * error; --target_age / --reference_age are refused): the SNPs `--mode mut` uses become the rows and tables
 * through colate_interval_cells (the host twin without a device or with COLATE_DEVICE_INTERVAL=0, after a line on stderr;
 * same bytes), stderr shows `Number of blocks`, `Number of rows` and `SNPs beyond the age grid`, and --write_rows writes
 * them in the --rows format (17 significant digits; a block without a positive cell keeps a line of weight 0), from which
 * --rows gives the same OUT.coal.
 * `--mode mut_interval --pairs LIST --mut P [--chr FILE] (--bins x,y,s and/or coal= per line)` with the same fit options is that
 * run for every line `target.colate.in reference.colate.in output [target_mask=PREFIX] [reference_mask=PREFIX] [coal=FILE]`
 * of LIST in one pass: every input file is read once, and the pairs with the same number of epochs, in order of first
 * appearance, go through one colate_interval_fit_groups call (its host twin without a device or with
 * COLATE_DEVICE_INTERVAL=0, after a line on stderr; same bytes).  Every pair draws its block weights from a std::mt19937 of its
 * own on the run's seed, so OUTPUT.coal is, byte for byte, the single run's with the same options, masks, warm start and
 * --seed.  An age token on a line is an error naming the line; --target_tmp, --reference_tmp, --rows, --write_rows, --output,
 * --target_mask, --reference_mask, --coal, --ranks, --target_age and --reference_age are refused by name; a line without coal=
 * needs --bins.  stderr: per pair `Pair i / P: T x R: Number of blocks: n`, then `Pair i ` in front of the single run's
 * `Number of rows`, `SNPs beyond the age grid` and `Bootstrap k: Total iterations` lines.  A pair that uses no SNP within the
 * age grid gets no file and an error line naming it; the others are written and the exit code is 1.
 * `--mode mut_interval --samples LIST --mut P -o PREFIX [--chr FILE] (--bins x,y,s | --coal FILE)` with the same fit options: LIST
 * has `NAME FILE.colate.in [mask=PREFIX] [role=target|reference]` lines (default role: both; blank lines skipped); every (target
 * line, reference line) of different lines, targets outermost, is fitted and written to PREFIX_<target NAME>_<reference NAME>.coal,
 * byte for byte the file `--pairs` writes for that pair given the expanded list.  The pairs are walked on the device over the
 * files' walk indices (colate_interval_fit_samples; its host twin without a device or with COLATE_DEVICE_INTERVAL=0); where a
 * sample has no walk index, or with COLATE_DEVICE_INTERVAL_WALK=0, the expanded list takes the `--pairs` path after one line on
 * stderr.  A repeated or missing NAME, a NAME with '/', an unknown key or role, an age token and a list without a target or
 * without a reference are errors naming the line; --pairs, --rows, --target_tmp, --reference_tmp, --write_rows, --target_mask,
 * --reference_mask, --ranks, --target_age and --reference_age are refused by name.  stderr: the `Pair i ...` lines of `--pairs`
 * and `S samples and M masks staged, P pairs walked on the device`. */
int colate_mut_main(int argc, char** argv);

#ifdef __cplusplus
}
#endif
#endif /* COLATE_AMD_H */
