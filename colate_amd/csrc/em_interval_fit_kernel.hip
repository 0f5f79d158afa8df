// colate_amd/csrc/em_interval_fit_kernel.hip -- colate_em_interval_batch on gfx950: the EM fit on interval-dated
// mutations, coal.cpp:3675-3827 with rows (kind, age_begin, age_end) for age bins, for B replicates that share the
// rows and weight them differently.
//
// Persistent: one workgroup per replicate, the whole EM loop inside it.  epochs, the replicate's rates, the exp table
// and A_ep / B_ep stay in LDS for the run (the layout of em_interval_wave.hpp plus two control words); the first
// 64 * WAVES rows stay in registers (wave w keeps its g-th row in lane g).  Per iteration the only global reads are
// the replicate's weight row and, where R > 64 * WAVES, the rows beyond those.
//
// One iteration: get_AB from the current rates; the rows in groups of WAVES, one wavefront per call (wave_call(), the
// phases of em_interval_kernel.hip); after each group the thread that owns epoch e adds the group's rows to its
// num / den accumulators in ascending row order, and thread 0 to the log-likelihood -- accumulators live in registers,
// there is no tree, no per-wave partial sum and no atomic: the order of summation is that of the host twin
// (em_interval_host.cpp) and of the reference; then the M-step and the stop rule of em_interval_fit.hpp, whose
// verdict thread 0 publishes through LDS.
//
// Control flow: every barrier is reached by every wave.  Trip counts depend on R, E, the weights of a group (every
// thread reads the same WAVES values and skips a group in which none is > 0) and the verdict that all threads read
// from LDS behind a barrier, so all threads leave the loop in the same iteration; max_iter bounds it.
//
// colate_interval_fit_groups launches the same body for G groups x B replicates at once (em_interval_fit_groups_kernel):
// rows, R, weights, epochs and starting rates then differ between workgroups, but within a workgroup each is one value
// that all threads read, so the above holds per workgroup.
#include <hip/hip_runtime.h>

#include "em_interval_fit.hpp"
#include "em_interval_wave.hpp"
#include "em_kernels.h"

namespace {

using namespace em_interval;

// The fit of one replicate by its workgroup: `wrow` = the replicate's R weights, `out_rates` = its E rates, `out_iters`,
// `out_ll`, `out_flags` = its three scalars; `smem` = the workgroup's dynamic LDS.  Both kernels below are this body.
// KOWN: epochs owned per thread (e = tid, tid + WAVES * 64, ...): WAVES * 64 * KOWN >= the largest E of the layout
template <int WAVES, int KOWN>
__device__ __forceinline__ void fit_replicate(
    double* smem, int R, int E, const int* __restrict__ kinds, const double* __restrict__ age_begin,
    const double* __restrict__ age_end, const double* __restrict__ wrow, const double* __restrict__ epochs,
    const double* __restrict__ init_rates, int max_iter, int min_iter, double rel_tol, double rate_floor,
    double* __restrict__ out_rates, int* __restrict__ out_iters, double* __restrict__ out_ll, int* __restrict__ out_flags) {
  constexpr int NT = WAVES * 64;
  double* tab = smem;
  double* ep = tab + em::kExpTableDoubles;
  double* rt = ep + E;
  double* A = rt + E;
  double* B = A + E;
  double* first_wave = B + E;
  double* ctl = first_wave + WAVES * wave_doubles(E);  // [0]: the verdict of the stop rule
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const WaveLds w = wave_lds(first_wave, E, wave);

  for (int i = tid; i < em::kExpTableDoubles; i += NT) tab[i] = em::kExpTableDevice[i];
  for (int e = tid; e < E; e += NT) ep[e] = epochs[e], rt[e] = init_rates[e];
  // the wave's g-th row (row g * WAVES + wave) in lane g
  const int r_own = (lane * WAVES + wave < R) ? lane * WAVES + wave : R - 1;
  const int own_kind = kinds[r_own];
  const double own_a0 = age_begin[r_own], own_a1 = age_end[r_own];
  __syncthreads();

  const EmMath m{tab};
  const View v{E, ep, rt, A, B};
  const int groups = (R + WAVES - 1) / WAVES;
  double nacc[KOWN], dacc[KOWN];
  double ll = log_zero(), prev_ll = log_zero();  // (thread 0's are the fit's)
  int flags = 0, iter = 0;
  for (; iter < max_iter; iter++) {
    // ---- coal_EM(epochs, rates): A_ep / B_ep
    if (tid == 0) ab_prefix(E, ep, rt, w.cse);  // (wave 0's cse: free until the barrier after ab_at)
    __syncthreads();
    for (int e = tid; e < E; e += NT) ab_at(m, E, ep, rt, first_wave, e, A, B);
    __syncthreads();
    // ---- the E-step over the rows
#pragma unroll
    for (int k = 0; k < KOWN; k++) nacc[k] = 0.0, dacc[k] = 0.0;
    prev_ll = ll;
    ll = 0.0;
    for (int g = 0; g < groups; g++) {
      double wg[WAVES];
      bool any = false;
#pragma unroll
      for (int i = 0; i < WAVES; i++) {
        const int r = g * WAVES + i;
        wg[i] = (r < R) ? wrow[r] : 0.0;
        any = any || wg[i] > 0;
      }
      if (!any) continue;  // (the same for every thread of the workgroup)
      const int r = g * WAVES + wave;
      const bool active = r < R && wrow[r] > 0;  // (the reference visits bins with a count only)
      int kind;
      double a0, a1;
      if (g < 64) {
        kind = __shfl(own_kind, g, 64), a0 = __shfl(own_a0, g, 64), a1 = __shfl(own_a1, g, 64);
      } else {
        const int rr = r < R ? r : R - 1;
        kind = kinds[rr], a0 = age_begin[rr], a1 = age_end[rr];
      }
      double logl;
      flags |= wave_call(m, v, kind, a0, a1, active, lane, w, &logl);
      if (lane == 0) w.misc[3] = logl;
      __syncthreads();
      // the group's rows into the accumulators, ascending (coal.cpp:3704-3733 with weights for counts)
#pragma unroll
      for (int k = 0; k < KOWN; k++) {
        const int e = tid + k * NT;
        if (e < E) {
#pragma unroll
          for (int i = 0; i < WAVES; i++) {
            if (wg[i] > 0) {
              const WaveLds wi = wave_lds(first_wave, E, i);
              nacc[k] += wg[i] * wi.num[e];
              dacc[k] += wg[i] * wi.den[e];
            }
          }
        }
      }
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < WAVES; i++)
          if (wg[i] > 0) ll += wg[i] * wave_lds(first_wave, E, i).misc[3];
      }
      __syncthreads();
    }
    // ---- M-step, floor, stop rule (em_interval_fit.hpp); wave 0's num holds the numerators for the carry
#pragma unroll
    for (int k = 0; k < KOWN; k++) {
      const int e = tid + k * NT;
      if (e < E) {
        first_wave[E + e] = nacc[k];
        if (nacc[k] != 0) rt[e] = mstep_own(nacc[k], dacc[k], rt[e], rate_floor);
      }
    }
    __syncthreads();
    if (tid == 0) {
      mstep_carry(E, first_wave + E, rt);
      ctl[0] = stop_rule(ll, prev_ll, rel_tol, iter, min_iter) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (ctl[0] != 0.0) break;
  }

  // ---- results: rates, "Total iterations", the last log-likelihood, the flags of all calls of all iterations
  for (int e = tid; e < E; e += NT) out_rates[e] = rt[e];
  if (lane == 0) w.misc[0] = (double)flags;  // (wave_call's flags are the same in all lanes)
  __syncthreads();
  if (tid == 0) {
    int f = (iter == max_iter) ? COLATE_FLAG_MAXITER : 0;
#pragma unroll
    for (int i = 0; i < WAVES; i++) f |= (int)wave_lds(first_wave, E, i).misc[0];
    *out_iters = iter;
    *out_ll = ll;
    *out_flags = f;
  }
}

// colate_em_interval_batch: workgroup b is replicate b of one set of rows
template <int WAVES, int KOWN>
__global__ __launch_bounds__(WAVES * 64) void em_interval_fit_kernel(
    int R, int E, const int* __restrict__ kinds, const double* __restrict__ age_begin, const double* __restrict__ age_end,
    const double* __restrict__ weights, const double* __restrict__ epochs, const double* __restrict__ init_rates,
    int max_iter, int min_iter, double rel_tol, double rate_floor, double* __restrict__ out_rates,
    int* __restrict__ out_iters, double* __restrict__ out_ll, int* __restrict__ out_flags) {
  extern __shared__ double smem[];
  const size_t b = blockIdx.x;
  fit_replicate<WAVES, KOWN>(smem, R, E, kinds, age_begin, age_end, weights + b * R, epochs, init_rates, max_iter, min_iter,
                             rel_tol, rate_floor, out_rates + b * E, out_iters + b, out_ll + b, out_flags + b);
}

// colate_interval_fit_groups: workgroup i is replicate i % B of group i / B, whose rows, weights, epochs and starting
// rates it finds through the group's descriptor.  A group without rows is left to the host (its rates are its starting
// rates): its workgroups return here, on a value all their threads read alike, before any barrier.
template <int WAVES, int KOWN>
__global__ __launch_bounds__(WAVES * 64) void em_interval_fit_groups_kernel(
    int B, int E, const ColateIntervalGroup* __restrict__ groups, int max_iter, int min_iter, double rel_tol,
    double rate_floor, double* __restrict__ out_rates, int* __restrict__ out_iters, double* __restrict__ out_ll,
    int* __restrict__ out_flags) {
  extern __shared__ double smem[];
  const size_t i = blockIdx.x;
  const ColateIntervalGroup g = groups[i / B];
  if (g.R < 1) return;
  const size_t b = i % B;
  fit_replicate<WAVES, KOWN>(smem, g.R, E, g.kinds, g.age_begin, g.age_end, g.W + b * g.R, g.epochs, g.init_rates, max_iter,
                             min_iter, rel_tol, rate_floor, out_rates + i * E, out_iters + i, out_ll + i, out_flags + i);
}

constexpr size_t fit_lds_bytes(int E, int waves) { return (lds_doubles(E, waves) + 2) * sizeof(double); }

}  // namespace

int colate_em_interval_fit_waves(int E) { return E <= 256 ? COLATE_EM_INTERVAL_FIT_WAVES : 1; }

hipError_t colate_em_interval_fit_launch(int B, int R, int E, const int* kinds, const double* age_begin,
                                         const double* age_end, const double* weights, const double* epochs,
                                         const double* init_rates, int max_iter, int min_iter, double rel_tol,
                                         double rate_floor, double* out_rates, int* out_iters, double* out_ll,
                                         int* out_flags, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  if (R < 1 || E < 1 || E > COLATE_EM_MAX_E) return hipErrorInvalidValue;
  if (E <= 256) {  // eight calls at a time, one epoch per thread: 57 KiB of LDS at E = 256
    constexpr int W = COLATE_EM_INTERVAL_FIT_WAVES;
    static_assert(W * 64 >= 256 && fit_lds_bytes(256, W) <= 64 * 1024, "one owner per epoch, LDS without an opt-in");
    em_interval_fit_kernel<W, 1><<<B, W * 64, fit_lds_bytes(E, W), stream>>>(
        R, E, kinds, age_begin, age_end, weights, epochs, init_rates, max_iter, min_iter, rel_tol, rate_floor, out_rates,
        out_iters, out_ll, out_flags);
  } else {  // one call at a time, up to 16 epochs per lane: 57 KiB at E = 1024
    static_assert(64 * 16 >= COLATE_EM_MAX_E && fit_lds_bytes(COLATE_EM_MAX_E, 1) <= 64 * 1024, "");
    em_interval_fit_kernel<1, 16><<<B, 64, fit_lds_bytes(E, 1), stream>>>(
        R, E, kinds, age_begin, age_end, weights, epochs, init_rates, max_iter, min_iter, rel_tol, rate_floor, out_rates,
        out_iters, out_ll, out_flags);
  }
  return hipGetLastError();
}

hipError_t colate_em_interval_fit_groups_launch(int G, int B, int E, const ColateIntervalGroup* groups, int max_iter,
                                                int min_iter, double rel_tol, double rate_floor, double* out_rates,
                                                int* out_iters, double* out_ll, int* out_flags, hipStream_t stream) {
  if (G < 1 || B < 1 || (long long)G * B > 0x7fffffffLL || E < 1 || E > COLATE_EM_MAX_E) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)((long long)G * B);
  if (E <= 256) {  // (the two instantiations and their LDS: colate_em_interval_fit_launch)
    constexpr int W = COLATE_EM_INTERVAL_FIT_WAVES;
    em_interval_fit_groups_kernel<W, 1><<<grid, W * 64, fit_lds_bytes(E, W), stream>>>(
        B, E, groups, max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_ll, out_flags);
  } else {
    em_interval_fit_groups_kernel<1, 16><<<grid, 64, fit_lds_bytes(E, 1), stream>>>(
        B, E, groups, max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_ll, out_flags);
  }
  return hipGetLastError();
}
