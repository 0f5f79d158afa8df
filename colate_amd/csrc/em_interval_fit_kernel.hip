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
#include <hip/hip_runtime.h>

#include "em_interval_fit.hpp"
#include "em_interval_wave.hpp"
#include "em_kernels.h"

namespace {

using namespace em_interval;

// KOWN: epochs owned per thread (e = tid, tid + WAVES * 64, ...): WAVES * 64 * KOWN >= the largest E of the layout
template <int WAVES, int KOWN>
__global__ __launch_bounds__(WAVES * 64) void em_interval_fit_kernel(
    int R, int E, const int* __restrict__ kinds, const double* __restrict__ age_begin, const double* __restrict__ age_end,
    const double* __restrict__ weights, const double* __restrict__ epochs, const double* __restrict__ init_rates,
    int max_iter, int min_iter, double rel_tol, double rate_floor, double* __restrict__ out_rates,
    int* __restrict__ out_iters, double* __restrict__ out_ll, int* __restrict__ out_flags) {
  constexpr int NT = WAVES * 64;
  extern __shared__ double smem[];
  double* tab = smem;
  double* ep = tab + em::kExpTableDoubles;
  double* rt = ep + E;
  double* A = rt + E;
  double* B = A + E;
  double* first_wave = B + E;
  double* ctl = first_wave + WAVES * wave_doubles(E);  // [0]: the verdict of the stop rule
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const WaveLds w = wave_lds(first_wave, E, wave);
  const double* wrow = weights + (size_t)blockIdx.x * R;

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
  for (int e = tid; e < E; e += NT) out_rates[(size_t)blockIdx.x * E + e] = rt[e];
  if (lane == 0) w.misc[0] = (double)flags;  // (wave_call's flags are the same in all lanes)
  __syncthreads();
  if (tid == 0) {
    int f = (iter == max_iter) ? COLATE_FLAG_MAXITER : 0;
#pragma unroll
    for (int i = 0; i < WAVES; i++) f |= (int)wave_lds(first_wave, E, i).misc[0];
    out_iters[blockIdx.x] = iter;
    out_ll[blockIdx.x] = ll;
    out_flags[blockIdx.x] = f;
  }
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
