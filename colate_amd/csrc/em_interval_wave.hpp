// colate_amd/csrc/em_interval_wave.hpp -- one call of coal_EM::EM_shared / EM_notshared by one wavefront of gfx950: the
// functions of em_interval.hpp with the epochs of the call strided over the 64 lanes, and the LDS layout around it.
// Shared by em_interval_kernel.hip (R calls, one E-step) and em_interval_fit_kernel.hip (the whole EM loop).  Device only.
//
// Whatever the reference sums from left to right -- the cumulative rate, the logsumexp fold of the normaliser, the
// `integ` recurrence -- is summed from left to right here too, by lane 0 of the call's wave over LDS, between phases
// in which all lanes work on their epochs: the device then equals the host twin (em_interval::call<EmMath>) bit for
// bit.  The addends of the cumulative rate are formed by all lanes; only the additions are serial.
//
// Every phase boundary is a workgroup barrier that all waves of the workgroup reach: wave_call() has the same six
// barriers whatever its arguments, and a wave that has no call (`active` false) only keeps the barriers.
#pragma once
#include <hip/hip_runtime.h>

#include "em_interval.hpp"

namespace em_interval {

__device__ __forceinline__ int wave_sum(int x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
__device__ __forceinline__ int wave_or(int x) {
  for (int o = 32; o > 0; o >>= 1) x |= __shfl_xor(x, o, 64);
  return x;
}

// LDS, in doubles: exp table [64] | epochs [E] | rates [E] | A_ep [E] | B_ep [E] | per wave: cse [E], num [E], den [E], misc [4]
__host__ __device__ constexpr size_t wave_doubles(int E) { return 3 * (size_t)E + 4; }
__host__ __device__ constexpr size_t lds_doubles(int E, int waves) {
  return em::kExpTableDoubles + 4 * (size_t)E + waves * wave_doubles(E);
}

struct WaveLds {  // one wave's part of the LDS
  double *cse, *num, *den, *misc;
};
__device__ __forceinline__ WaveLds wave_lds(double* first_wave, int E, int wave) {
  WaveLds w;
  w.cse = first_wave + wave * wave_doubles(E);
  w.num = w.cse + E;
  w.den = w.num + E;
  w.misc = w.den + E;
  return w;
}

// One call (kind, a0, a1) against v by the calling wave.  On return w.num[e] / w.den[e] hold the call's num / denom
// (written by the lane that owns e = lane, lane + 64, ...: visible to other lanes after the next barrier), *logl what
// the reference returns (0 where its normaliser is not finite: coal_EM.cpp:288-292, 461-465), and the return value the
// call's COLATE_FLAG_NAN / COLATE_FLAG_NEG, the same in all lanes.  w.misc[0..2] are used.
__device__ __forceinline__ int wave_call(const EmMath& m, const View& v, int kind, double a0, double a1, bool active,
                                         int lane, const WaveLds& w, double* logl) {
  const int E = v.E;
  Call c;
  c.kind = kind, c.a0 = a0, c.a1 = a1;
  c.point = c.a0 == c.a1;
  c.csb = 0.0, c.csa = 0.0;
  c.eb = 0, c.ee = 0;
  if (active) {
    int nb = 0, ne = 0;  // epoch_of(), the count shared among the lanes
    for (int e = lane; e < E; e += 64) nb += (v.ep[e] <= c.a0) ? 1 : 0, ne += (v.ep[e] <= c.a1) ? 1 : 0;
    c.eb = wave_sum(nb) - 1, c.ee = wave_sum(ne) - 1;
    for (int e = lane; e < E; e += 64)
      if (e > 0) w.cse[e] = step_product(v, c, e);
  }
  __syncthreads();
  if (active && lane == 0) {
    cum_fold(v, c, w.cse);
    w.misc[0] = c.csb, w.misc[1] = c.csa;
  }
  __syncthreads();
  if (active) {
    c.csb = w.misc[0], c.csa = w.misc[1];
    for (int e = lane; e < E; e += 64) log_values(m, v, c, w.cse, e, w.num, w.den);
  }
  __syncthreads();
  if (active && lane == 0) w.misc[2] = normaliser(m, v, c, w.num);
  __syncthreads();
  const double nc = active ? w.misc[2] : 0.0;
  const bool failed = inf_or_nan(nc);
  const Closing k = closing_of(v, c);
  if (active && !failed)
    for (int e = lane; e < E; e += 64) exp_at(m, v, k, nc, e, w.num, w.den);
  __syncthreads();
  if (active && lane == 0 && !failed) integ_fold(k, w.num, w.cse);
  __syncthreads();
  int flags = 0;
  if (active) {
    for (int e = lane; e < E; e += 64) {
      if (failed) w.num[e] = 0.0, w.den[e] = 0.0;
      else finish_at(v, c, k, w.cse, e, w.num, w.den);
      flags |= value_flags(w.num[e], w.den[e]);
    }
    flags = wave_or(flags);
  }
  *logl = failed ? 0.0 : nc;
  return flags;
}

}  // namespace em_interval
