// colate_amd/csrc/em_interval_fit.hpp
//
// What closes one iteration of the EM fit on interval-dated mutations (colate_em_interval_batch): the M-step with its
// floor (coal.cpp:3771-3815, regularise == 2) and the stop rule (coal.cpp:3822) -- once, for the host twin
// (em_interval_host.cpp) and for gfx950 (em_interval_fit_kernel.hip).  Build with -ffp-contract=off.
//
// The reference's M-step is one ascending loop in which an epoch without a numerator takes the NEW rate of the epoch
// before it.  Only those epochs depend on a neighbour, so the loop is split without changing a value: mstep_own() for
// the epochs that have a numerator (any thread, from the accumulators it holds), then mstep_carry() for the others,
// ascending (one thread).  mstep() is the two in order.
#pragma once
#include "em_interval.hpp"

namespace em_interval {

// rate of an epoch with num != 0: unchanged where den == 0, else num / den, not below the floor
EM_HD double mstep_own(double num, double den, double rate, double rate_floor) {
  if (den == 0) return rate;
  double r = num / den;
  if (r < rate_floor) r = rate_floor;
  return r;
}
// epochs with num == 0 take the rate in front of them (0 at e == 0); rates[] already holds mstep_own() elsewhere
EM_HD void mstep_carry(int E, const double* num, double* rates) {
  for (int e = 0; e < E; e++)
    if (num[e] == 0) rates[e] = (e > 0) ? rates[e - 1] : 0.0;
}
EM_HD void mstep(int E, const double* num, const double* den, double rate_floor, double* rates) {
  for (int e = 0; e < E; e++)
    if (num[e] != 0) rates[e] = mstep_own(num[e], den[e], rates[e], rate_floor);
  mstep_carry(E, num, rates);
}

// coal.cpp:3822, with prev_ll = log(0) before the first iteration
EM_HD bool stop_rule(double ll, double prev_ll, double rel_tol, int iter, int min_iter) {
  return (ll / prev_ll > 1.0 - rel_tol) & (iter > min_iter);
}

}  // namespace em_interval
